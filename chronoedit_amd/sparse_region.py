"""Sparse region edits: on most steps of a region-limited edit the DiT runs only on the tokens under the mask.

The region blend (chronoedit_amd/region.py) overwrites the sample with the noised source wherever w == 0, after every step: what the model
predicts there is thrown away, and those tokens matter only as keys and values for the tokens under the mask.  Every step of an edit is
therefore one of

    "compute"   the plain forward, launch for launch
    "refresh"   the plain forward, which also keeps every layer's K (after norm + RoPE) and V^T of ALL tokens in a per-edit cache
    "sparse"    the forward on the ACTIVE token rows only - the patches the mask touches plus a margin; self-attention reads the cached
                K / V^T of all tokens, in which the active tokens' entries were just replaced by this step's; the prediction is 0 elsewhere

the region-KV-cache idea of RegionE and SIGE.  Like TeaCache's and guidance reuse's, the plan is a function of the schedule and the mask
alone: it is made before the first step and nothing is read back per step, so a hipGraph-replayed loop needs one captured graph per kind.

Host side only; the device passes are csrc/ce_sparse.hip (gather / scatter around the unchanged GEMM and attention kernels)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import torch

KINDS = ("compute", "refresh", "sparse")
PAD = 8  # active rows per sample come in multiples of 8 (the GEMMs' row granularity for the transposed V product)


@dataclass(frozen=True)
class SparseRegionConfig:
    """refresh_every: one step in `refresh_every` is dense and refills the cache (1: every step is dense, nothing is sparse).
    start: fraction of the schedule that runs dense before the first sparse step may happen.  margin: patches (Chebyshev distance) the
    active set is dilated by around the mask."""
    refresh_every: int
    start: float = 0.0
    margin: int = 1

    def __post_init__(self):
        _validate(self)


def _validate(cfg) -> Tuple[int, float, int]:
    re_, mg = cfg.refresh_every, cfg.margin
    if isinstance(re_, bool) or int(re_) != re_ or int(re_) < 1:
        raise ValueError(f"sparse region: refresh_every must be an integer >= 1, got {re_!r}")
    if isinstance(mg, bool) or int(mg) != mg or int(mg) < 0:
        raise ValueError(f"sparse region: margin must be an integer >= 0, got {mg!r}")
    try:
        st = float(cfg.start)
    except (TypeError, ValueError):
        raise ValueError(f"sparse region: start must be a fraction of the schedule, got {cfg.start!r}") from None
    if not 0.0 <= st <= 1.0:  # (a NaN fails both comparisons)
        raise ValueError(f"sparse region: start must lie in [0, 1], got {cfg.start!r}")
    return int(re_), st, int(mg)


def active_tokens(w: torch.Tensor, T: int, margin: int = 1) -> Tuple[torch.Tensor, int]:
    """w = fp32 [h, w] (region.latent_weights), T latent frames -> (ids, n_active).
    A patch (i, j) of the (h/2) x (w/2) grid is active when any of its 2 x 2 latent cells has w > 0; the active patches are dilated by
    `margin` patches (Chebyshev distance) and taken in all T frames.  ids = the sorted unique int64 token indices (t * Hp + i) * Wp + j (the
    order of the patchify pass), padded to a multiple of 8 with the lowest-index inactive tokens (real tokens: computed, and harmless);
    n_active = their number before the padding.  A grid that is active everywhere returns all its tokens."""
    if w.dim() != 2 or w.shape[0] % 2 or w.shape[1] % 2:
        raise ValueError(f"active_tokens: need [h, w] weights with even h and w, got {tuple(w.shape)}")
    if isinstance(margin, bool) or int(margin) != margin or margin < 0 or T < 1:
        raise ValueError(f"active_tokens: margin must be an integer >= 0 and T >= 1, got margin={margin!r}, T={T!r}")
    w = w.detach().to(device="cpu", dtype=torch.float32)
    Hp, Wp = w.shape[0] // 2, w.shape[1] // 2
    act = (w.view(Hp, 2, Wp, 2) > 0).any(3).any(1)
    if margin > 0 and bool(act.any()):
        k = 2 * int(margin) + 1
        act = torch.nn.functional.max_pool2d(act.to(torch.float32)[None, None], k, stride=1, padding=int(margin))[0, 0] > 0
    flat = act.reshape(-1)
    n_plane = int(flat.sum())
    n_active = n_plane * int(T)
    N = T * Hp * Wp
    mask = flat.repeat(int(T))
    short = -n_active % PAD
    if short:
        free = torch.nonzero(~mask).reshape(-1)[:short]  # the lowest-index inactive tokens (fewer than asked: the grid is full)
        mask[free] = True
    ids = torch.nonzero(mask).reshape(-1).to(torch.int64)
    assert ids.numel() <= N
    return ids, n_active


def validate_ids(ids: torch.Tensor, n_tokens: int) -> torch.Tensor:
    """The once-per-edit check of an id list (the kernels trust it): integer, 1-D, non-empty, sorted, unique, inside [0, n_tokens)."""
    if ids.dim() != 1 or ids.numel() == 0 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"sparse region: ids must be a non-empty 1-D int32 / int64 tensor, got {ids.dtype} {tuple(ids.shape)}")
    c = ids.detach().to(device="cpu", dtype=torch.int64)
    if int(c[0]) < 0 or int(c[-1]) >= int(n_tokens) or (c.numel() > 1 and not bool((c[1:] > c[:-1]).all())):
        raise ValueError(f"sparse region: ids must be sorted, unique and inside [0, {n_tokens})")
    return c


def plan(n_steps: int, cfg: SparseRegionConfig, forced: Iterable[int] = (), full: bool = False) -> List[str]:
    """The kind of every step.  first = ceil(start * n_steps).  Step i is dense when i < first, when i is in `forced`, or when
    (i - base) % refresh_every == 0, where base = first, or the index behind the last forced step (the count restarts there).  A dense step
    is a "refresh" only when the step behind it is "sparse" - otherwise nobody would read what it stores and it is a "compute".  So
    refresh_every == 1 gives no sparse step, and neither does full = True (the active set is the whole grid: nothing to save)."""
    re_, st, _ = _validate(cfg)
    n = int(n_steps)
    forced = {int(f) for f in forced}
    first = int(math.ceil(st * n))
    dense, base = [], first
    for i in range(n):
        if full or i < first or i in forced:
            dense.append(True)
            base = max(base, i + 1)
        else:
            dense.append((i - base) % re_ == 0)
    return ["sparse" if not d else "refresh" if i + 1 < n and not dense[i + 1] else "compute" for i, d in enumerate(dense)]


def report(plan_: Sequence[str], n_active: int, n_tokens: int) -> dict:
    """What `denoise` leaves on `transformer.sparse_report`: the plan, how often each kind runs, the active rows per sample of a sparse step
    (padding included) and the tokens per sample of the shape the sparse steps run at."""
    plan_ = [str(k) for k in plan_]
    return {"plan": plan_, **{k: plan_.count(k) for k in KINDS}, "active": int(n_active), "tokens": int(n_tokens)}


class SparseRegionState:
    """The sparse region of one running edit (`loop.denoise(sparse_region=)`; needs `region=` or a detecting `auto_region=`: a ValueError
    without).  config: a SparseRegionConfig for this call; None = whatever `transformer.enable_sparse_region()` set, which an edit without a
    region ignores.  The "compute" / "refresh" / "sparse" plan of the whole edit is made in `setup` - before the first step for an explicit
    region, behind the detecting step for an automatic one - from the schedule and the mask alone (every step in `forced` is dense: with
    temporal reasoning every step up to and including the truncation step, with an automatic region every step up to the detecting one;
    the active tokens are those of the shape the sparse steps run at); `transformer.sparse_report` then holds {"plan", "compute",
    "refresh", "sparse", "active", "tokens"}, None for an edit without a plan.  A sparse step runs the model on the active token rows only,
    against the K / V^T the last refresh step stored (DiTEngine.sparse_begin has the sizes); the blend keeps the source where w == 0
    exactly, as ever.  A callback that replaces the latents or an embedding makes the next step dense, and the plan is remade from there
    (`replaced`).  With TeaCache or guidance reuse (enabled or measuring) it is a ValueError (raised by the loop, in front of every
    feature's setup); with fp8 GEMMs or attention, without the transposed-V self-attention, with sharded tokens or CFG parallelism a
    NotImplementedError (the engine's `sparse_check`, and the region's own refusal)."""

    def __init__(self, transformer, config: SparseRegionConfig, n_steps: int):
        self.transformer, self.config, self.n_steps = transformer, config, int(n_steps)
        self.plan = self.ids = self.tokens = self.full = None
        self.forced = set()

    @classmethod
    def begin(cls, transformer, config: Optional[SparseRegionConfig], n_steps: int) -> Optional["SparseRegionState"]:
        """Resets the report; None without a config (the caller passes none for an edit without a region)."""
        if hasattr(transformer, "sparse_report"):
            transformer.sparse_report = None
        if config is None:
            return None
        transformer.engine().sparse_check()
        return cls(transformer, config, n_steps)

    def setup(self, w: torch.Tensor, forced: Iterable[int], n_samples: int, T: int, h: int, wl: int):
        """The plan, the active ids and the engine's cache (reserved here: outside any capture) for the weights w, for forwards of n_samples
        samples at T latent frames of h x wl cells."""
        self.forced = set(forced)
        self.ids, _ = active_tokens(w, T, self.config.margin)  # (the one device-to-host read: the latent weights)
        self.tokens = T * (h // 2) * (wl // 2)
        self.full = self.ids.numel() >= self.tokens or self.ids.numel() % PAD != 0  # the whole grid: nothing to leave out
        self.plan = plan(self.n_steps, self.config, self.forced, full=self.full)
        self.transformer.sparse_report = report(self.plan, self.ids.numel(), self.tokens)
        if "sparse" in self.plan:
            self.transformer.engine().sparse_begin(self.ids, n_samples, T, h, wl)

    def replaced(self, i: int) -> bool:
        """A callback replaced the latents or an embedding behind step i: the cached K / V^T of the inactive tokens belong to the old ones, so
        the next step is dense and the count restarts behind it.  True when the plan changed."""
        if self.plan is None or i + 1 >= len(self.plan):
            return False
        self.forced = self.forced | {i + 1}
        self.plan = self.plan[: i + 1] + plan(len(self.plan), self.config, self.forced, full=self.full)[i + 1:]
        self.transformer.sparse_report = report(self.plan, self.ids.numel(), self.tokens)
        return True
