"""Guidance reuse for the denoising loop: run the unconditional sample of the guidance pair only on planned steps.

Between neighbouring steps the guidance direction d = c - u (conditional minus unconditional prediction) moves far more slowly than c
itself (FasterCache's "CFG cache"), and guidance applied only inside an interval of the schedule costs less and often looks better
(Kynkaanniemi et al., 2024).  Every step of an edit is therefore one of

    "pair"    both samples run, as in the plain loop; the step also stores d = bf16(c - u)
    "reuse"   the conditional sample runs alone; the combine uses the stored d:  u' = bf16(c - d), v = bf16(u' + bf16(g * d))
    "off"     the conditional sample runs alone, no guidance (the launch of an unguided edit)

Like TeaCache's, the plan is a function of the schedule alone: it is made before the first step and nothing is read back per step, so a
hipGraph-replayed loop needs one captured graph per kind of step (loop.GraphedDenoiser).  `GuidanceState` is what one edit keeps.

Host side only; the device pass is ce_cfg_unipc_step_delta (csrc/ce_sched.hip)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

KINDS = ("pair", "reuse", "off")
SHARDED = "guidance reuse with {} is not implemented (the stored direction is latent-local; nothing sharded has been tested with it)"


@dataclass(frozen=True)
class GuidanceReuseConfig:
    """pair_every: one step in `pair_every` inside the interval runs the pair, the others reuse its direction (1: every step runs the
    pair).  interval (lo, hi), fractions of the schedule: step i of n is guided when lo * n <= i < hi * n; the other steps are "off"."""
    pair_every: int = 2
    interval: Tuple[float, float] = (0.0, 1.0)

    def __post_init__(self):
        _validate(self)


def _validate(cfg) -> Tuple[int, float, float]:
    pe = cfg.pair_every
    if isinstance(pe, bool) or int(pe) != pe or int(pe) < 1:
        raise ValueError(f"guidance reuse: pair_every must be an integer >= 1, got {pe!r}")
    try:
        lo, hi = (float(v) for v in cfg.interval)
    except (TypeError, ValueError):
        raise ValueError(f"guidance reuse: interval must be a pair (lo, hi), got {cfg.interval!r}") from None
    if not 0.0 <= lo <= hi <= 1.0:  # (a NaN fails every comparison)
        raise ValueError(f"guidance reuse: interval must satisfy 0 <= lo <= hi <= 1, got {cfg.interval!r}")
    return int(pe), lo, hi


def plan(num_steps: int, cfg: GuidanceReuseConfig, forced_pairs: Iterable[int] = ()) -> List[str]:
    """The kind of every step of an edit.  Steps outside the interval are "off".  The first inside step, and the first inside step after
    an "off" run, is a "pair"; the pair_every - 1 inside steps after a "pair" are "reuse".  Every index of `forced_pairs` that lies inside
    the interval is a "pair" and restarts the count (a step whose latent shape or conditioning differs from the stored direction's)."""
    pe, lo, hi = _validate(cfg)
    forced = {int(f) for f in forced_pairs}
    out, since = [], None  # since: inside steps since the last "pair", that one included; None: no direction is stored
    for i in range(int(num_steps)):
        if not lo * num_steps <= i < hi * num_steps:
            out.append("off")
            since = None
        elif since is None or since >= pe or i in forced:
            out.append("pair")
            since = 1
        else:
            out.append("reuse")
            since += 1
    return out


def report(plan_: Sequence[str]) -> dict:
    """What `denoise` leaves on `transformer.guidance_report` after a guided edit with guidance reuse."""
    plan_ = [str(k) for k in plan_]
    return {"plan": plan_, **{k: plan_.count(k) for k in KINDS}}


def rel_l2_from_sums(sums, max_age: int, history: Sequence[int]) -> List[List[float]]:
    """ce_cfg_unipc_step_delta's measured sums [steps, max_age + 1] (per step: sum (d_new - d_age a)^2 for a = 1..max_age, then
    sum d_new^2) -> rel_l2[step][a - 1] = sqrt(sum diff^2 / sum d_new^2) in float64.  history[step] = how many earlier directions of
    this step's shape the ring held: older ages are NaN, as is every entry of a step that was not measured or whose direction is all zeros."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, max_age + 1)
    out = []
    for row, have in zip(sums, history):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.sqrt(row[:max_age] / row[max_age])
        out.append([float(v) if a < have and np.isfinite(v) else float("nan") for a, v in enumerate(r)])
    return out


class GuidanceState:
    """Guidance reuse in one running edit (`loop.denoise(guidance_reuse=, guidance_measure=, keep_deltas=)`).
    config: a GuidanceReuseConfig for this call; None = whatever `transformer.enable_guidance_reuse()` set (nothing: every guided step runs
    the pair).  The "pair" / "reuse" / "off" plan of the whole edit is made in `begin`, before the first step, from the schedule alone
    (`forced`, the truncation step, is always a "pair": an 8-frame direction does not fit 2-frame latents); `transformer.guidance_report`
    then holds {"plan", "pair", "reuse", "off"}.  An edit without guidance ignores the config and its report is None.  The stored direction
    `delta` is one bf16 tensor of the latents' shape that this object owns: a second edit never sees the first one's.  A callback that
    replaces the latents keeps it; one that replaces an embedding makes the next guided step a "pair" (`replaced`).
    measure = A (1..4): every step a "pair" whose store pass also measures, on the device, how far the direction is from those of the
    1..A steps before - `delta` is then a ring of the last A directions of this latent shape, `delta_measure` the step's (slot, table,
    row); one read-back after the last step (`finish`).  The latents are the plain loop's; the edit runs eagerly.  Afterwards
    `transformer.guidance_measurement` holds {"timesteps", "rel_l2": [steps][A] (NaN where no direction of that age and shape exists)} and,
    with keep_deltas, "deltas": the per-step directions (bf16, on the CPU)."""

    def __init__(self, transformer, config: GuidanceReuseConfig, n_steps: int, forced: Iterable[int], device, max_age: Optional[int] = None,
                 keep_deltas: bool = False):
        self.transformer, self.config, self.forced, self.keep_deltas = transformer, config, set(forced), bool(keep_deltas)
        self.plan = plan(n_steps, config, self.forced)
        self.delta = self.delta_measure = None
        self.valid = False  # has a "pair" step of this edit, at this latent shape and conditioning, written the direction?
        self.table = None if max_age is None else torch.full((n_steps, int(max_age) + 1), float("nan"), dtype=torch.float32, device=device)
        self.seen, self.history, self.kept = 0, [0] * n_steps, []  # measuring: directions of this shape stored so far; per step, how many the ring held
        transformer.guidance_report = report(self.plan)

    @property
    def measuring(self) -> bool:
        return self.table is not None

    @classmethod
    def begin(cls, transformer, n_steps: int, device, guided: bool, config=None, measure: Optional[int] = None, keep_deltas: bool = False,
              forced: Iterable[int] = (), tea_active: bool = False) -> Optional["GuidanceState"]:
        """Resets the report; None when the edit has no guidance reuse.  Refusals, in this order: measuring an unguided edit (ValueError);
        together with TeaCache, enabled or measuring (ValueError); sharded tokens or CFG parallelism (NotImplementedError); measuring with
        a `config` of the call's own, then a max_age outside 1..CFG_MAX_AGE (ValueError)."""
        if hasattr(transformer, "guidance_report"):
            transformer.guidance_report = None
        cfg = config if config is not None else getattr(transformer, "_guidance_reuse", None)
        if measure is not None and not guided:
            raise ValueError("guidance_measure needs a guided edit (guidance_scale > 1 and negative_prompt_embeds)")
        if not guided or (cfg is None and measure is None):
            return None
        if tea_active:
            raise ValueError("guidance reuse and TeaCache (enabled or measuring) exclude each other: the cached residual has the guidance "
                             "pair's row count, which a single-sample step does not match")
        from .loop import refuse_sharded
        refuse_sharded(transformer, SHARDED)
        if measure is not None:
            from . import ops
            if config is not None:
                raise ValueError("guidance_measure measures the plain loop (every step a pair): it takes no guidance_reuse plan")
            if not 1 <= int(measure) <= ops.CFG_MAX_AGE:
                raise ValueError(f"guidance_measure: max_age must be in 1..{ops.CFG_MAX_AGE}, got {measure}")
            cfg = GuidanceReuseConfig(pair_every=1)
        return cls(transformer, cfg, n_steps, forced, device, measure, keep_deltas)

    def before_step(self, i: int, latents: torch.Tensor):
        """Make the direction buffer (the ring) of the latents' shape - at the first step and again behind the truncation, never under a
        capture - and check that a planned reuse has a stored direction."""
        if self.table is not None:
            A = self.table.shape[1] - 1
            if self.delta is None or self.delta.shape[1:] != latents.shape:
                self.delta, self.seen = torch.zeros((A,) + tuple(latents.shape), dtype=torch.bfloat16, device=latents.device), 0
            self.delta_measure = (self.seen % A, self.table, i)
            self.history[i] = min(self.seen, A)
        elif self.delta is None or self.delta.shape != latents.shape:
            self.delta, self.valid = torch.zeros(latents.shape, dtype=torch.bfloat16, device=latents.device), False
        if self.plan[i] == "reuse" and not self.valid:
            raise RuntimeError(f"guidance reuse: step {i} is planned to reuse a direction no step has stored")

    def after_step(self, i: int):
        if self.table is not None:
            if self.keep_deltas:
                self.kept.append(self.delta[self.delta_measure[0]].clone())
            self.seen += 1
        if self.plan[i] != "reuse":
            self.valid = self.plan[i] == "pair"

    def replaced(self, i: int) -> bool:
        """A callback replaced an embedding behind step i: the stored direction belongs to the old conditioning, so the next guided step
        runs the pair and the count restarts there.  True when the plan changed."""
        if self.table is not None or i + 1 >= len(self.plan):
            return False
        self.forced = self.forced | {i + 1}
        self.plan = self.plan[: i + 1] + plan(len(self.plan), self.config, self.forced)[i + 1:]
        if self.plan[i + 1] == "reuse":  # (an inside step: forced)
            raise RuntimeError("guidance reuse: the re-planned step is not a pair")
        self.transformer.guidance_report = report(self.plan)
        self.valid = False
        return True

    def finish(self, timesteps: torch.Tensor):
        """Measuring: the one read of the table, after the last step."""
        if self.table is None:
            return
        m = {"timesteps": [int(v) for v in timesteps.tolist()],
             "rel_l2": rel_l2_from_sums(self.table.cpu().numpy(), self.table.shape[1] - 1, self.history)}
        if self.keep_deltas:
            m["deltas"] = [d.cpu() for d in self.kept]
        self.transformer.guidance_measurement = m
