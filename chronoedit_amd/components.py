"""Connected components of a byte plane, with the small ones dropped: speckle removal for sketched and detected regions.

Foreground is a non-zero byte.  The neighbourhood is 8-connected: two pixels that touch only diagonally are one component.

    roots   int32 [H, W]   for a foreground pixel the smallest linear index y * W + x over the pixels of its component, -1 for background.
                           No order of evaluation enters this label: a parallel implementation is compared with it bit for bit
    sums    int32 [H, W]   at each root's own position the number of pixels of its component whose `weight` byte is non-zero (no weight
                           plane: every pixel counts), 0 everywhere else
    keep    uint8 [H, W]   the plane where the component's weight is >= the least weight kept, else 0 - and stats int32 [4] = (components
                           kept, components dropped, weight dropped, largest weight).  The least weight is an int >= 1, or for a float in
                           (0, 1) ceil(fraction * largest weight), the fraction read as the nearest one with a denominator <= 65536 (the
                           idiom of `sketch.pixels` and `focus.focus_box`) and the ceiling exact

`filter` is the three in a row where the bytes lie: the device passes for a CUDA tensor (csrc/ce_components.hip: a block-based union-find,
integer atomics only, no host read), the numpy expression below for a CPU tensor - `reference`, the definition and the host path.  The
host form works on ROW RUNS: the runs of every row, then a union-find over the runs of adjacent rows that overlap or touch diagonally, so
that its cost follows the number of runs and not the number of pixels.  All integers: both sides give the same bits.  H * W < 2^31; there
is no radius."""
from __future__ import annotations

from fractions import Fraction
from typing import Optional, Tuple, Union

import numpy as np
import torch

ENTRY_POINTS = ("ce_components_roots_i32", "ce_components_sums_i32", "ce_components_keep_u8", "ce_components_seeds_f32", "ce_components_masked_f32")
TILE = (32, 64)  # (rows, columns) of the tile a workgroup labels in the LDS (CC_TH, CC_TW of csrc/ce_components_core.h)


def check_min_weight(v, name: str = "min_weight", zero_is_off: bool = False) -> Union[int, float]:
    """Validates a least weight: an int >= 1 (zero_is_off: >= 0), or a float strictly inside (0, 1).  A bool is refused."""
    low = 0 if zero_is_off else 1
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"components: {name} must be an int >= {low} or a float in (0, 1) (a fraction of the largest component), got {v!r}")
    if isinstance(v, int):
        if v < low or v >= 1 << 31:
            raise ValueError(f"components: {name} as an int must lie in {low}..2^31 - 1, got {v}")
        return v
    if not (0.0 < v < 1.0):  # (a NaN fails the comparison)
        raise ValueError(f"components: {name} as a float must lie strictly inside (0, 1), got {v!r}")
    if fraction(v)[0] == 0 or fraction(v)[0] == fraction(v)[1]:
        raise ValueError(f"components: {name} = {v!r} is 0 or 1 as a fraction with a denominator <= 65536")
    return float(v)


def fraction(v: float) -> Tuple[int, int]:
    """A float -> (num, den) of the nearest fraction with a denominator <= 65536."""
    f = Fraction(v).limit_denominator(1 << 16)
    return f.numerator, f.denominator


def least_weight(mw, largest: int) -> int:
    """The least weight kept: mw itself, or ceil(fraction * largest) in exact integers."""
    if isinstance(mw, int):
        return mw
    num, den = fraction(mw)
    return (num * int(largest) + den - 1) // den


def _check_plane(plane: torch.Tensor, name: str, dtype=torch.uint8):
    if not isinstance(plane, torch.Tensor) or plane.dtype != dtype or plane.dim() != 2 or plane.numel() == 0:
        raise ValueError(f"components: {name} must be a non-empty {dtype} [H, W] tensor, got "
                         f"{(plane.dtype, tuple(plane.shape)) if isinstance(plane, torch.Tensor) else type(plane)}")
    if plane.numel() >= 1 << 31:
        raise ValueError(f"components: need H * W < 2^31, got {tuple(plane.shape)}")


# ---- the host form ------------------------------------------------------------------------------------------------------------------
def _runs(fg: np.ndarray):
    """fg bool [H, W] -> (row, start, end) of every row run, int64, in row-major order; end is one past the run's last column."""
    H, W = fg.shape
    edge = np.zeros((H, W + 2), dtype=np.int8)
    edge[:, 1:-1] = fg
    step = np.diff(edge, axis=1)  # [H, W + 1]: +1 in front of a run's first column, -1 behind its last
    row, start = np.nonzero(step == 1)
    end = np.nonzero(step == -1)[1]
    return row.astype(np.int64), start.astype(np.int64), end.astype(np.int64)


def _run_components(row: np.ndarray, start: np.ndarray, end: np.ndarray, W: int) -> np.ndarray:
    """The smallest run index of every run's component.  Two runs of adjacent rows are joined when [start - 1, end + 1) of one meets the
    other; hooking every root onto the smallest root it touches and flattening at least halves the joinable components per round."""
    n = row.size
    parent = np.arange(n, dtype=np.int64)
    if n == 0:
        return parent
    K = W + 2
    key_s, key_e = row * K + start, row * K + end  # both increase with the run's index
    lo = np.searchsorted(key_e, (row - 1) * K + start, side="left")   # the first run above whose end reaches start (a diagonal touch counts)
    hi = np.searchsorted(key_s, (row - 1) * K + end, side="right")    # one past the last run above that starts at or before end
    cnt = np.maximum(hi - lo, 0)
    total = int(cnt.sum())
    if total == 0:
        return parent
    b = np.repeat(np.arange(n, dtype=np.int64), cnt)
    a = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    while True:
        pa, pb = parent[a], parent[b]
        live = pa != pb
        if not live.any():
            return parent
        a, b, pa, pb = a[live], b[live], pa[live], pb[live]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:  # flatten: parent[i] <= i, so this ends with every run below its root
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp


def _roots_np(plane: np.ndarray) -> np.ndarray:
    H, W = plane.shape
    fg = plane != 0
    row, start, end = _runs(fg)
    comp = _run_components(row, start, end, W)
    label = (row * W + start)[comp]  # runs are in row-major order: the smallest run holds the smallest pixel
    out = np.full(H * W, -1, dtype=np.int32)
    out[np.flatnonzero(fg)] = np.repeat(label, end - start).astype(np.int32)
    return out.reshape(H, W)


def _sums_np(roots: np.ndarray, weight: Optional[np.ndarray]) -> np.ndarray:
    counted = roots >= 0
    if weight is not None:
        counted &= weight != 0
    return np.bincount(roots[counted].astype(np.int64), minlength=roots.size).astype(np.int32).reshape(roots.shape)


def _keep_np(plane: np.ndarray, roots: np.ndarray, sums: np.ndarray, mw) -> Tuple[np.ndarray, np.ndarray]:
    flat_r, flat_s = roots.reshape(-1), sums.reshape(-1)
    at = np.flatnonzero(flat_r == np.arange(flat_r.size, dtype=np.int64))  # the roots' own positions
    w = flat_s[at].astype(np.int64)
    largest = int(w.max()) if w.size else 0
    thr = least_weight(mw, largest)
    fg = flat_r >= 0
    keep = np.zeros(flat_r.size, dtype=bool)
    keep[fg] = flat_s[flat_r[fg]] >= thr
    out = np.where(keep.reshape(plane.shape), plane, np.uint8(0)).astype(np.uint8)
    stats = np.array([int((w >= thr).sum()), int((w < thr).sum()), int(w[w < thr].sum()), largest], dtype=np.int32)
    return out, stats


# ---- the three functions, where the bytes lie -----------------------------------------------------------------------------------------
def roots(plane: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [H, W] -> int32 [H, W]: the smallest linear index of the pixel's component, -1 for background."""
    _check_plane(plane, "plane")
    if plane.is_cuda:
        from . import ops
        return ops.components_roots_i32(plane.contiguous(), out)
    return torch.from_numpy(_roots_np(plane.contiguous().numpy()))


def sums(roots: torch.Tensor, weight: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 [H, W] roots (+ uint8 [H, W] weight) -> int32 [H, W]: at each root the number of its component's pixels with a non-zero weight
    byte (no weight: of its pixels), 0 elsewhere."""
    _check_plane(roots, "roots", torch.int32)
    if weight is not None:
        _check_plane(weight, "weight")
        if weight.shape != roots.shape or weight.device != roots.device:
            raise ValueError(f"components: weight {tuple(weight.shape)} on {weight.device} does not match roots {tuple(roots.shape)} on {roots.device}")
    if roots.is_cuda:
        from . import ops
        return ops.components_sums_i32(roots.contiguous(), None if weight is None else weight.contiguous(), out)
    return torch.from_numpy(_sums_np(roots.contiguous().numpy(), None if weight is None else weight.contiguous().numpy()))


def keep(plane: torch.Tensor, roots: torch.Tensor, sums: torch.Tensor, min_weight, out: Optional[torch.Tensor] = None,
         stats: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out uint8 [H, W], stats int32 [4]): the plane without the components below the least weight; stats = (components kept, components
    dropped, weight dropped, largest weight)."""
    mw = check_min_weight(min_weight)
    _check_plane(plane, "plane"), _check_plane(roots, "roots", torch.int32), _check_plane(sums, "sums", torch.int32)
    if not (plane.shape == roots.shape == sums.shape) or not (plane.device == roots.device == sums.device):
        raise ValueError(f"components: plane {tuple(plane.shape)}, roots {tuple(roots.shape)} and sums {tuple(sums.shape)} must share shape and device")
    if plane.is_cuda:
        from . import ops
        num, den = (0, 0) if isinstance(mw, int) else fraction(mw)
        return ops.components_keep_u8(plane.contiguous(), roots.contiguous(), sums.contiguous(), mw if isinstance(mw, int) else 0, num, den, out, stats)
    o, s = _keep_np(plane.contiguous().numpy(), roots.contiguous().numpy(), sums.contiguous().numpy(), mw)
    return torch.from_numpy(o), torch.from_numpy(s)


def scratch_bytes(H: int, W: int) -> int:
    """The scratch of one `filter` on the device: the label plane, the sums plane and the counters."""
    from . import ops
    return ops.components_scratch_bytes(H, W)


def filter(plane: torch.Tensor, min_weight, weight: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`roots`, `sums` and `keep` in a row -> (out, stats).  On the device: six launches and two memsets, no host read; scratch: uint8,
    at least `scratch_bytes(H, W)`, 4-byte aligned (made here when not given; `stats` is a view of its last 16 bytes)."""
    _check_plane(plane, "plane")
    if not plane.is_cuda:
        r = roots(plane)
        return keep(plane, r, sums(r, weight), min_weight)
    H, W = plane.shape
    need = scratch_bytes(H, W)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=plane.device)
    if scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need or scratch.data_ptr() % 4 or scratch.device != plane.device:
        raise ValueError(f"components: scratch must be a contiguous, 4-byte aligned uint8 tensor of at least {need} bytes on {plane.device}")
    n = 4 * H * W
    lab, sm, st = scratch[:n].view(torch.int32).view(H, W), scratch[n:2 * n].view(torch.int32).view(H, W), scratch[2 * n:2 * n + 16].view(torch.int32)
    roots(plane, lab), sums(lab, weight, sm)
    return keep(plane, lab, sm, min_weight, out, st)


def reference(plane: torch.Tensor, min_weight, weight: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """THE definition, and the host path: `filter` on the host."""
    return filter(plane.cpu(), min_weight, None if weight is None else weight.cpu())
