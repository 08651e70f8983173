"""TeaCache step skipping for the denoising loop (the reference's `TeaCache`, wan_video_new_chronoedit.py:1190-1239).

On a step whose timestep modulation has moved little since the last step, the block stack is not run: the residual it added on the
last computed step (tokens behind the stack minus tokens in front of it) is added to this step's patch-embedded tokens instead.

The quantity the rule watches is the time-projection output of the step - a function of the timestep and the weights alone, not of
the latents, the prompt or the guidance branch.  So the whole compute / skip plan of an edit is a function of the schedule: it is
computed here BEFORE the loop (one device-to-host read per edit, none per step), the conditional and unconditional passes share it,
and a hipGraph-replayed loop needs just a second captured graph for the skipped steps (loop.GraphedDenoiser).  `TeaCacheState` is
what one edit keeps.

Host side only: `plan_from_ratios`, the bf16 arithmetic of the ratios and the fit of the rescaling polynomial (`fit_calibration`, from the
points a measured edit yields) need no device; the device passes are csrc/ce_tea.hip."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

SHARDED = "TeaCache with {} is not implemented (the cached residual is row-local; nothing sharded has been tested with it)"


@dataclass(frozen=True)
class TeaCacheConfig:
    """rel_l1_thresh: a step is skipped while the accumulated (rescaled) relative L1 distance stays below it.  coefficients: the
    rescaling polynomial, highest power first (np.poly1d order).  The default is the identity, poly(r) = r: no polynomial ships for
    ChronoEdit; callers pass the one published for their model family, or the one `calibrate_teacache` fits on the loaded checkpoint."""
    rel_l1_thresh: float
    coefficients: Tuple[float, ...] = (1.0, 0.0)


def bf16_round(v: float) -> float:
    """v rounded to fp32, then to bf16 (round to nearest even), as a Python float: what `torch.tensor(v).bfloat16()` holds."""
    with np.errstate(over="ignore"):
        bits = int(np.asarray(v, dtype=np.float32).view(np.uint32))
    if (bits & 0x7F800000) == 0x7F800000:  # inf stays inf; a NaN keeps its sign and becomes quiet
        bits = bits & 0xFFFF0000 if not bits & 0x007FFFFF else (bits & 0xFFFF0000) | 0x00400000
    else:
        bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return float(np.asarray(bits, dtype=np.uint32).view(np.float32))


def ratios_from_sums(sums, n: int) -> List[float]:
    """The relative L1 distance of every step to the step before it, from ce_tea_rel_l1_bf16's fp32 sums [S, 2] over rows of n
    elements, in the reference's bf16 arithmetic (:1219 - both means and their quotient are bf16 tensors):
    m1 = bf16(sum|d| / n), m0 = bf16(sum|prev| / n), ratio = bf16(m1 / m0), each division in fp32.  Entry 0 is 0.0 (never looked at)."""
    sums = np.asarray(sums, dtype=np.float32).reshape(-1, 2)
    out = [0.0]
    with np.errstate(divide="ignore", invalid="ignore"):
        for s1, s0 in sums[1:]:
            m1 = np.float32(bf16_round(float(s1 / np.float32(n))))
            m0 = np.float32(bf16_round(float(s0 / np.float32(n))))
            out.append(bf16_round(float(m1 / m0)))
    return out


def plan_from_ratios(ratios: Sequence[float], num_steps: int, rel_l1_thresh: float, coefficients: Sequence[float],
                     forced: Iterable[int] = ()) -> List[bool]:
    """The compute (True) / skip (False) decision of every step of an edit.

    ratios[i] compares step i with step i - 1 whether or not step i - 1 was computed.  The first and the last step compute.  On every
    other step the rescaled ratio - polyval(coefficients, ratios[i]) in float64, highest power first - is added to an accumulator; the
    step is skipped while the accumulator is below rel_l1_thresh, otherwise it computes.  Every computed step zeroes the accumulator.
    Steps in `forced` compute whatever the accumulator says (a step whose token count differs from the cached residual's)."""
    forced = {int(f) for f in forced}
    coef = np.asarray(coefficients, dtype=np.float64)
    plan, acc = [], 0.0
    for i in range(num_steps):
        compute = i == 0 or i == num_steps - 1 or i in forced
        if not compute:
            with np.errstate(all="ignore"):  # (a NaN or infinite ratio: the comparison below then fails and the step computes)
                acc += float(np.polyval(coef, np.float64(ratios[i])))
            compute = not acc < rel_l1_thresh
        if compute:
            acc = 0.0
        plan.append(compute)
    return plan


def report(plan: Sequence[bool], ratios: Sequence[float]) -> dict:
    """What `denoise` leaves on `transformer.teacache_report` after an edit."""
    plan = [bool(c) for c in plan]
    return {"plan": plan, "computed": sum(plan), "skipped": len(plan) - sum(plan), "ratios": [float(r) for r in ratios]}


# ---- calibration: the rescaling polynomial fitted on the loaded checkpoint ---------------------------------------------------------
# The polynomial maps what the rule watches (ratios: the relative L1 change of the time projection, a function of the schedule) to what
# a skipped step gets wrong (distances: the relative L1 change of the block stack's residual, which a skipped step reuses unchanged).
# A measured edit (loop.denoise(teacache_measure=True)) yields one (ratio, distance) point per step; the fit is least squares.
@dataclass(frozen=True)
class TeaCacheCalibration:
    """coefficients: highest power first, what `enable_teacache(thresh, coefficients)` and TeaCacheConfig take.  degree: the degree
    fitted (lower than asked for when the points hold too few distinct ratios).  points: the (ratio, distance) pairs used.
    max_residual / rms_residual: the largest and the root-mean-square |polyval(coefficients, ratio) - distance| over the points."""
    coefficients: Tuple[float, ...]
    degree: int
    points: Tuple[Tuple[float, float], ...]
    max_residual: float
    rms_residual: float


def _is_edit_list(v) -> bool:
    return len(v) > 0 and not np.isscalar(v[0]) and np.ndim(v[0]) >= 1


def fit_calibration(ratios, distances, degree: int = 4) -> TeaCacheCalibration:
    """ratios / distances: the per-step lists of ONE measured edit, or a list of such lists (several edits, pooled).  Entry 0 of every edit
    (no step before it) and every point with a non-finite member (a step whose residual had no predecessor: the first one after the
    temporal-reasoning truncation) are dropped.  np.polyfit in float64; with fewer than degree + 1 distinct ratios the degree drops to
    distinct - 1.  Fewer than 2 usable points: ValueError."""
    if int(degree) < 0:
        raise ValueError(f"fit_coefficients: degree {degree} is negative")
    if not _is_edit_list(ratios):
        ratios, distances = [ratios], [distances]
    if len(ratios) != len(distances):
        raise ValueError(f"fit_coefficients: {len(ratios)} ratio lists for {len(distances)} distance lists")
    xs, ys = [], []
    for r, d in zip(ratios, distances):
        r, d = np.asarray(r, dtype=np.float64).reshape(-1), np.asarray(d, dtype=np.float64).reshape(-1)
        if r.shape != d.shape:
            raise ValueError(f"fit_coefficients: {r.size} ratios for {d.size} distances in one edit")
        keep = np.isfinite(r) & np.isfinite(d)
        keep[:1] = False
        xs.append(r[keep])
        ys.append(d[keep])
    x, y = np.concatenate(xs), np.concatenate(ys)
    if x.size < 2:
        raise ValueError(f"fit_coefficients: {x.size} usable (ratio, distance) points, at least 2 are needed")
    deg = max(min(int(degree), np.unique(x).size - 1), 0)
    coef = np.polyfit(x, y, deg)
    res = np.abs(np.polyval(coef, x) - y)
    return TeaCacheCalibration(tuple(float(c) for c in coef), deg, tuple((float(a), float(b)) for a, b in zip(x, y)),
                               float(res.max()), float(np.sqrt(np.mean(res * res))))


def fit_coefficients(ratios, distances, degree: int = 4) -> Tuple[float, ...]:
    """The coefficients of fit_calibration alone: highest power first, the order plan_from_ratios and TeaCacheConfig use."""
    return fit_calibration(ratios, distances, degree).coefficients


def distances_from_sums(sums) -> List[float]:
    """ce_tea_store_dist_bf16's fp32 sums [steps, 2] -> sum|r_i - r_{i-1}| / sum|r_{i-1}| per step in float64; NaN where nothing was
    measured (the table starts as NaN) or the previous residual was all zeros."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = sums[:, 0] / sums[:, 1]
    return [float(v) if np.isfinite(v) else float("nan") for v in d]


class TeaCacheState:
    """TeaCache in one running edit (`loop.denoise(teacache=, teacache_measure=)`).
    config: a TeaCacheConfig for this call; None = whatever `transformer.enable_teacache()` set (nothing: no step is skipped).  The compute /
    skip plan of the whole edit is made in `begin`, before the first step (`forced`, the truncation step, always computes: the 8-frame
    residual does not fit 2-frame tokens); `transformer.teacache_report` then holds {"plan", "computed", "skipped", "ratios"}, and the
    engine has dropped the previous edit's residual.
    measure (`teacache_measure`, or `transformer.calibrate_teacache` around the call): calibration instead of skipping - `plan` is None.
    Every step computes - the latents are the plain loop's - and the pass that stores the block stack's residual also measures its relative
    L1 distance to the previous step's residual, on the device, into a table read back once after the last step (`finish`): afterwards
    `transformer.teacache_measurement` holds {"ratios": teacache_ratios(timesteps), "distances": per step, NaN for step 0 and for the first
    step after the truncation} - the points fit_calibration fits.  A measured edit always runs eagerly (the table row changes per step,
    and calibration is offline).  Together with a skip plan it is a ValueError (raised by the loop, in front of every feature's setup)."""

    def __init__(self, transformer, plan: Optional[List[bool]], ratios: Sequence[float]):
        self.transformer, self.plan, self.ratios = transformer, plan, ratios

    @classmethod
    def begin(cls, transformer, timesteps, config: Optional[TeaCacheConfig], measure: bool, forced: Iterable[int] = ()) -> Optional["TeaCacheState"]:
        """None when the edit neither skips nor measures.  With sharded tokens or CFG parallelism a NotImplementedError."""
        if config is None and not measure:
            return None
        from .loop import refuse_sharded
        refuse_sharded(transformer, SHARDED)
        ratios = transformer.teacache_ratios(timesteps)  # the one device-to-host read of the edit
        if config is None:
            transformer.engine().tea_measure_begin(len(timesteps))
            return cls(transformer, None, ratios)
        plan = plan_from_ratios(ratios, len(timesteps), config.rel_l1_thresh, config.coefficients, forced)
        transformer.teacache_report = report(plan, ratios)
        transformer.engine().tea_drop()  # nothing of the previous edit's residual may be reused
        return cls(transformer, plan, ratios)

    def finish(self):
        """Measuring: the one read of the table, after the last step."""
        if self.plan is None:
            sums = self.transformer.engine().tea_measure_end()
            self.transformer.teacache_measurement = {"ratios": [float(r) for r in self.ratios], "distances": distances_from_sums(sums.numpy())}
