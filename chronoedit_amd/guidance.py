"""Guidance reuse for the denoising loop: run the unconditional sample of the guidance pair only on planned steps.

Between neighbouring steps the guidance direction d = c - u (conditional minus unconditional prediction) moves far more slowly than c
itself (FasterCache's "CFG cache"), and guidance applied only inside an interval of the schedule costs less and often looks better
(Kynkaanniemi et al., 2024).  Every step of an edit is therefore one of

    "pair"    both samples run, as in the plain loop; the step also stores d = bf16(c - u)
    "reuse"   the conditional sample runs alone; the combine uses the stored d:  u' = bf16(c - d), v = bf16(u' + bf16(g * d))
    "off"     the conditional sample runs alone, no guidance (the launch of an unguided edit)

Like TeaCache's, the plan is a function of the schedule alone: it is made before the first step and nothing is read back per step, so a
hipGraph-replayed loop needs one captured graph per kind of step (pipeline.GraphedDenoiser).

Host side only; the device pass is ce_cfg_unipc_step_delta (csrc/ce_sched.hip)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, List, Sequence, Tuple

import numpy as np

KINDS = ("pair", "reuse", "off")


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
