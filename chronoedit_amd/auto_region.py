"""Automatic edit regions: an instruction-only edit finds its own region after a few dense steps and continues as a region-limited edit.

`ChronoEditPipeline.__call__` takes an image and an instruction, no mask.  After step k = `detect_step` the scheduler's predict-x0 history
slot already shows where the edit is (the detection half of RegionE): compare it with the source latents, threshold the difference, and
go on as chronoedit_amd/region.py would with a caller-given mask - blend, sparse steps (chronoedit_amd/sparse_region.py), paste-back.

    d      fp32 [h, w]    on the LAST latent frame: max over samples of ((sum over channels, in order, of (x0 - z_src)^2) / C)
    thr    one float      a number t (RMS units of the normalised latents): fp32(t) * fp32(t); "otsu": Otsu's threshold of a 256-bin
                          histogram of d over [0, dmax], at least floor^2 - on the device, nothing is read back for it
    w      fp32 [h, w]    seed = d > thr, dilated by `dilate` cells (Chebyshev) at weight 1, then a linear ramp over `feather` cells to 0.
                          With `min_area` the seed set first loses its speckle (chronoedit_amd/components.py): its 8-connected components
                          of fewer cells than min_area (an int), or than that fraction of the largest one (a float), are taken out:
                          d' = where(kept, d, -1), w = the ramp of d'.  d is a mean of squares and no threshold is below 0, so a cell at
                          -1 is no seed and the ramp pass itself is untouched
    mask   uint8 [8h, 8w] rint(255 * w) of the pixel's cell: the mask of the paste-back, and what `set_edit_region` takes back

Then ONE device-to-host read (w, thr, dmax) and the decision: no active cell, or more active patches than `max_area` of the grid, and the
edit stays the plain loop to its end - a global edit has no region to speak of.

Host side only; the device passes are csrc/ce_region_auto.hip.  Every pass below is ALSO a torch expression for tensors on the CPU, with
the same bits (the tests compare them with torch.equal), as region.latent_weights is."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

MAX_RADIUS = 8  # dilate + feather: the window of the ramp pass


@dataclass(frozen=True)
class AutoRegionConfig:
    """detect_step: the step behind whose scheduler update the region is looked for (with temporal reasoning: the first step at or behind
    it that runs at the truncated shape; past the last step: nothing is detected).  threshold: "otsu", or a number in RMS units of the
    normalised latents.  floor: the least RMS change Otsu's threshold may call an edit.  dilate / feather: cells of weight 1 around the
    seed, and cells of the ramp to 0 behind them.  max_area: the largest fraction of the patch grid an accepted region may cover.
    composite: paste the source back in pixel space behind the decode.  min_area: 0 is off; an int >= 1 is the least number of cells a
    component of the seed set must hold, a float in (0, 1) that fraction of the largest component's."""
    detect_step: int
    threshold: Union[str, float] = "otsu"
    floor: float = 0.0
    dilate: int = 1
    feather: int = 1
    max_area: float = 0.5
    composite: bool = True
    min_area: Union[int, float] = 0

    def __post_init__(self):
        ds = self.detect_step
        if isinstance(ds, bool) or not isinstance(ds, int) or ds < 0:
            raise ValueError(f"auto region: detect_step must be an integer >= 0, got {ds!r}")
        th = self.threshold
        if isinstance(th, str):
            if th != "otsu":
                raise ValueError(f"auto region: threshold must be 'otsu' or a number, got {th!r}")
        elif isinstance(th, bool) or not isinstance(th, (int, float)) or not (math.isfinite(th) and th >= 0):
            raise ValueError(f"auto region: threshold must be 'otsu' or a finite number >= 0, got {th!r}")
        fl = self.floor
        if isinstance(fl, bool) or not isinstance(fl, (int, float)) or not (math.isfinite(fl) and fl >= 0):
            raise ValueError(f"auto region: floor must be a finite number >= 0, got {fl!r}")
        for name in ("dilate", "feather"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"auto region: {name} must be an integer >= 0, got {v!r}")
        if self.dilate + self.feather > MAX_RADIUS:
            raise ValueError(f"auto region: dilate + feather must not exceed {MAX_RADIUS}, got {self.dilate} + {self.feather}")
        ma = self.max_area
        if isinstance(ma, bool) or not isinstance(ma, (int, float)) or not 0.0 < ma <= 1.0:  # (a NaN fails the comparison)
            raise ValueError(f"auto region: max_area must lie in (0, 1], got {ma!r}")
        from .components import check_min_weight
        object.__setattr__(self, "min_area", check_min_weight(self.min_area, "auto region: min_area", zero_is_off=True))
        # (a dropped seed is marked by d' = -1: that is below every threshold, because none is negative - a number and the floor are checked
        # above, and Otsu's is a bin edge of [0, dmax] or the floor's square)
        assert isinstance(th, str) or th >= 0


class AutoRegion:
    """What `loop.denoise(auto_region=)` takes for ONE edit: the config (None: the transformer's switch decides) and z_src = fp32 source latents of the latents' shape
    (region.static_source_latents).  measure: run the plain loop and record every step's change map instead of detecting
    (`measure_auto_region`).  The loop leaves `report` (see `report`) and `mask_u8` (the device mask of an accepted region, else None)
    here.  on_accept: a callable (the device mask of an accepted region) -> bool; True ends the loop behind the detecting step, with
    `exited` set (the scout of an auto-focused edit, chronoedit_amd/autofocus.py)."""

    def __init__(self, config: Optional[AutoRegionConfig], z_src: torch.Tensor, measure: bool = False, on_accept=None):
        self.config, self.z_src, self.measure = config, z_src, bool(measure)
        self.report: Optional[dict] = None
        self.mask_u8: Optional[torch.Tensor] = None
        self.on_accept = on_accept
        self.exited = False


class AutoRegionState:
    """The automatic region of one running edit (`loop.denoise(auto_region=)`: an AutoRegion - the config, None: whatever
    `transformer.enable_auto_region()` set - and z_src = fp32 static-source latents of the latents' shape).  An explicit `region=` wins: the
    detector is not run and the report is None.
    Detecting: the state keeps a clone of the latents the loop starts from (the blend's eps); steps 0 .. k run as the plain loop (k =
    detect_step, or with temporal reasoning the first step at or behind it that runs at the truncated shape; past the last step nothing
    is detected).  After step k's scheduler update, before `on_step_end`, four device passes (csrc/ce_region_auto.hip) turn x0 =
    scheduler.model_outputs[-1] and z_src into the weights w and the pixel mask, and ONE read brings w to the host (`after_step`).
    Declined (no active cell, or more active patches than max_area of the grid - with the sparse margin when a sparse region is enabled):
    the edit stays the plain loop, bit for bit.  Accepted: a RegionState is built from (w, z_src, eps, sigma_next), the blend runs after
    step k itself and after every later step, the loop rebuilds its graphed form (a region is another warm shape), and with a sparse
    region config makes the plan now, every step <= k forced dense, so that step k + 1 is the first refresh.  Composition and refusals
    are those of an explicit region.  Afterwards `transformer.auto_region_report` and `auto_region.report` hold {"step", "threshold",
    "dmax", "active_fraction", "accepted", "reason", "w", "mask"} and `auto_region.mask_u8` the device mask of an accepted region.
    auto_region.measure: every step runs the plain loop and writes its change map into a [steps, h, w] device table, read back once after
    the last step (`finish`): `transformer.auto_region_measurement` then holds one row per step (`measurement`).
    auto_region.on_accept: a callable (the device pixel mask of an accepted region) -> bool, asked before anything of the region is set
    up; True ends the loop behind step k (its `on_step_end` still runs) with `auto_region.exited` and this state's `exiting` set - the
    scout of an auto-focused edit (chronoedit_amd/autofocus.py); False, or none: as above."""

    def __init__(self, transformer, auto: AutoRegion, config: AutoRegionConfig, latents: torch.Tensor, n_steps: int, k: Optional[int]):
        self.transformer, self.auto, self.config, self.k = transformer, auto, config, k  # k: the step the detection follows
        self.detecting, self.exiting = not auto.measure, False
        self.z = auto.z_src.to(device=latents.device, dtype=torch.float32).contiguous()
        self.eps = latents.clone() if self.detecting else None  # the blend's eps, should a region be found
        self.table = None if self.detecting else torch.zeros((n_steps,) + tuple(latents.shape[-2:]), dtype=torch.float32, device=latents.device)

    @classmethod
    def begin(cls, transformer, auto_region: Optional[AutoRegion], region, latents: torch.Tensor, n_steps: int,
              enable_temporal_reasoning: bool = False, num_temporal_reasoning_steps: int = 0) -> Optional["AutoRegionState"]:
        """Resets the reports; None when nothing is to be detected or measured (no AutoRegion, an explicit region, or no config anywhere).
        With sharded tokens or CFG parallelism a NotImplementedError, then a z_src of another shape than the latents a ValueError."""
        auto = auto_region if region is None else None  # an explicit mask wins
        cfg = None
        if auto is not None:  # (no config of its own: whatever `transformer.enable_auto_region()` set - nothing: the plain loop)
            cfg = auto.config if auto.config is not None else getattr(transformer, "_auto_region", None)
        if hasattr(transformer, "auto_region_report"):
            transformer.auto_region_report = None
        if auto_region is not None:
            auto_region.report = auto_region.mask_u8 = None
        if cfg is None:
            return None
        from .loop import refuse_sharded
        from .region import SHARDED
        refuse_sharded(transformer, SHARDED)
        if tuple(auto.z_src.shape) != tuple(latents.shape):
            raise ValueError(f"auto region: z_src {tuple(auto.z_src.shape)} does not have the latents' shape {tuple(latents.shape)}")
        k = None if auto.measure else detect_index(cfg, n_steps, enable_temporal_reasoning, num_temporal_reasoning_steps)
        return cls(transformer, auto, cfg, latents, n_steps, k)

    def truncated(self, latents: torch.Tensor):
        """The temporal-reasoning truncation: z_src and eps are sliced exactly as the latents are."""
        if self.z is not None and self.z.shape[-3] != latents.shape[-3]:
            self.z = self.z[:, :, [0, -1]].contiguous()
            self.eps = None if self.eps is None else self.eps[:, :, [0, -1]].contiguous()

    def after_step(self, i: int, scheduler, latents: torch.Tensor, margin: int = 0):
        """Measuring: this step's change map into its row of the table.  Detecting, behind step k: the four passes on the estimate of the
        final image the step kernel just wrote, one read, the decision.  -> (the RegionState of an accepted region, already blended into
        step k's latents; w on the CPU), else None."""
        if self.table is not None:
            from . import ops
            ops.auto_region_change(scheduler.model_outputs[-1], self.z, -1, out=self.table[i])
            return None
        if i != self.k or self.z is None:
            return None
        from . import region as _rg
        auto, found = self.auto, None
        w, mask, w_cpu, thr, dmax, *counters = detect(scheduler.model_outputs[-1], self.z, self.config)
        ok, why, frac = decide(w_cpu, self.config, margin)
        auto.report = self.transformer.auto_region_report = report(i, thr, dmax, frac, ok, why, w_cpu)
        if counters:  # (min_area is on)
            auto.report.update(min_area=self.config.min_area, components=counters[0][0], dropped_components=counters[0][1], dropped_cells=counters[0][2])
        if ok and auto.on_accept is not None and auto.on_accept(mask):
            auto.mask_u8, auto.exited, self.exiting = mask, True, True  # the caller goes on from here (the history is as step k left it)
        elif ok:
            state = _rg.RegionState(w, self.z, self.eps, _rg.sigma_next_table(scheduler, latents.device),
                                    bf16_state=scheduler.trajectory_dtype == torch.bfloat16)
            auto.mask_u8 = mask
            state.blend(latents, i)  # the blend after step k itself
            found = (state, w_cpu)
        self.z = self.eps = None
        return found

    def finish(self, timesteps: torch.Tensor):
        """Measuring: the one read of the table, after the last step."""
        if self.table is not None:
            self.transformer.auto_region_measurement = {"timesteps": [int(v) for v in timesteps.tolist()],
                                                        "steps": measurement(self.table.cpu(), self.config)}


def detect_index(cfg: AutoRegionConfig, n_steps: int, enable_temporal_reasoning: bool = False, num_temporal_reasoning_steps: int = 0) -> Optional[int]:
    """The step k the detection follows, or None when it lies past the last step."""
    k = int(cfg.detect_step)
    if enable_temporal_reasoning and 0 <= int(num_temporal_reasoning_steps) < n_steps:
        k = max(k, int(num_temporal_reasoning_steps))  # the truncation happens in front of that step: it is the first 2-frame step
    return k if k < n_steps else None


# ---------------------------------------------------------------------------------------------------------------------------------------
# the passes: the device kernel for a tensor on the GPU, the torch expression for one on the CPU - the same bits
# ---------------------------------------------------------------------------------------------------------------------------------------
def change_map(x0: torch.Tensor, z_src: torch.Tensor, frame: int = -1) -> torch.Tensor:
    """x0, z_src fp32 [B, C, T, h, w] -> d fp32 [h, w] on one latent frame."""
    if x0.is_cuda:
        from . import ops
        return ops.auto_region_change(x0.contiguous(), z_src.contiguous(), frame)
    df = x0[:, :, frame].to(torch.float32) - z_src[:, :, frame].to(torch.float32)
    sq = df * df
    acc = sq[:, 0]
    for c in range(1, sq.shape[1]):  # in channel order: one rounded add each
        acc = acc + sq[:, c]
    return torch.amax(acc / torch.tensor(float(sq.shape[1]), dtype=torch.float32), dim=0)  # (amax keeps a NaN, as the kernel does)


def number_threshold(t: float) -> torch.Tensor:
    """A threshold given as a number, in RMS units -> the fp32 value d is compared with."""
    v = torch.tensor(float(t), dtype=torch.float32)
    return (v * v).reshape(1)


def otsu_bins(d: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """d -> (int64 bin per cell, dmax); the CPU expression of the histogram's input."""
    d = d.detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    ok = d[~torch.isnan(d)]
    dmax = torch.clamp(ok.max(), min=0.0) if ok.numel() else torch.zeros((), dtype=torch.float32)
    scale = torch.tensor(256.0, dtype=torch.float32) / dmax
    v = d * scale
    b = torch.where(v >= 0, torch.clamp(v, max=255.0), torch.zeros_like(v))  # a NaN (of d, or of inf * 0) goes to bin 0
    return b.to(torch.int64), dmax


def otsu_threshold(d: torch.Tensor, floor: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """d fp32 (>= 0 or NaN) -> (thr, dmax), one fp32 element each."""
    if d.is_cuda:
        from . import ops
        return ops.auto_region_otsu(d.contiguous(), floor)
    bins, dmax = otsu_bins(d)
    if not bool(dmax > 0):
        return torch.full((1,), float("inf"), dtype=torch.float32), dmax.reshape(1)
    N = bins.numel()
    hist = torch.bincount(bins, minlength=256)
    idx = torch.arange(256, dtype=torch.int64)
    w0, s0 = torch.cumsum(hist, 0), torch.cumsum(idx * hist, 0)
    S = s0[-1]
    valid = (w0 > 0) & (w0 < N)
    t = 0
    if bool(valid.any()):
        num = (s0 * N - S * w0).to(torch.float64)
        den = (w0 * (N - w0)).to(torch.float64)
        score = torch.where(valid, num * num / torch.where(valid, den, torch.ones_like(den)), torch.full_like(den, -1.0))
        t = int(torch.nonzero(score == score.max())[0])  # the lowest of equal maxima
    fl = torch.tensor(float(floor), dtype=torch.float32)
    thr = torch.tensor(float(t + 1), dtype=torch.float32) * (dmax / torch.tensor(256.0, dtype=torch.float32))
    return torch.maximum(thr, fl * fl).reshape(1), dmax.reshape(1)


def ramp_value(r: int, dilate: int, feather: int) -> torch.Tensor:
    if r <= dilate:
        return torch.ones((), dtype=torch.float32)
    return torch.tensor(float(feather + 1 - (r - dilate)), dtype=torch.float32) / torch.tensor(float(feather + 1), dtype=torch.float32)


def ramp_weights(d: torch.Tensor, thr: torch.Tensor, dilate: int = 1, feather: int = 1) -> torch.Tensor:
    """d fp32 [h, w], thr one float -> w fp32 [h, w]."""
    if dilate < 0 or feather < 0 or dilate + feather > MAX_RADIUS:
        raise ValueError(f"auto region: dilate + feather must lie in 0..{MAX_RADIUS}, got {dilate} + {feather}")
    if d.is_cuda:
        from . import ops
        return ops.auto_region_ramp(d.contiguous(), thr.to(d.device).reshape(1).contiguous(), dilate, feather)
    seed = (d.to(torch.float32) > thr.reshape(()).to(torch.float32)).to(torch.float32)[None, None]
    w = torch.zeros(d.shape, dtype=torch.float32)
    for r in range(dilate + feather, -1, -1):  # from the rim inwards: a nearer seed overwrites with the larger value
        reach = torch.nn.functional.max_pool2d(seed, 2 * r + 1, stride=1, padding=r)[0, 0] > 0
        w = torch.where(reach, ramp_value(r, dilate, feather), w)
    return w


def seed_plane(d: torch.Tensor, thr: torch.Tensor) -> torch.Tensor:
    """d fp32 [h, w], thr one float -> uint8 [h, w]: 255 where d > thr (a seed), else 0."""
    if d.is_cuda:
        from . import ops
        return ops.components_seeds(d.contiguous(), thr.to(d.device).reshape(1).contiguous())
    return (d.to(torch.float32) > thr.reshape(()).to(torch.float32)).to(torch.uint8) * 255


def masked_map(d: torch.Tensor, kept: torch.Tensor) -> torch.Tensor:
    """d' = where(kept, d, -1): the change map without the seeds that were dropped."""
    if d.is_cuda:
        from . import ops
        return ops.components_masked(d.contiguous(), kept.contiguous())
    return torch.where(kept != 0, d.to(torch.float32), torch.tensor(-1.0, dtype=torch.float32))


def kept_map(d: torch.Tensor, thr: torch.Tensor, min_area) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (d', stats): the seed set d > thr without its components below `min_area` (components.filter, weight = cells), as the change map
    the ramp pass takes, and int32 [4] = (components kept, components dropped, cells dropped, the largest component's cells) where d lies."""
    from . import components
    kept, stats = components.filter(seed_plane(d, thr), min_area)
    return masked_map(d, kept), stats


def pixel_mask(w: torch.Tensor) -> torch.Tensor:
    """w fp32 [h, w] -> uint8 [8h, 8w]."""
    if w.is_cuda:
        from . import ops
        return ops.auto_region_mask_u8(w.contiguous())
    b = torch.round(torch.tensor(255.0, dtype=torch.float32) * w.to(torch.float32)).clamp(0, 255).to(torch.uint8)
    return b.repeat_interleave(8, 0).repeat_interleave(8, 1).contiguous()


def weights(x0: torch.Tensor, z_src: torch.Tensor, cfg: AutoRegionConfig):
    """All passes on whatever device x0 lives on -> (d, thr, dmax, w): what a second implementation needs."""
    d = change_map(x0, z_src)
    thr, dmax = otsu_threshold(d, cfg.floor)
    if cfg.threshold != "otsu":
        thr = number_threshold(cfg.threshold).to(d.device)
    if cfg.min_area:
        return d, thr, dmax, ramp_weights(kept_map(d, thr, cfg.min_area)[0], thr, cfg.dilate, cfg.feather)
    return d, thr, dmax, ramp_weights(d, thr, cfg.dilate, cfg.feather)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the detection of one edit, the decision and the report
# ---------------------------------------------------------------------------------------------------------------------------------------
def detect(x0: torch.Tensor, z_src: torch.Tensor, cfg: AutoRegionConfig):
    """The four device passes and the ONE read behind them -> (w on the device, mask_u8 on the device, w on the CPU, thr, dmax).  w, thr and
    dmax share one buffer, so one copy brings all three.  With cfg.min_area the speckle filter runs in front of the ramp pass, its four
    counters ride in the same buffer (their int32 bits in four more fp32 slots) and a sixth element, a tuple of the four, is returned."""
    from . import ops
    h, wl = x0.shape[-2:]
    d = ops.auto_region_change(x0, z_src, -1)
    extra = 4 if cfg.min_area else 0
    buf = torch.empty(h * wl + 2 + extra, dtype=torch.float32, device=x0.device)
    w, thr, dmax = buf[:h * wl].view(h, wl), buf[h * wl:h * wl + 1], buf[h * wl + 1:h * wl + 2]
    ops.auto_region_otsu(d, cfg.floor, thr, dmax)  # (with a number for a threshold: for dmax, which the report carries)
    if cfg.threshold != "otsu":
        thr.copy_(number_threshold(cfg.threshold), non_blocking=True)  # staged from the host
    if extra:
        d, stats = kept_map(d, thr, cfg.min_area)
        buf[h * wl + 2:].view(torch.int32).copy_(stats)
    ops.auto_region_ramp(d, thr, cfg.dilate, cfg.feather, out=w)
    mask = ops.auto_region_mask_u8(w)
    host = buf.cpu()  # the one device-to-host read: what sparse_region.active_tokens reads anyway
    out = (w, mask, host[:h * wl].view(h, wl).clone(), float(host[h * wl]), float(host[h * wl + 1]))
    return out + (tuple(host[h * wl + 2:].view(torch.int32).tolist()),) if extra else out


def decide(w_cpu: torch.Tensor, cfg: AutoRegionConfig, margin: int = 0) -> Tuple[bool, str, float]:
    """-> (accepted, reason, active_fraction).  active_fraction = the active patches (sparse_region.active_tokens: any of the 2 x 2 cells has
    w > 0, dilated by `margin` patches) over the patch grid.  Declined: "empty" (no active cell) or "max_area"."""
    from .sparse_region import active_tokens
    _, n_active = active_tokens(w_cpu, 1, margin)
    frac = n_active / float((w_cpu.shape[0] // 2) * (w_cpu.shape[1] // 2))
    if n_active == 0:
        return False, "empty", 0.0
    if frac > cfg.max_area:
        return False, "max_area", frac
    return True, "accepted", frac


def report(step: Optional[int], thr: float, dmax: float, frac: float, accepted: bool, reason: str, w_cpu: Optional[torch.Tensor]) -> dict:
    """What the loop leaves on `transformer.auto_region_report`.  mask: a PIL "L" image of the pixel mask - a front end can show it, let the
    user repaint it and hand it back through `set_edit_region`."""
    mask = None
    if w_cpu is not None:
        from PIL import Image
        mask = Image.fromarray(pixel_mask(w_cpu).numpy(), mode="L")
    return {"step": step, "threshold": thr, "dmax": dmax, "active_fraction": frac, "accepted": bool(accepted), "reason": reason,
            "w": w_cpu, "mask": mask}


def measurement(table: torch.Tensor, cfg: AutoRegionConfig) -> list:
    """table = fp32 [steps, h, w] change maps on the CPU -> per step {"step", "threshold", "active_fraction", "iou", "components",
    "largest_fraction"}: the threshold of that step's map, the fraction of cells above it, the IoU of that seed set with the last step's
    (1 for two empty sets), the number of 8-connected components of the seed set and the largest one's share of the seeds (0 without
    seeds) - what `min_area` is chosen from."""
    from . import components
    seeds, rows = [], []
    for i in range(table.shape[0]):
        d = table[i]
        thr = otsu_threshold(d, cfg.floor)[0] if cfg.threshold == "otsu" else number_threshold(cfg.threshold)
        seeds.append(d > thr.reshape(()))
        stats = components.filter(seeds[-1].to(torch.uint8), 1)[1].tolist()
        n_seeds = int(seeds[-1].sum())
        rows.append({"step": i, "threshold": float(thr), "active_fraction": float(seeds[-1].float().mean()), "components": stats[0],
                     "largest_fraction": stats[3] / n_seeds if n_seeds else 0.0})
    last = seeds[-1]
    for row, s in zip(rows, seeds):
        union = int((s | last).sum())
        row["iou"] = 1.0 if union == 0 else int((s & last).sum()) / union
    return rows
