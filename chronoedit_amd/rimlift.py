"""Mask-aware detail lift: the fit of a focused crop's lift under the region's weights.

A region edit blends its latents with the source, so the frames E of a focused crop carry a TAPERED change, roughly d = w d* with d* the
edit's change and w = m / 255 the region's weight.  `lift.fit_reference` regresses d on the source with one affine map per window: along a
feathered rim that model is wrong, the residual rises, the gate hands the rim to the Lanczos upsample, and the paste tapers the result a
second time with the photo-size mask.  Under `enable_detail_lift(focus=True, mask_aware=True)` the fit knows the weights: per window it
solves the least squares problem

    255 d  ~  a (m I) + b m                          (that is d ~ w (a I + b))

for the UNTAPERED map (a, b), smooths the maps with the weights, and measures the residual of the tapered model.  The gate and the apply
stage are lift.py's, unchanged: q = p + (abar p + bbar) is then the edit at full strength, and the paste's photo-size mask tapers it once,
at the photo's resolution.  Where the frames' real taper disagrees with m the tapered model misfits, the residual rises and the gate falls
back to the upsample, as it does without the switch.

I, d, r, eps_q and max_gain are those of lift.py; m is the edit-size weight plane uint8 [H, W] - `mask.crop(box).resize((width, height),
BILINEAR)`, what `focus.inputs` hands the region edit -, shared by the frames and the colours; box() is `lift.box_sum`.

`fit_reference` / `smooth_reference` (CPU torch, one torch op per rounded operation) are the definition and the host path; the device passes
(csrc/ce_rimlift.hip) are bit-equal to them.  The statistics are exact integers, so no summation order can change a bit."""
from __future__ import annotations

from typing import Optional

import torch

from . import lift as _lf

ENTRY_POINTS = ("ce_rimlift_fit_q16", "ce_rimlift_smooth_f32")

MAX_B = 4096.0  # the bound of |b|: rint(65536 b) stays in int32 (a weight of 1 under a change of 255 would ask for b = 65025)


def _weights(M: torch.Tensor, L: torch.Tensor) -> torch.Tensor:
    """m int64 [H, W]."""
    if M.dtype != torch.uint8 or M.dim() != 2 or tuple(M.shape) != tuple(L.shape[:2]):
        raise ValueError(f"rimlift: need M uint8 {tuple(L.shape[:2])}, got {M.dtype} {tuple(M.shape)}")
    return M.to(torch.int64)


def fit_reference(L: torch.Tensor, E: torch.Tensor, M: torch.Tensor, cfg: _lf.LiftConfig) -> torch.Tensor:
    """Stage 1 -> int32 [F, H, W, 6]: A_rgb, B_rgb = rint(65536 a), rint(65536 b), the normal equations of 255 d ~ a (m I) + b m.
    Every sum is an exact integer below 2^53 (T_qII <= 1089 * 255^4 < 2^43), so its conversion to double is exact; the products are rounded
    doubles.  With I <= 255, T_qI^2 <= T_q T_qII <= 65025 T_q^2 (Cauchy-Schwarz): the exact T_q T_qII - T_qI^2 is non-negative and the rounding
    error of its two products is below 2^-36 T_q^2, while the eps term is at least T_q^2 - more than 2^30 times as much - so den > 0
    exactly when T_q > 0."""
    I, d = _lf._planes(L, E)
    m = _weights(M, L)
    r = cfg.radius
    q = m * m
    T_q, T_qI, T_qII = _lf.box_sum(q, r).double(), _lf.box_sum(q * I, r).double(), _lf.box_sum(q * I * I, r).double()
    T_md, T_mId = _lf.box_sum(m * d, r).double(), _lf.box_sum(m * I * d, r).double()
    on = T_q > 0
    num = T_q * T_mId - T_qI * T_md
    den = (T_q * T_qII - T_qI * T_qI) + (T_q * float(cfg.eps_q)) * T_q
    one = torch.ones_like(T_q)
    a = ((num * 255.0) / torch.where(on, den, one)).clamp(-cfg.max_gain, cfg.max_gain).float()
    u = T_md * 255.0 - a.double() * T_qI
    b = (u / torch.where(on, T_q, one)).clamp(-MAX_B, MAX_B).float()
    zero = torch.zeros((), dtype=torch.float32)
    a, b = torch.where(on, a, zero), torch.where(on, b, zero)
    A, B = torch.round(a * 65536.0).to(torch.int32), torch.round(b * 65536.0).to(torch.int32)
    return torch.cat([A, B], dim=1).permute(0, 2, 3, 1).contiguous()


def smooth_reference(L: torch.Tensor, E: torch.Tensor, AB: torch.Tensor, M: torch.Tensor, cfg: _lf.LiftConfig):
    """Stage 2 -> (the cells fp32 [F, H, W, 8] with the weighted means abar_rgb, bbar_rgb and zeros in slots 6, 7; R int32 [F, H, W], the
    residual of the TAPERED model) - `lift.smooth_reference`'s layout."""
    I, d = _lf._planes(L, E)
    m = _weights(M, L)
    r = cfg.radius
    n_m = _lf.box_sum(m, r)
    s = _lf.box_sum(m * AB.permute(0, 3, 1, 2).to(torch.int64), r)  # [F, 6, H, W]
    on = n_m > 0
    mean = (s.double() / torch.where(on, n_m * 65536, torch.ones_like(n_m)).double()).float()
    mean = torch.where(on, mean, torch.zeros((), dtype=torch.float32))
    abar, bbar = mean[:, 0:3], mean[:, 3:6]
    w = M.to(torch.float32) / 255.0
    t = abar * I.float()
    u = t + bbar
    e = u * w
    res = (d.float() - e).abs().amax(dim=1)
    R = torch.round(res.clamp(max=255.0) * 256.0).to(torch.int32)
    coef = torch.zeros(mean.shape[0], mean.shape[2], mean.shape[3], _lf.CELL, dtype=torch.float32)
    coef[..., 0:6] = mean.permute(0, 2, 3, 1)
    return coef, R.contiguous()


def coefficients_reference(L: torch.Tensor, E: torch.Tensor, M: torch.Tensor, cfg: _lf.LiftConfig) -> torch.Tensor:
    """Stages 1 to 3 -> the cells fp32 [F, H, W, 8]; the gate is `lift.gate_reference`."""
    coef, R = smooth_reference(L, E, fit_reference(L, E, M, cfg), M, cfg)
    if cfg.gate is not None:
        coef[..., 6] = _lf.gate_reference(R, cfg)
    return coef


def reference(P: torch.Tensor, L: torch.Tensor, E: torch.Tensor, M: torch.Tensor, U: Optional[torch.Tensor] = None,
              cfg: Optional[_lf.LiftConfig] = None, return_coef: bool = False):
    """`lift.reference` with the two masked stages: P uint8 [SH, SW, 3], L uint8 [H, W, 3], E uint8 [F, H, W, 3], M uint8 [H, W], U uint8
    [F, SH, SW, 3] (required unless cfg.gate is None) -> uint8 [F, SH, SW, 3], the edit at full strength (and the cells)."""
    cfg = cfg or _lf.LiftConfig()
    P, L, E, M = P.cpu(), L.cpu(), E.cpu(), M.cpu()
    _lf._check_planes(P, E, U, cfg)
    coef = coefficients_reference(L, E, M, cfg)
    out = _lf.apply_reference(P, coef, _lf.tables((P.shape[1], P.shape[0]), tuple(L.shape[:2])), U.cpu() if cfg.gate is not None else None)
    return (out, coef) if return_coef else out


def device_coefficients(L: torch.Tensor, E: torch.Tensor, M: torch.Tensor, cfg: _lf.LiftConfig) -> torch.Tensor:
    """Stages 1 to 3 on the device: the two masked passes, then ce_lift_gate_f32 -> the cells.  Nothing is read back."""
    from . import ops
    AB = ops.rimlift_fit_q16(L, E, M, cfg.radius, cfg.eps_q, cfg.max_gain)
    coef, R = ops.rimlift_smooth(L, E, M, AB, cfg.radius)
    if cfg.gate is not None:
        ops.lift_gate(R, coef, cfg.radius, *cfg.gate)
    return coef
