"""Guided detail lift: whole-image edits returned at the photo's size.

A focused edit (chronoedit_amd/focus.py) needs a region small enough to crop to.  "Make it winter" has none: the edit runs on the whole photo
resized to width x height and its frames have that size.  The lift carries the edit-size CHANGE up to the photo's pixel grid without throwing
the photo's detail away - guided upsampling (He & Sun's fast guided filter, Chen et al.'s bilateral guided upsampling), no model:

    fit      per edit-size cell, colour and frame an affine map a * I + b from the edit-size source L to the change d = E - L, least squares
             over the (2 r + 1)^2 window, regularised by eps, |a| <= max_gain
    smooth   the box mean of the maps, and the residual the smoothed map leaves at every cell
    gate     the box mean of the residual -> g in [0, 1]: 0 where the affine model explains the change, 1 where structure was replaced
    apply    a, b, g sampled bilinearly at the photo's pixel centres;  out = p + (a p + b), then out + g (U - out) with U the plain Lanczos
             upsample of the edited frame

P = the photo uint8 [SH, SW, 3]; L = its Lanczos resize to the edit's size, uint8 [H, W, 3] - the bytes the pre-processing feeds the VAE;
E = the frames uint8 [F, H, W, 3] as `ops.video_to_u8` makes them; U = uint8 [F, SH, SW, 3] or None (gate=None: no fallback).

`reference` (CPU torch, one torch op per rounded operation) is the definition.  The device passes (csrc/ce_lift.hip) are bit-equal to its
stages, and it is the host path itself.  Statistics are exact integers and the maps are stored in 16.16 fixed point, so the box sums of
every stage are exact and no summation order can change a bit.  What follows from the arithmetic:

  * E == L gives out == P byte for byte (a = b = g = 0, p + (0 p + 0) = p);
  * wherever E == L over the +-(3 r + 1)-cell neighbourhood of a pixel's four bilinear corners, the pixel is the photo's;
  * wherever g_up == 1 the pixel is U's.

Which radius / eps / gate suit a trained checkpoint is the checkpoint's business; `fallback_fraction` (the mean of g) says how much of a
picture was plain upsampling."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

MAX_RADIUS = 16
MAX_EPS = float(1 << 30)
CELL = 8  # floats per coefficient cell: abar_rgb, bbar_rgb, g, 0


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_num(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


@dataclass(frozen=True)
class LiftConfig:
    """radius: the window's half width in edit-size cells, 1..16.  eps: the regulariser of the fit in squared byte units (26 = (0.02 * 255)^2),
    used as eps_q = max(1, rint(eps)).  gate: (t0, t1), 0 <= t0 < t1 - the mean residual in bytes at which the fallback starts and at which
    it is complete - or None: no fallback, no Lanczos pass.  max_gain: the bound of |a|, 1..8."""
    radius: int = 4
    eps: float = 26.0
    gate: Optional[Tuple[float, float]] = (4.0, 12.0)
    max_gain: float = 8.0

    def __post_init__(self):
        if not _is_int(self.radius) or not 1 <= self.radius <= MAX_RADIUS:
            raise ValueError(f"detail lift: radius must be an integer in 1..{MAX_RADIUS}, got {self.radius!r}")
        if not _is_num(self.eps) or not 0.0 < float(self.eps) <= MAX_EPS:
            raise ValueError(f"detail lift: eps must be a number in (0, 2^30], got {self.eps!r}")
        if self.gate is not None:
            g = self.gate
            if not isinstance(g, (tuple, list)) or len(g) != 2 or not all(_is_num(v) for v in g):
                raise ValueError(f"detail lift: gate must be (t0, t1) or None, got {g!r}")
            t0, t1 = float(np.float32(g[0])), float(np.float32(g[1]))
            if not (0.0 <= t0 < t1 < math.inf):
                raise ValueError(f"detail lift: gate needs 0 <= t0 < t1 (distinct as fp32, finite), got {g!r}")
            object.__setattr__(self, "gate", (t0, t1))
        if not _is_num(self.max_gain) or not 1.0 <= float(self.max_gain) <= 8.0:
            raise ValueError(f"detail lift: max_gain must be a number in [1, 8], got {self.max_gain!r}")
        object.__setattr__(self, "radius", int(self.radius))
        object.__setattr__(self, "eps", float(self.eps))
        object.__setattr__(self, "max_gain", float(np.float32(self.max_gain)))

    @property
    def eps_q(self) -> int:
        return max(1, int(round(self.eps)))  # (Python rounds halves to even, as rint does)


# ---- box sums --------------------------------------------------------------------------------------------------------------------------
def box_sum(x: torch.Tensor, r: int) -> torch.Tensor:
    """x integer [..., H, W] -> int64 [..., H, W]: the sum over the window [y - r, y + r] x [x - r, x + r] clipped to the image."""
    x = x.to(torch.int64)
    for dim in (-1, -2):
        n = x.shape[dim]
        c = torch.cat([torch.zeros_like(x.narrow(dim, 0, 1)), x.cumsum(dim)], dim=dim)
        i = torch.arange(n)
        x = c.index_select(dim, (i + r + 1).clamp(max=n)) - c.index_select(dim, (i - r).clamp(min=0))
    return x


def box_count(H: int, W: int, r: int) -> torch.Tensor:
    """int64 [H, W]: the window's cell count n."""
    return box_sum(torch.ones(H, W, dtype=torch.int64), r)


# ---- the axis tables ------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=64)
def _axis_table(n_out: int, n: int):
    i0, i1, t = np.empty(n_out, np.int32), np.empty(n_out, np.int32), np.empty(n_out, np.float32)
    for o in range(n_out):
        u = Fraction(2 * o + 1, 2) * n / n_out - Fraction(1, 2)
        u = min(max(u, Fraction(0)), Fraction(n - 1))
        a = u.__floor__()
        i0[o], i1[o], t[o] = a, min(a + 1, n - 1), np.float32(float(u - a))
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(t)


def axis_table(n_out: int, n: int):
    """Half-pixel-centre bilinear sampling of n cells at the centres of n_out pixels: pixel o sits at u = (o + 1/2) * n / n_out - 1/2 in cell
    units, clamped to [0, n - 1] -> (i0 = floor(u), i1 = min(i0 + 1, n - 1), t = fp32(u - i0)) as int32 [n_out], int32 [n_out], fp32 [n_out].
    Exact rationals.  (`autofocus.axis_table` samples a grid at the centres of as many cells as the grid has - the whole photo as its box is
    the identity - so it cannot serve here.)"""
    n_out, n = int(n_out), int(n)
    if n_out < 1 or n < 1:
        raise ValueError(f"axis_table: empty axis ({n_out}, {n})")
    return _axis_table(n_out, n)


def tables(src_size: Tuple[int, int], grid: Tuple[int, int], device=None):
    """src_size = (SW, SH), grid = (H, W) -> (ix0, ix1, tx, iy0, iy1, ty), on `device` when given."""
    tabs = axis_table(src_size[0], grid[1]) + axis_table(src_size[1], grid[0])
    return tuple(v.to(device) for v in tabs) if device is not None else tabs


# ---- the stages: CPU torch, the definition -----------------------------------------------------------------------------------------------
def _planes(L: torch.Tensor, E: torch.Tensor):
    """I int64 [3, H, W], d int64 [F, 3, H, W]."""
    if L.dtype != torch.uint8 or E.dtype != torch.uint8 or L.dim() != 3 or E.dim() != 4 or L.shape[2] != 3 or tuple(E.shape[1:]) != tuple(L.shape):
        raise ValueError(f"lift: need L uint8 [H, W, 3] and E uint8 [F, H, W, 3], got {L.dtype} {tuple(L.shape)} and {E.dtype} {tuple(E.shape)}")
    I = L.permute(2, 0, 1).to(torch.int64)
    return I, E.permute(0, 3, 1, 2).to(torch.int64) - I


def fit_reference(L: torch.Tensor, E: torch.Tensor, cfg: LiftConfig) -> torch.Tensor:
    """Stage 1 -> int32 [F, H, W, 6]: A_rgb, B_rgb = rint(65536 a), rint(65536 b)."""
    I, d = _planes(L, E)
    r = cfg.radius
    n = box_count(I.shape[1], I.shape[2], r)
    S_I, S_d, S_II, S_Id = box_sum(I, r), box_sum(d, r), box_sum(I * I, r), box_sum(I * d, r)
    num = n * S_Id - S_I * S_d
    den = n * S_II - S_I * S_I + cfg.eps_q * n * n
    a = (num.double() / den.double()).clamp(-cfg.max_gain, cfg.max_gain).float()
    m = a.double() * S_I.double()
    u = S_d.double() - m
    b = (u / n.double()).float()
    A, B = torch.round(a * 65536.0).to(torch.int32), torch.round(b * 65536.0).to(torch.int32)
    return torch.cat([A, B], dim=1).permute(0, 2, 3, 1).contiguous()


def smooth_reference(L: torch.Tensor, E: torch.Tensor, AB: torch.Tensor, cfg: LiftConfig):
    """Stage 2 -> (the cells fp32 [F, H, W, 8] with abar_rgb, bbar_rgb and zeros in slots 6, 7; R int32 [F, H, W])."""
    I, d = _planes(L, E)
    r = cfg.radius
    n = box_count(I.shape[1], I.shape[2], r)
    s = box_sum(AB.permute(0, 3, 1, 2), r)  # [F, 6, H, W]
    mean = (s.double() / (n * 65536).double()).float()
    abar, bbar = mean[:, 0:3], mean[:, 3:6]
    m = abar * I.float()
    e = m + bbar
    res = (d.float() - e).abs().amax(dim=1)
    R = torch.round(res.clamp(max=255.0) * 256.0).to(torch.int32)
    coef = torch.zeros(mean.shape[0], mean.shape[2], mean.shape[3], CELL, dtype=torch.float32)
    coef[..., 0:6] = mean.permute(0, 2, 3, 1)
    return coef, R.contiguous()


def gate_reference(R: torch.Tensor, cfg: LiftConfig) -> torch.Tensor:
    """Stage 3 -> g fp32 [F, H, W]."""
    t0, t1 = (torch.tensor(v, dtype=torch.float32) for v in cfg.gate)
    n = box_count(R.shape[1], R.shape[2], cfg.radius)
    m = (box_sum(R, cfg.radius).double() / (n * 256).double()).float()
    up = m - t0
    dn = t1 - t0
    return (up / dn).clamp(0.0, 1.0)


def coefficients_reference(L: torch.Tensor, E: torch.Tensor, cfg: LiftConfig) -> torch.Tensor:
    """Stages 1 to 3 -> the cells fp32 [F, H, W, 8]."""
    coef, R = smooth_reference(L, E, fit_reference(L, E, cfg), cfg)
    if cfg.gate is not None:
        coef[..., 6] = gate_reference(R, cfg)
    return coef


def _lerp(a, b, t):
    """a * (1 - t) + b * t: a subtraction, two multiplies, one add (the order of ce_preview_rgb_u8)."""
    s = 1.0 - t
    left = a * s
    right = b * t
    return left + right


def apply_reference(P: torch.Tensor, coef: torch.Tensor, tabs, U: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Stage 4 -> uint8 [F, SH, SW, 3]."""
    ix0, ix1, tx, iy0, iy1, ty = (t.cpu() for t in tabs)
    xa, xb, ya, yb = ix0.long(), ix1.long(), iy0.long(), iy1.long()
    txv, tyv = tx.view(1, -1, 1), ty.view(-1, 1, 1)
    p = P.to(torch.float32)
    out = torch.empty((coef.shape[0],) + tuple(P.shape), dtype=torch.uint8)
    for f in range(coef.shape[0]):
        r0, r1 = coef[f, ya], coef[f, yb]
        top = _lerp(r0[:, xa], r0[:, xb], txv)
        bot = _lerp(r1[:, xa], r1[:, xb], txv)
        v = _lerp(top, bot, tyv)
        m = v[..., 0:3] * p
        e = m + v[..., 3:6]
        q = p + e
        if U is not None:
            dlt = U[f].to(torch.float32) - q
            m = v[..., 6:7] * dlt
            q = q + m
        q = torch.where(q != q, torch.zeros_like(q), q).clamp(0.0, 255.0)
        out[f] = torch.round(q).to(torch.uint8)
    return out


def reference(P: torch.Tensor, L: torch.Tensor, E: torch.Tensor, U: Optional[torch.Tensor] = None, cfg: Optional[LiftConfig] = None,
              return_coef: bool = False):
    """The definition: P uint8 [SH, SW, 3], L uint8 [H, W, 3], E uint8 [F, H, W, 3], U uint8 [F, SH, SW, 3] (required unless cfg.gate is None,
    ignored then) -> uint8 [F, SH, SW, 3] (and the cells)."""
    cfg = cfg or LiftConfig()
    P, L, E = P.cpu(), L.cpu(), E.cpu()
    _check_planes(P, E, U, cfg)
    coef = coefficients_reference(L, E, cfg)
    out = apply_reference(P, coef, tables((P.shape[1], P.shape[0]), tuple(L.shape[:2])), U.cpu() if cfg.gate is not None else None)
    return (out, coef) if return_coef else out


def _check_planes(P, E, U, cfg):
    if P.dtype != torch.uint8 or P.dim() != 3 or P.shape[2] != 3:
        raise ValueError(f"lift: need P uint8 [SH, SW, 3], got {P.dtype} {tuple(P.shape)}")
    if cfg.gate is not None:
        want = (E.shape[0],) + tuple(P.shape)
        if U is None or U.dtype != torch.uint8 or tuple(U.shape) != want:
            raise ValueError(f"lift: with a gate U must be uint8 {want}, got {None if U is None else (U.dtype, tuple(U.shape))}")


# ---- either device -----------------------------------------------------------------------------------------------------------------------
def lift(P: torch.Tensor, L: torch.Tensor, E: torch.Tensor, U: Optional[torch.Tensor], cfg: LiftConfig):
    """(the lifted frames uint8 [F, SH, SW, 3], the mean of g as a 0-d float64 tensor) on P's device: the four device passes for tensors on
    the GPU, `reference` for tensors on the CPU - the same bytes.  Nothing is read back here."""
    if not P.is_cuda:
        out, coef = reference(P, L, E, U, cfg, return_coef=True)
        return out, coef[..., 6].double().mean()
    from . import ops
    _check_planes(P, E, U, cfg)
    P, L, E = P.contiguous(), L.contiguous(), E.contiguous()
    AB = ops.lift_fit_q16(L, E, cfg.radius, cfg.eps_q, cfg.max_gain)
    coef, R = ops.lift_smooth(L, E, AB, cfg.radius)
    if cfg.gate is not None:
        ops.lift_gate(R, coef, cfg.radius, *cfg.gate)
    tabs = tables((P.shape[1], P.shape[0]), tuple(L.shape[:2]), P.device)
    out = ops.lift_apply_u8(P, coef, tabs, U.contiguous() if cfg.gate is not None else None)
    return out, coef[..., 6].double().mean()


# ---- the output stage of a lifted call ---------------------------------------------------------------------------------------------------
def report_entry(size, edit_size, reason: str) -> dict:
    """One sample's `lift_report` entry: "ok" is the lift, "same" (the image has the edit's size already) and "focus" are not."""
    return {"size": size, "edit_size": (int(edit_size[0]), int(edit_size[1])), "applied": reason == "ok", "reason": reason, "fallback_fraction": None}


def output(video: torch.Tensor, cfg: LiftConfig, kept, imgs, image_of, height: int, width: int, output_type: str):
    """(every sample's frames lifted to its image's size, in postprocess_video's layouts - None when every image already has the edit's
    size: the caller then returns the plain frames -, the `lift_report`).  kept: per image (P, L) on the device
    (`image_io.preprocess_pil`), or None: the host form.  The gate means of all samples are read back once."""
    from PIL import Image
    from . import image_io, ops
    image_io.check_output_type(output_type)
    B = video.shape[0]
    same = [imgs[image_of(b)].size == (width, height) for b in range(B)]
    report = [report_entry(imgs[image_of(b)].size, (width, height), "same" if same[b] else "ok") for b in range(B)]
    if all(same):
        return None, report
    on_device = kept is not None and image_io.device_video(video)
    u8 = ops.video_to_u8(video.contiguous()) if on_device else None
    out, fractions = [], []
    for b in range(B):
        im = imgs[image_of(b)]
        if on_device:
            E = u8[b]
        else:
            frames = image_io.postprocess_video(video[b:b + 1], "pil")[0]
            E = torch.from_numpy(np.stack([np.asarray(f, dtype=np.uint8) for f in frames]))
        if same[b]:
            out.append(E)
            continue
        if on_device:
            P, L = kept[image_of(b)]
            U = None if cfg.gate is None else torch.stack([image_io.resize_u8(f, im.size, image_io.LANCZOS) for f in E])
        else:
            rgb = im.convert("RGB")
            P = torch.from_numpy(np.array(rgb, dtype=np.uint8))
            L = torch.from_numpy(np.array(rgb.resize((width, height), Image.LANCZOS), dtype=np.uint8))
            U = None if cfg.gate is None else torch.from_numpy(np.stack([np.asarray(f.resize(im.size, Image.LANCZOS), dtype=np.uint8) for f in frames]))
        o, frac = lift(P, L, E, U, cfg)
        out.append(o)
        fractions.append((b, frac))
    if fractions:
        for (b, _), v in zip(fractions, torch.stack([f for _, f in fractions]).cpu().tolist()):
            report[b]["fallback_fraction"] = float(v)
    return image_io.frames_from_u8([o.cpu().numpy() for o in out], output_type), report
