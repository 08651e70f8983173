"""Auto-focused edits: an instruction-only edit finds its region on the whole photo, then edits the region's crop at the photo's size.

`ChronoEditPipeline.__call__(image, prompt)` takes no mask.  With `enable_auto_region` and `enable_auto_focus`, one call is

    scout     today's auto-region call on the whole photo resized to width x height, up to and including step k's detection
              (chronoedit_amd/auto_region.py); declined, or no box worth cropping to: the scout runs on and IS the call's result
    lift      the detected edit-size mask -> the photo's size (`focus.resize_l8` on the device, PIL's bilinear resize on the host: the same
              bytes); its bounding box and non-zero count by one device reduction (`mask_box`), the box by `focus.focus_box`, the mask's
              share of the box by a second reduction over the box's view of the mask
    focused   the explicit-mask focused region edit (chronoedit_amd/focus.py) of the crop, from the call's ONE noise tensor: all steps (cold
              start: bit for bit the call `set_edit_region(report mask)` + `enable_region_focus(context)` would make), or from step k + 1
              (warm start) on latents = (1 - s) * R(x0) + s * eps: x0 the scout's estimate of the final image behind step k, R the crop of
              the scout's latent grid to the box, bilinearly resampled to the crop's latent grid (`restart_tables`), s the schedule's
              sigma at index k + 1, eps the noise

Host side only; the device passes are csrc/ce_autofocus.hip.  `mask_box` and `restart` are ALSO torch expressions for tensors on the CPU,
with the same bits (the tests compare them with torch.equal), as auto_region.py's passes are.  Whether step k's estimate locates a real
edit, and whether a checkpoint rebuilds detail from a resampled estimate, is the checkpoint's business."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple

import numpy as np
import torch

from .focus import Box, focus_box


@dataclass(frozen=True)
class AutoFocusConfig:
    """context: `focus.focus_box`'s padding around the detected region's bounding box.  warm_start: the focused pass starts behind the
    scout's last step instead of at step 0."""
    context: float = 0.25
    warm_start: bool = False

    def __post_init__(self):
        focus_box(None, (1, 1), (1, 1), self.context)  # (validates the context)
        if not isinstance(self.warm_start, bool):
            raise ValueError(f"auto focus: warm_start must be a bool, got {self.warm_start!r}")


# ---- the tables of the warm start -----------------------------------------------------------------------------------------------
def axis_table(lo: int, extent: int, n: int, src: int):
    """One axis of R: output cell x of n has its centre at photo coordinate lo + (x + 1/2) * extent / n, which is u = that * n / src - 1/2 in
    units of the scout's grid (n cells over the src photo pixels), clamped to [0, n - 1] -> (i0 = floor(u), i1 = min(i0 + 1, n - 1),
    f = fp32(u - i0)) as int32 [n], int32 [n], fp32 [n].  Exact rationals; the whole photo (lo = 0, extent = src) gives i0 = x, f = 0."""
    lo, extent, n, src = int(lo), int(extent), int(n), int(src)
    if n < 1 or src < 1 or extent < 1 or lo < 0 or lo + extent > src:
        raise ValueError(f"axis_table: [{lo}, {lo + extent}) does not lie inside [0, {src}), or an empty grid ({n})")
    i0, i1, f = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
    for x in range(n):
        u = (lo + Fraction(2 * x + 1, 2) * extent / n) * n / src - Fraction(1, 2)
        u = min(max(u, Fraction(0)), Fraction(n - 1))
        a = u.__floor__()
        i0[x], i1[x], f[x] = a, min(a + 1, n - 1), np.float32(float(u - a))
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(f)


def restart_tables(box: Box, src_size: Tuple[int, int], grid: Tuple[int, int], device=None):
    """box = (left, top, right, bottom) in the photo of src_size = (SW, SH), grid = (h, w) latent cells (of the scout AND of the crop: one
    edit size) -> (ix0, ix1, fx, iy0, iy1, fy), on `device` when given."""
    l, t, r, b = box
    h, w = grid
    tabs = axis_table(l, r - l, w, src_size[0]) + axis_table(t, b - t, h, src_size[1])
    return tuple(v.to(device) for v in tabs) if device is not None else tabs


# ---- the two passes: the device kernel for a tensor on the GPU, the torch expression for one on the CPU - the same bits ------------
def bbox_counts(mask_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [H, W] (any row stride) -> int32 [5] on the mask's device: left, top, right, bottom (half open) of mask > 0 and the count of
    non-zero bytes; W, H, 0, 0, 0 for an empty mask."""
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 2:
        raise ValueError(f"bbox_counts: need a uint8 [H, W] mask, got {mask_u8.dtype} {tuple(mask_u8.shape)}")
    if mask_u8.is_cuda:
        from . import ops
        return ops.autofocus_bbox_u8(mask_u8)
    H, W = mask_u8.shape
    nz = mask_u8 > 0
    rows, cols = torch.nonzero(nz.any(1)).reshape(-1), torch.nonzero(nz.any(0)).reshape(-1)
    if rows.numel() == 0:
        return torch.tensor([W, H, 0, 0, 0], dtype=torch.int32)
    return torch.tensor([int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1, int(nz.sum())], dtype=torch.int32)


def mask_box(mask_u8: torch.Tensor) -> Tuple[Optional[Box], int]:
    """(`focus.mask_bbox`, the count of non-zero bytes) of a mask on either device: on the GPU one reduction and ONE read of five integers."""
    l, t, r, b, n = (int(v) for v in bbox_counts(mask_u8).tolist())
    return (None if n == 0 else (l, t, r, b)), n


def restart(x0: torch.Tensor, eps: torch.Tensor, tables, s: float, bf16_state: bool = False) -> torch.Tensor:
    """x0, eps fp32 [..., h, w] -> a new fp32 tensor (1 - s) * R(x0) + s * eps:
        top = a00 + fx * (a01 - a00),  bot = a10 + fx * (a11 - a10),  v = top + fy * (bot - top)
    every operation rounded in fp32; bf16_state: rounded to a bf16 value."""
    if x0.is_cuda:
        from . import ops
        return ops.autofocus_restart(x0.contiguous(), eps.contiguous(), tuple(t.to(x0.device).contiguous() for t in tables), s, bf16_state)
    ix0, ix1, fx, iy0, iy1, fy = (t.cpu() for t in tables)
    x0, eps = x0.to(torch.float32), eps.to(torch.float32)
    xa, xb, ya, yb = ix0.long(), ix1.long(), iy0.long(), iy1.long()
    r0, r1 = x0.index_select(-2, ya), x0.index_select(-2, yb)
    a00, a01, a10, a11 = r0.index_select(-1, xa), r0.index_select(-1, xb), r1.index_select(-1, xa), r1.index_select(-1, xb)
    fyc = fy.reshape(-1, 1)
    top = a00 + fx * (a01 - a00)
    bot = a10 + fx * (a11 - a10)
    v = top + fyc * (bot - top)
    s32 = torch.tensor(float(s), dtype=torch.float32)
    out = (torch.tensor(1.0, dtype=torch.float32) - s32) * v + s32 * eps
    return out.to(torch.bfloat16).to(torch.float32) if bf16_state else out


# ---- the host planning of one call ------------------------------------------------------------------------------------------------
def lift_mask(mask_u8: torch.Tensor, src_size: Tuple[int, int]) -> torch.Tensor:
    """The detection's edit-size mask uint8 [H, W] -> the photo's size uint8 [SH, SW], on the mask's device: `focus.resize_l8` on the GPU,
    PIL's Image.resize(..., BILINEAR) on the host - the same bytes."""
    SW, SH = int(src_size[0]), int(src_size[1])
    if mask_u8.is_cuda:
        from .focus import resize_l8
        return resize_l8(mask_u8.contiguous(), (SW, SH))
    from PIL import Image
    m = Image.fromarray(mask_u8.numpy())
    if m.size != (SW, SH):
        m = m.resize((SW, SH), Image.BILINEAR)
    return torch.from_numpy(np.array(m, dtype=np.uint8))


def plan(mask_src: torch.Tensor, edit_size: Tuple[int, int], context: float) -> dict:
    """mask_src = the lifted mask uint8 [SH, SW] (either device), edit_size = (width, height) -> the entries of `focus.plan`, from two
    reductions: the whole mask (the bounding box), then the box's view of it (the mask's share of the box)."""
    SH, SW = mask_src.shape
    W, H = int(edit_size[0]), int(edit_size[1])
    bbox, _ = mask_box(mask_src)
    box, reason = focus_box(bbox, (SW, SH), (W, H), context)
    l, t, r, b = box
    return {"box": box, "reason": reason, "source_size": (SW, SH), "edit_size": (W, H), "scale": (r - l) / W,
            "mask_fraction_of_box": float(mask_box(mask_src[t:b, l:r])[1]) / ((r - l) * (b - t))}


def worth_focusing(report: dict) -> bool:
    """Does the plan crop at all?  Not when the box is the whole photo ("fit", "empty", or a region that fills it)."""
    SW, SH = report["source_size"]
    return report["reason"] == "ok" and tuple(report["box"]) != (0, 0, SW, SH)
