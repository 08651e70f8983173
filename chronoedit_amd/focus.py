"""Focused region edits: crop to the mask, edit the crop at the model's resolution, paste back at the photo's size.

A region edit (chronoedit_amd/region.py) works at the edit's own size: the whole photo is resized to width x height and every returned
frame has that size.  With focus (`ChronoEditPipeline.enable_region_focus`) and a mask given at the PHOTO's size, per image

    box     a rectangle of the edit's aspect ratio around the mask's bounding box, with some context (`focus_box`)
    in      image.crop(box) -> Lanczos resize to (width, height) -> the VAE and CLIP;  mask.crop(box) -> bilinear resize -> the edit's region
    edit    an ordinary region edit of the crop (sparse steps, TeaCache, guidance reuse, graph replay: unchanged)
    out     every frame -> uint8 -> Lanczos resize to the box -> Image.paste(frame, (left, top), mask) into the untouched photo

so the returned frames have the photo's size and carry the photo's own bytes wherever the mask is 0, and the model's pixels go to what
the mask marks.  The box is pure integer arithmetic; the byte passes are PIL's (csrc/ce_image.hip, csrc/ce_focus.hip on the device, PIL
itself on the host: `host_inputs`, `host_paste` - the two forms give the same bytes).  How well a checkpoint edits a crop, or blends its
seam, is the checkpoint's business."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Any, List, Optional, Tuple

import torch

Box = Tuple[int, int, int, int]  # (left, top, right, bottom), half open


def _ceil(q: Fraction) -> int:
    return -((-q.numerator) // q.denominator)


def focus_box(bbox: Optional[Box], src_size: Tuple[int, int], edit_size: Tuple[int, int], context: float = 0.25) -> Tuple[Box, str]:
    """bbox = the half-open bounding box of mask > 0 at the source's resolution (None: an empty mask), src_size = (SW, SH), edit_size =
    (W, H) -> ((left, top, right, bottom), reason).  Integers and exact rationals only (context is read as the nearest fraction with a
    denominator <= 65536: 0.1 is 1 / 10).

    "empty"  no mask: the whole image.
    "ok"     the bbox padded by ceil(context * its longer side) on every side, raised to at least W x H (the crop is never UP-sampled into
             the model while the photo has the pixels), widened to the edit's aspect ratio, centred on the bbox and shifted - never shrunk -
             into the image.  When that does not fit, the largest box of the edit's aspect ratio that does (the padding is given up).
    "fit"    even that box is narrower or lower than the bare bbox: the whole image, as an unfocused edit sees it.

    The box lies inside the image and contains the bbox; with "ok", |bw H - bh W| < max(W, H), and bw >= W, bh >= H when SW >= W, SH >= H."""
    SW, SH = int(src_size[0]), int(src_size[1])
    W, H = int(edit_size[0]), int(edit_size[1])
    if SW < 1 or SH < 1 or W < 1 or H < 1:
        raise ValueError(f"focus_box: sizes must be positive, got source {src_size} and edit {edit_size}")
    ctx = float(context)
    if not (0.0 <= ctx < math.inf):  # (a NaN fails the comparison)
        raise ValueError(f"focus_box: context must be a finite number >= 0, got {context!r}")
    if bbox is None:
        return (0, 0, SW, SH), "empty"
    l, t, r, b = (int(v) for v in bbox)
    if not (0 <= l < r <= SW and 0 <= t < b <= SH):
        raise ValueError(f"focus_box: the bbox {bbox} does not lie inside the {SW}x{SH} source")
    bbw, bbh = r - l, b - t
    pad = _ceil(Fraction(ctx).limit_denominator(1 << 16) * max(bbw, bbh))
    want_w, want_h = max(bbw + 2 * pad, W), max(bbh + 2 * pad, H)
    s = max(Fraction(want_w, W), Fraction(want_h, H))
    bw, bh = _ceil(s * W), _ceil(s * H)
    if bw > SW or bh > SH:
        s = min(Fraction(SW, W), Fraction(SH, H))
        bw, bh = (s * W).__floor__(), (s * H).__floor__()
        if bw < bbw or bh < bbh:
            return (0, 0, SW, SH), "fit"
    cx, cy = (l + r) // 2, (t + b) // 2
    left = min(max(cx - bw // 2, 0), SW - bw)
    top = min(max(cy - bh // 2, 0), SH - bh)
    return (left, top, left + bw, top + bh), "ok"


def mask_bbox(mask_u8: torch.Tensor) -> Optional[Box]:
    """The half-open bounding box (left, top, right, bottom) of mask > 0 for a uint8 [H, W] mask on the host; None when the mask is empty."""
    nz = mask_u8 > 0
    rows, cols = torch.nonzero(nz.any(1)).reshape(-1), torch.nonzero(nz.any(0)).reshape(-1)
    if rows.numel() == 0:
        return None
    return int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1


def _plan(image_size, mask, height: int, width: int, context: float):
    from . import region as _rg
    SW, SH = int(image_size[0]), int(image_size[1])
    mask_u8 = _rg.normalize_mask(mask, SH, SW)
    box, reason = focus_box(mask_bbox(mask_u8), (SW, SH), (width, height), context)
    l, t, r, b = box
    report = {"box": box, "reason": reason, "source_size": (SW, SH), "edit_size": (int(width), int(height)), "scale": (r - l) / int(width),
              "mask_fraction_of_box": float((mask_u8[t:b, l:r] > 0).sum()) / ((r - l) * (b - t))}
    return report, mask_u8


def plan(image_size: Tuple[int, int], mask, height: int, width: int, context: float = 0.25) -> dict:
    """What a focused call would do for an image of image_size = (SW, SH) and this mask (whatever `region.normalize_mask` takes, at the
    source's size; a PIL mask of another size is resized to it), without running anything: {"box", "reason" ("ok" / "fit" / "empty"),
    "source_size", "edit_size" (both (width, height)), "scale" = box width / edit width, "mask_fraction_of_box" = the share of the box's
    pixels with mask > 0}.  The entries of `pipe.focus_report`."""
    return _plan(image_size, mask, height, width, context)[0]


# ---- the host form: PIL itself ------------------------------------------------------------------------------------------------
def _mask_pil(mask_u8: torch.Tensor):
    from PIL import Image
    return Image.fromarray(mask_u8.numpy())


def host_inputs(image, mask_u8: torch.Tensor, box: Box, width: int, height: int):
    """(the crop as an RGB PIL image - what preprocessing and CLIP get -, the edit's region mask uint8 [height, width] on the host):
    image.crop(box), and mask.crop(box).resize((width, height), Image.BILINEAR) when the sizes differ."""
    from . import region as _rg
    return image.convert("RGB").crop(box), _rg.normalize_mask(_mask_pil(mask_u8).crop(box), height, width)


def host_paste(image, frames, mask_u8: Optional[torch.Tensor], box: Box) -> list:
    """Per frame (PIL, the edit's size): out = image.copy(); out.paste(frame.resize((bw, bh), Image.LANCZOS), (left, top), mask.crop(box)) -
    mask_u8 None: without a mask, the whole box is replaced.  PIL frames of the image's size."""
    from PIL import Image
    l, t, r, b = box
    src = image.convert("RGB")
    m = None if mask_u8 is None else _mask_pil(mask_u8).crop(box)
    out = []
    for f in frames:
        o = src.copy()
        o.paste(f.resize((r - l, b - t), Image.LANCZOS), (l, t), m)
        out.append(o)
    return out


# ---- the device form ---------------------------------------------------------------------------------------------------------
def resize_l8(mask_u8: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """Image.resize((W2, H2), Image.BILINEAR) of an "L" image held as uint8 [H, W] on the device - or a VIEW of one with any row stride, such
    as mask[top:bottom, left:right]: horizontal pass, then vertical over the rounded bytes; an unchanged axis launches nothing."""
    from . import image_io, ops
    W2, H2 = int(size[0]), int(size[1])
    H, W = mask_u8.shape
    out = mask_u8
    if W2 != W:
        out = ops.focus_resample_l8(out, 0, *image_io._device_tables(W, W2, image_io.BILINEAR, mask_u8.device))
    if H2 != H:
        out = ops.focus_resample_l8(out, 1, *image_io._device_tables(H, H2, image_io.BILINEAR, mask_u8.device))
    return out.contiguous()


def device_inputs(src_u8: torch.Tensor, mask_dev: torch.Tensor, box: Box, width: int, height: int):
    """host_inputs on the device: src_u8 = the photo's bytes uint8 [SH, SW, 3], mask_dev uint8 [SH, SW] -> (the crop resized to the edit's
    size uint8 [height, width, 3], the edit's region mask uint8 [height, width])."""
    from . import image_io
    l, t, r, b = box
    crop = image_io.resize_u8(src_u8[t:b, l:r].contiguous(), (width, height), image_io.LANCZOS)
    return crop, resize_l8(mask_dev[t:b, l:r], (width, height))


def device_paste(frames_u8: torch.Tensor, src_u8: torch.Tensor, mask_dev: Optional[torch.Tensor], box: Box) -> torch.Tensor:
    """host_paste on the device: frames_u8 uint8 [F, H, W, 3] (ops.video_to_u8 of one sample) -> uint8 [F, SH, SW, 3]."""
    from . import image_io, ops
    l, t, r, b = box
    size = (r - l, b - t)
    if tuple(frames_u8.shape[1:3]) != (size[1], size[0]):
        frames_u8 = torch.stack([image_io.resize_u8(f, size, image_io.LANCZOS) for f in frames_u8])
    return ops.focus_paste_u8(frames_u8.contiguous(), src_u8, mask_dev, l, t)


def masks_for(masks, n_img: int) -> List:
    """One mask for every image, or a list with one per image -> a list of n_img."""
    if isinstance(masks, list):
        if len(masks) != n_img:
            raise ValueError(f"the edit region holds {len(masks)} masks, but the call has {n_img} image(s): pass one mask, or one per image")
        return masks
    return [masks] * n_img


# ---- one image of a focused call --------------------------------------------------------------------------------------------------
@dataclass
class FocusPlan:
    """What a focused edit knows about one image; the mask lies on the host, on the device, or both."""
    image: Any  # the PIL photo the crop is cut from: the VAE and CLIP see its crop
    report: dict  # `plan`'s entries; report["box"] is the crop
    mask_u8: Optional[torch.Tensor] = None  # the source-size mask on the host
    mask_dev: Optional[torch.Tensor] = None  # ... on the device
    src_u8: Optional[torch.Tensor] = None  # the photo's bytes on the device: set when the device passes run
    paste_image: Any = None  # a second source the frames are pasted into (a sketch edit's background); None: `image`
    paste_u8: Optional[torch.Tensor] = None  # its bytes on the device
    lift_L: Optional[torch.Tensor] = None  # the crop at the edit's size uint8 [height, width, 3] as the VAE got it, where the passes run: kept for boxlift.py
    lift_M: Optional[torch.Tensor] = None  # the edit's region mask uint8 [height, width] beside it: the weight plane of the mask-aware fit (rimlift.py)

    @classmethod
    def make(cls, image, report: dict, mask: torch.Tensor, device=None, paste_image=None, uploaded=None) -> "FocusPlan":
        """mask: uint8 [SH, SW] where it lies.  device: set for the device passes - the photo is uploaded once (uploaded = (the photo's
        bytes, the paste source's) when they are up there already) and a host mask goes with it; None: PIL on the host."""
        from . import image_io
        p = cls(image, report, paste_image=paste_image)
        if mask.is_cuda:
            p.mask_dev = mask
        else:
            p.mask_u8 = mask
        if device is not None:
            p.src_u8, p.paste_u8 = uploaded if uploaded is not None else (image_io.upload_rgb(image, device), None)
            if p.mask_dev is None:
                p.mask_dev = mask.to(device)
        return p

    @property
    def box(self) -> Box:
        return self.report["box"]

    def host_mask(self) -> torch.Tensor:
        """The mask on the host: a mask that was made on the device is copied once, when somebody asks."""
        if self.mask_u8 is None:
            self.mask_u8 = self.mask_dev.cpu()
        return self.mask_u8


def setup(image, masks, height: int, width: int, context: float, output_type, device=None) -> List[FocusPlan]:
    """Per image of a focused call its FocusPlan (device as in `FocusPlan.make`), or the refusals of `enable_region_focus`."""
    from . import image_io
    imgs = image_io._pil_list(image) if image is not None else None
    if imgs is None:
        raise ValueError("region focus needs PIL input (one image or a list): an array or tensor `image` has no full-resolution bytes to "
                         "paste the edit back into - pass PIL images, or disable_region_focus()")
    if output_type in ("np", "pt") and len({im.size for im in imgs}) > 1:
        raise ValueError(f"region focus returns frames of the sources' sizes {[im.size for im in imgs]}: output_type={output_type!r} "
                         'needs sources of one size, use "pil"')
    return [FocusPlan.make(im, *_plan(im.size, m, height, width, context), device) for im, m in zip(imgs, masks_for(masks, len(imgs)))]


def inputs(plans: List[FocusPlan], height: int, width: int, device, keep_L: bool = False):
    """(img bf16 [n, 3, height, width] as preprocessing leaves it, the edit-size region masks uint8 [height, width] on the device) of
    the crops: the device passes, or PIL itself (`host_inputs`).  keep_L: every plan keeps the resized crop's bytes and the edit-size mask (`lift_L`,
    `lift_M`: the detail lift inside the box works from them) - on the host the crop is then resized here, once, and preprocessing takes it as it is."""
    from . import image_io, ops
    if plans[0].src_u8 is not None:
        img = torch.empty((len(plans), 3, height, width), dtype=torch.bfloat16, device=device)
        masks = []
        for j, p in enumerate(plans):
            crop, m = device_inputs(p.src_u8, p.mask_dev, p.box, width, height)
            ops.image_u8_lut_planar(crop, image_io.vae_lut(torch.device(device)), img[j])
            masks.append(m)
            if keep_L:
                p.lift_L, p.lift_M = crop, m
        return img, masks
    host = [host_inputs(p.image, p.host_mask(), p.box, width, height) for p in plans]
    if keep_L:
        import numpy as np
        from PIL import Image
        host = [(c.resize((int(width), int(height)), Image.LANCZOS), m) for c, m in host]
        for p, (c, m) in zip(plans, host):
            p.lift_L, p.lift_M = torch.from_numpy(np.array(c, dtype=np.uint8)), m
    img = image_io.preprocess_image([c for c, _ in host], height, width).to(device=device, dtype=torch.bfloat16)
    return img, [m.to(device) for _, m in host]


def paste(video: torch.Tensor, plans: List[FocusPlan], image_of, output_type: str, composite: bool, lift=None, report: Optional[list] = None,
          mask_aware: bool = False):
    """The source-size paste-back of every sample's frames (reasoning frames included), in postprocess_video's layouts: through the mask
    (composite), or the whole box.  A plan with a second source is pasted into that one.  lift: a lift.LiftConfig - every sample is lifted
    inside its box from its plan's `lift_L` before the paste (boxlift.output), and `report` receives one `lift_report` entry per sample;
    mask_aware: the fit runs under the plan's `lift_M` (boxlift.py)."""
    import numpy as np
    from . import image_io, ops
    image_io.check_output_type(output_type)
    if lift is not None:
        from . import boxlift
        frames, entries = boxlift.output(video, plans, image_of, None, lift, output_type, composite, mask_aware)
        if report is not None:
            report.extend(entries)
        return frames
    on_device = plans[0].src_u8 is not None and image_io.device_video(video)
    u8 = ops.video_to_u8(video.contiguous()) if on_device else None
    out = []
    for b in range(video.shape[0]):
        p = plans[image_of(b)]
        if on_device:
            out.append(device_paste(u8[b], p.src_u8 if p.paste_u8 is None else p.paste_u8, p.mask_dev if composite else None, p.box).cpu().numpy())
        else:
            frames = image_io.postprocess_video(video[b:b + 1], "pil")[0]
            pasted = host_paste(p.image if p.paste_image is None else p.paste_image, frames, p.host_mask() if composite else None, p.box)
            out.append(np.stack([np.asarray(f, dtype=np.uint8) for f in pasted]))
    return image_io.frames_from_u8(out, output_type)
