"""Sketch edits: the user draws on the photo, the region of the edit is where the drawing is.

An image editor (gradio's `ImageEditor`, the reference's scripts/gradio_paintbrush.py) hands over {"background", "layers", "composite"}:
the photo, and the photo with the strokes on it.  With `ChronoEditPipeline.enable_sketch_region` one call is

    mask      at the PHOTO's size, before the first step: changed -> grown -> feathered (`reference` below is the definition)
                changed  255 where max over the channels of |composite - background| > threshold, else 0
                grown    the square maximum filter of radius R = grow + feather, the window clipped to the image
                mask     the box mean of radius feather, horizontal then vertical over the rounded bytes, edges replicated; per axis, with
                         n = 2 feather + 1 and ww = 2^24 // n:  out = (window sum * ww + 2^23) >> 24
              which is ImageChops.difference -> the bands' maximum -> point(v > threshold) -> MaxFilter(2 R + 1) -> BoxBlur(feather) of PIL,
              byte for byte (tests/test_sketch_cpu.py) - without MaxFilter's cost, which is quadratic in the window
    focused   the explicit-mask focused region edit (chronoedit_amd/focus.py) with that mask: the crop the model sees is the COMPOSITE's (it
              must see the sketch), the frames are pasted into the BACKGROUND (the strokes do not come back where the mask keeps the photo)

What follows from the arithmetic: every pixel within `grow` (Chebyshev distance) of a changed pixel is 255 exactly, every pixel farther
than grow + 2 feather from all of them is 0, and with threshold = 0 composite and background carry the same bytes wherever the mask is below
255.  All integers: the device passes (csrc/ce_sketch.hip) give `reference`'s bits.  What the paint-brush LoRA makes of a sketch inside a
crop is the checkpoint's business.

With `min_stroke` the chain drops speckle (chronoedit_amd/components.py) between the two filters:

    changed -> grown -> the 8-connected components of GROWN, each weighted by its CHANGED pixels -> kept -> box mean

A component of the grown plane is a CLUSTER of strokes that lie within 2 R of each other; clusters with fewer changed pixels than
`min_stroke` (an int), or than that fraction of the heaviest cluster (a float), leave the grown plane before the box mean.  Dotted or
hatched strokes are many tiny components of `changed` but one cluster; a speck beside a stroke lies inside the region anyway; a speck far
from every stroke is a cluster of its own with next to no weight, and goes.  The guarantees above then speak of the changed pixels of KEPT
clusters, and "composite and background agree wherever the mask is below 255" holds outside the dropped clusters: the frames are pasted
into the background, so a dropped speck does not come back.

With `strokes="layers"` the `changed` plane is not the difference but the editor's layers' alpha above `alpha_threshold`, and a value
without a composite gets one built from background + layers (chronoedit_amd/layers.py); every chain below takes such a plane as
`changed_plane`, and everything behind `changed` is as above."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import components as _cc
from .focus import _ceil, focus_box

ENTRY_POINTS = ("ce_sketch_changed_u8", "ce_sketch_dilate_u8", "ce_sketch_box_u8")
MAX_GROWN, MAX_FEATHER = 4096, 1024  # the largest grow + feather and feather, in pixels (the passes' LDS and their 32-bit sums are sized for them)


def _length(v, name: str):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"sketch region: {name} must be an int (pixels) or a float in [0, 1) (a fraction of the photo's longer side), got {v!r}")
    if isinstance(v, int):
        if v < 0:
            raise ValueError(f"sketch region: {name} must be >= 0, got {v}")
        return v
    if not (0.0 <= v < 1.0):  # (a NaN fails the comparison)
        raise ValueError(f"sketch region: {name} as a float must lie in [0, 1), got {v!r}")
    return float(v)


@dataclass(frozen=True)
class SketchConfig:
    """grow, feather: an int is pixels of the photo, a float in [0, 1) that fraction of the photo's longer side (`pixels`).  threshold: a
    pixel counts as drawn on when a channel differs by MORE than this (0..254).  context, composite: `enable_region_focus`'s and
    `set_edit_region`'s.  The defaults are choices, not measurements: a margin of 2 % of the photo around the strokes belongs to the
    model, a further 1 % (twice: the box mean spreads over 2 feather) fades into the photo, and a lossless editor changes no byte it was
    not asked to (a front end that re-encodes its composite needs a threshold above its codec's error).  min_stroke: 0 is off; an int >= 1
    is the least number of changed pixels a cluster of strokes must hold, a float in (0, 1) that fraction of the heaviest cluster's.
    max_crops: 1 is one box around every kept stroke; 2..16: up to that many crops, one per group of clusters (chronoedit_amd/clusters.py).
    strokes: "difference" finds the strokes where composite and background differ; "layers" where a layer's alpha is greater than
    alpha_threshold (0..254; chronoedit_amd/layers.py).  layer_prompts: one prompt per layer (strokes="layers" only)."""
    grow: Union[int, float] = 0.02
    feather: Union[int, float] = 0.01
    threshold: int = 0
    context: float = 0.25
    composite: bool = True
    min_stroke: Union[int, float] = 0
    max_crops: int = 1
    strokes: str = "difference"
    alpha_threshold: int = 0
    layer_prompts: bool = False

    def __post_init__(self):
        object.__setattr__(self, "grow", _length(self.grow, "grow"))
        object.__setattr__(self, "feather", _length(self.feather, "feather"))
        if isinstance(self.threshold, bool) or not isinstance(self.threshold, int) or not 0 <= self.threshold <= 254:
            raise ValueError(f"sketch region: threshold must be an int in 0..254, got {self.threshold!r}")
        focus_box(None, (1, 1), (1, 1), self.context)  # (validates the context)
        if not isinstance(self.composite, bool):
            raise ValueError(f"sketch region: composite must be a bool, got {self.composite!r}")
        object.__setattr__(self, "min_stroke", _cc.check_min_weight(self.min_stroke, "sketch region: min_stroke", zero_is_off=True))
        from .clusters import check_max_crops
        check_max_crops(self.max_crops)
        from .layers import check_alpha_threshold, check_strokes
        check_strokes(self.strokes), check_alpha_threshold(self.alpha_threshold)
        if not isinstance(self.layer_prompts, bool):
            raise ValueError(f"sketch region: layer_prompts must be a bool, got {self.layer_prompts!r}")
        if self.layer_prompts and self.strokes != "layers":
            raise ValueError('sketch region: layer_prompts=True needs strokes="layers": a prompt per layer has no meaning for strokes found by difference')
        _check_pixels(self.grow if isinstance(self.grow, int) else 0, self.feather if isinstance(self.feather, int) else 0)  # (fractions: at the call)

    def pixels(self, src_size: Tuple[int, int]) -> Tuple[int, int]:
        """(grow, feather) in pixels for a photo of src_size = (SW, SH)."""
        g, f = pixels(self.grow, src_size), pixels(self.feather, src_size)
        _check_pixels(g, f)
        return g, f


def _check_pixels(grow: int, feather: int):
    if grow < 0 or feather < 0 or grow + feather > MAX_GROWN or feather > MAX_FEATHER:
        raise ValueError(f"sketch region: need 0 <= grow, 0 <= feather <= {MAX_FEATHER} and grow + feather <= {MAX_GROWN} pixels, got grow "
                         f"{grow} and feather {feather}")


def pixels(v, src_size: Tuple[int, int]) -> int:
    """An int is pixels; a float in [0, 1) is ceil(that fraction * the photo's longer side), the fraction read as the nearest one with a
    denominator <= 65536 (0.02 is 1 / 50: 0.02 of 4032 is 81), the idiom of `focus.focus_box`."""
    v = _length(v, "a length")
    if isinstance(v, int):
        return v
    return _ceil(Fraction(v).limit_denominator(1 << 16) * max(int(src_size[0]), int(src_size[1])))


# ---- the editor's value -------------------------------------------------------------------------------------------------------------
def is_editor_value(image) -> bool:
    """A dict, or a non-empty list / tuple of dicts: what `__call__(image=...)` takes as an image editor's value(s)."""
    if isinstance(image, dict):
        return True
    return isinstance(image, (list, tuple)) and len(image) > 0 and all(isinstance(v, dict) for v in image)


def editor_images(value, need_composite: bool = True) -> Tuple[list, list]:
    """One editor value or a list of them -> (backgrounds, composites), PIL images; keys other than "background" and "composite" (such as
    "layers") are ignored.  A missing or None entry, an entry that is no PIL image, or two sizes in one value are a ValueError.
    need_composite False (strokes="layers", where it can be built): a missing or None "composite" comes back as None."""
    from .image_io import _is_pil
    values = [value] if isinstance(value, dict) else list(value)
    bgs, cps = [], []
    for i, v in enumerate(values):
        for key in ("background", "composite"):
            if v.get(key) is None:
                if key == "composite" and not need_composite:
                    continue
                raise ValueError(f'sketch region: the editor value {i} has no "{key}" (got the keys {sorted(map(str, v))}): it needs PIL images '
                                 'under "background" and "composite"')
            if not _is_pil(v[key]):
                raise ValueError(f'sketch region: "{key}" of the editor value {i} must be a PIL image, got {type(v[key])}')
        if v.get("composite") is not None and v["background"].size != v["composite"].size:
            raise ValueError(f'sketch region: "background" {v["background"].size} and "composite" {v["composite"].size} of the editor value {i} '
                             "differ in size")
        bgs.append(v["background"]), cps.append(v.get("composite"))
    return bgs, cps


def rgb_bytes(image) -> torch.Tensor:
    """A PIL image (`convert("RGB")`), or a uint8 [SH, SW, 3] array / tensor -> a uint8 [SH, SW, 3] tensor where it lies."""
    if isinstance(image, torch.Tensor):
        t = image
    elif isinstance(image, np.ndarray):
        t = torch.from_numpy(image)
    else:
        t = torch.from_numpy(np.array(image.convert("RGB"), dtype=np.uint8))
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.numel() == 0:
        raise ValueError(f"sketch: need RGB bytes uint8 [SH, SW, 3], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


# ---- the stages: the device pass for a tensor on the GPU, the torch expression for one on the CPU - the same bits ---------------------
def changed(background: torch.Tensor, composite: torch.Tensor, threshold: int = 0) -> torch.Tensor:
    """Two uint8 [SH, SW, 3] -> uint8 [SH, SW]: 255 where max over the channels of |composite - background| > threshold, else 0."""
    if background.shape != composite.shape:
        raise ValueError(f"sketch: background {tuple(background.shape[:2])} and composite {tuple(composite.shape[:2])} differ in size")
    if background.is_cuda:
        from . import ops
        return ops.sketch_changed_u8(background, composite, threshold)
    d = (composite.to(torch.int16) - background.to(torch.int16)).abs().amax(dim=2)
    return (d > int(threshold)).to(torch.uint8) * 255


def _window_sums(x: torch.Tensor, r: int, axis: int, replicate: bool) -> torch.Tensor:
    """int32 [H, W] -> the sums over [i - r, i + r] along `axis` (0: horizontal), the line continued by its edge values (replicate) or by
    zeros: one running sum, whatever the radius."""
    x = x if axis == 0 else x.t().contiguous()
    n = x.shape[1]
    if replicate:
        idx = torch.arange(-r, n + r).clamp_(0, n - 1)
        line = x.index_select(1, idx)
    else:
        line = torch.nn.functional.pad(x, (r, r))
    c = torch.nn.functional.pad(line.cumsum(1, dtype=torch.int64), (1, 0))
    s = c[:, 2 * r + 1:] - c[:, :n]
    return s if axis == 0 else s.t().contiguous()


def dilate(plane: torch.Tensor, radius: int, axis: int) -> torch.Tensor:
    """One axis (0: horizontal, 1: vertical) of the maximum filter of a 0 / 255 plane uint8 [SH, SW], window [i - radius, i + radius]
    clipped to the image: 255 where the window holds a non-zero byte, else 0 - a new tensor."""
    _check_pixels(int(radius), 0)
    if plane.is_cuda:
        from . import ops
        return ops.sketch_dilate_u8(plane, axis, int(radius))
    return (_window_sums((plane != 0).to(torch.int32), int(radius), axis, False) > 0).to(torch.uint8) * 255


def box(plane: torch.Tensor, radius: int, axis: int) -> torch.Tensor:
    """One axis of the box mean of uint8 [SH, SW], window [i - radius, i + radius] over the edge-replicated line:
    out = (sum * (2^24 // (2 radius + 1)) + 2^23) >> 24 - a new tensor."""
    _check_pixels(0, int(radius))
    if plane.is_cuda:
        from . import ops
        return ops.sketch_box_u8(plane, axis, int(radius))
    ww = (1 << 24) // (2 * int(radius) + 1)
    return ((_window_sums(plane.to(torch.int32), int(radius), axis, True) * ww + (1 << 23)) >> 24).to(torch.uint8)


def _grown(background, composite, grow: int, feather: int, threshold, changed_plane: Optional[torch.Tensor] = None):
    """The checks, then (changed, grown) where the images lie: what every chain below starts with.  changed_plane: the `changed` plane
    itself, uint8 [SH, SW] of 0 / 255 where the chain is to run (layers.strokes) - the two images are then not looked at."""
    _check_pixels(grow, feather)
    if isinstance(threshold, bool) or not 0 <= int(threshold) <= 254:
        raise ValueError(f"sketch: threshold must be an int in 0..254, got {threshold!r}")
    if changed_plane is not None:
        if changed_plane.dtype != torch.uint8 or changed_plane.dim() != 2 or changed_plane.numel() == 0:
            raise ValueError(f"sketch: need a changed plane uint8 [SH, SW], got {changed_plane.dtype} {tuple(changed_plane.shape)}")
        ch = changed_plane.contiguous()
    else:
        ch = changed(rgb_bytes(background), rgb_bytes(composite), int(threshold))
    if grow + feather:
        return ch, dilate(dilate(ch, grow + feather, 0), grow + feather, 1)
    return ch, ch


def _feathered(plane: torch.Tensor, feather: int) -> torch.Tensor:
    return box(box(plane, feather, 0), feather, 1) if feather else plane


def stages(background, composite, grow: int, feather: int, threshold: int = 0, changed_plane=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(changed, grown, mask), uint8 [SH, SW] each, where the images lie (two PIL images: on the host).  grow, feather in pixels.  A radius
    of 0 runs no pass: with grow = feather = 0 the three are one tensor.  changed_plane: `_grown`'s, here and in the chains below."""
    grow, feather = int(grow), int(feather)
    ch, grown = _grown(background, composite, grow, feather, threshold, changed_plane)
    return ch, grown, _feathered(grown, feather)


def filtered_stages(background, composite, grow: int, feather: int, threshold: int = 0, min_stroke=1, scratch=None, changed_plane=None):
    """`stages` with the speckle filter between the two filters -> (changed, grown, kept, mask, stats): kept = the grown plane without the
    clusters that hold fewer changed pixels than min_stroke (components.filter of grown, weighted by changed), mask its box mean, stats
    int32 [4] = (clusters kept, clusters dropped, changed pixels dropped, the heaviest cluster's changed pixels) where the images lie -
    nothing is read back.  scratch: components.filter's, on the device."""
    grow, feather = int(grow), int(feather)
    ch, grown = _grown(background, composite, grow, feather, threshold, changed_plane)
    kept, stats = _cc.filter(grown, min_stroke, ch, scratch)
    return ch, grown, kept, _feathered(kept, feather), stats


def labelled_stages(background, composite, grow: int, feather: int, threshold: int = 0, min_stroke=0, changed_plane=None):
    """`filtered_stages` that keeps its label planes, and labels with min_stroke == 0 too (kept = grown then, stats None) -> (changed, grown,
    roots, sums, kept, mask, stats): what chronoedit_amd/clusters.py builds its table from.  The mask is `mask`'s, bit for bit."""
    grow, feather = int(grow), int(feather)
    ch, grown = _grown(background, composite, grow, feather, threshold, changed_plane)
    roots = _cc.roots(grown)
    sums = _cc.sums(roots, ch)
    kept, stats = _cc.keep(grown, roots, sums, min_stroke) if min_stroke else (grown, None)
    return ch, grown, roots, sums, kept, _feathered(kept, feather), stats


def reference(background, composite, grow: int, feather: int, threshold: int = 0, min_stroke=0) -> torch.Tensor:
    """THE definition, and the host path: two images (PIL, or uint8 [SH, SW, 3]) -> the mask uint8 [SH, SW] on the host.  grow, feather in
    pixels of the photo."""
    bg, cp = rgb_bytes(background).cpu(), rgb_bytes(composite).cpu()
    if min_stroke:
        return filtered_stages(bg, cp, grow, feather, threshold, min_stroke)[3]
    return stages(bg, cp, grow, feather, threshold)[2]


def mask(background: torch.Tensor, composite: torch.Tensor, grow: int, feather: int, threshold: int = 0, min_stroke=0) -> torch.Tensor:
    """`reference` where the bytes lie: uint8 [SH, SW, 3] twice, on the GPU (five launches at most - eleven and two memsets with min_stroke -, no host
    read) or on the host."""
    if min_stroke:
        return filtered_stages(background, composite, grow, feather, threshold, min_stroke)[3]
    return stages(background, composite, grow, feather, threshold)[2]


# ---- the masks of one call ---------------------------------------------------------------------------------------------------------
def masks(cfg: SketchConfig, bgs, cps, device=None, layers=None) -> list:
    """Per editor value {"background", "composite", "mask_u8" (host; None on the device path: `host_mask` copies it when the edit is done),
    "grow_px", "feather_px", "bbox" (None: no strokes), "mask_pixels", "changed_pixels"} and, on the device path (device set), "bg_u8",
    "cp_u8", "mask_dev": each image uploaded once, two reductions and ONE read of their ten integers per value - nothing else comes back.
    With cfg.min_stroke the mask is the filtered chain's, the entry also holds "clusters", "dropped_clusters" and "dropped_pixels", and the
    filter's four counters come back in the same read: fourteen integers ("changed_pixels" still counts every changed pixel).
    With cfg.max_crops >= 2 the labelling runs whatever min_stroke is (`labelled_stages`: the same mask), and the cluster table rides on that
    read: the entry also holds "count" (kept clusters, exact), "rows" (the table on the host, a list of clusters.ROWS rows) and the planes
    "roots", "kept" and "table" where they lie, for clusters.plan.
    With cfg.strokes == "layers" (layers: per value its RGBA PIL layers, layers.editor_layers) `changed` is the layers' alpha above
    cfg.alpha_threshold (one launch per layer with a box, on the layer's box), the read is the same read, and a composite of None is
    built from background + layers (the entry then holds "built": True, and "composite" is the built PIL image)."""
    from . import image_io
    from . import layers as _ly
    out = []
    for i, (bg, cp) in enumerate(zip(bgs, cps)):
        e = {"background": bg, "composite": cp}
        ch = None
        if cfg.strokes == "layers":
            # the strokes from the layers' alpha; the composite, when the value has none, from background + layers: each layer's box
            # is uploaded once and serves both passes.  The host's copy of a built composite (CLIP's crop is PIL's, and the report
            # shows it) is made by the host form: no read
            if layers is None:
                raise ValueError('sketch: strokes="layers" needs the layers of every editor value')
            host = _ly.boxes(layers[i])
            lbs = _ly.uploaded(host, device)
            ch = _ly.strokes(lbs, bg.size, cfg.alpha_threshold, device)
            if device is not None:
                e["bg_u8"] = image_io.upload_rgb(bg, device)
                e["cp_u8"] = _ly.composite_u8(e["bg_u8"], lbs) if cp is None else image_io.upload_rgb(cp, device)
            if cp is None:
                e["composite"], e["built"] = _ly.composite(bg, host), True
        elif device is not None:
            e["bg_u8"], e["cp_u8"] = image_io.upload_rgb(bg, device), image_io.upload_rgb(cp, device)
        out.append(_entry(cfg, e, ch))
    return out


def layer_entries(cfg: SketchConfig, bg, layers: list, device=None, host=None) -> list:
    """One editor value under `layer_prompts`: per layer None (no stroke) or the `masks` entry of (background, composite_k = layer k alone
    over the background, changed_k = layer k's alpha), plus "layer": k - the background uploaded once, ONE read per layer with strokes.
    host: the layers' boxes (layers.boxes, or those of them worth planning) when the caller has them already."""
    from PIL import Image
    from . import layers as _ly
    bg_host = rgb_bytes(bg)  # (converted once: every layer's host composite starts from it)
    bg_u8 = bg_host.to(device) if device is not None else None
    out = [None] * len(layers)
    for lb in _ly.boxes(layers) if host is None else host:
        mine = _ly.uploaded([lb], device)
        e = {"background": bg, "composite": Image.fromarray(_ly.composite_u8(bg_host, [lb]).numpy(), mode="RGB"), "built": True, "layer": lb.index}
        if device is not None:
            e["bg_u8"], e["cp_u8"] = bg_u8, _ly.composite_u8(bg_u8, mine)
        e = _entry(cfg, e, _ly.strokes(mine, bg.size, cfg.alpha_threshold, device))
        out[lb.index] = e if e["bbox"] is not None else None  # (a box whose alpha stays at or below the threshold: no stroke either)
    return out


def _entry(cfg: SketchConfig, e: dict, ch: Optional[torch.Tensor]) -> dict:
    """The chain and the one read of one `masks` entry that holds its images (and their uploads: the device path).  ch: the changed plane
    where the chain runs (strokes from layers), or None: by difference."""
    from . import autofocus as _af
    from . import clusters as _cl
    bg = e["background"]
    g, f = cfg.pixels(bg.size)
    e.update(grow_px=g, feather_px=f)
    on_device = "bg_u8" in e
    planes = (e["bg_u8"], e["cp_u8"]) if on_device else (bg, e["composite"])
    stats, table = None, []
    if cfg.max_crops >= 2:
        ch, _, e["roots"], sm, e["kept"], m, stats = labelled_stages(*planes, g, f, cfg.threshold, cfg.min_stroke, ch)
        count, e["table"] = _cl.table(e["roots"], sm, e["kept"])
        table = [count, e["table"].reshape(-1)]
    elif cfg.min_stroke:
        ch, _, _, m, stats = filtered_stages(*planes, g, f, cfg.threshold, cfg.min_stroke, None, ch)
    else:
        ch, _, m = stages(*planes, g, f, cfg.threshold, ch)
    counts = torch.cat([_af.bbox_counts(m), _af.bbox_counts(ch)] + ([] if stats is None else [stats]) + table).tolist()  # the one read
    if on_device:
        e["mask_dev"], e["mask_u8"] = m, None
    else:
        e["mask_u8"] = m
    if table:
        n = len(counts) - 1 - 8 * _cl.ROWS
        e["count"], e["rows"] = int(counts[n]), [counts[n + 1 + 8 * i:n + 9 + 8 * i] for i in range(_cl.ROWS)]
    e["bbox"] = tuple(int(v) for v in counts[:4]) if counts[4] else None
    e["mask_pixels"], e["changed_pixels"] = int(counts[4]), int(counts[9])
    if cfg.min_stroke:
        e["clusters"], e["dropped_clusters"], e["dropped_pixels"] = int(counts[10]), int(counts[11]), int(counts[12])
    return e


def host_mask(e: dict) -> torch.Tensor:
    """The mask of one `masks` entry on the host: the device path's 12 MB copy, made once and behind the edit (an empty mask needs no
    copy)."""
    if e["mask_u8"] is None:
        e["mask_u8"] = e["mask_dev"].cpu() if e["bbox"] is not None else torch.zeros(tuple(e["mask_dev"].shape), dtype=torch.uint8)
    return e["mask_u8"]


def focus_plan(e: dict, width: int, height: int, context: float):
    """The focus.FocusPlan of one `masks` entry: the crop is the COMPOSITE's, the frames are pasted into the BACKGROUND."""
    from .focus import FocusPlan
    SW, SH = e["background"].size
    box, reason = focus_box(e["bbox"], (SW, SH), (width, height), context)
    l, t, r, b = box
    # (the box holds the mask's bounding box, so the mask's share of the box is its count over the box's area)
    report = {"box": box, "reason": reason, "source_size": (SW, SH), "edit_size": (int(width), int(height)), "scale": (r - l) / int(width),
              "mask_fraction_of_box": float(e["mask_pixels"]) / ((r - l) * (b - t))}
    if "mask_dev" not in e:
        return FocusPlan.make(e["composite"], report, e["mask_u8"], paste_image=e["background"])
    p = FocusPlan.make(e["composite"], report, e["mask_dev"], e["mask_dev"].device, e["background"], uploaded=(e["cp_u8"], e["bg_u8"]))
    if e["bbox"] is None:
        p.mask_u8 = host_mask(e)  # (no copy)
    return p
