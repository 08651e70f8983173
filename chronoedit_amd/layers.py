"""Sketch edits from the editor's layers: the strokes are where a layer's alpha says the user drew, and a layer can carry its own prompt.

An image editor (gradio's `ImageEditor`) hands over {"background", "layers", "composite"}.  The sketch chain (chronoedit_amd/sketch.py) finds
the strokes as "where the composite differs from the background": a black stroke on a dark part of the photo changes no byte and is not
found, and a composite that went through a lossy codec differs everywhere.  The layers are RGBA and their alpha is non-zero only under the
brush.  With `enable_sketch_region(strokes="layers")`:

    strokes    changed = 255 where max over the layers of alpha > alpha_threshold, else 0, uint8 [SH, SW] - PIL's
               `layer.getchannel("A").point(lambda v: 255 if v > alpha_threshold else 0)`, combined by `ImageChops.lighter` over the layers.
               Everything behind `changed` is sketch.py's chain, unchanged
    composite  canvas = background.convert("RGB"); per layer in order canvas = Image.alpha_composite(canvas.convert("RGBA"), layer)
               .convert("RGB").  Over an opaque canvas that is, per channel and with the layer's (s, a) over the canvas's d,
                   u = s * a + d * (255 - a) + 128;  d = ((u >> 8) + u) >> 8
               (the output alpha is 255, `convert("RGB")` keeps the bytes) - PIL's paste with the alpha as the mask: focus.host_paste's
               arithmetic.  Built when the value carries no "composite", and per layer for a prompt per layer
    upload     a layer reaches the device as its alpha bounding box only (`layer.getbbox()`, which looks at the alpha alone for RGBA):
               uint8 [bh, bw, 4] at (left, top); outside it the alpha is 0 by construction, a layer without a box is skipped

The functions below are THE definition (torch on CPU tensors) and the host path; for CUDA tensors `strokes` and `over` are the passes of
csrc/ce_layers.hip - integers only, the same bits."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .focus import Box

ENTRY_POINTS = ("ce_layers_strokes_u8", "ce_layers_over_u8")
STROKES = ("difference", "layers")


def check_strokes(v) -> str:
    if not isinstance(v, str) or v not in STROKES:
        raise ValueError(f'sketch region: strokes must be "difference" or "layers", got {v!r}')
    return v


def check_alpha_threshold(v) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 254:
        raise ValueError(f"sketch region: alpha_threshold must be an int in 0..254, got {v!r}")
    return v


# ---- the editor's value ---------------------------------------------------------------------------------------------------------------
def editor_layers(value: dict, i: int = 0, layers=None) -> list:
    """The "layers" of editor value i (or `layers`, when given) -> a list of RGBA PIL images of the background's size.  A missing entry,
    one that is no list, a member that is no PIL image, whose mode has no alpha channel or whose size is not the background's: ValueError."""
    from .image_io import _is_pil
    ls = value.get("layers") if layers is None else layers
    if not isinstance(ls, (list, tuple)):
        raise ValueError(f'sketch region: strokes="layers" needs a list of PIL images under "layers" of the editor value {i} (got '
                         f"{type(ls).__name__}; the value has the keys {sorted(map(str, value))})")
    bg = value.get("background")
    out = []
    for k, layer in enumerate(ls):
        if not _is_pil(layer):
            raise ValueError(f'sketch region: layer {k} of the editor value {i} must be a PIL image, got {type(layer)}')
        if layer.mode[-1:] not in ("A", "a"):
            raise ValueError(f'sketch region: layer {k} of the editor value {i} has mode "{layer.mode}", which has no alpha channel: the strokes '
                             "are read from the alpha")
        if bg is not None and layer.size != bg.size:
            raise ValueError(f'sketch region: layer {k} {layer.size} and "background" {bg.size} of the editor value {i} differ in size')
        out.append(layer if layer.mode == "RGBA" else layer.convert("RGBA"))
    return out


@dataclass
class LayerBox:
    """One layer with strokes, as it travels: its alpha bounding box and the bytes inside it."""
    index: int  # the layer's place in the editor's list
    box: Box  # (left, top, right, bottom) = layer.getbbox()
    rgba: torch.Tensor  # uint8 [bh, bw, 4], on the host or on the device


def boxes(layers: Sequence) -> List[LayerBox]:
    """The layers (RGBA PIL images) that have an alpha bounding box, in order, each cut to it, on the host.  The boxes are host data."""
    out = []
    for k, layer in enumerate(layers):
        box = layer.getbbox()
        if box is None:
            continue
        out.append(LayerBox(k, tuple(int(v) for v in box), torch.from_numpy(np.array(layer.crop(box), dtype=np.uint8))))
    return out


# ---- the two passes: the device pass for tensors on the GPU, the torch expression for ones on the CPU - the same bits --------------------
def strokes(lbs: Sequence[LayerBox], size: Tuple[int, int], alpha_threshold: int = 0, device=None) -> torch.Tensor:
    """-> changed uint8 [SH, SW] for a photo of size = (SW, SH): 255 where some layer's alpha > alpha_threshold, else 0 - on `device` (one
    memset and one launch per layer), or on the host."""
    check_alpha_threshold(alpha_threshold)
    SW, SH = int(size[0]), int(size[1])
    plane = torch.zeros((SH, SW), dtype=torch.uint8, device=device)
    for lb in lbs:
        l, t, r, b = lb.box
        if plane.is_cuda:
            from . import ops
            ops.layers_strokes_u8(lb.rgba, l, t, plane, alpha_threshold)
        else:
            plane[t:b, l:r][lb.rgba[:, :, 3] > alpha_threshold] = 255
    return plane


def over(canvas: torch.Tensor, lb: LayerBox) -> torch.Tensor:
    """Image.alpha_composite(canvas, layer) IN PLACE: canvas uint8 [SH, SW, 3] where the layer's bytes lie -> canvas."""
    l, t, r, b = lb.box
    if canvas.is_cuda:
        from . import ops
        return ops.layers_over_u8(lb.rgba, l, t, canvas)
    d = canvas[t:b, l:r].to(torch.int32)
    s, a = lb.rgba[:, :, :3].to(torch.int32), lb.rgba[:, :, 3:].to(torch.int32)
    u = s * a + d * (255 - a) + 128
    canvas[t:b, l:r] = (((u >> 8) + u) >> 8).to(torch.uint8)
    return canvas


def composite_u8(background_u8: torch.Tensor, lbs: Sequence[LayerBox]) -> torch.Tensor:
    """The layers over the background, in order -> a new uint8 [SH, SW, 3] where background_u8 lies."""
    canvas = background_u8.clone()
    for lb in lbs:
        over(canvas, lb)
    return canvas


def composite(background, lbs: Sequence[LayerBox]):
    """THE composite of an editor value as a PIL image, by the host form (lbs = `boxes(layers)`, on the host): PIL's chained
    `alpha_composite`, byte for byte (tests/test_layers_cpu.py)."""
    from PIL import Image
    return Image.fromarray(composite_u8(torch.from_numpy(np.array(background.convert("RGB"), dtype=np.uint8)), lbs).numpy(), mode="RGB")


def uploaded(lbs: Sequence[LayerBox], device) -> List[LayerBox]:
    """Host boxes -> the same on `device` (None: as they are): the one upload per layer, of its box only."""
    return list(lbs) if device is None else [LayerBox(lb.index, lb.box, lb.rgba.to(device)) for lb in lbs]
