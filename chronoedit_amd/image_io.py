"""Image pre- and post-processing on the device, bit-equal to the host path (PIL, numpy, the injected CLIPImageProcessor).

What `ChronoEditPipeline.__call__` does around the encoders and behind the VAE when it is handed PIL images and asked for PIL frames:

  preprocess_pil     VideoProcessor.preprocess: Lanczos resize, / 255, 2x - 1, bf16           (pipeline.preprocess_image on the host)
  clip_pixel_values  CLIPImageProcessor: bicubic resize of the shortest edge, centre crop,
                     rescale, normalise                                                       (the processor itself on the host)
  frames_to_pil      VideoProcessor.postprocess_video(..., "pil"): / 2 + 0.5, clamp, * 255,
                     round, uint8, channels last                                              (pipeline.postprocess_video on the host)

The arithmetic is integer or table driven.  PIL resamples 8-bit images in 22-bit fixed point with coefficients it derives in double
precision: `resize_tables` derives the same integers on the host (they depend on the two extents and the filter alone, and are cached on
the device), csrc/ce_image.hip runs the passes.  Everything behind the resize is a function of (channel, byte): a 3 x 256 table built by
the host path's own expressions - for CLIP by calling the processor itself on the 256 byte values - so the device result carries whatever
the installed numpy / transformers compute.  Only `Image.convert("RGB")` and `Image.fromarray` stay on the host.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import List, Optional, Tuple

import torch

from . import ops

LANCZOS, BICUBIC, BILINEAR = "lanczos", "bicubic", "bilinear"
PRECISION_BITS = 32 - 8 - 2  # PIL's Resample.c: coefficients of the 8-bit passes are fixed point with 22 fractional bits


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x: float) -> float:
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


_FILTERS = {LANCZOS: (_lanczos, 3.0), BICUBIC: (_bicubic, 2.0), BILINEAR: (_bilinear, 1.0)}


def resize_tables(in_len: int, out_len: int, filter: str) -> Tuple[List[List[int]], List[Tuple[int, int]], int]:
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for one axis: (coeff [out_len][ksize] as ints with 22 fractional bits,
    bounds [out_len] of (first, count), ksize).  Python floats and math.sin - the doubles and the libm PIL's C code uses - in PIL's
    order of operations (the argument of the filter is multiplied by 1 / filterscale, the weights are summed one by one)."""
    filt, base = _FILTERS[filter]
    scale = in_len / out_len
    fs = max(scale, 1.0)
    support = base * fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    one = float(1 << PRECISION_BITS)
    coeff, bounds = [], []
    for o in range(out_len):
        c = (o + 0.5) * scale
        first = max(int(c - support + 0.5), 0)
        count = min(int(c + support + 0.5), in_len) - first
        w = [filt((k + first - c + 0.5) * inv) for k in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        row = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        coeff.append(row + [0] * (ksize - count))
        bounds.append((first, count))
    return coeff, bounds, ksize


_TABLES: "OrderedDict" = OrderedDict()  # (in_len, out_len, filter, device) -> (coeff int32 [out, ksize], bounds int32 [out, 2]) on the device
_TABLES_MAX = 32


def _device_tables(in_len: int, out_len: int, filter: str, device: torch.device):
    key = (in_len, out_len, filter, str(device))
    hit = _TABLES.get(key)
    if hit is None:
        coeff, bounds, _ = resize_tables(in_len, out_len, filter)
        hit = (torch.tensor(coeff, dtype=torch.int32).to(device), torch.tensor(bounds, dtype=torch.int32).to(device))
        _TABLES[key] = hit
        while len(_TABLES) > _TABLES_MAX:
            _TABLES.popitem(last=False)
    else:
        _TABLES.move_to_end(key)
    return hit


def resize_u8(img_u8: torch.Tensor, size: Tuple[int, int], filter: str) -> torch.Tensor:
    """Image.resize((W2, H2), filter) of an RGB image held as uint8 [H, W, 3] on the device: the horizontal pass if the width changes,
    then the vertical pass - over the horizontal result rounded to uint8, PIL's order - if the height changes.  An unchanged axis launches
    nothing (an unchanged image is returned as it is)."""
    W2, H2 = int(size[0]), int(size[1])
    H, W, _ = img_u8.shape
    out = img_u8
    if W2 != W:
        out = ops.image_resample_u8(out, 0, *_device_tables(W, W2, filter, img_u8.device))
    if H2 != H:
        out = ops.image_resample_u8(out, 1, *_device_tables(H, H2, filter, img_u8.device))
    return out


def _is_pil(x) -> bool:
    try:
        from PIL import Image
    except ImportError:
        return False
    return isinstance(x, Image.Image)


def _pil_list(images) -> Optional[list]:
    imgs = list(images) if isinstance(images, (list, tuple)) else [images]
    return imgs if imgs and all(_is_pil(i) for i in imgs) else None


def on_device(enabled: bool, device) -> bool:
    """Do the image passes of this call run on the device?  `enable_device_image_io` is on and the pipeline lies on a GPU."""
    return bool(enabled) and torch.device(device).type == "cuda"


def device_video(video: torch.Tensor) -> bool:
    """A decoded video that `ops.video_to_u8` takes where it lies."""
    return video.is_cuda and video.dtype in (torch.bfloat16, torch.float32)


def upload_rgb(image, device) -> torch.Tensor:
    """A PIL image as uint8 [H, W, 3] on the device (`convert("RGB")` on the host, then the raw bytes)."""
    import numpy as np
    return torch.from_numpy(np.array(image.convert("RGB"), dtype=np.uint8)).to(device)


_VAE_LUT = {}  # device -> bf16 [3, 256]


def vae_table(device=None) -> torch.Tensor:
    """bf16 [3, 256]: what pipeline.preprocess_image(...).to(bfloat16) makes of each byte, by its own expressions."""
    import numpy as np
    x = torch.from_numpy(np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0)
    x = 2.0 * x - 1.0
    lut = x.to(torch.bfloat16)[None].repeat(3, 1).contiguous()
    return lut if device is None else lut.to(device)


def vae_lut(device) -> torch.Tensor:
    """vae_table on the device, made once per device."""
    lut = _VAE_LUT.get(str(device))
    if lut is None:
        lut = _VAE_LUT[str(device)] = vae_table(device)
    return lut


def preprocess_pil(images, height: int, width: int, device, keep: Optional[list] = None) -> torch.Tensor:
    """pipeline.preprocess_image(images, height, width).to(device, bfloat16) for a PIL image or a list of them: bf16 [B, 3, height, width].
    keep: a list that receives, per image, (the photo's bytes uint8 [SH, SW, 3], their Lanczos resize uint8 [height, width, 3]) as they lie
    on the device - what the detail lift (lift.py) works from, with no second upload."""
    imgs = _pil_list(images)
    if imgs is None:
        raise ValueError("preprocess_pil takes a PIL image or a list of PIL images")
    device = torch.device(device)
    lut = vae_lut(device)
    out = torch.empty((len(imgs), 3, height, width), dtype=torch.bfloat16, device=device)
    for b, im in enumerate(imgs):
        src = upload_rgb(im, device)
        small = resize_u8(src, (width, height), LANCZOS)
        ops.image_u8_lut_planar(small, lut, out[b])
        if keep is not None:
            keep.append((src, small))
    return out


def _field(d, key):
    if d is None:
        return None
    if isinstance(d, dict):
        return d.get(key)
    try:
        return d[key]
    except (KeyError, TypeError, IndexError, AttributeError):
        return getattr(d, key, None)


def clip_recipe(processor):
    """(shortest_edge, crop_h, crop_w, do_convert_rgb) when `processor` is a CLIPImageProcessor on its PIL backend that does exactly
    bicubic shortest-edge resize, centre crop, rescale, normalise; None otherwise."""
    name = type(processor).__name__
    if not name.startswith("CLIPImageProcessor") or name.endswith("Fast") or getattr(processor, "backend", "pil") != "pil":
        return None
    g = lambda k: getattr(processor, k, None)
    if not (g("do_resize") and g("do_center_crop") and g("do_rescale") and g("do_normalize")) or g("do_pad"):
        return None
    resample = g("resample")
    if resample is None or int(resample) != 3:  # PIL.Image.BICUBIC
        return None
    size, crop = g("size"), g("crop_size")
    s, ch, cw = _field(size, "shortest_edge"), _field(crop, "height"), _field(crop, "width")
    if not (s and ch and cw) or any(_field(size, k) for k in ("height", "width", "longest_edge", "max_height", "max_width")):
        return None
    return int(s), int(ch), int(cw), bool(g("do_convert_rgb"))


_CLIP_LUT: "OrderedDict" = OrderedDict()  # (rescale_factor, mean, std, device) -> fp32 [3, 256]


def clip_table(processor, device=None) -> Optional[torch.Tensor]:
    """fp32 [3, 256]: what the processor's rescale + normalise make of byte v in channel c - obtained by calling the processor, with the
    resize and the crop switched off, on a 16 x 16 image that holds all 256 values in every channel.  None if that call fails."""
    import numpy as np
    from PIL import Image
    try:
        key = (float(processor.rescale_factor), tuple(float(m) for m in processor.image_mean), tuple(float(s) for s in processor.image_std),
               str(device))
    except (AttributeError, TypeError, ValueError):
        return None
    hit = _CLIP_LUT.get(key)
    if hit is not None:
        return hit
    probe = Image.fromarray(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2))
    try:
        px = processor(images=probe, do_resize=False, do_center_crop=False, return_tensors="pt")["pixel_values"]
    except Exception:
        return None
    if not isinstance(px, torch.Tensor) or tuple(px.shape) != (1, 3, 16, 16) or px.dtype != torch.float32:
        return None
    lut = px[0].reshape(3, 256).contiguous()
    if device is not None:
        lut = lut.to(device)
    _CLIP_LUT[key] = lut
    while len(_CLIP_LUT) > 8:
        _CLIP_LUT.popitem(last=False)
    return lut


def clip_pixel_values(processor, images, device) -> Optional[torch.Tensor]:
    """processor(images=images, return_tensors="pt")["pixel_values"] on the device, fp32 [B, 3, crop_h, crop_w] - or None when the
    processor is not the plain CLIP recipe (see clip_recipe), the input is not PIL, or the crop would have to pad: the caller then runs
    the processor."""
    imgs = _pil_list(images)
    recipe = clip_recipe(processor) if imgs is not None else None
    if recipe is None:
        return None
    s, ch, cw, to_rgb = recipe
    if not to_rgb and any(im.mode != "RGB" for im in imgs):
        return None
    plans = []
    for im in imgs:
        w, h = im.size
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = s, int(s * long / short)  # transformers' get_resize_output_image_size(default_to_square=False)
        W2, H2 = (new_short, new_long) if w <= h else (new_long, new_short)
        if ch > H2 or cw > W2:
            return None
        plans.append((W2, H2))
    device = torch.device(device)
    lut = clip_table(processor, device)
    if lut is None:
        return None
    out = torch.empty((len(imgs), 3, ch, cw), dtype=torch.float32, device=device)
    for b, (im, (W2, H2)) in enumerate(zip(imgs, plans)):
        ops.image_u8_lut_planar(resize_u8(upload_rgb(im, device), (W2, H2), BICUBIC), lut, out[b], top=(H2 - ch) // 2, left=(W2 - cw) // 2)
    return out


def preprocess_image(image, height: int, width: int) -> torch.Tensor:
    """VideoProcessor.preprocess(image, height=, width=): PIL / array / tensor -> [B,3,height,width] in [-1, 1] (fp32, CPU or
    the tensor's device).  PIL images are resized with Lanczos, arrays / tensors with F.interpolate's default mode (nearest) - both as
    diffusers' VaeImageProcessor.resize does; arrays / tensors are taken as [0, 1] unless they already carry negative values
    (diffusers' own rule)."""
    import numpy as np
    if _is_pil(image) or (isinstance(image, (list, tuple)) and all(_is_pil(i) for i in image)):
        from PIL import Image
        imgs = list(image) if isinstance(image, (list, tuple)) else [image]
        arr = np.stack([np.asarray(i.convert("RGB").resize((width, height), Image.LANCZOS), dtype=np.float32) / 255.0 for i in imgs])
        x = torch.from_numpy(arr).permute(0, 3, 1, 2)
    elif isinstance(image, np.ndarray):
        x = torch.from_numpy(image.astype(np.float32))
        x = x[None] if x.dim() == 3 else x
        x = x.permute(0, 3, 1, 2)
    elif isinstance(image, torch.Tensor):
        x = image.float()
        x = x[None] if x.dim() == 3 else x
    else:
        raise ValueError(f"`image` has to be of type `torch.Tensor` or `PIL.Image.Image` but is {type(image)}")
    if x.shape[-2:] != (height, width):
        x = torch.nn.functional.interpolate(x, size=(height, width))  # arrays / tensors: F.interpolate's default (nearest), as diffusers' VaeImageProcessor.resize
    if x.min() >= 0:
        x = 2.0 * x - 1.0
    return x.contiguous()


def check_output_type(output_type):
    if output_type not in ("np", "pt", "pil"):
        raise ValueError(f"{output_type} does not exist. Please choose one of ['np', 'pt', 'pil']")


def postprocess_video(video: torch.Tensor, output_type: str = "np"):
    """VideoProcessor.postprocess_video: [B,3,F,H,W] in [-1,1] -> per sample F frames in [0,1]: "np" [B,F,H,W,3] float32,
    "pt" [B,F,3,H,W], "pil" list of lists of PIL images."""
    v = (video.float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 1, 3, 4)  # [B,F,3,H,W]
    if output_type == "pt":
        return v
    arr = v.permute(0, 1, 3, 4, 2).cpu().numpy()
    if output_type == "np":
        return arr
    check_output_type(output_type)
    from PIL import Image
    return [[Image.fromarray((f * 255).round().astype("uint8")) for f in sample] for sample in arr]


def frames_from_u8(samples, output_type: str):
    """Per sample the bytes uint8 [F, H, W, 3] (numpy, on the host) in postprocess_video's layouts: "pil" the frames themselves, "np" /
    "pt" the bytes / 255 (the samples must then share a size)."""
    import numpy as np
    if output_type == "pil":
        from PIL import Image
        return [[Image.fromarray(f) for f in sample] for sample in samples]
    arr = np.stack(samples).astype(np.float32) / 255.0  # [B, F, H, W, 3]
    return arr if output_type == "np" else torch.from_numpy(arr).permute(0, 1, 4, 2, 3)


def frames_to_pil(video: torch.Tensor):
    """pipeline.postprocess_video(video, "pil") for a bf16 / fp32 video [B, 3, F, H, W] on the device: one pass to uint8 [B, F, H, W, 3], one
    device-to-host copy of the bytes, Image.fromarray per frame."""
    return frames_from_u8(ops.video_to_u8(video.contiguous()).cpu().numpy(), "pil")
