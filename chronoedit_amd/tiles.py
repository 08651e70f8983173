"""Tiled edits: a whole photo at full size, denoised as overlapping model-size tiles whose latents are made to agree after every step
(MultiDiffusion: Bar-Tal et al. 2023).

With `ChronoEditPipeline.enable_tiled_edit` a call on ONE PIL image

    plan    the target (the photo's size, a given size or a scale of it) rounded up to multiples of 16 is the CANVAS; per axis the fewest
            tiles of the edit's width x height that cover it with at least `overlap` in common, at origins that are multiples of 16
            (`axis_origins`, `plan`: integers and exact rationals only)
    in      the target image, padded right and bottom by edge replication to the canvas, is cut into the tiles; each tile gets its own VAE
            condition and its CLIP row; ONE noise canvas is cut into the tiles' latents (ce_tiles_scatter_f32)
    step    the tiles are the samples of one batched pass; behind every scheduler update the tiles' latents are averaged on the canvas under
            separable integer tent weights (ce_tiles_fuse_f32) and every tile takes its cells back (ce_tiles_scatter_f32): `TileState.fuse`,
            two launches inside the captured step.  The scheduler's history stays per tile
    out     all tiles are decoded and converted to bytes, then blended under the same tents in pixels, in exact integers, straight into the
            target's frame (ce_tiles_blend_u8): the canvas cropped back to the target, no second resampling

`reference_fuse`, `reference_scatter` and `reference_blend` are the definitions, on the CPU, one torch op per rounded operation; the three
kernels of csrc/ce_tiles.hip give their bits.  Whether a checkpoint edits the tiles of one photo consistently is the checkpoint's business."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Sequence, Tuple

import torch

ENTRY_POINTS = ("ce_tiles_fuse_f32", "ce_tiles_scatter_f32", "ce_tiles_blend_u8")
MAX_TILES = 16  # the kernels' loops are bounded by it
STEP = 16  # origins, canvas sides and overlaps are multiples of it: 8 pixels per latent cell, 2 cells per token


def _ceil(q: Fraction) -> int:
    return -((-q.numerator) // q.denominator)


# ---- the plan: integers and exact rationals -------------------------------------------------------------------------------------
def overlap_px(overlap, tile_side: int) -> int:
    """The least overlap in pixels on an axis whose tile side is `tile_side`: a float in (0, 0.5] is that fraction of the side (read as the
    nearest fraction with a denominator <= 65536) rounded UP to a multiple of 16; an int is pixels, a multiple of 16.  Less than the side."""
    T = int(tile_side)
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float)):
        raise ValueError(f"tiled edit: overlap must be a float in (0, 0.5] or an int multiple of {STEP}, got {overlap!r}")
    if isinstance(overlap, int):
        v = overlap
        if v <= 0 or v % STEP:
            raise ValueError(f"tiled edit: an int overlap is pixels and must be a positive multiple of {STEP}, got {overlap}")
    else:
        if not (0.0 < overlap <= 0.5):  # (a NaN fails the comparison)
            raise ValueError(f"tiled edit: a float overlap must lie in (0, 0.5], got {overlap!r}")
        v = STEP * _ceil(Fraction(overlap).limit_denominator(1 << 16) * T / STEP)
    if v >= T:
        raise ValueError(f"tiled edit: the overlap of {v} px is not smaller than the tile's side of {T} px")
    return v


def axis_origins(C: int, T: int, v: int) -> Tuple[int, ...]:
    """Origins of the tiles of side T that cover a canvas side C with at least v (up to rounding to 16: at least v - 15) in common between
    neighbours: n = 1 if C == T else max(2, ceil((C - v) / (T - v))), o_i = 16 floor(i (C - T) / (16 (n - 1))).  C and T are multiples of
    16, C >= T > v >= 0.  o_0 = 0, o_last = C - T, strictly increasing, n minimal."""
    C, T, v = int(C), int(T), int(v)
    if C % STEP or T % STEP or T <= 0:
        raise ValueError(f"tiled edit: canvas side {C} and tile side {T} must be positive multiples of {STEP}")
    if C < T:
        raise ValueError(f"tiled edit: the canvas side of {C} px is smaller than the tile's side of {T} px: use the plain call, or a smaller tile")
    if not (0 <= v < T):
        raise ValueError(f"tiled edit: the overlap of {v} px must lie in [0, {T})")
    if C == T:
        return (0,)
    n = max(2, _ceil(Fraction(C - v, T - v)))
    return tuple(STEP * ((i * (C - T)) // (STEP * (n - 1))) for i in range(n))


def target_size(size, image_size: Tuple[int, int]) -> Tuple[int, int]:
    """`enable_tiled_edit(size=)` for a photo of image_size = (W, H) -> the target (W, H): None is the photo's size, (W, H) that size, a
    float > 0 that scale of the photo's size, rounded to integers."""
    W, H = int(image_size[0]), int(image_size[1])
    if size is None:
        return W, H
    if isinstance(size, (tuple, list)):
        if len(size) != 2 or any(isinstance(s, bool) or not isinstance(s, int) or s < 1 for s in size):
            raise ValueError(f"tiled edit: size must be None, (width, height) in positive integers or a scale > 0, got {size!r}")
        return int(size[0]), int(size[1])
    if isinstance(size, bool) or not isinstance(size, (int, float)) or not (0.0 < float(size) < math.inf):
        raise ValueError(f"tiled edit: size must be None, (width, height) in positive integers or a scale > 0, got {size!r}")
    s = Fraction(size).limit_denominator(1 << 16)
    return max(1, round(s * W)), max(1, round(s * H))


@dataclass(frozen=True)
class TileConfig:
    """The options of `enable_tiled_edit`, validated."""
    size: object = None
    overlap: object = 0.25
    clip: str = "tile"
    max_tiles: int = MAX_TILES

    def __post_init__(self):
        target_size(self.size, (1, 1))
        overlap_px(self.overlap, 1 << 20)
        if self.clip not in ("tile", "photo"):
            raise ValueError(f"tiled edit: clip must be 'tile' or 'photo', got {self.clip!r}")
        if isinstance(self.max_tiles, bool) or not isinstance(self.max_tiles, int) or not (1 <= self.max_tiles <= MAX_TILES):
            raise ValueError(f"tiled edit: max_tiles must be an int in 1..{MAX_TILES}, got {self.max_tiles!r}")


@dataclass(frozen=True)
class TilePlan:
    """One tiled edit's geometry, in pixels: the target, the canvas, the tile and the tiles' origins per axis.  Tiles are numbered row-major
    (y outer, x inner): that is the batch order."""
    source: Tuple[int, int]
    target: Tuple[int, int]
    canvas: Tuple[int, int]
    tile: Tuple[int, int]
    overlap: Tuple[int, int]  # the least overlap asked for, per axis
    xs: Tuple[int, ...]
    ys: Tuple[int, ...]

    @property
    def count(self) -> int:
        return len(self.xs) * len(self.ys)

    @property
    def single(self) -> bool:
        return self.count == 1

    @property
    def origins(self) -> list:
        return [(x, y) for y in self.ys for x in self.xs]

    @property
    def cells(self):
        """(xs, ys, th, tw, ch, cw) in latent cells: what `TileState` and the latent kernels take."""
        return (tuple(x // 8 for x in self.xs), tuple(y // 8 for y in self.ys), self.tile[1] // 8, self.tile[0] // 8,
                self.canvas[1] // 8, self.canvas[0] // 8)

    @property
    def report(self) -> dict:
        ov = lambda o, T: tuple(a + T - b for a, b in zip(o, o[1:]))
        return {"source_size": self.source, "target": self.target, "canvas": self.canvas, "tile": self.tile, "origins": self.origins,
                "grid": (len(self.xs), len(self.ys)), "overlaps": (ov(self.xs, self.tile[0]), ov(self.ys, self.tile[1])),
                "min_overlap": self.overlap, "count": self.count,
                "frames": self.tile if self.single else self.target}  # (one tile: the plain call, whose frames have the tile's size)


def plan(image_size: Tuple[int, int], height: int, width: int, size=None, overlap=0.25, max_tiles: int = MAX_TILES) -> TilePlan:
    """The plan of a tiled edit of a photo of image_size = (W, H) with tiles of width x height.  ValueError: a tile side that is no multiple
    of 16, a canvas smaller than the tile, more than `max_tiles` tiles (the message names the count and the plan)."""
    TW, TH = int(width), int(height)
    if TW % STEP or TH % STEP or TW <= 0 or TH <= 0:
        raise ValueError(f"`height` and `width` have to be divisible by 16 but are {height} and {width}.")
    tgt = target_size(size, image_size)
    CW, CH = -(-tgt[0] // STEP) * STEP, -(-tgt[1] // STEP) * STEP
    vx, vy = overlap_px(overlap, TW), overlap_px(overlap, TH)
    p = TilePlan((int(image_size[0]), int(image_size[1])), tgt, (CW, CH), (TW, TH), (vx, vy), axis_origins(CW, TW, vx), axis_origins(CH, TH, vy))
    if p.count > int(max_tiles):
        raise ValueError(f"tiled edit: the plan has {p.count} tiles, more than max_tiles = {max_tiles}: canvas {CW}x{CH}, tile {TW}x{TH}, origins x "
                         f"{list(p.xs)}, y {list(p.ys)} - lower the size, raise the tile or lower the overlap (chunked passes are out of scope)")
    return p


def tent(T: int) -> torch.Tensor:
    """int64 [T]: w(x) = min(x + 1, T - x)."""
    x = torch.arange(int(T), dtype=torch.int64)
    return torch.minimum(x + 1, int(T) - x)


# ---- the definitions (CPU torch; one op per rounded operation) ------------------------------------------------------------------
def _check_axis(o: Sequence[int], T: int, C: int, name: str):
    o = [int(v) for v in o]
    if not o or o[0] != 0 or o[-1] + T != C or any(b <= a or b > a + T for a, b in zip(o, o[1:])):
        raise ValueError(f"tiles: the {name} origins {o} do not cover [0, {C}) with tiles of side {T}")
    return o


def reference_fuse(tiles: torch.Tensor, xs: Sequence[int], ys: Sequence[int], ch: int, cw: int) -> torch.Tensor:
    """tiles fp32 [n, ..., th, tw] (n = len(ys) * len(xs), row-major), origins in cells -> the canvas fp32 [..., ch, cw]: per cell, in double,
    acc = sum over the covering tiles in ascending index of double(w_t) * double(x_t) - every product and every add rounded on its own, the
    first product taken as it is -, one division by double(sum of w_t), one rounding to fp32.  w_t = wx * wy, tents in cells."""
    t = tiles.detach().to("cpu")
    if t.dtype != torch.float32 or t.dim() < 3:
        raise ValueError(f"reference_fuse: need fp32 [n, ..., th, tw], got {t.dtype} {tuple(t.shape)}")
    th, tw = t.shape[-2:]
    xs, ys = _check_axis(xs, tw, cw, "x"), _check_axis(ys, th, ch, "y")
    if t.shape[0] != len(xs) * len(ys):
        raise ValueError(f"reference_fuse: {t.shape[0]} tiles for a {len(xs)}x{len(ys)} grid")
    w = (tent(th)[:, None] * tent(tw)[None, :]).to(torch.float64)
    lead = tuple(t.shape[1:-2])
    acc = torch.zeros(lead + (ch, cw), dtype=torch.float64)
    wsum = torch.zeros((ch, cw), dtype=torch.float64)
    seen = torch.zeros((ch, cw), dtype=torch.bool)
    k = 0
    for y in ys:
        for x in xs:
            prod = w * t[k].to(torch.float64)
            sl = (Ellipsis, slice(y, y + th), slice(x, x + tw))
            acc[sl] = torch.where(seen[sl[1:]], acc[sl] + prod, prod)
            wsum[sl[1:]] += w
            seen[sl[1:]] = True
            k += 1
    return (acc / wsum).to(torch.float32)


def reference_scatter(canvas: torch.Tensor, xs: Sequence[int], ys: Sequence[int], th: int, tw: int) -> torch.Tensor:
    """canvas [..., ch, cw] -> tiles [n, ..., th, tw]: every tile cell takes its canvas cell."""
    c = canvas.detach().to("cpu")
    xs, ys = _check_axis(xs, tw, c.shape[-1], "x"), _check_axis(ys, th, c.shape[-2], "y")
    return torch.stack([c[..., y:y + th, x:x + tw] for y in ys for x in xs]).contiguous()


def reference_blend(frames: torch.Tensor, xs: Sequence[int], ys: Sequence[int], target: Tuple[int, int]) -> torch.Tensor:
    """frames uint8 [n, F, TH, TW, 3] (the decoded tiles, row-major), origins in pixels, target = (W, H) -> uint8 [F, H, W, 3]: per pixel,
    channel and frame (sum of w_t e_t + W // 2) // W with W = sum of w_t over the covering tiles, tents in pixels, exact integers; the canvas
    cropped to the target."""
    f = torch.as_tensor(frames).detach().to("cpu")
    if f.dtype != torch.uint8 or f.dim() != 5 or f.shape[-1] != 3:
        raise ValueError(f"reference_blend: need uint8 [n, F, TH, TW, 3], got {f.dtype} {tuple(f.shape)}")
    n, F, TH, TW, _ = f.shape
    W, H = int(target[0]), int(target[1])
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    CW, CH = xs[-1] + TW, ys[-1] + TH
    _check_axis(xs, TW, CW, "x"), _check_axis(ys, TH, CH, "y")
    if n != len(xs) * len(ys) or not (1 <= W <= CW and 1 <= H <= CH):
        raise ValueError(f"reference_blend: {n} tiles for a {len(xs)}x{len(ys)} grid, or a target {W}x{H} outside the canvas {CW}x{CH}")
    w = tent(TH)[:, None] * tent(TW)[None, :]
    acc = torch.zeros((F, CH, CW, 3), dtype=torch.int64)
    wsum = torch.zeros((CH, CW), dtype=torch.int64)
    k = 0
    for y in ys:
        for x in xs:
            acc[:, y:y + TH, x:x + TW] += w[None, :, :, None] * f[k].to(torch.int64)
            wsum[y:y + TH, x:x + TW] += w
            k += 1
    wsum = wsum[None, :, :, None]
    out = torch.div(acc + torch.div(wsum, 2, rounding_mode="floor"), wsum, rounding_mode="floor")
    return out[:, :H, :W].to(torch.uint8).contiguous()


def blend_step_bound(T: int, v: int, span: int = 255) -> int:
    """The most two neighbouring pixels of a blended row can differ when two tiles of side T overlap by v pixels on that axis and each tile
    is constant (bytes a and b, |a - b| <= span).  The row's weights on the other axis are common to both tiles and cancel, so the exact
    blend is r = b + (a - b) p with p = wl / S, S = wl + wr, and the kernel's value is r rounded to nearest: within 1/2 of it.  From one
    pixel to the next wl and wr each move by dl, dr in {-1, 0, +1} (a tent, read as 0 just outside its tile), so
    |p' - p| = |dl wr - dr wl| / (S S') <= S / (S S') = 1 / S', and by symmetry <= 1 / S: the step of r is at most span / S_min, S_min the
    smallest weight sum over the overlap and the pixel on either side of it; the two roundings add at most 1/2 each, and the difference of
    two integers is an integer: |d| <= floor(span / S_min + 1) = span // S_min + 1."""
    T, v = int(T), int(v)
    w = lambda x: min(x + 1, T - x) if 0 <= x < T else 0
    S_min = min(w(x) + w(x - (T - v)) for x in range(T - v - 1, T + 1))
    return int(span) // S_min + 1


# ---- inputs: the target image, the canvas, the tiles -----------------------------------------------------------------------------
def target_image(image, size: Tuple[int, int], device=None):
    """The photo as an RGB PIL image of the target's size: Lanczos when the sizes differ - on `device` (image_io.resize_u8, the same bytes)
    or, device None, PIL's own."""
    from PIL import Image
    rgb = image.convert("RGB")
    if rgb.size == tuple(size):
        return rgb
    if device is None:
        return rgb.resize(tuple(size), Image.LANCZOS)
    from . import image_io
    return Image.fromarray(image_io.resize_u8(image_io.upload_rgb(rgb, device), tuple(size), image_io.LANCZOS).cpu().numpy())


def padded_canvas(image, canvas: Tuple[int, int]):
    """The target image padded right and bottom by edge replication to the canvas (one indexing op), as a PIL image."""
    import numpy as np
    from PIL import Image
    W, H = image.size
    CW, CH = canvas
    if (W, H) == (CW, CH):
        return image
    a = torch.from_numpy(np.array(image))
    iy, ix = torch.arange(CH).clamp_(max=H - 1), torch.arange(CW).clamp_(max=W - 1)
    return Image.fromarray(a[iy[:, None], ix[None, :]].numpy())


def tile_images(image, p: TilePlan) -> list:
    """The tiles of the padded canvas of the target image `image`, row-major, as PIL images."""
    c = padded_canvas(image, p.canvas)
    TW, TH = p.tile
    return [c.crop((x, y, x + TW, y + TH)) for x, y in p.origins]


# ---- the state of one running edit -----------------------------------------------------------------------------------------------
class TileState:
    """The tiles of one running edit: the geometry in latent cells and the canvas buffer fp32 [16, T, ch, cw] the fusion goes through.
    `cut` cuts a canvas (the noise) into the tiles' latents; `fuse` is the moment behind every scheduler update: two launches, no host
    read, nothing allocated - a captured step replays it."""

    def __init__(self, p: TilePlan, channels: int, frames: int, device):
        self.plan = p
        self.xs, self.ys, self.th, self.tw, self.ch, self.cw = p.cells
        self.canvas = torch.zeros((int(channels), int(frames), self.ch, self.cw), dtype=torch.float32, device=device)

    @property
    def latent_shape(self) -> tuple:
        return (self.plan.count,) + tuple(self.canvas.shape[:2]) + (self.th, self.tw)

    def cut(self, canvas: torch.Tensor) -> torch.Tensor:
        """canvas fp32 [1, C, T, ch, cw] or [C, T, ch, cw] on the device -> the tiles' latents fp32 [n, C, T, th, tw]."""
        from . import ops
        c = canvas.reshape(self.canvas.shape).to(torch.float32).contiguous()
        return ops.tiles_scatter(c, torch.empty(self.latent_shape, dtype=torch.float32, device=c.device), self.xs, self.ys)

    def fuse(self, latents: torch.Tensor) -> torch.Tensor:
        """In place on the tiles' latents fp32 [n, C, T, th, tw]: tiles -> canvas (weighted mean), canvas -> tiles."""
        from . import ops
        if tuple(latents.shape) != self.latent_shape:
            raise ValueError(f"tiles: the latents {tuple(latents.shape)} are not the plan's {self.latent_shape}")
        ops.tiles_fuse(latents, self.canvas, self.xs, self.ys)
        return ops.tiles_scatter(self.canvas, latents, self.xs, self.ys)


SHARDED = "tiled edits (enable_tiled_edit) with {} are not implemented (nothing sharded has been tested with them)"
