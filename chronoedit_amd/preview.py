"""Live previews: a picture that sharpens while the steps run, without making the loop wait.

After every step the scheduler's predict-x0 slot `scheduler.model_outputs[-1]` holds the model's estimate of the FINAL latents.  One latent
frame of it goes through a linear map 16 channels -> RGB (`factors`, fp32 [17, 3]: rows 0..15 the channel weights, row 16 the bias) and a
bilinear upsample by 1, 2, 4 or 8 into bytes - one small launch (csrc/ce_preview.hip) behind the step, outside its captured graph - then an
asynchronous copy into a pinned host buffer and an event.  The preview of step i is handed to `on_preview` once step i + lag has been
enqueued: by then its event has long fired, and the loop never waits for a step that has no later step queued behind it.  Everything
outstanding is delivered before `denoise` returns.  A preview only reads the loop's state: the trajectory is the plain loop's bit for bit.

With an edit region and `composite` the cells the region keeps show the source latents (w * x0 + (1 - w) * z_src per cell), as the returned
frames will; under a sparse plan always, because on sparse steps the prediction is 0 outside the active tokens.

The map is fitted on the loaded VAE (`ChronoEditPipeline.fit_preview_factors`): images -> encode -> normalised posterior mode z -> decode ->
pixels y; ce_preview_gram_f64 sums v v^T over all latent cells, v = (z_0..z_15, 1, r, g, b) with r, g, b the 8x8 box mean of the cell's
pixels, in float64 and a fixed order; `solve_factors` solves the 17 x 3 least-squares problem from that matrix alone.  How well a linear map
fits is the checkpoint's business: `solve_factors`' report (rms and r2 per colour) says so.

`rgb_u8_reference` and `gram_reference` are the contract of the two device passes: CPU torch expressions, one torch op per operation."""
from __future__ import annotations

import math
from collections import deque
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

SCALES = (1, 2, 4, 8)


def as_factors(factors) -> torch.Tensor:
    """Anything array-like of shape [17, 3] with finite entries -> a contiguous fp32 CPU tensor."""
    t = factors.detach().cpu() if isinstance(factors, torch.Tensor) else torch.from_numpy(np.asarray(factors, dtype=np.float64))
    if tuple(t.shape) != (17, 3):
        raise ValueError(f"preview factors: need shape (17, 3) - 16 channel rows and the bias - got {tuple(t.shape)}")
    t = t.to(torch.float32).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("preview factors: every entry must be finite")
    return t


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


@dataclass
class PreviewConfig:
    """What `pipeline.denoise(preview=)` takes.  on_preview: called with one dict per previewed step (its return value is ignored);
    every: preview the steps with (i + 1) % every == 0, and the last; scale: preview pixels per latent cell and axis; frame: the latent
    frame, counted on the shape the step ran at (-1: the edited frame, before and behind the truncation); composite: with a region, show
    the source where the region keeps it; lag: deliver step i's preview once step i + lag is enqueued (0: wait for it at once);
    factors: fp32 [17, 3]."""
    on_preview: Callable
    every: int = 1
    scale: int = 2
    frame: int = -1
    composite: bool = True
    lag: int = 1
    factors: Optional[torch.Tensor] = None

    def __post_init__(self):
        if not callable(self.on_preview):
            raise ValueError("preview: on_preview must be callable")
        if not _is_int(self.every) or self.every < 1:
            raise ValueError(f"preview: every must be an integer >= 1, got {self.every!r}")
        if not _is_int(self.scale) or self.scale not in SCALES:
            raise ValueError(f"preview: scale must be one of {SCALES}, got {self.scale!r}")
        if not _is_int(self.frame):
            raise ValueError(f"preview: frame must be an integer, got {self.frame!r}")
        if not isinstance(self.composite, bool):
            raise ValueError(f"preview: composite must be a bool, got {self.composite!r}")
        if not _is_int(self.lag) or self.lag < 0:
            raise ValueError(f"preview: lag must be an integer >= 0, got {self.lag!r}")
        self.every, self.scale, self.frame, self.lag = int(self.every), int(self.scale), int(self.frame), int(self.lag)
        if self.factors is not None:
            self.factors = as_factors(self.factors)


def due(i: int, n_steps: int, every: int) -> bool:
    """Is step i of n_steps previewed?"""
    return (i + 1) % every == 0 or i == n_steps - 1


# -- the contract of ce_preview_rgb_u8 ------------------------------------------------------------------------------------------------
def _taps(n_out: int, n: int, scale: int):
    """Half-pixel centres: f = (o + 0.5) / scale - 0.5 clamped to [0, n - 1] -> i0 = floor(f), i1 = min(i0 + 1, n - 1), t = f - i0."""
    o = torch.arange(n_out, dtype=torch.float32)
    f = (o + 0.5) / float(scale)
    f = f - 0.5
    f = f.clamp(0.0, float(n - 1))
    fl = torch.floor(f)
    i0 = fl.to(torch.int64)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, f - fl


def _lerp(a, b, t):
    """a * (1 - t) + b * t: a subtraction, two multiplies, one add."""
    s = 1.0 - t
    left = a * s
    right = b * t
    return left + right


def project_reference(x0: torch.Tensor, factors: torch.Tensor, frame: int = -1, w: Optional[torch.Tensor] = None,
                      z_src: Optional[torch.Tensor] = None, order=None) -> torch.Tensor:
    """The cell values and the projection: fp32 [B, 3, h, w].  order: the channel order of the sum (default 0..15, the kernel's)."""
    x = x0[:, :, frame].to(torch.float32)
    F = factors.to(torch.float32)
    if w is not None:
        z = z_src[:, :, frame].to(torch.float32)
        iw = 1.0 - w
        a = w * x
        b = iw * z
        u = a + b
    else:
        u = x
    B, _, h, wl = u.shape
    p = F[16].view(1, 3, 1, 1).expand(B, 3, h, wl).clone()
    for k in (range(16) if order is None else order):
        t = F[k].view(1, 3, 1, 1) * u[:, k:k + 1]
        p = p + t
    return p


def byte_reference(v: torch.Tensor) -> torch.Tensor:
    """ce_video_to_u8's byte: (v * 0.5 + 0.5) clamped to [0, 1], times 255, half to even; NaN -> 0, +inf -> 255, -inf -> 0."""
    f = v * 0.5
    f = f + 0.5
    f = torch.where(f != f, torch.zeros_like(f), f)
    f = f.clamp(0.0, 1.0)
    return torch.round(f * 255.0).to(torch.uint8)


def rgb_u8_reference(x0: torch.Tensor, factors: torch.Tensor, scale: int = 2, frame: int = -1, w: Optional[torch.Tensor] = None,
                     z_src: Optional[torch.Tensor] = None, order=None, vertical_first: bool = False) -> torch.Tensor:
    """x0 fp32 [B, 16, T, h, w] (CPU) -> uint8 [B, h scale, w scale, 3]: what ce_preview_rgb_u8 computes, bit for bit.  Per pixel
    top = p(y0, x0) * (1 - tx) + p(y0, x1) * tx, bot likewise on row y1, v = top * (1 - ty) + bot * ty, all four taps always evaluated: an
    infinite cell therefore makes a NaN (byte 0) of a pixel that takes it with weight 0, and its own colour where the weight is not.  `order` and
    `vertical_first` evaluate the same map in ANOTHER order of operations - for tests that show the data tells the orders apart."""
    if int(scale) not in SCALES:
        raise ValueError(f"scale: must be one of {SCALES}, got {scale}")
    if (w is None) != (z_src is None):
        raise ValueError("w and z_src: the composite takes both or neither")
    p = project_reference(x0, factors, frame, w, z_src, order)
    h, wl = p.shape[-2:]
    y0, y1, ty = _taps(h * scale, h, scale)
    xa, xb, tx = _taps(wl * scale, wl, scale)
    ty = ty.view(-1, 1)
    if not vertical_first:
        r0, r1 = p[:, :, y0], p[:, :, y1]
        top = _lerp(r0[..., xa], r0[..., xb], tx)
        bot = _lerp(r1[..., xa], r1[..., xb], tx)
        v = _lerp(top, bot, ty)
    else:
        c0, c1 = p[..., xa], p[..., xb]
        left = _lerp(c0[:, :, y0], c0[:, :, y1], ty)
        right = _lerp(c1[:, :, y0], c1[:, :, y1], ty)
        v = _lerp(left, right, tx)
    return byte_reference(v).permute(0, 2, 3, 1).contiguous()


# -- the fit ----------------------------------------------------------------------------------------------------------------------------
def box_mean_reference(y: torch.Tensor) -> torch.Tensor:
    """y [B, 3, 8h, 8w] (fp32 / bf16) -> fp32 [B, 3, h, w]: the fp32 sum of a cell's 64 pixels in row-major order, times 1 / 64."""
    B, C, H, W = y.shape
    t = y.to(torch.float32).view(B, C, H // 8, 8, W // 8, 8)
    s = torch.zeros(B, C, H // 8, W // 8, dtype=torch.float32)
    for r in range(8):
        for q in range(8):
            s = s + t[:, :, :, r, :, q]
    return s * 0.015625


def gram_reference(z: torch.Tensor, y: torch.Tensor, frame: int = -1) -> torch.Tensor:
    """z fp32 [B, 16, T, h, w], y [B, 3, 8h, 8w] (CPU) -> float64 [20, 20] = sum over cells of v v^T, v = (z_0..z_15, 1, r, g, b)."""
    zf = z[:, :, frame].to(torch.float32)
    B, _, h, wl = zf.shape
    if tuple(y.shape) != (B, 3, 8 * h, 8 * wl):
        raise ValueError(f"gram_reference: y must be [{B}, 3, {8 * h}, {8 * wl}], got {tuple(y.shape)}")
    v = torch.cat([zf, torch.ones(B, 1, h, wl), box_mean_reference(y)], dim=1).permute(0, 2, 3, 1).reshape(-1, 20).to(torch.float64)
    return v.T @ v


def solve_factors(G):
    """The Gram matrix [20, 20] -> (factors fp32 [17, 3], report).  factors = the least-squares solution of G[:17, :17] X = G[:17, 17:] in
    float64 (numpy.linalg.lstsq), rounded to fp32.  report = {"rms": per colour, "r2": per colour} of THOSE factors, from G alone:
    rss = G_cc - 2 x . G[:17, c] + x^T G[:17, :17] x over n = G[16][16] cells; r2 = 1 - rss / (G_cc - G[16][c]^2 / n)."""
    G = np.asarray(G.detach().cpu() if isinstance(G, torch.Tensor) else G, dtype=np.float64)
    if G.shape != (20, 20):
        raise ValueError(f"solve_factors: need the [20, 20] Gram matrix, got {G.shape}")
    A, Bm = G[:17, :17], G[:17, 17:]
    X = np.linalg.lstsq(A, Bm, rcond=None)[0]
    F32 = X.astype(np.float32)
    Xr = F32.astype(np.float64)
    n = G[16, 16]
    rms, r2 = [], []
    for c in range(3):
        x = Xr[:, c]
        rss = max(float(G[17 + c, 17 + c] - 2.0 * x @ Bm[:, c] + x @ A @ x), 0.0)
        tss = float(G[17 + c, 17 + c] - G[16, 17 + c] ** 2 / n) if n > 0 else 0.0
        rms.append(math.sqrt(rss / n) if n > 0 else float("nan"))
        r2.append(1.0 - rss / tss if tss > 0 else float("nan"))
    return torch.from_numpy(F32).contiguous(), {"rms": rms, "r2": r2}


# -- delivery ---------------------------------------------------------------------------------------------------------------------------
class PreviewDelivery:
    """The previews of ONE running loop: the factors on the device, one device byte buffer (launches and copies are ordered on the stream),
    lag + 1 pinned host buffers, and per previewed step an asynchronous copy and an event.  `submit` enqueues, `deliver(upto)` hands out
    every pending preview of a step <= upto (waiting on its event), `flush` all of them."""

    def __init__(self, config: PreviewConfig, device, timesteps):
        if config.factors is None:
            raise ValueError("preview: no factors - pass factors=, or fit them on the loaded VAE (ChronoEditPipeline.fit_preview_factors)")
        self.config = config
        self.factors = config.factors.to(device)
        self.timesteps = timesteps  # host values, read once before the first step
        self.dev = None
        self.slots, self.free, self.pending = [], deque(), deque()

    def _buffers(self, shape, device):
        if self.dev is None or tuple(self.dev.shape) != shape:
            self.flush()
            self.dev = torch.empty(shape, dtype=torch.uint8, device=device)
            self.slots = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(self.config.lag + 1)]
            self.free = deque(range(len(self.slots)))

    def submit(self, i: int, step: int, x0: torch.Tensor, w: Optional[torch.Tensor] = None, z_src: Optional[torch.Tensor] = None):
        """Step i of the loop (reported as `step`): the kernel, the copy and the event, on the current stream."""
        from . import ops
        c = self.config
        B, _, T, h, wl = x0.shape
        if not -T <= c.frame < T:
            raise ValueError(f"preview: frame {c.frame} is outside the {T} latent frames of step {step}")
        self._buffers((B, h * c.scale, wl * c.scale, 3), x0.device)
        if not self.free:  # (cannot happen while the loop delivers as documented; never overwrite an undelivered slot)
            self._pop()
        slot = self.free.popleft()
        ops.preview_rgb_u8(x0, self.factors, c.scale, c.frame, w, z_src, out=self.dev)
        self.slots[slot].copy_(self.dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.pending.append((i, step, self.timesteps[i], slot, ev))

    def _pop(self):
        from PIL import Image
        i, step, t, slot, ev = self.pending.popleft()
        ev.synchronize()
        host = self.slots[slot].numpy()
        images = [Image.fromarray(host[b].copy()) for b in range(host.shape[0])]
        self.free.append(slot)
        for b, im in enumerate(images):
            d = {"step": step, "timestep": t, "image": im}
            if len(images) > 1:
                d["sample"] = b
            self.config.on_preview(d)

    def deliver(self, upto: int):
        while self.pending and self.pending[0][0] <= upto:
            self._pop()

    def flush(self):
        while self.pending:
            self._pop()
