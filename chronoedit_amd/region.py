"""Region-limited edits: change what the mask marks, keep the source everywhere else.

The caller gives ONE single-channel mask of the edit's height x width (255 = edit here, 0 = keep the source; grey values are weights and
are never thresholded, so a soft mask feathers the seam).  Per edit:

    w      fp32 [H/8, W/8]   the 8x8 box mean of the mask: float(sum of the 64 bytes) / 16320
    z_src  fp32, latents'    the VAE posterior mode of the STATIC video [image] * num_frames, normalised like the condition
    eps    fp32, latents'    a copy of the latents the loop starts from (the drawn noise, or the caller's `latents=`)
    sigma_next[i] = scheduler.sigmas[i + 1], an fp32 table on the device (the last entry is 0)

After step i's scheduler update - and before the caller's `on_step_end` - every element of the sample is blended in place

    k = (1 - s) * z_src + s * eps          s = sigma_next[i]:  the source, noised to the level the sample now has
    x = w * x + (1 - w) * k

the flow-matching form of the loop of diffusers' inpaint pipelines.  Only the sample is blended; `last_sample` and the model-output history
stay as the step wrote them.  After the decode the source image is pasted back in pixel space with the full-resolution mask
(`composite`): where the mask is 0 the returned frames carry the source's bytes exactly; where it is 255 (w == 1) the trajectory is the
unmasked loop's bit for bit.  How well the model fills a masked region is the checkpoint's business.

Host side only; the device passes are csrc/ce_region.hip, each bit-equal to the torch expression above evaluated op by op."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

SHARDED = "an edit region with {} is not implemented (the blend runs on replicated latents; nothing sharded has been tested with it)"


def normalize_mask(mask, height: int, width: int) -> torch.Tensor:
    """Whatever a caller may pass as a mask -> uint8 [height, width] on the CPU.
    PIL image: `convert("L")`, and `resize((width, height), Image.BILINEAR)` on the host when its size differs.  numpy array / torch tensor
    [height, width]: bool (True = 255), uint8 (taken as it is) or floating point in [0, 1] (round(255 * m), half to even, computed in
    float64).  An array or tensor of another shape, or a float outside [0, 1], is a ValueError; another type or dtype a TypeError."""
    import numpy as np
    try:
        from PIL import Image
    except ImportError:  # pragma: no cover
        Image = None
    if Image is not None and isinstance(mask, Image.Image):
        m = mask.convert("L")
        if m.size != (width, height):
            m = m.resize((width, height), Image.BILINEAR)
        return torch.from_numpy(np.array(m, dtype=np.uint8))
    if isinstance(mask, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(mask))
    elif isinstance(mask, torch.Tensor):
        t = mask.detach().cpu()
    else:
        raise TypeError(f"mask: expected a PIL image, a numpy array or a torch tensor, got {type(mask)}")
    if tuple(t.shape) != (height, width):
        raise ValueError(f"mask: expected shape ({height}, {width}), got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        return (t.to(torch.uint8) * 255).contiguous()
    if t.dtype == torch.uint8:
        return t.contiguous().clone()
    if t.is_floating_point():
        t = t.double()
        if not bool(((t >= 0) & (t <= 1)).all()):  # (a NaN fails both comparisons)
            raise ValueError("mask: a floating-point mask must lie in [0, 1]")
        return torch.round(t * 255.0).to(torch.uint8).contiguous()
    raise TypeError(f"mask: expected bool, uint8 or a floating-point dtype, got {t.dtype}")


def device_masks(masks: list, height: int, width: int, device) -> list:
    """Per image its mask (whatever `normalize_mask` takes) -> uint8 [height, width] on the device; a mask that several images share is
    normalised and uploaded once (and is ONE tensor afterwards too)."""
    seen = {}
    for m in masks:
        if id(m) not in seen:
            seen[id(m)] = normalize_mask(m, height, width).to(device)
    return [seen[id(m)] for m in masks]


def latent_weights(mask_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [H, W] -> fp32 [H/8, W/8], the 8x8 box mean: ce_region_weights_u8 for a tensor on the device, the torch expression for one on
    the CPU (the same bits: the sum is an integer, the division one fp32 operation)."""
    if mask_u8.dtype != torch.uint8 or mask_u8.dim() != 2:
        raise ValueError(f"latent_weights: need a uint8 [H, W] mask, got {mask_u8.dtype} {tuple(mask_u8.shape)}")
    H, W = mask_u8.shape
    if H % 8 or W % 8:
        raise ValueError(f"latent_weights: the mask's height and width must be multiples of 8, got {H} x {W}")
    if mask_u8.is_cuda:
        from . import ops
        return ops.region_weights_u8(mask_u8.contiguous())
    return mask_u8.contiguous().view(H // 8, 8, W // 8, 8).sum((1, 3)).to(torch.float32) / 16320.0


def latent_stats(vae, device, dtype=torch.bfloat16):
    """(latents_mean, 1 / latents_std) of the VAE's config as [1, z, 1, 1, 1] tensors: what normalises a posterior mode,
    (z - mean) * inv_std, and takes latents back in front of the decode, z / inv_std + mean."""
    z = vae.config.z_dim
    mean = torch.tensor(vae.config.latents_mean, device=device, dtype=dtype).view(1, z, 1, 1, 1)
    inv_std = (1.0 / torch.tensor(vae.config.latents_std)).to(device=device, dtype=dtype).view(1, z, 1, 1, 1)
    return mean, inv_std


@torch.no_grad()
def static_source_latents(vae, image: torch.Tensor, num_frames: int) -> torch.Tensor:
    """image [B, 3, H, W] in [-1, 1] -> fp32 [B, z, T, h, w]: the VAE posterior mode of the video that shows the image in EVERY frame,
    normalised with the latent mean / inverse std in the bf16 expressions `pipeline.prepare_latents` uses for the condition.  (The
    condition's video is [image, 0, 0, ...]: its later latent frames encode the black frames, not the source.)  One VAE encode of the
    condition encode's shape."""
    video = image.unsqueeze(2).repeat(1, 1, num_frames, 1, 1).to(torch.bfloat16)
    mean, inv_std = latent_stats(vae, image.device)
    lat = vae.encode(video).latent_dist.mode()
    lat = (lat - mean) * inv_std
    return lat.float().contiguous()


def sigma_next_table(scheduler, device=None) -> torch.Tensor:
    """fp32 [num_inference_steps]: sigma_next[i] = scheduler.sigmas[i + 1], the noise level the sample has after step i (the last is 0)."""
    return scheduler.sigmas[1:].to(device=device, dtype=torch.float32).contiguous()


@dataclass
class RegionConfig:
    """What `loop.denoise(region=)` takes for ONE edit: w = fp32 [h, w] on the device (`latent_weights`), z_src = fp32 of the latents'
    shape (`static_source_latents`).  The loop itself adds what only it knows - the noise it starts from and the schedule's sigmas - and
    builds the `RegionState`."""
    w: torch.Tensor
    z_src: torch.Tensor


class RegionState:
    """The region of one running edit: w, z_src, eps, the sigma_next device table and the one-float staging buffer the blend reads its
    sigma from (a device-to-device copy per step, no host round trip: a captured step replays for every step)."""

    def __init__(self, w: torch.Tensor, z_src: torch.Tensor, eps: torch.Tensor, sigma_next: torch.Tensor, bf16_state: bool = False):
        if w.dtype != torch.float32 or w.dim() != 2 or tuple(w.shape) != tuple(eps.shape[-2:]):
            raise ValueError(f"region: w must be fp32 [h, w] = the latents' last two axes {tuple(eps.shape[-2:])}, got {w.dtype} {tuple(w.shape)}")
        if tuple(z_src.shape) != tuple(eps.shape):
            raise ValueError(f"region: z_src {tuple(z_src.shape)} does not have the latents' shape {tuple(eps.shape)}")
        dev = eps.device
        self.w = w.to(dev).contiguous()
        self.z_src = z_src.to(device=dev, dtype=torch.float32).contiguous()
        self.eps = eps.to(torch.float32).clone(memory_format=torch.contiguous_format)
        self.sigma_next = sigma_next.to(device=dev, dtype=torch.float32).contiguous()
        self.sigma_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        self.bf16_state = bool(bf16_state)

    @classmethod
    def begin(cls, config: RegionConfig, latents: torch.Tensor, scheduler) -> "RegionState":
        """At loop entry, after `scheduler.set_timesteps`: eps is taken from the latents the loop starts from."""
        return cls(config.w, config.z_src, latents, sigma_next_table(scheduler, latents.device),
                   bf16_state=scheduler.trajectory_dtype == torch.bfloat16)

    def truncate(self):
        """The temporal-reasoning truncation: z_src and eps are sliced exactly as the latents are."""
        self.z_src = self.z_src[:, :, [0, -1]].contiguous()
        self.eps = self.eps[:, :, [0, -1]].contiguous()

    def stage(self, i: int):
        """sigma_next[i] -> the staging float (device to device)."""
        self.sigma_buf.copy_(self.sigma_next[i:i + 1])

    def blend(self, latents: torch.Tensor, i: Optional[int] = None) -> torch.Tensor:
        """The blend after step i, in place on the latents.  i None: the sigma is already staged (a captured step)."""
        from . import ops
        if i is not None:
            self.stage(i)
        return ops.region_blend_(latents, self.z_src, self.eps, self.w, self.sigma_buf, bf16_state=self.bf16_state)


def composite(video: torch.Tensor, src: torch.Tensor, mask_u8: torch.Tensor) -> torch.Tensor:
    """The paste-back behind the decode: video [B, 3, F, H, W] (bf16 / fp32, in [-1, 1]), src bf16 [B, 3, H, W] (the image the VAE was fed),
    mask uint8 [H, W] -> a new fp32 video, m * video + (1 - m) * src with m = mask / 255."""
    from . import ops
    return ops.region_composite(video.contiguous(), src.contiguous(), mask_u8.to(video.device).contiguous())
