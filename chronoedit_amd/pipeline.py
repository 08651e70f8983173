"""ChronoEditPipeline on the HIP engine: the drop-in for the reference pipeline of the same name
(chronoedit_diffusers/pipeline_chronoedit.py), with `prepare_latents` and `decode_latents` around the denoising loop.

The loop itself - `denoise`, `denoise_step`, `GraphedDenoiser`, the text-compaction helpers, `make_cfg_inputs` - lives in
chronoedit_amd/loop.py; every name of it that callers, tests and tools import from here is re-exported below (the same objects).
"""
from __future__ import annotations

import contextlib
import html
import inspect
import re
from dataclasses import dataclass, make_dataclass, replace
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import torch

from . import auto_region as _ar, autofocus as _af, clusters as _cl, focus as _fc, image_io, layers as _ly, lift as _lf, preview as _pv, region as _rg, sketch as _sk, tiles as _tl
from .loop import (GraphedDenoiser, _capturable, _sharded_batchable, _shared_inputs, _token_sharded, _warmup_stream,  # noqa: F401
                   compact_text_context, denoise, denoise_step, make_cfg_inputs, refuse_sharded, text_compaction_plan, text_real_lengths)
from .scheduler import FlowUniPCMultistepScheduler
from .transformer import ChronoEditTransformer3DModel


def prompt_clean(text: str) -> str:
    """pipeline_chronoedit.py:98-112: ftfy.fix_text (when ftfy is installed, as in the reference), double html.unescape,
    whitespace collapse."""
    try:
        import ftfy
        text = ftfy.fix_text(text)
    except ImportError:
        pass
    text = html.unescape(html.unescape(text)).strip()
    return re.sub(r"\s+", " ", text).strip()


# ---------------------------------------------------------------------------------------------------------------
# The edit: prepare_latents -> denoise -> decode  (pipeline_chronoedit.py:392-456, 694-781)
# ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def prepare_latents(vae, image: torch.Tensor, num_frames: int, latents: Optional[torch.Tensor] = None, generator=None):
    """image [B,3,H,W] in [-1,1] -> (latents fp32 [B,16,T,h,w], condition bf16 [B,20,T,h,w]).
    pipeline_chronoedit.py:392-456: the condition video is [image, 0, 0, ...]; its VAE posterior mode is normalised with the
    latent mean/std; a 4-channel first-frame mask is stacked in front."""
    B, _, H, W = image.shape
    dev = image.device
    tds = 2 ** sum(vae.temperal_downsample)
    T = (num_frames - 1) // tds + 1
    h, w = H // 8, W // 8
    z = vae.config.z_dim
    if latents is None:
        latents = torch.randn((B, z, T, h, w), generator=generator, device=dev, dtype=torch.float32)
    else:
        latents = latents.to(device=dev, dtype=torch.float32)
    video = torch.cat([image.unsqueeze(2), image.new_zeros(B, 3, num_frames - 1, H, W)], dim=2).to(torch.bfloat16)
    mean, inv_std = _rg.latent_stats(vae, dev)
    cond = vae.encode(video).latent_dist.mode()
    cond = (cond - mean) * inv_std
    mask = torch.ones(B, 1, num_frames, h, w, device=dev)
    mask[:, :, 1:] = 0
    first = torch.repeat_interleave(mask[:, :, 0:1], dim=2, repeats=tds)
    mask = torch.cat([first, mask[:, :, 1:]], dim=2).view(B, -1, tds, h, w).transpose(1, 2)
    return latents.contiguous(), torch.cat([mask.to(cond.dtype), cond], dim=1).contiguous()


@torch.no_grad()
def decode_latents(vae, latents: torch.Tensor, enable_temporal_reasoning: bool = False, num_temporal_reasoning_steps: int = 0):
    """pipeline_chronoedit.py:765-781: de-normalise, decode; in reasoning mode the edit frames and the reasoning frames are
    decoded separately and concatenated."""
    latents = latents.to(torch.bfloat16)
    mean, inv_std = _rg.latent_stats(vae, latents.device)
    latents = latents / inv_std + mean
    if enable_temporal_reasoning and num_temporal_reasoning_steps > 0 and latents.shape[2] > 2:
        edit = vae.decode(latents[:, :, [0, -1]], return_dict=False)[0]
        reason = vae.decode(latents[:, :, :-1], return_dict=False)[0]
        return torch.cat([reason, edit[:, :, 1:]], dim=2)
    return vae.decode(latents, return_dict=False)[0]


def _blend_tiles(video: torch.Tensor, p) -> torch.Tensor:
    """The decoded tiles [n, 3, F, TH, TW] on the device -> the target's frames uint8 [F, H, W, 3]: ce_video_to_u8, then ce_tiles_blend_u8."""
    from . import ops
    return ops.tiles_blend_u8(ops.video_to_u8(video.contiguous()), p.xs, p.ys, p.target)


@dataclass
class WanPipelineOutput:
    """diffusers.pipelines.wan.pipeline_output.WanPipelineOutput: `.frames` is what callers index
    (run_inference_diffusers.py:441 `.frames[0]`)."""
    frames: Any


@dataclass
class FocusPass:
    """A focused pass that its caller planned - a sketch edit, or the scout of an auto-focused call - in place of the user's switches."""
    plans: list  # one focus.FocusPlan per image
    composite: bool  # paste the frames through the masks (else: the whole box)
    start: Optional[dict] = None  # the warm start {"step", "x0", "sigma"}: begin at that step on the scout's resampled estimate
    preview_tag: Optional[str] = None  # the "pass" entry of this pass's previews
    guarded: bool = False  # the text guardrail has seen the call's prompt already
    crop_of: Optional[list] = None  # a sketch edit with several crops per photo: per plan (editor value, crop), chained into one video per value


@dataclass
class EditSources:
    """What one pass edits, resolved once at its top (`ChronoEditPipeline._resolve`)."""
    pil: Optional[list] = None  # the call's PIL images; None: arrays or tensors
    focus: Optional[list] = None  # a focused region edit: per image its focus.FocusPlan (the encoders then see the crops)
    masks: Any = None  # an unfocused region edit: the explicit edit-size mask(s)
    composite: bool = False  # paste the source back through the masks behind the decode
    auto_focus: Any = None  # the autofocus.AutoFocusConfig when this pass is a scout
    lift: Any = None  # the lift.LiftConfig while the detail lift is on (a focused pass only reports it, unless lift_focus)
    lift_focus: bool = False  # enable_detail_lift(focus=True): a focused pass lifts every crop inside its box before the paste (boxlift.py)
    lift_mask_aware: bool = False  # enable_detail_lift(focus=True, mask_aware=True): those fits run under the crops' edit-size masks (rimlift.py)
    crop_of: Optional[list] = None  # per focus plan (editor value, crop) when the crops of a value are chained into one video (clusters.paste)


def _randn_tensor(shape, generator, device, dtype):
    """diffusers.utils.torch_utils.randn_tensor semantics (pipeline_chronoedit.py:418): the noise is drawn on the GENERATOR's
    device (a CPU generator gives CPU-reproducible noise that is then moved), one generator per sample when a list is given."""
    device = torch.device(device)
    gens = generator if isinstance(generator, (list, tuple)) else [generator] * 1
    if isinstance(generator, (list, tuple)):
        shape1 = (1,) + tuple(shape[1:])
        return torch.cat([_randn_tensor(shape1, g, device, dtype) for g in generator], dim=0)
    g = gens[0]
    gdev = device if g is None else torch.device(g.device)
    if gdev.type != device.type:
        if gdev.type == "cpu":
            return torch.randn(shape, generator=g, device="cpu", dtype=dtype).to(device)
        raise ValueError(f"Cannot generate a {device.type} tensor from a generator of type {gdev.type}.")
    return torch.randn(shape, generator=g, device=device, dtype=dtype)


class ChronoEditPipeline:
    """MI355X drop-in for the reference pipeline of the same name (chronoedit_diffusers/pipeline_chronoedit.py:124-812): the same
    constructor components, `from_pretrained`, `encode_prompt` / `encode_image`, `check_inputs`, `prepare_latents`, LoRA entry
    points and `__call__(image=, prompt=, negative_prompt=, height=, width=, num_frames=, num_inference_steps=, guidance_scale=,
    ..., offload_model=) -> WanPipelineOutput(frames=...)`, so `scripts/run_inference_diffusers.py:428-441` drives it unchanged.
    Every tensor op behind it runs on the HIP kernels (DiT, UniPC+CFG, VAE, UMT5, CLIP drop-ins); the tokenizer and the CLIP
    image processor are the reference's host-side transformers objects and are injected (`tokenizer=`, `image_processor=`).
    Guardrails are out of scope: `text_guardrail_runner` / `video_guardrail_runner` stay None unless the
    caller installs callables, which are then honoured with the reference's error behaviour (:621-629, :784-799)."""

    model_cpu_offload_seq = "text_encoder->image_encoder->transformer->vae"
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]

    def __init__(self, tokenizer=None, text_encoder=None, image_encoder=None, image_processor=None,
                 transformer: Optional[ChronoEditTransformer3DModel] = None, vae=None,
                 scheduler: Optional[FlowUniPCMultistepScheduler] = None, disable_guardrails: bool = True):
        self.tokenizer, self.text_encoder, self.image_encoder, self.image_processor = tokenizer, text_encoder, image_encoder, image_processor
        self.vae, self.transformer, self.scheduler = vae, transformer, scheduler  # chronoedit_amd drop-ins
        tds = getattr(vae, "temperal_downsample", None)
        self.vae_scale_factor_temporal = 2 ** sum(tds) if tds is not None else 4      # :185
        self.vae_scale_factor_spatial = 2 ** len(tds) if tds is not None else 8       # :186
        self.guardrail_enabled = not disable_guardrails
        self.text_guardrail_runner = None
        self.video_guardrail_runner = None
        # Defaults of the product pipeline (bit-identical to the eager / uncached loop: tests/test_pipeline_gpu.py): every step of the
        # loop is ONE hipGraph replay (GraphedDenoiser; two graphs when temporal reasoning truncates 8 -> 2 frames), and the
        # step-invariant text / image context projections are computed once per edit (`denoise` clears them at
        # the start of every edit).  `pipe.use_graph = False` / `pipe.transformer.cache_context = False` switch either off.  The VAE
        # follows `use_graph`: from the second edit of a shape on its encode / decode are one graph replay each.
        self.use_graph = True
        self._graph_warm = set()  # (latent shape, guided) pairs whose lazy initialisations have already happened in this process
        if transformer is not None and hasattr(transformer, "cache_context"):
            transformer.cache_context = True
        self._guidance_scale, self._attention_kwargs, self._current_timestep, self._interrupt, self._num_timesteps = 1.0, None, None, False, 0
        self._guidance_measure = None  # (max_age, keep_deltas) while measure_guidance_reuse runs its edits
        # PIL in, PIL out: the resize / normalise passes in front of the encoders and the uint8 packing behind the VAE run on the device
        # (image_io.py, bit-equal to the host path); arrays, tensors, "np" and "pt" keep the host code.  enable_device_image_io(False): A/B.
        self.device_image_io = True
        self._edit_region = None  # (mask or list of masks, composite) while set_edit_region is in force
        self._auto_region_measure = None  # the detector options while measure_auto_region runs
        self.auto_region_report = None  # the last call's auto-region report (a list of them for a call with several samples); None without a detection
        self._region_focus = None  # the context fraction while enable_region_focus is in force
        self.focus_report = None  # the last call's focus plans, one dict per image (focus.plan); None when focus did not run
        self._auto_focus = None  # the autofocus.AutoFocusConfig while enable_auto_focus is in force
        self._preview = None  # the options of `enable_preview` while it is in force
        self.preview_factors = None  # fp32 [17, 3]: the latent -> RGB map of the previews (`fit_preview_factors`, or set by hand)
        self.preview_fit_report = None  # {"rms", "r2"} per colour of the last fit
        self.preview_fit_gram = None  # float64 [20, 20] on the CPU: the Gram matrix the last fit solved
        self._detail_lift = None  # the lift.LiftConfig while enable_detail_lift is in force
        self._detail_lift_focus = False  # enable_detail_lift(focus=True): focused passes lift inside their boxes
        self._detail_lift_mask_aware = False  # enable_detail_lift(focus=True, mask_aware=True): ... fitted under the region's weights
        self.lift_report = None  # the last call's detail-lift report, one dict per sample; None when the switch is off (or "latent" was asked for)
        self._sketch_region = None  # the sketch.SketchConfig while enable_sketch_region is in force
        self.sketch_report = None  # the last call's sketch plans, one dict per editor value; None when the call got no editor value
        self._tiled = None  # the tiles.TileConfig while enable_tiled_edit is in force
        self.tile_report = None  # the last call's tile plan (tiles.TilePlan.report) plus "reason"; None when tiled edits were off

    # -- properties of the reference pipeline (:458-478) ---------------------------------------------------------------
    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def current_timestep(self):
        return self._current_timestep

    @property
    def interrupt(self):
        return self._interrupt

    @property
    def attention_kwargs(self):
        return self._attention_kwargs

    @property
    def _execution_device(self) -> torch.device:
        for m in (self.transformer, self.vae, self.text_encoder, self.image_encoder):
            d = getattr(m, "device", None)
            if d is not None:
                return torch.device(d)
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")

    def enable_device_image_io(self, flag: bool = True):
        """Image pre- / post-processing of `__call__` on the device (default) or, `flag=False`, on the host as before: the same bits."""
        self.device_image_io = bool(flag)
        return self

    def to(self, device=None, dtype=None):
        """`pipe.to(device)` (run_inference_diffusers.py:386): moves every nn.Module component.  The engine computes in bf16 (the
        reference runner hard-codes it, :344-362): any other `dtype` is refused rather than ignored."""
        if dtype is not None and dtype != torch.bfloat16:
            raise ValueError(f"chronoedit_amd components compute in torch.bfloat16; pipe.to(dtype={dtype}) is not supported")
        for m in (self.text_encoder, self.image_encoder, self.transformer, self.vae):
            if m is not None and hasattr(m, "to") and device is not None:
                m.to(device)
        return self

    def maybe_free_model_hooks(self):
        return None

    @classmethod
    def from_pretrained(cls, path: str, transformer=None, vae=None, text_encoder=None, image_encoder=None, scheduler=None,
                        tokenizer=None, image_processor=None, torch_dtype: torch.dtype = torch.bfloat16, device="cuda:0",
                        load_encoders: bool = True, disable_guardrails: bool = True):
        """``ChronoEditPipeline.from_pretrained(model_path, image_encoder=..., transformer=..., vae=..., torch_dtype=bf16,
        disable_guardrails=...)`` (run_inference_diffusers.py:357-364): components handed in are used as they are, the others
        are read from the diffusers directory layout (``transformer/``, ``vae/``, ``text_encoder/``, ``image_encoder/``,
        ``scheduler/scheduler_config.json``; ``tokenizer/`` and ``image_processor/`` through transformers when present).
        The scheduler defaults to the diffusers sigma grid - the class the reference runner installs (:379-382)."""
        import json
        import os

        from .vae import AutoencoderKLWan
        if transformer is None:
            transformer = ChronoEditTransformer3DModel.from_pretrained(path, subfolder="transformer", torch_dtype=torch_dtype, device=device)
        if vae is None:
            vae = AutoencoderKLWan.from_pretrained(path, subfolder="vae", torch_dtype=torch_dtype, device=device)
        if scheduler is None:
            cfg_file = os.path.join(path, "scheduler", "scheduler_config.json")
            cfg = {}
            if os.path.exists(cfg_file):
                with open(cfg_file) as f:
                    cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
            cfg.setdefault("sigma_grid", "diffusers")
            scheduler = FlowUniPCMultistepScheduler.from_config(cfg)
        if load_encoders:
            if text_encoder is None and os.path.isdir(os.path.join(path, "text_encoder")):
                from .umt5 import UMT5EncoderModel
                text_encoder = UMT5EncoderModel.from_pretrained(path, subfolder="text_encoder", torch_dtype=torch_dtype, device=device)
            if image_encoder is None and os.path.isdir(os.path.join(path, "image_encoder")):
                from .clip_vision import CLIPVisionModel
                image_encoder = CLIPVisionModel.from_pretrained(path, subfolder="image_encoder", torch_dtype=torch_dtype, device=device)
            if tokenizer is None and os.path.isdir(os.path.join(path, "tokenizer")):
                from transformers import AutoTokenizer
                tokenizer = AutoTokenizer.from_pretrained(os.path.join(path, "tokenizer"))
            if image_processor is None and os.path.isdir(os.path.join(path, "image_processor")):
                from transformers import CLIPImageProcessor
                image_processor = CLIPImageProcessor.from_pretrained(os.path.join(path, "image_processor"))
        return cls(tokenizer=tokenizer, text_encoder=text_encoder, image_encoder=image_encoder, image_processor=image_processor,
                   transformer=transformer, vae=vae, scheduler=scheduler, disable_guardrails=disable_guardrails)

    # -- conditioning (pipeline_chronoedit.py:205-330) -------------------------------------------------------------------
    def _get_t5_prompt_embeds(self, prompt=None, num_videos_per_prompt: int = 1, max_sequence_length: int = 512, device=None, dtype=None):
        """:205-243: clean, tokenise to max_length, encode, zero the padding rows, repeat per video."""
        if self.tokenizer is None or self.text_encoder is None:
            raise ValueError("`prompt` strings need the pipeline's tokenizer and text_encoder; pass `prompt_embeds` instead")
        from .umt5 import t5_prompt_embeds
        device = device or self._execution_device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        prompt = [prompt_clean(u) for u in prompt]
        batch_size = len(prompt)
        text_inputs = self.tokenizer(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                                     add_special_tokens=True, return_attention_mask=True, return_tensors="pt")
        ids, mask = text_inputs.input_ids, text_inputs.attention_mask
        prompt_embeds = t5_prompt_embeds(self.text_encoder, ids.to(device), mask.to(device))
        if dtype is not None:
            prompt_embeds = prompt_embeds.to(dtype)
        _, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_videos_per_prompt, 1)
        return prompt_embeds.view(batch_size * num_videos_per_prompt, seq_len, -1)

    def encode_prompt(self, prompt=None, negative_prompt=None, do_classifier_free_guidance: bool = True, num_videos_per_prompt: int = 1,
                      prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                      max_sequence_length: int = 226, device=None, dtype=None, *, input_ids: Optional[torch.Tensor] = None,
                      attention_mask: Optional[torch.Tensor] = None, negative_input_ids: Optional[torch.Tensor] = None,
                      negative_attention_mask: Optional[torch.Tensor] = None):
        """:258-330 (strings through the injected tokenizer).  Tokenizer-free form for callers that tokenise themselves:
        `encode_prompt(input_ids=, attention_mask=, negative_input_ids=, negative_attention_mask=)` (ids padded to max length)."""
        if input_ids is not None:
            from .umt5 import t5_prompt_embeds
            if self.text_encoder is None:
                raise ValueError("this pipeline was built without a text_encoder: pass prompt_embeds instead")
            pos = t5_prompt_embeds(self.text_encoder, input_ids, attention_mask)
            neg = None if negative_input_ids is None else t5_prompt_embeds(self.text_encoder, negative_input_ids, negative_attention_mask)
            return pos, neg
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt) if prompt is not None else prompt_embeds.shape[0]
        if prompt_embeds is None:
            prompt_embeds = self._get_t5_prompt_embeds(prompt, num_videos_per_prompt, max_sequence_length, device, dtype)
        if do_classifier_free_guidance and negative_prompt_embeds is None:
            negative_prompt = negative_prompt or ""
            negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
            if prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} != {type(prompt)}.")
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: {prompt} has "
                                 f"batch size {batch_size}. Please make sure that passed `negative_prompt` matches the batch size of `prompt`.")
            negative_prompt_embeds = self._get_t5_prompt_embeds(negative_prompt, num_videos_per_prompt, max_sequence_length, device, dtype)
        return prompt_embeds, negative_prompt_embeds

    def encode_image(self, image, device=None) -> torch.Tensor:
        """:247-256: CLIP penultimate hidden state.  `image`: whatever the injected CLIPImageProcessor accepts, or - without a
        processor - the pixel_values tensor [B,3,224,224] it would have produced."""
        if self.image_encoder is None:
            raise ValueError("this pipeline was built without an image_encoder: pass image_embeds instead")
        device = device or self._execution_device
        if self.image_processor is not None and not (isinstance(image, torch.Tensor) and image.dim() == 4 and image.is_floating_point()
                                                     and image.shape[1] == 3 and image.min() < 0):
            pixel_values = None
            if image_io.on_device(self.device_image_io, device):
                pixel_values = image_io.clip_pixel_values(self.image_processor, image, device)  # None: not the plain CLIP recipe on PIL input
            if pixel_values is None:
                pixel_values = self.image_processor(images=image, return_tensors="pt")["pixel_values"]
        elif isinstance(image, torch.Tensor):
            pixel_values = image
        else:
            raise ValueError("encode_image needs the pipeline's image_processor for non-tensor images")
        return self.image_encoder(pixel_values=pixel_values.to(device), output_hidden_states=True).hidden_states[-2]

    def check_inputs(self, prompt, negative_prompt, image, height, width, prompt_embeds=None, negative_prompt_embeds=None,
                     image_embeds=None, callback_on_step_end_tensor_inputs=None):
        """:332-390, message for message - with ONE rule relaxed: the reference rejects `image` together with `image_embeds`
        although its own `__call__` needs `image` for `prepare_latents`, which makes `image_embeds` unusable there; here
        both may be given (the embeds then skip the CLIP encoder).  A non-empty list of PIL images is taken as well (one image per
        prompt, as a batched tensor is: what preprocessing and the CLIP path already handle, and a focused region edit of several photos
        needs - their sizes may differ)."""
        if image is None and image_embeds is None:
            raise ValueError("Provide either `image` or `prompt_embeds`. Cannot leave both `image` and `image_embeds` undefined.")
        if image is not None and not isinstance(image, torch.Tensor) and not image_io._is_pil(image) and image_io._pil_list(image) is None:
            raise ValueError(f"`image` has to be of type `torch.Tensor` or `PIL.Image.Image` but is {type(image)}")
        if height % 16 != 0 or width % 16 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 16 but are {height} and {width}.")
        if callback_on_step_end_tensor_inputs is not None and not all(k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found "
                             f"{[k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to only forward one of the two.")
        elif negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`: {negative_prompt_embeds}. "
                             "Please make sure to only forward one of the two.")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        elif negative_prompt is not None and (not isinstance(negative_prompt, str) and not isinstance(negative_prompt, list)):
            raise ValueError(f"`negative_prompt` has to be of type `str` or `list` but is {type(negative_prompt)}")

    def prepare_latents(self, image: torch.Tensor, batch_size: int, num_channels_latents: int = 16, height: int = 480, width: int = 832,
                        num_frames: int = 81, dtype: Optional[torch.dtype] = None, device=None, generator=None,
                        latents: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """:392-456 with the reference's argument list: returns (latents in `dtype`, condition [B,20,T,h,w])."""
        device = device or self._execution_device
        T = (num_frames - 1) // self.vae_scale_factor_temporal + 1
        shape = (batch_size, num_channels_latents, T, height // self.vae_scale_factor_spatial, width // self.vae_scale_factor_spatial)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            latents = _randn_tensor(shape, generator, device, dtype or torch.bfloat16)
        else:
            latents = latents.to(device=device, dtype=dtype or latents.dtype)
        if image.shape[-2:] != (height, width):
            raise ValueError(f"image is {tuple(image.shape[-2:])}, expected ({height}, {width}) after preprocessing")
        _, condition = prepare_latents(self.vae, image.to(device), num_frames, latents=latents)
        if condition.shape[0] != batch_size:
            condition = condition.repeat(batch_size, 1, 1, 1, 1)
        return latents, condition

    # LoRA entry points of the reference runner (run_inference_diffusers.py:370-374); the adapters target the transformer
    def load_lora_weights(self, path_or_state, adapter_name: str = "default"):
        self.transformer.load_lora_weights(path_or_state, adapter_name=adapter_name)
        return self

    def fuse_lora(self, adapter_names=None, lora_scale: float = 1.0):
        self.transformer.fuse_lora(adapter_names=adapter_names, lora_scale=lora_scale)
        return self

    # switching adapters between edits (diffusers' LoraBaseMixin surface; weights.LoraMixin has the semantics and the memory cost)
    def set_adapters(self, adapter_names, adapter_weights=None):
        self.transformer.set_adapters(adapter_names, adapter_weights)
        return self

    def disable_lora(self):
        self.transformer.disable_lora()
        return self

    def enable_lora(self):
        self.transformer.enable_lora()
        return self

    def unfuse_lora(self):
        self.transformer.unfuse_lora()
        return self

    def delete_adapters(self, adapter_names):
        self.transformer.delete_adapters(adapter_names)
        return self

    def get_active_adapters(self) -> List[str]:
        return self.transformer.get_active_adapters()

    def get_list_adapters(self) -> Dict[str, List[str]]:
        """{component: loaded adapter names}, as diffusers returns it; the adapters target the transformer only."""
        return {"transformer": self.transformer.get_list_adapters()}

    def unload_lora_weights(self):
        self.transformer.unload_lora_weights()
        return self

    # TeaCache step skipping (chronoedit_amd/teacache.py): a switch on the pipeline, `__call__` keeps the reference's signature
    def enable_teacache(self, rel_l1_thresh: float, coefficients=(1.0, 0.0)):
        self.transformer.enable_teacache(rel_l1_thresh, coefficients)
        return self

    def disable_teacache(self):
        self.transformer.disable_teacache()
        return self

    def calibrate_teacache(self, edits, num_inference_steps: int, guidance_scale: float = 5.0, degree: int = 4, **call_kwargs):
        """Fit TeaCache's rescaling polynomial on the loaded checkpoint (after `set_adapters`: LoRA changes the network).  edits: a list of
        keyword dicts, each one edit - the arguments of `edit_tensors` when it carries prompt_embeds, negative_prompt_embeds and image_embeds
        and nothing `edit_tensors` does not take, of `__call__` otherwise; call_kwargs are added to every edit.  Each edit runs measured (`denoise`: every step computes, eagerly; no frames are
        decoded), the (ratio, distance) points of all of them are pooled and fitted.  Returns the teacache.TeaCacheCalibration, whose
        `.coefficients` `enable_teacache(thresh, coefficients)` takes as they are; TeaCache itself is NOT switched on."""
        runs = [lambda kw=kw: self._run_edit(kw, call_kwargs, num_inference_steps, guidance_scale) for kw in edits]
        return self.transformer.calibrate_teacache(runs, degree=degree)

    def _run_edit(self, kw: dict, common: dict, num_inference_steps: int, guidance_scale: float) -> torch.Tensor:
        """One edit dict of `calibrate_teacache` and the measuring methods, `common` added: through `edit_tensors` when it carries the three
        embeds and nothing `edit_tensors` does not take, through `__call__` otherwise -> the edit's final latents."""
        kw = dict(common, **kw, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, output_type="latent")
        tensor_args = set(inspect.signature(self.edit_tensors).parameters)
        res = (self.edit_tensors if {"prompt_embeds", "negative_prompt_embeds", "image_embeds"} <= set(kw) <= tensor_args else self.__call__)(**kw)
        return res if isinstance(res, torch.Tensor) else res.frames

    # Guidance reuse (chronoedit_amd/guidance.py): the unconditional sample only on planned steps.  Off by default; a switch on the
    # pipeline, `__call__` keeps the reference's signature and `edit_tensors` honours it too
    def enable_guidance_reuse(self, pair_every: int = 2, interval=(0.0, 1.0)):
        self.transformer.enable_guidance_reuse(pair_every, interval)
        return self

    def disable_guidance_reuse(self):
        self.transformer.disable_guidance_reuse()
        return self

    def enable_sparse_region(self, refresh_every: int, start: float = 0.0, margin: int = 1):
        """Sparse region edits (chronoedit_amd/sparse_region.py): while an edit region is set (`set_edit_region`), one step in `refresh_every`
        runs the whole model and the others only the tokens under the mask (dilated by `margin` patches), against the keys and values the
        dense step stored; the first `start` of the schedule runs dense.  Off by default; no effect without an edit region."""
        self.transformer.enable_sparse_region(refresh_every, start, margin)
        return self

    def disable_sparse_region(self):
        self.transformer.disable_sparse_region()
        return self

    # Automatic edit regions (chronoedit_amd/auto_region.py): an edit without a mask finds its own region.  Off by default; an explicit
    # `set_edit_region` mask wins
    def enable_auto_region(self, detect_step: int, threshold="otsu", floor: float = 0.0, dilate: int = 1, feather: int = 1,
                           max_area: float = 0.5, composite: bool = True, min_area=0):
        """Behind step `detect_step` the model's estimate of the final image is compared with the source latents (one more VAE encode per
        call, as for an explicit region), the difference thresholded ("otsu", or a number in RMS units of the normalised latents; `floor`
        bounds Otsu's from below), dilated by `dilate` cells and feathered over `feather`; when the region covers at most `max_area` of
        the grid the edit continues as a region-limited one - with `enable_sparse_region`, as a sparse one - and with `composite` the
        source is pasted back behind the decode.  Otherwise it stays the plain edit.  `auto_region_report` tells what happened; its
        "mask" can be repainted and handed to `set_edit_region`.
        min_area (0: off, today's call bit for bit): the seed set - the cells above the threshold - first loses its speckle: its 8-connected
        components of fewer cells than `min_area` (an int >= 1), or than that fraction of the largest one (a float in (0, 1)), are dropped
        on the device (chronoedit_amd/components.py) before it is dilated and feathered; the decision, the sparse plan, the paste-back mask
        and `enable_auto_focus` see the filtered region, the detection step still reads the device once, and `auto_region_report` also
        holds "min_area", "components" (kept), "dropped_components" and "dropped_cells".  `measure_auto_region`'s rows carry "components"
        and "largest_fraction" per step to choose it from."""
        self.transformer.enable_auto_region(detect_step, threshold, floor, dilate, feather, max_area, composite, min_area)
        return self

    def disable_auto_region(self):
        self.transformer.disable_auto_region()
        return self

    # -- live previews (chronoedit_amd/preview.py): off by default
    def enable_preview(self, on_preview, every: int = 1, scale: int = 2, frame: int = -1, composite: bool = True, lag: int = 1, factors=None):
        """While the steps run, `on_preview` gets {"step", "timestep", "image": PIL RGB, "sample", "pass"} for every `every`-th step and the
        last: latent frame `frame` of the model's current estimate of the result through a linear map (`factors`, default
        `preview_factors` as `fit_preview_factors` left it) at `scale` pixels per latent cell.  Step i's picture arrives once step
        i + lag is enqueued, so the loop never waits for it; `pipe._interrupt = True` from the callback stops the edit early.  With an edit
        region and `composite` the kept area shows the source; under region focus the picture is the crop's.  "pass" is "scout" / "focus"
        in an auto-focused call, else None.  The returned frames are those of the call without previews, bit for bit."""
        if factors is None and self.preview_factors is None:
            raise ValueError("enable_preview: no factors - pass factors=, or fit them on the loaded VAE with fit_preview_factors(images)")
        _pv.PreviewConfig(on_preview, every, scale, frame, composite, lag, factors if factors is not None else self.preview_factors)  # validates
        self._preview = dict(on_preview=on_preview, every=every, scale=scale, frame=frame, composite=composite, lag=lag,
                             factors=None if factors is None else _pv.as_factors(factors))
        return self

    def disable_preview(self):
        self._preview = None
        return self

    def _preview_config(self, sample: int = 0, tag=None, crop=None):
        """The preview.PreviewConfig of sample `sample` of this call (None: previews are off): the user's callback gets the loop's dict
        with "sample" and "pass" added - and "crop" = (editor value, crop) when the sample is one crop of a sketch edit with several."""
        if self._preview is None:
            return None
        o = dict(self._preview)
        user = o["on_preview"]
        o["on_preview"] = lambda d: user({**d, "sample": sample, "pass": tag, **({} if crop is None else {"crop": tuple(crop)})})
        if o["factors"] is None:
            if self.preview_factors is None:
                raise ValueError("previews are enabled but preview_factors is None: fit_preview_factors(images), or enable_preview(factors=)")
            o["factors"] = self.preview_factors
        return _pv.PreviewConfig(**o)

    @torch.no_grad()
    def preview_fit_tensors(self, images, height: Optional[int] = None, width: Optional[int] = None):
        """What the fit is made from: (z fp32 [N, 16, 1, h, w], y [N, 3, H, W]) on the device.  Every image goes through the ordinary
        pre-processing and ONE single-frame VAE encode; z is the posterior mode normalised with latents_mean / latents_std as in
        `prepare_latents`; y is z decoded again."""
        height, width = 480 if height is None else int(height), 832 if width is None else int(width)
        if height % 16 != 0 or width % 16 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 16 but are {height} and {width}.")
        images = list(images) if isinstance(images, (list, tuple)) else [images]
        if not images:
            raise ValueError("fit_preview_factors: no images")
        device = self._execution_device
        mean, inv_std = _rg.latent_stats(self.vae, device)
        zs, ys = [], []
        for im in images:
            if image_io.on_device(self.device_image_io, device) and image_io._is_pil(im):
                img = image_io.preprocess_pil(im, height, width, device)
            else:
                img = self.preprocess_image(im, height, width).to(device=device, dtype=torch.bfloat16)
            lat = self.vae.encode(img.unsqueeze(2).to(torch.bfloat16)).latent_dist.mode()
            z = (lat - mean) * inv_std
            y = self.vae.decode(z / inv_std + mean, return_dict=False)[0]
            zs.append(z.float())
            ys.append(y[:, :, 0])
        return torch.cat(zs, dim=0).contiguous(), torch.cat(ys, dim=0).contiguous()

    @torch.no_grad()
    def fit_preview_factors(self, images, height: Optional[int] = None, width: Optional[int] = None):
        """Fit the previews' latent -> RGB map on the loaded VAE: `preview_fit_tensors`, ONE ce_preview_gram_f64 over all images, then
        preview.solve_factors.  Sets `preview_factors`, `preview_fit_report` ({"rms", "r2"} per colour: how well a linear map fits THIS
        checkpoint) and `preview_fit_gram`; returns the factors (fp32 [17, 3])."""
        from . import ops
        z, y = self.preview_fit_tensors(images, height, width)
        if y.dtype not in (torch.bfloat16, torch.float32):
            y = y.float()
        self.preview_fit_gram = ops.preview_gram(z, y.contiguous(), 0).cpu()
        self.preview_factors, self.preview_fit_report = _pv.solve_factors(self.preview_fit_gram)
        return self.preview_factors

    def _auto_region_config(self):
        """(config, measuring) of the next edit without an explicit region; (None, False): the detector is off."""
        if self._auto_region_measure is not None:
            return self._auto_region_measure, True
        return getattr(self.transformer, "_auto_region", None), False

    def measure_auto_region(self, edits, num_inference_steps: int, guidance_scale: float = 5.0, **options):
        """How early the region of an edit shows on the loaded checkpoint: what tells which `detect_step`, threshold and `max_area` suit
        it.  edits: a list of keyword dicts as `calibrate_teacache` takes them; options: the detector's (threshold, floor, dilate, feather,
        max_area), anything else is added to every edit.  Each edit runs the plain loop - the latents are the plain loop's - and every
        step also writes its change map into a [steps, h, w] device table, read back once after the last step.  Returns per edit
        {"timesteps", "steps": per step {"step", "threshold", "active_fraction", "iou" (of that step's seed set with the last step's),
        "components" (8-connected, of the seed set), "largest_fraction" (the largest one's share of the seeds): what `min_area` is chosen
        from}, "latents"}.  The detector itself is NOT switched on, an enabled one and an edit region are ignored here."""
        det = {k: options.pop(k) for k in ("threshold", "floor", "dilate", "feather", "max_area", "min_area") if k in options}
        cfg = _ar.AutoRegionConfig(detect_step=0, **det)
        out, saved = [], self._edit_region
        self._auto_region_measure, self._edit_region = cfg, None
        try:
            for kw in edits:
                self.transformer.auto_region_measurement = None
                latents = self._run_edit(kw, options, num_inference_steps, guidance_scale)
                if self.transformer.auto_region_measurement is None:
                    raise RuntimeError("measure_auto_region: the edit was not measured")
                out.append(dict(self.transformer.auto_region_measurement, latents=latents))
        finally:
            self._auto_region_measure, self._edit_region = None, saved
        return out

    def measure_guidance_reuse(self, edits, num_inference_steps: int, max_age: int = 3, guidance_scale: float = 5.0, keep_deltas: bool = False,
                               **call_kwargs):
        """How fast the guidance direction bf16(c - u) moves on the loaded checkpoint: what tells how large `pair_every` may be.  edits: a
        list of keyword dicts as `calibrate_teacache` takes them.  Each edit runs with every step a "pair" whose store pass also measures
        (`denoise(guidance_measure=max_age)`: eagerly, one read-back per edit after the last step; the latents are the plain loop's; no frames
        are decoded).  Returns per edit {"timesteps", "rel_l2": [steps][max_age]} - rel_l2[i][a - 1] = ||d_i - d_(i-a)|| / ||d_i||, NaN
        where no direction of that age and latent shape exists - plus, with keep_deltas, "deltas" (the per-step directions, on the CPU)
        and always "latents" (the edit's final latents).  Guidance reuse itself is NOT switched on, and an enabled one is ignored here."""
        out = []
        self._guidance_measure = (int(max_age), bool(keep_deltas))
        try:
            for kw in edits:
                self.transformer.guidance_measurement = None
                latents = self._run_edit(kw, call_kwargs, num_inference_steps, guidance_scale)
                if self.transformer.guidance_measurement is None:
                    raise RuntimeError("measure_guidance_reuse: the edit was not measured (more than one sample per call, or no guidance)")
                out.append(dict(self.transformer.guidance_measurement, latents=latents))
        finally:
            self._guidance_measure = None
        return out

    # Region-limited edits (chronoedit_amd/region.py): change what the mask marks, keep the source elsewhere.  Off by default; a switch on
    # the pipeline, `__call__` keeps the reference's signature
    def set_edit_region(self, mask, composite: bool = True):
        """mask: ONE mask for every image of the next calls, or a list with one mask per image - a PIL image, a numpy / torch bool or uint8
        array [height, width], or a float array in [0, 1] (region.normalize_mask; 255 = edit here, 0 = keep the source, greys are weights).
        Stays set until `clear_edit_region()`.  composite: also paste the source back in pixel space behind the decode (the returned
        frames then carry the source's bytes exactly where the mask is 0); False: the latent-space blend alone.
        With `enable_region_focus()` the mask is taken at the SOURCE image's size and the edit runs on a crop around it."""
        if mask is None:
            raise ValueError("set_edit_region needs a mask (clear_edit_region() switches the region off)")
        self._edit_region = (list(mask) if isinstance(mask, (list, tuple)) else mask, bool(composite))
        return self

    def clear_edit_region(self):
        self._edit_region = None
        return self

    # Focused region edits (chronoedit_amd/focus.py): crop to the mask, edit the crop, paste back at the source's size.  Off by default
    def enable_region_focus(self, context: float = 0.25):
        """While an edit region is set (`set_edit_region`, its mask now at the SOURCE image's size - a PIL mask of another size is resized
        to it, an array or tensor must be [source height, source width]), every call crops a box of the edit's aspect ratio around the
        mask's bounding box, padded by `context` times its longer side (focus.focus_box), edits the crop at width x height as an ordinary
        region edit - sparse steps, TeaCache, guidance reuse, temporal reasoning and graph replay compose and refuse as they do there -
        and pastes every returned frame, scaled back to the box, into the untouched source: "pil" frames have the SOURCE's size, "np" /
        "pt" carry the same bytes / 255 (the sources of one call must then share a size), "latent" returns the crop's latents.
        composite=True pastes through the source-size mask (the source's bytes exactly where it is 0), composite=False replaces the whole
        box.  `image` must be PIL, one or a list (a ValueError otherwise: an array has no full-resolution bytes to paste into).
        `focus_report` holds one dict per image afterwards (focus.plan shows the same before an edit is spent).
        No effect without an explicit mask: with only `enable_auto_region` the call is the plain call - a detected mask arrives mid-edit,
        which is too late to re-crop; `enable_auto_focus` is the switch that starts over on the crop."""
        _fc.focus_box(None, (1, 1), (1, 1), context)  # (validates the context)
        self._region_focus = float(context)
        return self

    def disable_region_focus(self):
        self._region_focus = None
        return self

    # Auto-focused edits (chronoedit_amd/autofocus.py): find the region on the whole photo, then edit its crop at the photo's size.  Off by default
    def enable_auto_focus(self, context: float = 0.25, warm_start: bool = False):
        """While `enable_auto_region` is on and no `set_edit_region` mask is set (an explicit mask wins, as ever), a call with ONE PIL
        image first runs the auto-region call on the whole photo up to and including the detection behind step k (the scout).  Declined,
        or a box that is the whole photo: the scout runs on to its end and the call returns exactly what the auto-region call returns,
        `focus_report[0]["reason"]` = "declined" / "whole".  Accepted: the detected mask is lifted to the photo's size on the device, and the
        call starts over as the focused region edit (`enable_region_focus`) of the crop around it, padded by `context`, from the SAME noise
        (the call's one draw, or `latents=`), composite as `enable_auto_region` says: the frames have the photo's size and carry its
        bytes wherever the mask is 0.  warm_start=False: all steps - bit for bit the call that `set_edit_region(focus_report[0]["mask"])`
        + `enable_region_focus(context)` would make with the same `latents`.  warm_start=True: from step k + 1, on the scout's estimate of
        the final image cropped and resampled to the crop's latent grid and noised to that step's level (autofocus.restart).
        `focus_report[0]` holds the focus plan plus "mask" (the photo-size mask, a PIL "L" image), "detect" (the scout's auto-region
        report) and "start_step"; `callback_on_step_end` sees the scout's steps 0..k, then the focused pass's.  An array or tensor image
        is a ValueError; more than one sample per call, temporal reasoning and `offload_model` a NotImplementedError."""
        self._auto_focus = _af.AutoFocusConfig(float(context), warm_start)
        return self

    def disable_auto_focus(self):
        self._auto_focus = None
        return self

    # Sketch edits (chronoedit_amd/sketch.py): the region is where the editor's composite differs from its background.  Off by default
    def enable_sketch_region(self, grow=0.02, feather=0.01, threshold: int = 0, context: float = 0.25, composite: bool = True, min_stroke=0,
                             max_crops: int = 1, strokes: str = "difference", alpha_threshold: int = 0, layer_prompts: bool = False):
        """While on and no `set_edit_region` mask is set, `__call__(image=...)` also takes an image editor's value: a dict with PIL images
        under "background" (the photo) and "composite" (the photo with the strokes on it) - other keys, such as "layers", are ignored -, or
        a list of such dicts, one per prompt.  Per value the mask is built at the PHOTO's size before the first step (sketch.reference:
        changed by more than `threshold` in a channel -> grown by grow + feather -> box mean of radius feather; on the device with
        `device_image_io`, csrc/ce_sketch.hip, the same bytes; one read of ten integers per image before the edit - the report's copy of
        the mask is made behind it), and the call goes on as the focused
        region edit (`enable_region_focus(context)`, `set_edit_region(mask, composite)`: what that call composes with or refuses, this one
        does) with ONE difference: the crop that the VAE, CLIP and the kept latents see is the COMPOSITE's, the frames are pasted into the
        BACKGROUND - the photo untouched wherever the mask is 0, the model's pixels where the user drew.  grow, feather: an int is pixels
        of the photo, a float in [0, 1) that fraction of its longer side, rounded up (grow + feather <= 4096, feather <= 1024 pixels, a
        ValueError otherwise - for fractions, at the call).  The defaults are choices, not measurements.
        No strokes in any value: the plain call on the composite(s), bit for bit, `sketch_report[i]["reason"]` = "empty".  A plain PIL
        image, array or tensor is the call it is without the switch (`sketch_report` None).  With a `set_edit_region` mask the explicit mask
        wins: an editor value then stands for its composite.  A value whose two images differ in size, or that lacks one, is a ValueError.
        `sketch_report` holds per value the focus plan's entries (`focus_report`'s) plus "mask" (PIL "L", the photo's size), "grow_px",
        "feather_px", "threshold" and "changed_pixels".
        min_stroke (0: off, today's call bit for bit, no launch): drop speckle.  The grown strokes fall into clusters - the 8-connected
        components of the grown plane, i.e. strokes within 2 (grow + feather) of each other -, each weighted by the changed pixels it holds;
        clusters below `min_stroke` changed pixels (an int >= 1), or below that fraction of the heaviest cluster (a float in (0, 1)), leave
        the mask before it is feathered (chronoedit_amd/components.py; csrc/ce_components.hip on the device, the same bits, and the
        one read grows to fourteen integers).  One stray pixel far from the sketch then no longer stretches the box to the whole photo.
        A dropped cluster's strokes are not pasted: there the frames carry the background, and "composite and background agree wherever
        the mask is below 255" holds outside the dropped clusters.  All clusters dropped (an int only): "empty", the plain call on the
        composite.  `sketch_report[i]` then also holds "min_stroke", "clusters" (kept), "dropped_clusters" and "dropped_pixels" (changed
        pixels of the dropped clusters); `sketch_mask` applies the filter too.
        max_crops (1: one box around every kept stroke, today's call bit for bit - same launches, same reads; an int in 1..16): with 2 or
        more, every editor value is edited as up to `max_crops` focused crops, one per GROUP of stroke clusters, and still returns ONE video
        at the photo's size (chronoedit_amd/clusters.py; csrc/ce_clusters.hip on the device, the same bytes).  The clusters' table - label,
        bounding box, pixels, weight per kept cluster - rides on the one read; clusters whose crops would intersect are grouped, then the
        groups whose union is smallest until at most `max_crops` are left (clusters.group: integers only); each group gets its own
        feathered mask and its own box through the single-box call's route, at the price of ONE more read of five integers per group.  The
        crops run as the samples of one focused call, one after the other - whatever composes with a focused region edit composes per
        crop -, each from ITS VALUE's prompt, noise row (drawn as the single-box call draws it, then repeated) and `image_embeds` row; the
        text encoder runs once per prompt, CLIP sees each crop.  Behind the decode the crops are pasted into the background in order
        (PIL's paste, chained: clusters.host_paste).  `sketch_report[i]` keeps its keys, computed from the union mask - its "box" is what
        the single-box call would have used - and gains "max_crops", "crops" (per crop that ran, in paste order: "box", "reason", "scale",
        "mask_fraction_of_box", "clusters" (labels), "mask") and "crops_reason": "crops" (two or more crops ran), or the single-box call,
        bit for bit, because of "single" (one group), "many" (more than 256 clusters) or "unfit" (some group's box is not "ok").
        `focus_report` is the flat list of the plans that ran; previews carry "sample" = the flat crop index and "crop" = (value, crop).
        output_type "latent" returns the crops' latents, flat.  `num_videos_per_prompt > 1` with a value of two or more crops is a
        NotImplementedError.  How a checkpoint edits two crops of one photo consistently is the checkpoint's business; the default of 1
        is a choice, not a measurement.
        strokes ("difference": today's call bit for bit, no new launch; "layers" is ignored then and layer_prompts=True a ValueError):
        with "layers" the strokes are where the editor's LAYERS say the user drew (chronoedit_amd/layers.py; csrc/ce_layers.hip on the
        device, the same bytes): changed = 255 where some layer's alpha > `alpha_threshold` (an int in 0..254) - a black stroke on a dark
        part of the photo is found, a lossy composite needs no threshold.  The value must hold "layers": a list (possibly empty) of PIL
        images of the background's size whose mode has an alpha channel, used as `convert("RGBA")`; anything else is a ValueError before
        anything runs.  Each layer is uploaded as its alpha bounding box only; the one read stays one read per value.  "composite" may be
        missing or None: it is then built, `Image.alpha_composite` of the layers over the background in order, and
        `sketch_report[i]["composite"]` holds it (PIL).  A given composite is what the model sees, as today.  `sketch_report[i]` gains
        "strokes" and "alpha_threshold"; everything behind `changed` is the chain above.
        layer_prompts (needs strokes="layers"): ONE editor value plus one prompt per layer (a list of L prompts, or L rows of
        `prompt_embeds`; a layer without strokes consumes its prompt) is ONE edit.  Each layer with strokes is an entry of its own -
        (background, the layer alone over the background, the layer's alpha) - through the chain above, with its own clusters, groups
        and crops under max_crops >= 2; all plans run as the samples of one focused pass, each from its LAYER's prompt row (the text
        encoder runs once per prompt, CLIP per crop, the noise drawn as the single-box call draws it for one value, then repeated), and
        are pasted into the BACKGROUND in layer order, then crop order: where two layers' masks overlap the later layer wins.  At most two
        host reads per layer with strokes in front of the edit (the layer's counts; its groups' boxes).  `sketch_report[0]` then holds
        "reason": "layers", "source_size", "edit_size", "grow_px", "feather_px", "threshold", "strokes", "alpha_threshold",
        "changed_pixels" (all layers'), "max_crops", "crops" (as above, each with "layer") and "layers": per layer {"bbox" (its mask's),
        "stroke_pixels", "reason"} - "empty" for a layer without strokes.  Refused on the host, before anything is uploaded or launched: a
        number of prompts other than L, no alpha above the threshold in any layer, more than 16 layers with strokes under max_crops == 1 and
        min_stroke == 0 (ValueError); a list of editor values, num_videos_per_prompt > 1 (NotImplementedError).  What only the chain knows
        is refused behind the layers' mask chains and before any encoder or the VAE runs: every stroke dropped by min_stroke, more than 16
        plans in all under min_stroke or max_crops >= 2 (ValueError).  An explicit `set_edit_region` mask still wins: the value stands for its composite (built if absent) and
        takes one prompt.  What a checkpoint makes of per-layer composites is the checkpoint's business."""
        self._sketch_region = _sk.SketchConfig(grow, feather, threshold, context, composite, min_stroke, max_crops, strokes, alpha_threshold,
                                               layer_prompts)
        return self

    def disable_sketch_region(self):
        self._sketch_region = None
        return self

    def _sketch_entry(self, background, composite, layers) -> dict:
        """The `sketch.masks` entry of one (background, composite, layers) with the enabled parameters: what sketch_mask / sketch_crops show."""
        cfg = self._sketch_region
        value = {"background": background, "composite": composite}
        by_layers = cfg.strokes == "layers"
        bgs, cps = _sk.editor_images(value, need_composite=not by_layers)
        lys = [_ly.editor_layers(value, 0, layers)] if by_layers else None
        device = self._execution_device
        return _sk.masks(cfg, bgs, cps, device if image_io.on_device(self.device_image_io, device) else None, lys)[0]

    def sketch_mask(self, background, composite, layers=None):
        """The mask a sketch call would build for this pair of PIL images with the enabled parameters, as a PIL "L" image of their size - for
        a front end to show before an edit is spent.  With strokes="layers": `layers` is the editor's list of layers (required; the
        composite may be None), and the mask is the union over the layers, whatever `layer_prompts` says."""
        from PIL import Image
        if self._sketch_region is None:
            raise ValueError("sketch_mask needs the parameters of enable_sketch_region(): the switch is off")
        e = self._sketch_entry(background, composite, layers)
        return Image.fromarray(_sk.host_mask(e).numpy(), mode="L")  # (no edit follows: the copy of the mask may be made here)

    def sketch_crops(self, background, composite, height: int, width: int, layers=None) -> list:
        """The crops a sketch call at width x height would run for this pair of PIL images with the enabled parameters, without running an
        edit: a list of {"box", "reason", "scale", "mask_fraction_of_box", "clusters" (labels), "mask" (PIL "L", the photo's size)} in paste
        order - `sketch_report[i]["crops"]`.  One entry (the single-box plan) with max_crops == 1 or when the call would fall back to it.
        With strokes="layers": `layers` as in `sketch_mask`; the crops are those of the union of the layers (a call with `layer_prompts`
        plans every layer on its own)."""
        if self._sketch_region is None:
            raise ValueError("sketch_crops needs the parameters of enable_sketch_region(): the switch is off")
        cfg = self._sketch_region
        e = self._sketch_entry(background, composite, layers)
        single = _sk.focus_plan(e, width, height, cfg.context)
        crops = _cl.plan(e, cfg.max_crops, width, height, cfg.context) if cfg.max_crops >= 2 else _cl.Crops("single")
        return _cl.crop_reports(crops, single)

    # Guided detail lift (chronoedit_amd/lift.py): whole-image edits returned at the photo's size.  Off by default
    def enable_detail_lift(self, radius: int = 4, eps: float = 26.0, gate=(4.0, 12.0), max_gain: float = 8.0, focus: bool = False,
                           mask_aware: bool = False):
        """While on, a call with PIL input (one image, or a list with one per prompt) and output_type "pil" / "np" / "pt" returns every frame
        - reasoning frames included, behind the edit-size region composite if there is one - at the IMAGE's own size: per edit-size
        neighbourhood and colour an affine map from the resized photo to the edit's change is fitted (window radius `radius` cells,
        regulariser `eps` in squared bytes, |slope| <= `max_gain`), the maps are smoothed, sampled at the photo's pixel centres and applied to
        the photo's own bytes; where the smoothed map leaves a mean residual between gate[0] and gate[1] bytes the plain Lanczos upsample
        of the edited frame is blended in, and beyond gate[1] it replaces the lift (gate=None: no fallback, and no Lanczos pass).  "np" /
        "pt" carry the "pil" bytes / 255 (the images of one call must then share a size), "latent" is untouched.  A focused call (an explicit
        mask under `enable_region_focus`, or an accepted auto focus) returns what focus returns: `lift_report` says "reason": "focus"; a
        declined auto focus is lifted.  An image already of the edit's size returns the plain frames ("reason": "same").  An array or tensor
        `image` is a ValueError.  The lift runs behind the decode (csrc/ce_lift.hip; lift.reference on the host with
        `enable_device_image_io(False)`, the same bytes), never inside a captured graph.  `lift_report` holds per sample {"size",
        "edit_size", "applied", "reason", "fallback_fraction"}: the last is the mean of the gate - how much of the picture was plain
        upsampling.
        focus=True: a focused pass - an explicit mask under `enable_region_focus`, an accepted auto focus (cold or warm start), a sketch
        edit with one box, with one crop per stroke cluster, or with a prompt per layer - no longer stands back: every crop is lifted
        INSIDE its box before the paste (chronoedit_amd/boxlift.py): P is the box of the image the VAE saw, L the resized crop the
        pre-processing fed it, and the lifted box goes through the photo-size mask into the paste source (csrc/ce_boxlift.hip fuses the
        apply with the paste; `boxlift.reference` on the host, the same bytes).  `lift_report` then holds one entry per sample - per
        crop - with "size" = the box's size, "reason" "ok" or "same" (a box of exactly the edit's size: the plain paste), and "box" and
        "scale" on top.  `focus_report` / `sketch_report`, and everything a focused edit composes with or refuses, stay as they are.
        mask_aware=True (needs focus=True): a region edit blends its latents with the source, so a crop's frames carry the change TAPERED by
        the region's weight, and the plain fit misreads the feathered rim.  Every crop that is lifted inside its box and pasted through
        its mask is then fitted under its edit-size mask (chronoedit_amd/rimlift.py, csrc/ce_rimlift.hip): the lift recovers the untapered
        edit and applies it at full strength, and the paste's photo-size mask tapers it once.  `composite=False` and boxes of the edit's
        size keep the plain path.  While it is on every `lift_report` entry says "mask_aware": whether that sample was fitted this way.  A
        rising `fallback_fraction` under the switch means the frames' taper does not follow the mask; the fallback is the plain upsample."""
        if self._tiled is not None:
            raise ValueError("enable_detail_lift while tiled edits are on (enable_tiled_edit): two ways to reach the photo's size - "
                             "disable_tiled_edit() first")
        if not isinstance(focus, bool):
            raise ValueError(f"detail lift: focus must be True or False, got {focus!r}")
        if not isinstance(mask_aware, bool):
            raise ValueError(f"detail lift: mask_aware must be True or False, got {mask_aware!r}")
        if mask_aware and not focus:
            raise ValueError("detail lift: mask_aware=True needs focus=True (the masked fit runs on the crops of focused edits)")
        self._detail_lift = _lf.LiftConfig(radius, eps, None if gate is None else tuple(gate) if isinstance(gate, (tuple, list)) else gate, max_gain)
        self._detail_lift_focus = focus
        self._detail_lift_mask_aware = mask_aware
        return self

    def disable_detail_lift(self):
        self._detail_lift = None
        self._detail_lift_focus = False
        self._detail_lift_mask_aware = False
        return self

    # Tiled edits (chronoedit_amd/tiles.py): a whole photo at full size as overlapping model-size tiles, fused per step.  Off by default
    def enable_tiled_edit(self, size=None, overlap=0.25, clip: str = "tile", max_tiles: int = _tl.MAX_TILES):
        """While on, `__call__(image, prompt, height=, width=)` with ONE PIL image edits the whole photo at the TARGET's size - `size` None: the
        photo's own, (W, H): that size, a float > 0: that scale of the photo's size (a photo of another size is first resized to the target,
        Lanczos, on the device or by PIL as `enable_device_image_io` says) - as overlapping tiles of width x height: height x width is the TILE.
        The target's sides rounded up to multiples of 16 are the canvas (the image is padded right and bottom by edge replication); per axis
        the fewest tiles cover it whose neighbours share at least `overlap` - a float in (0, 0.5]: that fraction of the tile's side, rounded
        up to a multiple of 16 px; an int: pixels, a multiple of 16 - at origins that are multiples of 16 (tiles.axis_origins; `tile_plan`
        shows the plan before an edit is spent, `tile_report` holds it afterwards plus "reason": "tiled" or "single").  The tiles run as the
        samples of ONE batched pass, each from the prompt's row, its own VAE condition and - clip="tile" - CLIP on its own pixels
        (clip="photo": CLIP once on the target image, the row repeated); `generator` draws ONE canvas of noise [1, 16, T, CH / 8, CW / 8]
        (`latents=` is taken at that shape) that is cut into the tiles.  Behind every scheduler update the tiles' latents are averaged on the
        canvas under integer tent weights and cut again (two launches, inside the captured step; csrc/ce_tiles.hip); the scheduler's history
        stays per tile.  All tiles are decoded and blended in exact integers under the same tents in pixels, straight into the target's
        frame: "pil" / "np" / "pt" frames have the TARGET's size ("np" / "pt": the bytes / 255), "latent" returns the canvas latents
        [1, 16, T, CH / 8, CW / 8].  With `enable_device_image_io(False)` the blend is tiles.reference_blend on the CPU, the same bytes.
        A canvas that equals one tile ("single") is the plain call on the image, bit for bit - its frames then have the TILE's size, which
        is the canvas's, also where the target is smaller (a 90x60 photo under a 96x64 tile); `tile_report["frames"]` says which size came
        back.  More than `max_tiles` (1..16) tiles, or a
        canvas side below the tile's, is a ValueError.  `callback_on_step_end` sees the tiles' latents [n, 16, T, th, tw] behind the fusion;
        latents it returns go into the next step as they are and are fused behind it, and behind the last step they are fused once more before
        they are decoded or returned.
        Refused while the switch is on, before anything runs - NotImplementedError: a list of images or prompts, num_videos_per_prompt > 1,
        temporal reasoning, previews, TeaCache, guidance reuse, offload_model, sharded tokens or CFG parallelism, a measuring edit
        (measure_guidance_reuse, measure_auto_region, calibrate_teacache); ValueError: an array or
        tensor image, an edit region in force (an explicit mask, auto region, auto focus, a sketch editor value) and `enable_detail_lift`.
        Whether a checkpoint edits the tiles of one photo consistently is the checkpoint's business."""
        cfg = _tl.TileConfig(tuple(size) if isinstance(size, list) else size, overlap, clip, max_tiles)
        if self._detail_lift is not None:
            raise ValueError("enable_tiled_edit while the detail lift is on (enable_detail_lift): two ways to reach the photo's size - "
                             "disable_detail_lift() first")
        self._tiled = cfg
        return self

    def disable_tiled_edit(self):
        self._tiled = None
        return self

    def tile_plan(self, image_size, height: int, width: int) -> dict:
        """The plan a tiled call at width x height would run for a photo of image_size = (W, H) with the enabled parameters, without running
        anything: {"source_size", "target", "canvas", "tile" (all (width, height)), "origins" (row-major, the batch order), "grid",
        "overlaps" (per axis, between neighbours), "min_overlap", "count", "frames" (the size of the returned frames: the target's, or - one
        tile - the tile's)} - `tile_report`'s entries."""
        if self._tiled is None:
            raise ValueError("tile_plan needs the parameters of enable_tiled_edit(): the switch is off")
        c = self._tiled
        return _tl.plan(image_size, height, width, c.size, c.overlap, c.max_tiles).report

    def _measure_kwargs(self) -> dict:
        """What `denoise` gets on top while measure_guidance_reuse runs."""
        if self._guidance_measure is None:
            return {}
        return {"guidance_measure": self._guidance_measure[0], "keep_deltas": self._guidance_measure[1]}

    # -- image pre / post processing (diffusers VideoProcessor, pipeline_chronoedit.py:673,801; the bodies are image_io's) ---
    preprocess_image = staticmethod(image_io.preprocess_image)
    postprocess_video = staticmethod(image_io.postprocess_video)

    # -- the call (pipeline_chronoedit.py:484-812) -----------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, image=None, prompt: Union[str, List[str], None] = None, negative_prompt: Union[str, List[str], None] = None,
                 height: int = 480, width: int = 832, num_frames: int = 81, num_inference_steps: int = 50, guidance_scale: float = 5.0,
                 num_videos_per_prompt: Optional[int] = 1, generator=None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                 image_embeds: Optional[torch.Tensor] = None, output_type: Optional[str] = "np", return_dict: bool = True,
                 attention_kwargs: Optional[Dict[str, Any]] = None, callback_on_step_end: Optional[Callable] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 512,
                 enable_temporal_reasoning: bool = False, num_temporal_reasoning_steps: int = 0, offload_model: bool = False):
        """Same arguments, defaults, checks and return value as the reference's `__call__`.  What differs is underneath: the two
        guidance passes run as ONE batched forward, CFG + flow-UniPC are one fused launch, the latents stay fp32 on the device
        (`scheduler.trajectory_dtype = torch.bfloat16` restores the reference's bf16 rounding of latents and history)."""
        args = CallArgs(**{k: v for k, v in locals().items() if k != "self"})  # (the first statement: the locals are the arguments)
        self.sketch_report = None
        if self._tiled is not None:  # tiled edits (chronoedit_amd/tiles.py): the whole photo at the target's size - or the refusal
            return self._tiled_edit(args)
        self.tile_report = None
        if _sk.is_editor_value(image):  # an image editor's value: the sketch edit (chronoedit_amd/sketch.py) - or its refusal
            return self._sketch_edit(args)
        return self._edit(args)

    def _sketch_edit(self, a: CallArgs):
        """`__call__` with an editor's value (or a list of them) as `image`: see `enable_sketch_region`."""
        from PIL import Image
        if self._sketch_region is None:
            raise ValueError("`image` is an image editor's value (a dict with \"background\" and \"composite\"): switch sketch edits on with "
                             "enable_sketch_region() first, or pass the composite itself")
        cfg = self._sketch_region
        by_layers = cfg.strokes == "layers"
        several = isinstance(a.image, (list, tuple))
        bgs, cps = _sk.editor_images(a.image, need_composite=not by_layers)
        lys = [_ly.editor_layers(v, i) for i, v in enumerate(a.image if several else [a.image])] if by_layers else None
        if self._edit_region is not None:  # an explicit mask wins: the editor value stands for its composite (built if it has none)
            if by_layers:
                cps = [cp if cp is not None else _ly.composite(bg, _ly.boxes(ls)) for bg, cp, ls in zip(bgs, cps, lys)]
            return self._edit(replace(a, image=cps if several else cps[0]))
        if cfg.layer_prompts:
            return self._sketch_layers_edit(a, cfg, several, bgs[0], lys[0])
        if a.output_type in ("np", "pt") and len({im.size for im in bgs}) > 1:
            raise ValueError(f"a sketch edit returns frames of the photos' sizes {[im.size for im in bgs]}: output_type={a.output_type!r} "
                             'needs photos of one size, use "pil"')
        device = self._execution_device
        entries = _sk.masks(cfg, bgs, cps, device if image_io.on_device(self.device_image_io, device) else None, lys)
        cps = [e["composite"] for e in entries]  # (a value without one: built from its layers)
        a = replace(a, image=cps if several else cps[0])
        plans = [_sk.focus_plan(e, a.width, a.height, cfg.context) for e in entries]
        crops = [_cl.plan(e, cfg.max_crops, a.width, a.height, cfg.context) for e in entries] if cfg.max_crops >= 2 else None
        if all(e["bbox"] is None for e in entries):  # no strokes anywhere: the plain call on the composite(s)
            out = self._edit(a)
        elif crops is not None and any(c.reason == "crops" for c in crops):
            out = self._sketch_crops_edit(a, cfg, plans, crops)
        else:
            out = self._edit(a, FocusPass(plans, cfg.composite))
        # behind the edit: the device path copies its masks to the host here, not in front of the first step
        self.sketch_report = [dict(p.report, mask=Image.fromarray(p.host_mask().numpy(), mode="L"), grow_px=e["grow_px"], feather_px=e["feather_px"],
                                   threshold=cfg.threshold, changed_pixels=e["changed_pixels"]) for p, e in zip(plans, entries)]
        if cfg.min_stroke:
            for rep, e in zip(self.sketch_report, entries):
                rep.update(min_stroke=cfg.min_stroke, clusters=e["clusters"], dropped_clusters=e["dropped_clusters"], dropped_pixels=e["dropped_pixels"])
        if crops is not None:
            for rep, p, c in zip(self.sketch_report, plans, crops):
                rep.update(max_crops=cfg.max_crops, crops=_cl.crop_reports(c, p), crops_reason=c.reason)
        if by_layers:
            for rep, e in zip(self.sketch_report, entries):
                rep.update(strokes=cfg.strokes, alpha_threshold=cfg.alpha_threshold, **({"composite": e["composite"]} if e.get("built") else {}))
        return out

    def _sketch_layers_edit(self, a: CallArgs, cfg, several: bool, bg, layers: list):
        """The sketch edit with a prompt per layer (`enable_sketch_region(strokes="layers", layer_prompts=True)`): every layer with strokes
        is planned on its own - the layer alone over the background, its alpha as `changed` - and all plans run as the samples of ONE focused
        pass, each from its layer's prompt row; `_output` chains them into one video over the background (clusters.paste), in layer order,
        then crop order.  In front of the edit at most two host reads per layer with strokes: the layer's counts, its groups' boxes."""
        if several:
            raise NotImplementedError("a sketch edit with a prompt per layer takes ONE editor value, not a list of them: run the values one call each")
        if a.num_videos_per_prompt != 1:
            raise NotImplementedError("a sketch edit with a prompt per layer and num_videos_per_prompt > 1 is not implemented: run the videos "
                                      "one call each")
        a, device = self._begin(replace(a, image=bg), guarded=False)  # (host checks only: nothing is launched)
        L, n = len(layers), self._prompt_count(a)
        if n != L:
            raise ValueError(f"a sketch edit with a prompt per layer needs one prompt per layer, empty layers included: got {n} prompt(s) for {L} layer(s)")
        # what the layers' bytes decide on the host, before anything is uploaded: no alpha above the threshold anywhere; and, where
        # neither the speck filter nor the grouping can change the number of plans, too many of them
        stroked = [lb for lb in _ly.boxes(layers) if bool((lb.rgba[:, :, 3] > cfg.alpha_threshold).any())]
        none = (f"a sketch edit with a prompt per layer found no stroke in any of the {L} layer(s): there is no plain call to fall back to with "
                "several prompts")
        many = f"a sketch edit with a prompt per layer runs at most {_cl.MAX_CROPS} crops in all, the layers ask for {{}}: lower max_crops, or merge layers"
        if not stroked:
            raise ValueError(none)
        if not cfg.min_stroke and cfg.max_crops == 1 and len(stroked) > _cl.MAX_CROPS:
            raise ValueError(many.format(len(stroked)))
        entries = _sk.layer_entries(cfg, bg, layers, device if image_io.on_device(self.device_image_io, device) else None, stroked)
        flat, crop_of, row_of, singles, crops = [], [], [], {}, {}
        for k, e in enumerate(entries):
            if e is None:
                continue
            singles[k] = _sk.focus_plan(e, a.width, a.height, cfg.context)
            crops[k] = _cl.plan(e, cfg.max_crops, a.width, a.height, cfg.context) if cfg.max_crops >= 2 else _cl.Crops("single")
            for q in crops[k].plans if crops[k].reason == "crops" else [singles[k]]:
                crop_of.append((0, len(flat))), flat.append(q), row_of.append(k)
        if not flat:  # (the speck filter dropped every stroke)
            raise ValueError(none)
        if len(flat) > _cl.MAX_CROPS:  # (known only behind the chain: the filter and the grouping decide how many plans there are)
            raise ValueError(many.format(len(flat)))
        _, prompt_embeds, negative_prompt_embeds = self._encode_text(a, device)  # the text encoder: once per prompt
        rows = torch.tensor(row_of, dtype=torch.long)
        repeat = lambda t: None if t is None else t.index_select(0, rows.to(t.device))
        noise = a.latents
        if noise is None:  # what the single-box call would draw for one value
            if isinstance(a.generator, list) and len(a.generator) != 1:
                raise ValueError(f"You have passed a list of generators of length {len(a.generator)}, but requested an effective batch"
                                 f" size of 1. Make sure the batch size matches the length of the generators.")
            T = (a.num_frames - 1) // self.vae_scale_factor_temporal + 1
            shape = (1, self.vae.config.z_dim, T, a.height // self.vae_scale_factor_spatial, a.width // self.vae_scale_factor_spatial)
            noise = _randn_tensor(shape, a.generator, device, torch.bfloat16)
        elif noise.shape[0] != 1:
            raise ValueError(f"`latents` carry {noise.shape[0]} samples, expected one for the editor value")
        image_embeds = a.image_embeds
        if image_embeds is not None:
            if image_embeds.shape[0] not in (1, len(flat)):
                raise ValueError(f"`image_embeds` carry {image_embeds.shape[0]} samples, expected 1 or one per crop ({len(flat)})")
        out = self._edit(replace(a, image=[q.image for q in flat], prompt=None, negative_prompt=None, prompt_embeds=repeat(prompt_embeds),
                                 negative_prompt_embeds=repeat(negative_prompt_embeds), image_embeds=image_embeds,
                                 latents=noise.repeat(len(flat), 1, 1, 1, 1), generator=None),
                         FocusPass(flat, cfg.composite, guarded=True, crop_of=crop_of))
        # behind the edit: the masks' copies for the report
        stroked = [e for e in entries if e is not None]
        per_crop = [dict(c, layer=k) for k in crops for c in _cl.crop_reports(crops[k], singles[k])]
        self.sketch_report = [dict(reason="layers", source_size=bg.size, edit_size=(int(a.width), int(a.height)), grow_px=stroked[0]["grow_px"],
                                   feather_px=stroked[0]["feather_px"], threshold=cfg.threshold, strokes=cfg.strokes,
                                   alpha_threshold=cfg.alpha_threshold, changed_pixels=sum(e["changed_pixels"] for e in stroked),
                                   max_crops=cfg.max_crops, crops=per_crop,
                                   layers=[{"bbox": None, "stroke_pixels": 0, "reason": "empty"} if e is None else
                                           {"bbox": e["bbox"], "stroke_pixels": e["changed_pixels"], "reason": singles[k].report["reason"]
                                            if crops[k].reason != "crops" else "crops"} for k, e in enumerate(entries)])]
        return out

    def _sketch_crops_edit(self, a: CallArgs, cfg, plans: list, crops: list):
        """The sketch edit in which some value has two or more crops: the flat list of crops - a value without them contributes its single-box
        plan - runs as the samples of ONE focused pass, each from its value's rows of the embeds and of the noise; `_output` chains the
        crops of a value into one video (clusters.paste)."""
        if a.num_videos_per_prompt != 1:
            raise NotImplementedError("a sketch edit with two or more crops per photo and num_videos_per_prompt > 1 is not implemented: "
                                      "run the videos one call each, or enable_sketch_region(max_crops=1)")
        a, device = self._begin(a, guarded=False)
        n, prompt_embeds, negative_prompt_embeds = self._encode_text(a, device)  # the text encoder: once per prompt
        if n != len(plans):
            raise ValueError(f"a sketch edit with several crops per photo needs one prompt per editor value: got {n} prompt(s) for {len(plans)} value(s)")
        flat, crop_of = [], []
        for v, (p, c) in enumerate(zip(plans, crops)):
            for g, q in enumerate(c.plans if c.reason == "crops" else [p]):
                flat.append(q), crop_of.append((v, g))
        rows = torch.tensor([v for v, _ in crop_of], dtype=torch.long)
        repeat = lambda t: None if t is None else t.index_select(0, rows.to(t.device))
        noise = a.latents
        if noise is None:  # what the single-box call would draw: one row per value
            if isinstance(a.generator, list) and len(a.generator) != n:
                raise ValueError(f"You have passed a list of generators of length {len(a.generator)}, but requested an effective batch"
                                 f" size of {n}. Make sure the batch size matches the length of the generators.")
            T = (a.num_frames - 1) // self.vae_scale_factor_temporal + 1
            shape = (n, self.vae.config.z_dim, T, a.height // self.vae_scale_factor_spatial, a.width // self.vae_scale_factor_spatial)
            noise = _randn_tensor(shape, a.generator, device, torch.bfloat16)
        elif noise.shape[0] != n:
            raise ValueError(f"`latents` carry {noise.shape[0]} samples, expected one per editor value: {n}")
        image_embeds = a.image_embeds
        if image_embeds is not None:
            if image_embeds.shape[0] not in (1, n, len(flat)):
                raise ValueError(f"`image_embeds` carry {image_embeds.shape[0]} samples, expected 1, one per editor value ({n}) or one per crop ({len(flat)})")
            if image_embeds.shape[0] == n:
                image_embeds = repeat(image_embeds)
        a = replace(a, image=[q.image for q in flat], prompt=None, negative_prompt=None, prompt_embeds=repeat(prompt_embeds),
                    negative_prompt_embeds=repeat(negative_prompt_embeds), image_embeds=image_embeds, latents=repeat(noise), generator=None)
        return self._edit(a, FocusPass(flat, cfg.composite, guarded=True, crop_of=crop_of))

    def _tiled_refusals(self, a: CallArgs):
        """What a tiled edit does not compose with, refused before anything runs; every message names the switch."""
        off = "disable_tiled_edit() first"
        if _sk.is_editor_value(a.image) or self._edit_region is not None or getattr(self.transformer, "_auto_region", None) is not None \
                or self._auto_focus is not None:
            raise ValueError("tiled edits (enable_tiled_edit) edit the whole photo: an edit region - set_edit_region, enable_auto_region, "
                             f"enable_auto_focus or a sketch editor value - is a second way to decide what is edited; clear it, or {off}")
        if self._detail_lift is not None:
            raise ValueError("tiled edits (enable_tiled_edit) and enable_detail_lift are two ways to reach the photo's size: "
                             f"disable_detail_lift(), or {off}")
        if isinstance(a.image, (list, tuple)) or isinstance(a.prompt, (list, tuple)) or (a.prompt_embeds is not None and a.prompt_embeds.shape[0] != 1):
            raise NotImplementedError(f"tiled edits (enable_tiled_edit) take ONE image and ONE prompt per call: run a list one call each, or {off}")
        if not image_io._is_pil(a.image):
            raise ValueError("tiled edits (enable_tiled_edit) need ONE PIL image: an array or tensor `image` has no full-resolution bytes to "
                             f"cut into tiles - pass a PIL image, or {off}")
        for bad, what in ((a.num_videos_per_prompt != 1, "num_videos_per_prompt > 1"), (a.enable_temporal_reasoning, "temporal reasoning"),
                          (self._preview is not None, "live previews (enable_preview)"),
                          (getattr(self.transformer, "_teacache", None) is not None, "TeaCache (enable_teacache)"),
                          (getattr(self.transformer, "_guidance_reuse", None) is not None, "guidance reuse (enable_guidance_reuse)"),
                          (a.offload_model, "offload_model"),
                          (self._guidance_measure is not None, "a measuring edit (measure_guidance_reuse)"),
                          (self._auto_region_measure is not None, "a measuring edit (measure_auto_region)"),
                          (bool(getattr(self.transformer, "_tea_measure", False)), "a measuring edit (calibrate_teacache)")):
            if bad:
                raise NotImplementedError(f"tiled edits (enable_tiled_edit) with {what} are not implemented: switch it off, or {off}")
        refuse_sharded(self.transformer, _tl.SHARDED)

    def _tiled_edit(self, a: CallArgs):
        """`__call__` while `enable_tiled_edit` is in force: the plan, the tiles as the samples of one batched pass fused behind every step
        (`denoise(tiles=)`), the weighted blend of the decoded tiles into the target's frame."""
        cfg = self._tiled
        self.tile_report = self.focus_report = self.lift_report = self.auto_region_report = None
        self._tiled_refusals(a)
        p = _tl.plan(a.image.size, a.height, a.width, cfg.size, cfg.overlap, cfg.max_tiles)
        if p.single:  # the canvas is one tile: the plain call on the image, no tiling code on the path
            out = self._edit(a)
            self.tile_report = dict(p.report, reason="single")
            return out
        a, device = self._begin(a, guarded=False)
        _, prompt_embeds, negative_prompt_embeds = self._encode_text(a, device)
        on_device = image_io.on_device(self.device_image_io, device)
        n = p.count
        target = _tl.target_image(a.image, p.target, device if on_device else None)
        crops = _tl.tile_images(target, p)
        image_embeds = a.image_embeds
        if image_embeds is None:  # clip="tile": the conditioning shows what the model edits; "photo": the whole target image, once
            image_embeds = self.encode_image(crops if cfg.clip == "tile" else target, device)
        image_embeds = image_embeds.to(device=device, dtype=self.transformer.dtype)
        if image_embeds.shape[0] not in (1, n):
            raise ValueError(f"`image_embeds` carry {image_embeds.shape[0]} samples, expected 1 or one per tile ({n})")
        if image_embeds.shape[0] != n:
            image_embeds = image_embeds.repeat(n, 1, 1)
        if hasattr(self.vae, "use_graph"):
            self.vae.use_graph = bool(self.use_graph)
        if on_device:
            img = image_io.preprocess_pil(crops, a.height, a.width, device)
        else:
            img = self.preprocess_image(crops, a.height, a.width).to(device=device, dtype=torch.bfloat16)
        z = self.vae.config.z_dim
        T = (a.num_frames - 1) // self.vae_scale_factor_temporal + 1
        state = _tl.TileState(p, z, T, device)
        shape = (1,) + tuple(state.canvas.shape)
        if a.latents is None:  # ONE canvas of noise
            if isinstance(a.generator, (list, tuple)) and len(a.generator) != 1:
                raise ValueError(f"You have passed a list of generators of length {len(a.generator)}, but requested an effective batch"
                                 f" size of 1. Make sure the batch size matches the length of the generators.")
            noise = _randn_tensor(shape, a.generator, device, torch.bfloat16)
        elif tuple(a.latents.shape) != shape:
            raise ValueError(f"tiled edits (enable_tiled_edit) take `latents` at the canvas shape {shape}, got {tuple(a.latents.shape)}")
        else:
            noise = a.latents
        latents = state.cut(noise.to(device=device, dtype=torch.float32))
        _, condition = prepare_latents(self.vae, img, a.num_frames, latents=latents)
        repeat = lambda t: None if t is None else t.repeat(n, 1, 1)
        embeds = {"prompt_embeds": repeat(prompt_embeds), "negative_prompt_embeds": repeat(negative_prompt_embeds)}

        self._num_timesteps = a.num_inference_steps
        lora_scale = getattr(self.transformer, "lora_scale", None)
        scaled = lora_scale((a.attention_kwargs or {}).get("scale")) if lora_scale is not None else contextlib.nullcontext()
        with scaled:
            latents = denoise(self.transformer, self.scheduler, latents, condition, embeds["prompt_embeds"],
                              embeds["negative_prompt_embeds"] if self.do_classifier_free_guidance else None, image_embeds,
                              a.num_inference_steps, a.guidance_scale, use_graph=self.use_graph, on_step_end=self._step_hook(a, embeds),
                              interrupted=lambda: self._interrupt, graph_warm=self._graph_warm, tiles=state)
        # once more behind the loop: the canvas and the tiles then agree whatever happened last - a callback that replaced the latents behind
        # the last step, an interrupt before the first (the canvas is then the noise); after an ordinary last step it changes no bit
        latents = state.fuse(latents)
        self._current_timestep = None
        self.tile_report = dict(p.report, reason="tiled")
        if a.output_type == "latent":
            video = state.canvas[None].clone()
        else:
            video = decode_latents(self.vae, latents)
            if self.video_guardrail_runner is not None:  # :784-799, on the tiles' frames
                video = self.video_guardrail_runner(video)
                if video is None:
                    raise Exception("Guardrail blocked video2world generation.")
            if on_device and image_io.device_video(video):
                blended = _blend_tiles(video, p).cpu().numpy()
            else:
                import numpy as np
                tiles_u8 = np.stack([np.stack([np.asarray(f) for f in sample]) for sample in self.postprocess_video(video, output_type="pil")])
                blended = _tl.reference_blend(torch.from_numpy(tiles_u8), p.xs, p.ys, p.target).numpy()
            video = image_io.frames_from_u8([blended], a.output_type)
        self.maybe_free_model_hooks()
        if not a.return_dict:
            return (video,)
        return WanPipelineOutput(frames=video)

    def _edit(self, a: CallArgs, fpass: Optional[FocusPass] = None):
        """The body of every call.  fpass: this is a focused pass somebody planned (a sketch edit, or the scout of an auto-focused call);
        None: what is edited follows from the user's switches (`_resolve`).  Nothing below `_resolve` reads them."""
        a, device = self._begin(a, guarded=fpass is not None and fpass.guarded)
        batch_size, prompt_embeds, negative_prompt_embeds = self._encode_text(a, device)
        what = self._resolve(a, fpass, batch_size, device)
        image_embeds = self._image_embeds(a, what.focus, batch_size, device)
        B = batch_size * a.num_videos_per_prompt
        img, focus_masks, lift_kept = self._preprocess(a, what, device)
        noise, condition = self.prepare_latents(img, B, self.vae.config.z_dim, a.height, a.width, a.num_frames, torch.bfloat16, device,
                                                a.generator, a.latents)
        latents, start_step, start_eps = noise, 0, None
        if fpass is not None and fpass.start is not None:
            # the warm start: the scout's estimate of the final image on the crop's latent grid, noised to the level of step k + 1
            st = fpass.start
            start_step, start_eps = st["step"], noise.to(torch.float32)
            tables = _af.restart_tables(what.focus[0].box, what.focus[0].image.size, tuple(noise.shape[-2:]), device)
            latents = _af.restart(st["x0"], start_eps, tables, st["sigma"], bf16_state=self.scheduler.trajectory_dtype == torch.bfloat16)
        n_img = img.shape[0]
        image_of = lambda b: b // a.num_videos_per_prompt if n_img > 1 else 0  # which image (and mask) sample b edits
        if what.masks is not None:
            focus_masks = _rg.device_masks(_fc.masks_for(what.masks, n_img), a.height, a.width, device)
        regions, autos = self._region_setup(img, a.num_frames, focus_masks, B, image_of)
        decision = {}
        if what.auto_focus is not None:  # this call is the scout: the detection decides whether a focused pass follows
            autos[0].on_accept = lambda m: decision.update(self._auto_focus_plan(what.pil[0], m, a.height, a.width, what.auto_focus, device)) or decision["go"]
        if a.offload_model and hasattr(self.vae, "clear_graphs"):
            self.vae.clear_graphs()  # a captured encode graph pins its activation pool next to the 14B DiT: the low-memory mode drops it
        if prompt_embeds.shape[0] != B or (negative_prompt_embeds is not None and negative_prompt_embeds.shape[0] != B):
            raise ValueError(f"prompt_embeds carry {prompt_embeds.shape[0]} samples, expected batch_size * num_videos_per_prompt = {B}")
        if image_embeds.shape[0] != B:
            image_embeds = image_embeds.repeat(B // image_embeds.shape[0], 1, 1)
        latents = self._denoise_samples(a, latents, condition, prompt_embeds, negative_prompt_embeds, image_embeds,
                                        None if regions is None else [regions[image_of(b)][1] for b in range(B)], autos, start_step, start_eps,
                                        fpass.preview_tag if fpass is not None else "scout" if what.auto_focus is not None else None, what.crop_of)
        if autos is not None and not autos[0].measure:
            self.auto_region_report = autos[0].report if B == 1 else [x.report for x in autos]
        if what.auto_focus is not None:
            if autos[0].exited:
                return self._focused_pass(a, decision["plan"], autos[0], what.auto_focus, noise, prompt_embeds, negative_prompt_embeds)
            # the scout ran to its end: the auto-region call, bit for bit
            declined = autos[0].report is None or not autos[0].report["accepted"]
            self.focus_report = [{"reason": "declined", "detect": autos[0].report} if declined else
                                 dict(decision["report"], box_reason=decision["report"]["reason"], reason="whole", detect=autos[0].report)]
        if a.offload_model and self.transformer is not None:
            self.transformer.cpu()
            torch.cuda.empty_cache()
        self._current_timestep = None
        video = latents if a.output_type == "latent" else self._output(a, what, latents, img, regions, autos, image_of, lift_kept, device)
        if a.offload_model and hasattr(self.vae, "clear_graphs"):
            self.vae.clear_graphs()
            torch.cuda.empty_cache()
        self.maybe_free_model_hooks()
        if not a.return_dict:
            return (video,)
        return WanPipelineOutput(frames=video)

    def _begin(self, a: CallArgs, guarded: bool):
        """The checks and resets every pass starts with -> (the arguments as the reference adjusts them, the device).  guarded: the text
        guardrail has seen this call's prompt already."""
        if hasattr(a.callback_on_step_end, "tensor_inputs"):
            a = replace(a, callback_on_step_end_tensor_inputs=a.callback_on_step_end.tensor_inputs)
        self.check_inputs(a.prompt, a.negative_prompt, a.image, a.height, a.width, a.prompt_embeds, a.negative_prompt_embeds, a.image_embeds,
                          a.callback_on_step_end_tensor_inputs)
        num_frames = a.num_frames
        if num_frames % self.vae_scale_factor_temporal != 1:  # :606-611
            num_frames = num_frames // self.vae_scale_factor_temporal * self.vae_scale_factor_temporal + 1
        a = replace(a, num_frames=max(num_frames, 1))
        self._guidance_scale, self._attention_kwargs, self._current_timestep, self._interrupt = a.guidance_scale, a.attention_kwargs, None, False
        device = self._execution_device
        if not guarded and self.text_guardrail_runner is not None and not self.text_guardrail_runner(a.prompt):  # :621-629
            raise Exception(f"Guardrail blocked text2world generation. Prompt: {a.prompt}")
        return a, device

    @staticmethod
    def _prompt_count(a: CallArgs) -> int:
        """How many prompts the call carries (:631-637), behind `check_inputs`."""
        if a.prompt is not None and isinstance(a.prompt, str):
            return 1
        if a.prompt is not None and isinstance(a.prompt, list):
            return len(a.prompt)
        return a.prompt_embeds.shape[0]

    def _encode_text(self, a: CallArgs, device):
        """-> (batch_size, prompt_embeds, negative_prompt_embeds) on the device in the transformer's dtype (:631-660)."""
        batch_size = self._prompt_count(a)
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt=a.prompt, negative_prompt=a.negative_prompt, do_classifier_free_guidance=self.do_classifier_free_guidance,
            num_videos_per_prompt=a.num_videos_per_prompt, prompt_embeds=a.prompt_embeds, negative_prompt_embeds=a.negative_prompt_embeds,
            max_sequence_length=a.max_sequence_length, device=device)
        if a.offload_model and self.text_encoder is not None:
            self.text_encoder.cpu()
        tdtype = self.transformer.dtype
        prompt_embeds = prompt_embeds.to(device=device, dtype=tdtype)
        if negative_prompt_embeds is not None:
            negative_prompt_embeds = negative_prompt_embeds.to(device=device, dtype=tdtype)
        return batch_size, prompt_embeds, negative_prompt_embeds

    def _resolve(self, a: CallArgs, fpass: Optional[FocusPass], batch_size: int, device) -> EditSources:
        """What this pass edits and how its frames go back - from the focus pass, else from the user's switches - and what must be refused."""
        pil = image_io._pil_list(a.image) if a.image is not None else None
        what = EditSources(pil=pil)
        self.focus_report = None
        if fpass is not None:  # (planned by the caller, the masks where they lie)
            what.focus, what.composite, what.crop_of = fpass.plans, fpass.composite, fpass.crop_of
        elif self._edit_region is not None:
            masks, what.composite = self._edit_region
            if self._region_focus is not None:
                what.focus = _fc.setup(a.image, masks, a.height, a.width, self._region_focus, a.output_type,
                                       device if image_io.on_device(self.device_image_io, device) else None)
            else:
                what.masks = masks
        if what.focus is not None:
            self.focus_report = [p.report for p in what.focus]
        # auto focus (chronoedit_amd/autofocus.py): this call is the scout, and starts the focused pass when the detection says so
        a_cfg, a_measure = self._auto_region_config()
        if fpass is None and self._auto_focus is not None and self._edit_region is None and a_cfg is not None and not a_measure:
            what.auto_focus = self._auto_focus
            if pil is None:
                raise ValueError("auto focus needs PIL input: an array or tensor `image` has no full-resolution bytes to paste the edit back "
                                 "into - pass a PIL image, or disable_auto_focus()")
            if batch_size * a.num_videos_per_prompt != 1 or len(pil) != 1:
                raise NotImplementedError("auto focus edits one photo per call: a list of images or prompts, or num_videos_per_prompt > 1, is not implemented")
            if a.enable_temporal_reasoning:
                raise NotImplementedError("auto focus with temporal reasoning is not implemented (the scout would run the reasoning steps "
                                          "twice, or the focused pass would start at the truncated shape)")
            if a.offload_model:
                raise NotImplementedError("auto focus with offload_model is not implemented (the encoders leave the device before the "
                                          "focused pass needs them)")
        # detail lift (chronoedit_amd/lift.py): the frames of an unfocused call go back at the images' own sizes
        self.lift_report = None
        if self._detail_lift is not None and a.output_type != "latent":
            if pil is None:
                raise ValueError("detail lift needs PIL input (one image or a list): an array or tensor `image` has no full-resolution bytes to "
                                 "lift the edit onto - pass PIL images, or disable_detail_lift()")
            what.lift, what.lift_focus, what.lift_mask_aware = self._detail_lift, self._detail_lift_focus, self._detail_lift_mask_aware
            if what.focus is None and a.output_type in ("np", "pt") and len({im.size for im in pil}) > 1:
                raise ValueError(f"detail lift returns frames of the images' sizes {[im.size for im in pil]}: output_type={a.output_type!r} "
                                 'needs images of one size, use "pil"')
        return what

    def _image_embeds(self, a: CallArgs, focus, batch_size: int, device) -> torch.Tensor:
        """The user's `image_embeds`, or CLIP on what the model edits: the image, or the crops of a focused pass."""
        image_embeds = a.image_embeds
        if image_embeds is None:
            if focus is None:
                image_embeds = self.encode_image(a.image, device)
            else:  # the conditioning shows what the model edits
                crops = [p.image.crop(p.box) for p in focus]
                image_embeds = self.encode_image(crops if isinstance(a.image, (list, tuple)) else crops[0], device)
        image_embeds = image_embeds.to(device=device, dtype=self.transformer.dtype)
        if image_embeds.shape[0] != batch_size:
            image_embeds = image_embeds.repeat(batch_size, 1, 1)
        if a.offload_model and self.image_encoder is not None:
            self.image_encoder.cpu()
        return image_embeds

    def _preprocess(self, a: CallArgs, what: EditSources, device):
        """-> (img bf16 [n, 3, height, width] on the device, the crops' edit-size masks of a focused pass or None, what the lift keeps on
        the device or None)."""
        if hasattr(self.vae, "use_graph"):  # the VAE replays captured graphs from the second edit of a shape on (vae.py)
            self.vae.use_graph = bool(self.use_graph)
        if what.focus is not None:
            return _fc.inputs(what.focus, a.height, a.width, device, keep_L=what.lift is not None and what.lift_focus) + (None,)
        if image_io.on_device(self.device_image_io, device) and what.pil is not None:
            lift_kept = [] if what.lift is not None else None  # (the photo's bytes stay on the device: one upload)
            return image_io.preprocess_pil(a.image, a.height, a.width, device, keep=lift_kept), None, lift_kept
        return self.preprocess_image(a.image, a.height, a.width).to(device=device, dtype=torch.bfloat16), None, None

    def _region_setup(self, img: torch.Tensor, num_frames: int, masks=None, n_samples: int = 1, image_of=lambda b: 0):
        """masks: per image of img its edit-size uint8 mask on the device, or None -> (per image (mask, region.RegionConfig), None), or
        without masks (None, per sample the auto_region.AutoRegion the loop fills in) when a detector is configured, else (None, None).
        Either costs one more VAE encode, of the condition encode's shape."""
        self.auto_region_report = None
        a_cfg, a_measure = self._auto_region_config()
        if masks is None and a_cfg is None:
            return None, None
        z_src = _rg.static_source_latents(self.vae, img, num_frames)
        if masks is None:
            return None, [_ar.AutoRegion(a_cfg, z_src[image_of(b):image_of(b) + 1], measure=a_measure) for b in range(n_samples)]
        weights = {}
        for m in masks:  # (one mask for all images: reduced once)
            if id(m) not in weights:
                weights[id(m)] = _rg.latent_weights(m)
        return [(m, _rg.RegionConfig(w=weights[id(m)], z_src=z_src[j:j + 1])) for j, m in enumerate(masks)], None

    def _step_hook(self, a: CallArgs, embeds: dict):
        """`denoise`'s on_step_end for one run of the loop: `callback_on_step_end` gets that run's tensors - the latents and `embeds`
        ({"prompt_embeds", "negative_prompt_embeds"}, updated in place when the callback replaces them) - and what it returns anew goes back
        to the loop (:741-749)."""
        def on_step_end(i, t, lat):
            self._current_timestep = t
            if a.callback_on_step_end is None:
                return None
            pool = {"latents": lat, **embeds}
            outs = a.callback_on_step_end(self, i, t, {k: pool[k] for k in a.callback_on_step_end_tensor_inputs})
            if not outs:
                return None
            new = {k: outs[k] for k in ("latents", "prompt_embeds", "negative_prompt_embeds") if k in outs and outs[k] is not pool[k]}
            embeds.update({k: v for k, v in new.items() if k != "latents"})
            return new or None
        return on_step_end

    def _denoise_samples(self, a: CallArgs, latents, condition, prompt_embeds, negative_prompt_embeds, image_embeds, regions, autos,
                         start_step: int, start_eps, preview_tag, crop_of=None) -> torch.Tensor:
        """The loop, sample by sample (regions, autos: per sample, or None; crop_of: per sample its (editor value, crop), or None) -> the
        final latents of all of them."""
        # The engine denoises ONE edit at a time (its batch axis carries the guidance pair); B = batch_size * num_videos_per_prompt
        # edits (pipeline_chronoedit.py:493,631-637,676-691) run one after the other on the same weights - the reference's batched
        # loop computes the same per-sample arithmetic.  `callback_on_step_end` is then called per sample and step with that
        # sample's tensors; returned `latents`, `prompt_embeds`, `negative_prompt_embeds` are honoured (:741-749).
        self._num_timesteps = a.num_inference_steps
        done = []
        # attention_kwargs={"scale": s} (diffusers' per-call LoRA scale): the active adapters times s for this call's denoising only
        lora_scale = getattr(self.transformer, "lora_scale", None)
        scaled = lora_scale((a.attention_kwargs or {}).get("scale")) if lora_scale is not None else contextlib.nullcontext()
        with scaled:
            for b in range(prompt_embeds.shape[0]):
                embeds = {"prompt_embeds": prompt_embeds[b:b + 1], "negative_prompt_embeds": None if negative_prompt_embeds is None else negative_prompt_embeds[b:b + 1]}
                done.append(denoise(self.transformer, self.scheduler, latents[b:b + 1], condition[b:b + 1], embeds["prompt_embeds"],
                                    embeds["negative_prompt_embeds"] if self.do_classifier_free_guidance else None, image_embeds[b:b + 1],
                                    a.num_inference_steps, a.guidance_scale, a.enable_temporal_reasoning, a.num_temporal_reasoning_steps,
                                    use_graph=self.use_graph, on_step_end=self._step_hook(a, embeds), interrupted=lambda: self._interrupt,
                                    graph_warm=self._graph_warm, region=None if regions is None else regions[b],
                                    auto_region=None if autos is None else autos[b], start_step=start_step,
                                    start_eps=None if start_eps is None else start_eps[b:b + 1],
                                    preview=self._preview_config(b, preview_tag, None if crop_of is None else crop_of[b]), **self._measure_kwargs()))
        return done[0] if len(done) == 1 else torch.cat(done, dim=0)

    def _composited(self, video: torch.Tensor, img: torch.Tensor, masks, image_of=lambda b: 0) -> List[torch.Tensor]:
        """The edit-size paste-back behind the decode: per sample its frames (reasoning frames included) with the source kept where that
        sample's mask says so - a new fp32 video; a sample without a mask (a declined detection) keeps its decoded frames."""
        return [video[b:b + 1].float() if m is None else _rg.composite(video[b:b + 1], img[image_of(b):image_of(b) + 1], m)
                for b, m in enumerate(masks)]

    def _output(self, a: CallArgs, what: EditSources, latents, img, regions, autos, image_of, lift_kept, device):
        """Decode, the video guardrail, the edit-size composite, then the focus paste, the lift or the plain frames."""
        video = decode_latents(self.vae, latents, a.enable_temporal_reasoning, a.num_temporal_reasoning_steps)
        if self.video_guardrail_runner is not None:  # :784-799
            video = self.video_guardrail_runner(video)
            if video is None:
                raise Exception("Guardrail blocked video2world generation.")
        B = video.shape[0]
        masks = None
        if what.focus is None and regions is not None and what.composite:
            masks = [regions[image_of(b)][0] for b in range(B)]
        elif autos is not None and autos[0].config.composite and any(x.mask_u8 is not None for x in autos):
            masks = [x.mask_u8 for x in autos]  # the detected ones
        if masks is not None:
            video = torch.cat(self._composited(video.to(device), img, masks, image_of), dim=0)
        if what.lift is not None and what.focus is None:
            lifted, self.lift_report = _lf.output(video, what.lift, lift_kept, what.pil, image_of, a.height, a.width, a.output_type)
            if what.lift_mask_aware:  # (a whole-photo lift has no crop to fit under a mask)
                for entry in self.lift_report:
                    entry["mask_aware"] = False
            if lifted is not None:
                return lifted
        if what.focus is not None:  # the source-size paste replaces the edit-size composite
            boxed, lifted = (what.lift if what.lift_focus else None), []  # focus=True: every crop is lifted inside its box (boxlift.py)
            masked = boxed is not None and what.lift_mask_aware
            if what.crop_of is not None:  # the crops of an editor value, chained into one video
                video = _cl.paste(video, what.focus, what.crop_of, a.output_type, what.composite, lift=boxed, report=lifted, mask_aware=masked)
            else:
                video = _fc.paste(video, what.focus, image_of, a.output_type, what.composite, lift=boxed, report=lifted, mask_aware=masked)
            if boxed is not None:
                self.lift_report = lifted
            elif what.lift is not None:
                self.lift_report = [_lf.report_entry(what.focus[image_of(b)].image.size, (a.width, a.height), "focus") for b in range(B)]
            return video
        if self.device_image_io and a.output_type == "pil" and image_io.device_video(video):
            return image_io.frames_to_pil(video)
        return self.postprocess_video(video, output_type=a.output_type)

    def _auto_focus_plan(self, image, mask_edit: torch.Tensor, height: int, width: int, cfg, device) -> dict:
        """The scout's decision: the detected edit-size mask (on the device) -> {"go", "report", "plan"}: the lifted mask, the box (two
        reductions, five integers read each) and, when the box is worth cropping to, the focus.FocusPlan."""
        on_device = image_io.on_device(self.device_image_io, device)
        mask_src = _af.lift_mask(mask_edit if on_device else mask_edit.cpu(), image.size)
        report = _af.plan(mask_src, (width, height), cfg.context)
        go = _af.worth_focusing(report)
        return {"go": go, "report": report, "plan": _fc.FocusPlan.make(image, report, mask_src, device if on_device else None) if go else None}

    def _focused_pass(self, a: CallArgs, plan, auto, cfg, noise, prompt_embeds, negative_prompt_embeds):
        """The focused pass of an auto-focused call: the explicit-mask focused region edit of the crop around the detected region, from the
        scout's noise and its encoded prompts (CLIP sees the crop unless the user gave `image_embeds`), then the report's new entries."""
        from PIL import Image
        k = auto.report["step"]
        start = None
        if cfg.warm_start and k + 1 < a.num_inference_steps:  # (a detection behind the last step leaves no tail: cold)
            start = {"step": k + 1, "x0": self.scheduler.model_outputs[-1], "sigma": float(self.scheduler.sigmas[k + 1])}
        a = replace(a, prompt=None, negative_prompt=None, num_videos_per_prompt=1, latents=noise, prompt_embeds=prompt_embeds,
                    negative_prompt_embeds=negative_prompt_embeds, num_temporal_reasoning_steps=0)
        out = self._edit(a, FocusPass([plan], bool(auto.config.composite), start=start, preview_tag="focus", guarded=True))
        self.auto_region_report = auto.report
        self.focus_report = [dict(plan.report, mask=Image.fromarray(plan.host_mask().numpy(), mode="L"), detect=auto.report,
                                  start_step=0 if start is None else start["step"])]
        return out

    @torch.no_grad()
    def edit_tensors(self, image: torch.Tensor, prompt_embeds: torch.Tensor, negative_prompt_embeds: Optional[torch.Tensor],
                     image_embeds: Optional[torch.Tensor], num_frames: int = 5, num_inference_steps: int = 50, guidance_scale: float = 5.0,
                     enable_temporal_reasoning: bool = False, num_temporal_reasoning_steps: int = 0, generator=None,
                     latents: Optional[torch.Tensor] = None, output_type: str = "pt", region_mask: Optional[torch.Tensor] = None,
                     composite: bool = True):
        """Tensor-level form of the same edit (no pre / post processing): image [1,3,H,W] in [-1,1] -> video [1,3,F,H,W] in
        [-1,1] ("pt") or the final latents ("latent").  What the parity tests and tools/full_edit.py drive.
        region_mask: a uint8 / bool / float tensor [H, W] for a region-limited edit (region.normalize_mask); `set_edit_region` is not
        looked at here.  composite: paste the source back behind the decode - the video is then a new fp32 tensor."""
        H, W = image.shape[-2:]
        if H % 16 != 0 or W % 16 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 16 but are {H} and {W}.")  # pipeline_chronoedit.py:361-362
        if num_frames % 4 != 1:
            num_frames = max(num_frames // 4 * 4 + 1, 1)  # :606-611
        latents, condition = prepare_latents(self.vae, image, num_frames, latents, generator)
        masks = None if region_mask is None else _rg.device_masks([region_mask], H, W, image.device)
        regions, autos = self._region_setup(image, num_frames, masks)
        region, auto = None if regions is None else regions[0][1], None if autos is None else autos[0]
        latents = denoise(self.transformer, self.scheduler, latents, condition, prompt_embeds, negative_prompt_embeds, image_embeds,
                          num_inference_steps, guidance_scale, enable_temporal_reasoning, num_temporal_reasoning_steps,
                          use_graph=self.use_graph, graph_warm=self._graph_warm, region=region, auto_region=auto,
                          preview=self._preview_config(), **self._measure_kwargs())
        if auto is not None and not auto.measure:
            self.auto_region_report = auto.report
        if output_type == "latent":
            return latents
        video = decode_latents(self.vae, latents, enable_temporal_reasoning, num_temporal_reasoning_steps)
        mask = masks[0] if masks is not None else auto.mask_u8 if auto is not None and auto.config.composite else None
        if mask is not None and composite:
            video = self._composited(video, image.to(torch.bfloat16), [mask])[0]
        return video


# The arguments of `__call__` - the reference's (pipeline_chronoedit.py:484-512) -, captured once per call; a pass that differs from the user's
# call (`dataclasses.replace`) says in what
CallArgs = make_dataclass("CallArgs", list(inspect.signature(ChronoEditPipeline.__call__).parameters)[1:])
