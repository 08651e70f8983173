"""Drop-in `ChronoEditTransformer3DModel` whose forward runs on the gfx950 HIP kernels.

Mirrors /root/reference/chronoedit_diffusers/transformer_chronoedit.py:298-476:
  * same constructor keyword arguments and `.config` fields (:341-360);
  * same parameter tree with the diffusers state-dict names (key list:
    chronoedit_diffsynth/wan_video_dit_chronoedit.py:439-496), built from real nn.Linear / nn.Conv3d
    / nn.LayerNorm modules so `load_state_dict`, `.to`, PEFT LoRA injection/fusion keep working;
  * same `forward(hidden_states, timestep, encoder_hidden_states, encoder_hidden_states_image,
    return_dict, attention_kwargs)` signature, return types and error behaviour (:397-476);
  * same dtype islands: `_keep_in_fp32_modules` parameters stay fp32 (:338).
The modules only HOLD parameters; the arithmetic is `DiTEngine` below, which sequences
libchronoedit_hip.so launches on the current stream (no torch math on the hot path).
"""
from __future__ import annotations

import inspect
import math
import re
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Dict, Optional, Tuple, Union

import torch
import torch.nn as nn

from . import ops, weights
from .weights import LoraMixin


@dataclass
class Transformer2DModelOutput:
    sample: torch.Tensor


class _Config(SimpleNamespace):
    def __getitem__(self, k):
        return getattr(self, k)

    def get(self, k, d=None):
        return getattr(self, k, d)


class RMSNormParams(nn.Module):
    """Parameter holder for diffusers RMSNorm (norm_q / norm_k / norm_added_k)."""

    def __init__(self, dim: int, eps: float, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim, device=device, dtype=dtype))


class AttentionParams(nn.Module):
    """Parameter holder with diffusers `Attention` attribute names (transformer_chronoedit.py:231-258)."""

    def __init__(self, dim: int, heads: int, eps: float, added_kv_proj_dim: Optional[int], device=None, dtype=None):
        super().__init__()
        kw = dict(device=device, dtype=dtype)
        self.heads = heads
        self.to_q = nn.Linear(dim, dim, **kw)
        self.to_k = nn.Linear(dim, dim, **kw)
        self.to_v = nn.Linear(dim, dim, **kw)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim, **kw), nn.Dropout(0.0)])
        self.norm_q = RMSNormParams(dim, eps, **kw)
        self.norm_k = RMSNormParams(dim, eps, **kw)
        self.add_k_proj = self.add_v_proj = self.norm_added_k = None
        if added_kv_proj_dim is not None:
            self.add_k_proj = nn.Linear(added_kv_proj_dim, dim, **kw)
            self.add_v_proj = nn.Linear(added_kv_proj_dim, dim, **kw)
            self.norm_added_k = RMSNormParams(dim, eps, **kw)


class _GELUProj(nn.Module):
    def __init__(self, din, dout, device=None, dtype=None):
        super().__init__()
        self.proj = nn.Linear(din, dout, device=device, dtype=dtype)


class FeedForwardParams(nn.Module):
    """diffusers FeedForward layout: net.0.proj, net.1 (Dropout), net.2."""

    def __init__(self, dim, inner, dim_out=None, device=None, dtype=None):
        super().__init__()
        self.net = nn.ModuleList([
            _GELUProj(dim, inner, device=device, dtype=dtype),
            nn.Dropout(0.0),
            nn.Linear(inner, dim_out if dim_out is not None else dim, device=device, dtype=dtype),
        ])


class BlockParams(nn.Module):
    """ChronoEditTransformerBlock parameters (transformer_chronoedit.py:216-265)."""

    def __init__(self, dim, ffn_dim, heads, cross_attn_norm, eps, added_kv_proj_dim, device=None, dtype=None):
        super().__init__()
        self.attn1 = AttentionParams(dim, heads, eps, None, device=device, dtype=dtype)
        self.attn2 = AttentionParams(dim, heads, eps, added_kv_proj_dim, device=device, dtype=dtype)
        # norm1 / norm3 have no affine parameters; norm2 is FP32LayerNorm(affine) kept in fp32 (:338)
        self.norm2 = nn.LayerNorm(dim, eps, elementwise_affine=True, device=device, dtype=torch.float32) if cross_attn_norm else nn.Identity()
        self.ffn = FeedForwardParams(dim, ffn_dim, device=device, dtype=dtype)
        self.scale_shift_table = nn.Parameter(torch.randn(1, 6, dim, device=device, dtype=torch.float32) / dim**0.5)


class _TimestepEmbedding(nn.Module):
    def __init__(self, din, dim, device=None):
        super().__init__()
        self.linear_1 = nn.Linear(din, dim, device=device, dtype=torch.float32)
        self.linear_2 = nn.Linear(dim, dim, device=device, dtype=torch.float32)


class _TextProjection(nn.Module):
    def __init__(self, din, dim, device=None, dtype=None):
        super().__init__()
        self.linear_1 = nn.Linear(din, dim, device=device, dtype=dtype)
        self.linear_2 = nn.Linear(dim, dim, device=device, dtype=dtype)


class _ImageEmbedding(nn.Module):
    def __init__(self, din, dout, device=None, dtype=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(din, device=device, dtype=torch.float32)
        self.ff = FeedForwardParams(din, din, dout, device=device, dtype=dtype)
        self.norm2 = nn.LayerNorm(dout, device=device, dtype=torch.float32)


class ConditionEmbedderParams(nn.Module):
    """ChronoEditTimeTextImageEmbedding parameters (transformer_chronoedit.py:126-145)."""

    def __init__(self, dim, time_freq_dim, time_proj_dim, text_embed_dim, image_embed_dim, device=None, dtype=None):
        super().__init__()
        self.time_embedder = _TimestepEmbedding(time_freq_dim, dim, device=device)
        self.time_proj = nn.Linear(dim, time_proj_dim, device=device, dtype=dtype)
        self.text_embedder = _TextProjection(text_embed_dim, dim, device=device, dtype=dtype)
        self.image_embedder = None
        if image_embed_dim is not None:
            self.image_embedder = _ImageEmbedding(image_embed_dim, dim, device=device, dtype=dtype)


import itertools

_GENERATION = itertools.count(1)


class ChronoEditTransformer3DModel(LoraMixin, nn.Module):
    """MI355X drop-in for the reference class of the same name (transformer_chronoedit.py:298)."""

    _supports_gradient_checkpointing = False
    _no_split_modules = ["BlockParams"]
    _keep_in_fp32_modules = ["time_embedder", "scale_shift_table", "norm1", "norm2", "norm3"]
    _keys_to_ignore_on_load_unexpected = ["norm_added_q"]

    def __init__(
        self,
        patch_size: Tuple[int, int, int] = (1, 2, 2),
        num_attention_heads: int = 40,
        attention_head_dim: int = 128,
        in_channels: int = 16,
        out_channels: int = 16,
        text_dim: int = 4096,
        freq_dim: int = 256,
        ffn_dim: int = 13824,
        num_layers: int = 40,
        cross_attn_norm: bool = True,
        qk_norm: Optional[str] = "rms_norm_across_heads",
        eps: float = 1e-6,
        image_dim: Optional[int] = None,
        added_kv_proj_dim: Optional[int] = None,
        rope_max_seq_len: int = 1024,
        rope_temporal_skip_len: int = 8,
        device=None,
        dtype: torch.dtype = torch.bfloat16,
    ) -> None:
        super().__init__()
        if qk_norm != "rms_norm_across_heads":
            raise NotImplementedError("only qk_norm='rms_norm_across_heads' (the ChronoEdit/Wan setting) is supported")
        if tuple(patch_size) != (1, 2, 2):
            raise NotImplementedError("patch_size must be (1, 2, 2)")
        if attention_head_dim != 128:
            raise NotImplementedError("the gfx950 attention kernel is specialised for head_dim 128")
        self.config = _Config(
            patch_size=tuple(patch_size), num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim,
            in_channels=in_channels, out_channels=out_channels or in_channels, text_dim=text_dim, freq_dim=freq_dim,
            ffn_dim=ffn_dim, num_layers=num_layers, cross_attn_norm=cross_attn_norm, qk_norm=qk_norm, eps=eps,
            image_dim=image_dim, added_kv_proj_dim=added_kv_proj_dim, rope_max_seq_len=rope_max_seq_len,
            rope_temporal_skip_len=rope_temporal_skip_len,
        )
        inner = num_attention_heads * attention_head_dim
        kw = dict(device=device, dtype=dtype)
        self.patch_embedding = nn.Conv3d(in_channels, inner, kernel_size=patch_size, stride=patch_size, **kw)
        self.condition_embedder = ConditionEmbedderParams(inner, freq_dim, inner * 6, text_dim, image_dim, **kw)
        self.blocks = nn.ModuleList(
            [BlockParams(inner, ffn_dim, num_attention_heads, cross_attn_norm, eps, added_kv_proj_dim, **kw) for _ in range(num_layers)]
        )
        self.proj_out = nn.Linear(inner, self.config.out_channels * math.prod(patch_size), **kw)
        self.scale_shift_table = nn.Parameter(torch.randn(1, 2, inner, device=device, dtype=torch.float32) / inner**0.5)
        self._engine: Optional["DiTEngine"] = None
        self._gen = next(_GENERATION)  # engine_generation(): see there
        self.cache_context = False  # reuse K3/K13 results while the conditioning tensors are unchanged
        self.gemm_dtype = "bf16"    # "fp8": the six large Linears of every block on the OCP-e4m3 MX matrix path
        self.fp8_linears = self.FP8_LINEARS  # which of them, once the fp8 mode is on (enable_fp8_gemms(linears= / policy=))
        self.attn_dtype = "bf16"    # "mxfp8": self-attention on the MX-fp8 matrix instruction (csrc/ce_attn_fp8.hip)
        self.v_transposed = True    # bf16 self-attention takes V^T straight from the projection (swapped GEMM) and stages it by LDS-DMA
        self.sp_batch_cfg = True    # sequence-parallel forwards take the guidance pair as one batch of two (blocked-layout kernels)
        self.fp8_fuse_quant = True  # MX fp8 mode: the FFN-up epilogue emits the FFN-down operand quantised (no bf16 hidden matrix, no quant pass)
        self.fp8_fuse_attn_quant = True  # ... and both attention kernels emit the out-projections' operands (A/B switch; needs fp8_fuse_quant)
        self.cross_vt = True        # cross-attention takes V^T of the text / image context straight from the context projections (LDS-DMA kernel)
        self._sp = None             # Ulysses sequence parallelism (chronoedit_amd.parallel), off by default
        self._cfgp = None           # CFG parallelism on top of it (two Ulysses groups), off by default
        self._teacache = None       # TeaCache step skipping (chronoedit_amd.teacache): a TeaCacheConfig once enable_teacache() was called
        self._tea_mode = None       # per forward, set by the denoising loop: None = off (the full forward), "compute", "skip" or "measure"
        self.teacache_report = None  # {"plan", "computed", "skipped", "ratios"} of the last edit that ran with TeaCache
        self._tea_measure = False   # calibrate_teacache(): the loop measures every edit instead of skipping steps
        self.teacache_measurement = None  # {"ratios", "distances"} of the last measured edit (pipeline.denoise(teacache_measure=True))
        self.shared_guidance = True  # run what the two samples of a guidance pair share once (enable_shared_guidance; needs _shared_inputs)
        self.text_compaction = True  # attend a text context's padding once, weighted (enable_text_compaction; needs the tensor's `_ce_compact`)
        self._shared_inputs = None  # per forward, set by the denoising loop: True = the two samples have the same latents, timestep and image context
        self._guidance_reuse = None  # guidance reuse (chronoedit_amd.guidance): a GuidanceReuseConfig once enable_guidance_reuse() was called
        self.guidance_report = None  # {"plan", "pair", "reuse", "off"} of the last guided edit that ran with guidance reuse; None otherwise
        self.guidance_measurement = None  # {"timesteps", "rel_l2"[, "deltas"]} of the last edit measured with denoise(guidance_measure=)
        self._sparse_region = None  # sparse region edits (chronoedit_amd/sparse_region.py): a SparseRegionConfig once enable_sparse_region() was called
        self._sparse_mode = None    # per forward, set by the denoising loop: None = off (the plain forward), "refresh" or "sparse"
        self.sparse_report = None   # {"plan", "compute", "refresh", "sparse", "active", "tokens"} of the last edit that ran with a sparse region plan
        self._auto_region = None    # automatic edit regions (chronoedit_amd/auto_region.py): an AutoRegionConfig once enable_auto_region() was called
        self.auto_region_report = None  # {"step", "threshold", "dmax", "active_fraction", "accepted", "reason", "w", "mask"} of the last edit that looked for its region
        self.auto_region_measurement = None  # {"timesteps", "steps"} of the last edit measured with denoise(auto_region=AutoRegion(measure=True))

    # -- reference-compatible helpers --------------------------------------------------
    @property
    def dtype(self) -> torch.dtype:
        return self.proj_out.weight.dtype

    @property
    def device(self) -> torch.device:
        return self.proj_out.weight.device

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None, torch_dtype: torch.dtype = torch.bfloat16,
                        device=None, **unused) -> "ChronoEditTransformer3DModel":
        """diffusers-layout checkpoint directory -> model (run_inference_diffusers.py:349-353): ``config.json`` gives the
        constructor arguments, the safetensors shard(s) the parameters; fp32 islands stay fp32 (``_keep_in_fp32_modules``)
        and ``norm_added_q`` keys are ignored (transformer_chronoedit.py:338-339)."""
        cfg = weights.read_config(path, subfolder)
        known = set(inspect.signature(cls.__init__).parameters) - {"self", "device", "dtype"}
        model = cls(**{k: v for k, v in cfg.items() if k in known}, device=device, dtype=torch_dtype)
        sd = weights.load_state_dict_files(weights.shard_files(path, subfolder))
        weights.assign_state_dict(model, sd, ignore_unexpected=cls._keys_to_ignore_on_load_unexpected)
        model.invalidate()
        return model

    def load_wan_native_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Load a checkpoint in the original Wan naming used by the reference's two sibling stacks (diffsynth ``WanModel``,
        ``_src`` ``wan2pt1``; correspondence: wan_video_dit_chronoedit.py:434-505)."""
        renamed = weights.wan_native_to_diffusers(sd, [k for k, _ in self.named_parameters()])
        weights.assign_state_dict(self, renamed, ignore_unexpected=self._keys_to_ignore_on_load_unexpected)
        self.invalidate()
        return self

    def wan_native_state_dict(self) -> Dict[str, torch.Tensor]:
        """The parameters under their Wan-native names (e.g. to hand LoRA-fused weights to the sibling stacks)."""
        return {weights.diffusers_to_wan_native_key(k): p.detach() for k, p in self.named_parameters()}

    def save_pretrained(self, path: str, max_shard_bytes: int = 5 << 30):
        """config.json + safetensors shard(s) in the layout from_pretrained reads."""
        return weights.save_pretrained(self, path, dict(vars(self.config)), max_shard_bytes, "ChronoEditTransformer3DModel")

    def load_synthetic_(self, params: Dict[str, torch.Tensor]):
        """Copy a {diffusers key: tensor} dict (e.g. oracle.make_synthetic_params) into the tree."""
        own = dict(self.named_parameters())
        missing = set(own) - set(params)
        extra = set(params) - set(own)
        if missing or extra:
            raise KeyError(f"state mismatch: missing {sorted(missing)[:4]} unexpected {sorted(extra)[:4]}")
        with torch.no_grad():
            for k, p in own.items():
                p.copy_(params[k].to(p.dtype))
        self.invalidate()
        return self

    def enable_sequence_parallel(self, group=None, force: bool = False, owned_comm: bool = False):
        """Shard the token axis over the ranks of `group` (Ulysses: three all-to-all per self-attention).  Every rank
        must call forward with the same (replicated) inputs and receives the full output.  force, owned_comm: see parallel.Ulysses
        (owned_comm = the exchanges on a RCCL communicator owned by libchronoedit_hip: the sharded step becomes hipGraph-capturable)."""
        from .parallel import Ulysses
        self._sp = Ulysses(group, force=force, owned_comm=owned_comm)
        if self.config.num_attention_heads % self._sp.world:
            raise ValueError(f"{self.config.num_attention_heads} heads do not divide over {self._sp.world} ranks")
        if self._engine is not None:
            self._engine._ws = {}  # workspaces carry the exchange buffers of the group
            self._engine.ws_generation += 1
        return self

    def enable_cfg_parallel(self):
        """World of W = 2 S ranks: the conditional / unconditional passes of a guidance step run side by side on two S-way
        Ulysses groups (parallel.CFGParallel); `pipeline.denoise_step` exchanges the two predictions.  Collective: every
        rank of the world must call it."""
        from .parallel import CFGParallel, Ulysses
        self._cfgp = CFGParallel()
        self._sp = Ulysses(self._cfgp.sp_group)
        if self.config.num_attention_heads % self._sp.world:
            raise ValueError(f"{self.config.num_attention_heads} heads do not divide over {self._sp.world} ranks")
        if self._engine is not None:
            self._engine._ws = {}
            self._engine.ws_generation += 1
        return self

    def clear_context_cache(self):
        if self._engine is not None:
            self._engine.clear_context_cache()

    @torch.no_grad()
    def prime_context(self, encoder_hidden_states: torch.Tensor, encoder_hidden_states_image: Optional[torch.Tensor]):
        """Compute the step-invariant conditioning work for exactly these tensors now, so that the next forward
        that receives them - e.g. the one a hipGraph capture records - finds the cache entry (with `cache_context`).  Without it, a compacted
        text context is still projected once here: its engine-owned V^T buffers depend on the prompt's length and must exist before a capture."""
        eng = self.engine()
        if self.cache_context or eng._text_compact(encoder_hidden_states, encoder_hidden_states_image) is not None:
            eng._context(encoder_hidden_states, encoder_hidden_states_image,
                         share_image=eng._share_image(encoder_hidden_states, encoder_hidden_states_image))

    def invalidate(self):
        """Call after changing parameters in place (LoRA fuse, load_state_dict): re-packs on next forward."""
        self._engine = None

    FP8_LINEARS = ("qkv", "o1", "q2", "o2", "f1", "f2")  # fused q|k|v, self-attention out, cross-attention q, cross-attention out, FFN up, FFN down
    # Mixed-precision policies of the fp8 mode (round 6): which of the six large Linears of a block run on the MX fp8 GEMM - the others stay
    # on the bf16 GEMM.  From the measurement in profiles/r06_fp8_sensitivity.txt (one full-width block at N = 7 200 against the fp32 oracle,
    # one Linear in fp8 at a time): the UNGATED cross-attention out-projection `o2` alone carries 3.3e-2 of the 3.7e-2 the fp8 mode adds to
    # the bf16 path's 4.8e-3 (its result enters the residual stream at full scale; `o1` and `f2` are multiplied by their AdaLN gates first,
    # `qkv` feeds a softmax); the MXFP8 self-attention adds 1.0e-3.  "fast" = all six (7.8 x the bf16 error per block); "accurate" = all but
    # `o2` (4.0 x) for one 5120 x 5120 GEMM per block back on the bf16 kernel.
    FP8_POLICIES = {"fast": ("qkv", "o1", "q2", "o2", "f1", "f2"), "accurate": ("qkv", "o1", "q2", "f1", "f2")}

    def enable_fp8_gemms(self, on: bool = True, mx: bool = True, linears=None, policy: Optional[str] = None):
        """BASELINE.json configs[4]: run the six large Linears of every block (fused q|k|v, the two output projections, the
        cross-attention query, FFN up / down) in fp8 e4m3 with fp32 accumulation on the MX matrix instruction.
        mx=True (default since round 4): OCP MXFP8 operands - one E8M0 scale per 32 consecutive input channels of every activation row and
        of every weight row, applied inside the matrix pipe (`ce_gemm_mxfp8`; quantisers `ce_quant_rows_mxfp8` / `ce_ln_affine_mxfp8`);
        mx=False: one fp32 scale per token row / per output channel (`ce_gemm_fp8`, the round-1..3 contract).  Weights are quantised once;
        attention, norms, the residual stream, the conditioning projections and the head stay bf16 / fp32.  The bf16 parameters are kept.
        linears / policy (round 6): a subset of FP8_LINEARS, or the name of one of FP8_POLICIES ("fast" = all six, the default; "accurate" = all but the
        ungated cross-attention out-projection, 4.0 x instead of 7.8 x the bf16 path's error per block) - Linears not named run the bf16 GEMM on bf16 activations."""
        if policy is not None:
            if linears is not None:
                raise ValueError("enable_fp8_gemms: give `linears` or `policy`, not both")
            if policy not in self.FP8_POLICIES:
                raise ValueError(f"enable_fp8_gemms: unknown policy {policy!r} (one of {sorted(self.FP8_POLICIES)})")
            linears = self.FP8_POLICIES[policy]
        linears = tuple(self.FP8_LINEARS if linears is None else linears)
        bad = [n for n in linears if n not in self.FP8_LINEARS]
        if bad:
            raise ValueError(f"enable_fp8_gemms: unknown Linear name(s) {bad} (of {self.FP8_LINEARS})")
        self.fp8_linears = tuple(n for n in self.FP8_LINEARS if n in linears)
        self.gemm_dtype = ("mxfp8" if mx else "fp8") if (on and self.fp8_linears) else "bf16"
        self._engine = None
        return self

    def enable_transposed_v(self, on: bool = True):
        """bf16 self-attention operand form (default on): the V third of the fused projection is taken as V^T = (h.W_v^T)^T (a GEMM
        whose epilogue stores the transpose, CE_EPI_BIAS_T) so that K and V^T tiles both reach the attention
        kernel's LDS by LDS-DMA (`ce_attention_vt_bf16`: +4.4 % on the kernel, no transpose pass).  Off = the fused q|k|v GEMM and
        the register-staged kernel; same arithmetic up to the summation order inside a key tile."""
        self.v_transposed = bool(on)
        if self._engine is not None:
            self._engine.v_transposed = self.v_transposed
            self._engine._ws = {}
            self._engine.ws_generation += 1
        return self

    def enable_cross_vt(self, on: bool = True):
        """Cross-attention operand form (default on): the V halves of the context projections are produced as V^T (the swapped-role GEMM,
        all layers in one launch per context stream) and both segments' K / V^T tiles reach the kernel's LDS by LDS-DMA
        (`ce_attention_2seg_vt_bf16`).  Off = row-major V and the register-staged two-segment kernel; same arithmetic up to the
        summation order inside a key tile."""
        self.cross_vt = bool(on)
        self._engine = None
        return self

    def enable_shared_guidance(self, on: bool = True):
        """The guidance pair's common work run once (default on).  `pipeline.denoise_step` / `GraphedDenoiser` feed both samples of the
        batched pair the same latents, timestep and image embedding and say so per call (`_shared_inputs`); the engine then runs the patch
        embedding, the modulation tables and block 0 up to its cross-attention on ONE sample's rows, projects the image context once, and
        fans out at block 0's cross-attention (shared-operand strides of the two-segment attention, residual row period of the GEMM).  Off =
        the stacked sequence for everything (A/B partner).  Only the unsharded bf16 path with the transposed-V cross-attention shares;
        every other mode runs the stacked sequence whatever this says.  A direct forward() never shares: nothing is inferred from tensors."""
        self.shared_guidance = bool(on)
        if self._engine is not None:
            self._engine.clear_context_cache()  # (a cached context was projected for the other form)
        return self

    def enable_text_compaction(self, on: bool = True):
        """The padding of a text context attended once, weighted (default on).  The reference re-pads every prompt to 512 rows and attends
        them unmasked; the embedder and the per-layer K / V projections act row by row, so the padding rows are (Tt - n) copies of ONE key /
        value pair, and a softmax over them equals one over a single key whose logit carries + ln(Tt - n).  Where the edit's context is built
        (`pipeline.make_cfg_inputs`, `pipeline.compact_text_context`) the padding is found once and the text tensor carries its compacted
        form; the engine then projects Lc = n_max + 1 (rounded up to 8) rows per sample and the cross-attention walks ceil((n + 1) / 64) text
        tiles per sample (`ce_attention_2seg_vt_weighted_bf16`).  Off = the full rows (A/B partner).  Only the unsharded bf16 path with the
        transposed-V cross-attention compacts; a tensor that was not examined - any direct forward() - never does."""
        self.text_compaction = bool(on)
        if self._engine is not None:
            self._engine.clear_context_cache()
        return self

    def enable_fp8_attention(self, on: bool = True, cross: bool = False):
        """BASELINE.json configs[4] "fp8 weights+attn": the attention of every block under the MXFP8 contract of
        csrc/ce_attn_fp8.hip - q / k (after RMSNorm + RoPE) in e4m3 with one E8M0 scale per 32 head channels, v per 32 keys,
        Q.K^T and P.V on v_mfma_scale_f32_32x32x64_f8f6f4, P in e4m3, fp32 accumulation.  cross (round 5): the cross-attention too - the
        text and the image segment each as one MXFP8 attention over the context's quantised K / V^T (made once per context: cached per
        edit), the image segment adding the text segment's bf16 result (`ce_attention_mxfp8_add`).  OFF by default - measured on MI355X at
        the full width (tools/fp8_cross_probe.py, profiles/r05_fp8_cross_attention_probe.txt): with 512 + 257 keys the two MXFP8 launches
        are prologue / epilogue bound (0.199 + 0.209 ms + 0.06 ms more producer work against 0.315 ms for the bf16 two-segment kernel with
        the fused MX output) and the block's error against fp32 rises from 7.85 x to 8.75 x the bf16 path's: slower AND less accurate, so
        the default keeps the 3 % of the attention flops that are cross-attention in bf16.  Everything else is unchanged; independent of
        enable_fp8_gemms."""
        self.attn_dtype = "mxfp8" if on else "bf16"
        self.fp8_cross = bool(on and cross)
        self._engine = None  # (the context operands and the workspaces depend on it)
        return self

    def enable_teacache(self, rel_l1_thresh: float, coefficients=(1.0, 0.0)):
        """TeaCache step skipping in `pipeline.denoise` (chronoedit_amd/teacache.py): a step is skipped - the cached residual of the block
        stack added to its patch-embedded tokens instead of running the blocks - while the accumulated relative L1 distance of the time
        modulation, rescaled by the polynomial `coefficients` (highest power first), stays below rel_l1_thresh.  The default polynomial
        is the identity: none has been fitted for ChronoEdit, callers pass the one published for their model family.  Only the loop
        skips; a direct forward call always runs the whole model.  Not available with the tokens sharded or with CFG parallelism."""
        from .teacache import TeaCacheConfig
        coefficients = tuple(float(c) for c in coefficients)
        if not coefficients:
            raise ValueError("enable_teacache: `coefficients` is empty")
        self._teacache = TeaCacheConfig(float(rel_l1_thresh), coefficients)
        return self

    def enable_guidance_reuse(self, pair_every: int = 2, interval=(0.0, 1.0)):
        """Guidance reuse in `pipeline.denoise` (chronoedit_amd/guidance.py): inside `interval` of the schedule one step in `pair_every`
        runs the guidance pair and stores the direction bf16(c - u); the others run the conditional sample alone and combine it with the
        stored direction; outside the interval the conditional sample runs unguided.  An edit without guidance ignores it.  Not together
        with TeaCache, not with the tokens sharded or with CFG parallelism."""
        from .guidance import GuidanceReuseConfig
        self._guidance_reuse = GuidanceReuseConfig(pair_every, tuple(interval))
        return self

    def disable_guidance_reuse(self):
        self._guidance_reuse = None
        return self

    def enable_sparse_region(self, refresh_every: int, start: float = 0.0, margin: int = 1):
        """Sparse region edits in `pipeline.denoise` (chronoedit_amd/sparse_region.py): in a region-limited edit (`region=`) one step in
        `refresh_every` runs the whole model and stores every layer's K / V^T of all tokens; the others run the model on the token rows under
        the mask (dilated by `margin` patches) only, their self-attention reading the stored K / V^T.  The first `start` of the schedule runs
        dense.  An edit without a region ignores it.  Not together with TeaCache or guidance reuse; only the default bf16 path with the
        transposed-V self-attention, not with the tokens sharded or with CFG parallelism."""
        from .sparse_region import SparseRegionConfig
        self._sparse_region = SparseRegionConfig(refresh_every, start, margin)
        return self

    def disable_sparse_region(self):
        self._sparse_region = None
        self._sparse_mode = None
        if self._engine is not None:
            self._engine.sparse_drop()
        return self

    def enable_auto_region(self, detect_step: int, threshold="otsu", floor: float = 0.0, dilate: int = 1, feather: int = 1,
                           max_area: float = 0.5, composite: bool = True, min_area=0):
        """Automatic edit regions (chronoedit_amd/auto_region.py): an edit without an explicit region looks for its own behind step
        `detect_step` and, when it finds one, continues as a region-limited edit (`pipeline.denoise(auto_region=)`; the pipeline supplies
        the source latents).  Off by default; an explicit region wins."""
        from .auto_region import AutoRegionConfig
        self._auto_region = AutoRegionConfig(detect_step, threshold, floor, dilate, feather, max_area, composite, min_area)
        return self

    def disable_auto_region(self):
        self._auto_region = None
        return self

    def disable_teacache(self):
        self._teacache = None
        self._tea_mode = None
        if self._engine is not None:
            self._engine.tea_release()
        return self

    @torch.no_grad()
    def calibrate_teacache(self, run_edits, degree: int = 4):
        """Fit the rescaling polynomial `enable_teacache` takes on THIS network (the loaded checkpoint with its active adapters).
        run_edits: callables, each running one edit through `pipeline.denoise` with this transformer; while they run the loop measures
        (every step computes, the latents are those of the plain loop) how far the block stack's residual moves from step to step - what
        a skipped step gets wrong.  The (ratio, distance) points of all edits are pooled and fitted (teacache.fit_calibration); returns
        the TeaCacheCalibration.  TeaCache itself is not switched on; an enabled TeaCache is refused by the loop."""
        from .teacache import fit_calibration
        ratios, distances = [], []
        self._tea_measure = True
        try:
            for run in run_edits:
                self.teacache_measurement = None
                run()
                if self.teacache_measurement is None:
                    raise RuntimeError("calibrate_teacache: the edit did not go through pipeline.denoise with this transformer")
                ratios.append(self.teacache_measurement["ratios"])
                distances.append(self.teacache_measurement["distances"])
        finally:
            self._tea_measure = False
        return fit_calibration(ratios, distances, degree)

    def teacache_ratios(self, timesteps: torch.Tensor):
        """Relative L1 distance of every scheduled step's time modulation to that of the step before it (entry 0 is 0.0): the time
        projections of all timesteps through the kernels the step itself uses, one reduction launch, ONE device-to-host read."""
        from .teacache import ratios_from_sums
        rows = self.engine().tea_tproj_rows(timesteps)
        return ratios_from_sums(ops.tea_rel_l1(rows).cpu().numpy(), rows.shape[1])

    def teacache_plan(self, timesteps: torch.Tensor, forced=()):
        """The compute (True) / skip (False) decision for every step of the schedule `timesteps` under the enabled threshold and
        polynomial; steps in `forced` compute."""
        from .teacache import plan_from_ratios
        if self._teacache is None:
            raise RuntimeError("teacache_plan: call enable_teacache(rel_l1_thresh) first")
        return plan_from_ratios(self.teacache_ratios(timesteps), int(timesteps.numel()), self._teacache.rel_l1_thresh,
                                self._teacache.coefficients, forced)

    def attention_path(self) -> str:
        """The self-attention arithmetic the next forward will actually run: "mxfp8" only when enable_fp8_attention() is on AND the
        tokens are not sharded - the sequence-parallel path exchanges bf16 q / k / v and runs the bf16 kernel (bench.py labels
        its lines from this, not from the flag)."""
        sharded = self._sp is not None and self._sp.sharded
        return "mxfp8" if (self.attn_dtype == "mxfp8" and not sharded) else "bf16"

    def _apply(self, fn, *a, **kw):  # .to() / .cuda() / .cpu() re-create storages
        self._engine = None
        out = super()._apply(fn, *a, **kw)
        self._lora_moved(fn)  # (the base store of switchable adapters is no parameter: it follows by hand)
        return out

    def load_state_dict(self, *a, **kw):
        self._engine = None
        return super().load_state_dict(*a, **kw)

    # Linear of a block -> the engine operand that shares its storage (DiTEngine.__init__): w_<slot> of the block's pack, or the all-layer
    # context buffers w_<slot>_all.  Every other Linear reaches the kernels as a padded or repacked copy (_pad_k / _pad_n, fp32 islands).
    _LORA_SLOTS = {"attn1.to_q": "qkv", "attn1.to_k": "qkv", "attn1.to_v": "qkv", "attn1.to_out.0": "o1", "attn2.to_q": "q2", "attn2.to_out.0": "o2",
                   "ffn.net.0.proj": "f1", "ffn.net.2": "f2", "attn2.to_k": "k_t", "attn2.to_v": "v_t", "attn2.add_k_proj": "k_i", "attn2.add_v_proj": "v_i"}
    _LORA_CONTEXT_SLOTS = ("k_t", "v_t", "k_i", "v_i")

    def _lora_weights_changed(self, modules):
        """An adapter switch rewrote these Linears' weights in place (weights.LoraMixin._lora_apply).  The packed engine stays: its block
        operands ARE the parameters' storage (the fused q|k|v and context buffers through the re-pointed row views).  What is derived from
        them is refreshed - the fp8 copies of the touched Linears, into their existing buffers, and the per-prompt context cache when a
        context projection changed.  A target whose operand is a padded or repacked copy drops the engine instead (re-packed by the next forward)."""
        eng = self._engine
        if eng is None:
            return
        own = dict(self.named_modules())
        requant, context = set(), False
        for m in modules:
            mt = re.match(r"^blocks\.(\d+)\.(.+)$", m)
            slot = self._LORA_SLOTS.get(mt.group(2)) if mt else None
            if slot is None:
                return self.invalidate()
            li = int(mt.group(1))
            op = getattr(eng, f"w_{slot}_all", None) if slot in self._LORA_CONTEXT_SLOTS else getattr(eng.blk[li], "w_" + slot, None)
            if op is None or op.untyped_storage().data_ptr() != own[m].weight.untyped_storage().data_ptr():
                return self.invalidate()
            context |= slot in self._LORA_CONTEXT_SLOTS
            if slot in eng.fp8_set:
                requant.add((li, slot))
        for li, slot in sorted(requant):
            p = eng.blk[li]
            q, s = getattr(p, "q_" + slot)
            (ops.quant_rows_mxfp8(getattr(p, "w_" + slot), out=q, scale=s, w_order=True) if eng.mx else
             ops.quant_rows_fp8(getattr(p, "w_" + slot), out=q, scale=s))
        if context:
            eng.clear_context_cache()

    def engine(self) -> "DiTEngine":
        rt = getattr(self, "_lora_rt", None)
        if rt is not None and rt.dirty:  # an adapter switch asked for before the model reached the GPU
            self._lora_apply()
        if self._engine is None:
            self._engine = DiTEngine(self)
            self._gen = next(_GENERATION)
        return self._engine

    def engine_generation(self):
        """A value that changes whenever something a captured step depends on may have been re-created lazily: the engine itself (packed
        weights), its workspaces, or a mode that alters the launch sequence (sequence / CFG parallelism, operand forms, fp8 switches, the
        RoPE spelling).  `pipeline.denoise` keys its "this shape has already run eagerly once" set on it, so a capture never records a
        first-time initialisation.  (Process-unique, unlike id(): a recycled address cannot alias an earlier model.)"""
        eng = self._engine
        sp = self._sp
        return (self._gen, None if eng is None else eng.ws_generation, self.gemm_dtype, self.fp8_linears, self.attn_dtype, self.v_transposed, self.cross_vt,
                self.sp_batch_cfg, bool(getattr(self, "rope_plain_temporal", False)), self.cache_context, self.shared_guidance, self.text_compaction,
                None if sp is None else (sp.world, sp.rank), self._cfgp is not None)

    @torch.no_grad()
    def forward(
        self,
        hidden_states: torch.Tensor,
        timestep: torch.LongTensor,
        encoder_hidden_states: torch.Tensor,
        encoder_hidden_states_image: Optional[torch.Tensor] = None,
        return_dict: bool = True,
        attention_kwargs: Optional[Dict[str, Any]] = None,
    ) -> Union[Transformer2DModelOutput, Tuple[torch.Tensor]]:
        if not hidden_states.is_cuda:
            raise ops.HipKernelError("ChronoEditTransformer3DModel (chronoedit_amd) runs only on an MI355X device: "
                                     "there is no CPU fallback (use oracle/ for CPU reference numbers)")
        B = hidden_states.shape[0]
        ts = timestep.reshape(-1)
        if ts.numel() == 1 and B > 1:
            ts = ts.expand(B)
        output = self.engine().forward(hidden_states, ts, encoder_hidden_states, encoder_hidden_states_image).to(hidden_states.dtype)
        if not return_dict:
            return (output,)
        return Transformer2DModelOutput(sample=output)


# ------------------------------------------------------------------------------------------
def rope_cos_sin(head_dim: int, max_len: int, skip_len: int, T: int, Hp: int, Wp: int, theta: float = 10000.0,
                 plain_temporal: bool = False) -> torch.Tensor:
    """[T*Hp*Wp, head_dim/2, 2] fp32 (cos, sin) of ChronoEditRotaryPosEmbed
    (transformer_chronoedit.py:168-213): per-axis dims (t, h, w) = (hd - 4*(hd//6), 2*(hd//6), 2*(hd//6)),
    angles in fp64; temporal indices {0, skip_len-1} when T == 2 (:205-207).  plain_temporal: indices 0..T-1 for any T,
    what the diffsynth call path uses (wan_video_new_chronoedit.py:1428-1432)."""
    assert plain_temporal or T == 2 or T == skip_len, f"num_frames must be 2 or {skip_len}, but got {T}"
    h_dim = w_dim = 2 * (head_dim // 6)
    t_dim = head_dim - h_dim - w_dim

    def ang(dim, idx):
        f = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float64)[: dim // 2] / dim))
        return torch.outer(idx.to(torch.float64), f)

    t_idx = torch.tensor([0, skip_len - 1]) if (T == 2 and not plain_temporal) else torch.arange(T)
    assert max(T, Hp, Wp, skip_len) <= max_len
    a_t = ang(t_dim, t_idx).view(T, 1, 1, -1).expand(T, Hp, Wp, -1)
    a_h = ang(h_dim, torch.arange(Hp)).view(1, Hp, 1, -1).expand(T, Hp, Wp, -1)
    a_w = ang(w_dim, torch.arange(Wp)).view(1, 1, Wp, -1).expand(T, Hp, Wp, -1)
    a = torch.cat([a_t, a_h, a_w], dim=-1).reshape(T * Hp * Wp, head_dim // 2)
    return torch.stack([torch.cos(a), torch.sin(a)], dim=-1).to(torch.float32).contiguous()


def _pad_k(w: torch.Tensor, mult: int = 64) -> torch.Tensor:
    K = w.shape[1]
    Kp = (K + mult - 1) // mult * mult
    if Kp == K:
        return w.contiguous()
    out = torch.zeros((w.shape[0], Kp), dtype=w.dtype, device=w.device)
    out[:, :K] = w
    return out


def _pad_n(w: torch.Tensor, b: Optional[torch.Tensor], mult: int = 8):
    N = w.shape[0]
    Np = (N + mult - 1) // mult * mult
    if Np == N:
        return w, b
    w2 = torch.zeros((Np, w.shape[1]), dtype=w.dtype, device=w.device)
    w2[:N] = w
    b2 = None
    if b is not None:
        b2 = torch.zeros((Np,), dtype=b.dtype, device=b.device)
        b2[:N] = b
    return w2, b2


class DiTEngine:
    """Packs the parameters once and runs the forward as a fixed sequence of HIP launches."""

    def __init__(self, model: ChronoEditTransformer3DModel):
        cfg = model.config
        self.cfg = cfg
        self.model = model
        dev = model.device
        if dev.type != "cuda":
            raise ops.HipKernelError("DiTEngine needs the model on the GPU")
        if model.dtype != torch.bfloat16:
            raise TypeError("the HIP path computes in bf16 (run_inference_diffusers.py hard-codes bf16, :344-362); "
                            f"got model dtype {model.dtype}")
        self.dev = dev
        self.D = cfg.num_attention_heads * cfg.attention_head_dim
        self.H = cfg.num_attention_heads
        self.F = cfg.ffn_dim
        self.L = cfg.num_layers
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        ce = model.condition_embedder

        # K1 patch embedding as a GEMM over im2col columns; K = C*4 zero-padded to 64
        self.kpatch = (cfg.in_channels * 4 + 63) // 64 * 64
        self.w_patch = _pad_k(model.patch_embedding.weight.detach().reshape(self.D, -1))
        self.b_patch = f32(model.patch_embedding.bias)

        # K2
        self.te_w1, self.te_b1 = ce.time_embedder.linear_1.weight.detach().contiguous(), f32(ce.time_embedder.linear_1.bias)
        self.te_w2, self.te_b2 = ce.time_embedder.linear_2.weight.detach().contiguous(), f32(ce.time_embedder.linear_2.bias)
        self.tp_w, self.tp_b = ce.time_proj.weight.detach().contiguous(), f32(ce.time_proj.bias)

        # K3
        self.tx_w1, self.tx_b1 = _pad_k(ce.text_embedder.linear_1.weight.detach()), f32(ce.text_embedder.linear_1.bias)
        self.tx_w2, self.tx_b2 = ce.text_embedder.linear_2.weight.detach().contiguous(), f32(ce.text_embedder.linear_2.bias)
        self.has_image = ce.image_embedder is not None
        if self.has_image:
            ie = ce.image_embedder
            self.im_n1 = (f32(ie.norm1.weight), f32(ie.norm1.bias), ie.norm1.eps)
            self.im_w1, self.im_b1 = _pad_k(ie.ff.net[0].proj.weight.detach()), f32(ie.ff.net[0].proj.bias)
            self.im_w2, self.im_b2 = _pad_k(ie.ff.net[2].weight.detach()), f32(ie.ff.net[2].bias)
            self.im_n2 = (f32(ie.norm2.weight), f32(ie.norm2.bias), ie.norm2.eps)

        # per-block packs.  Fused QKV / KV weights are single buffers; the module parameters are
        # re-pointed at views of them so the 14B model keeps ONE copy of every weight in HBM.
        self.blk = []
        tables = []
        for blk in model.blocks:
            p = SimpleNamespace()
            a1, a2 = blk.attn1, blk.attn2
            p.w_qkv = self._fuse([a1.to_q, a1.to_k, a1.to_v])
            p.b_qkv = torch.cat([f32(a1.to_q.bias), f32(a1.to_k.bias), f32(a1.to_v.bias)])
            p.nq1, p.nk1 = f32(a1.norm_q.weight), f32(a1.norm_k.weight)
            p.w_o1, p.b_o1 = a1.to_out[0].weight.detach().contiguous(), f32(a1.to_out[0].bias)
            p.w_q2, p.b_q2 = a2.to_q.weight.detach().contiguous(), f32(a2.to_q.bias)
            p.nq2, p.nk2 = f32(a2.norm_q.weight), f32(a2.norm_k.weight)
            p.has_img = a2.add_k_proj is not None
            if p.has_img:
                p.nk_i = f32(a2.norm_added_k.weight)
            p.w_o2, p.b_o2 = a2.to_out[0].weight.detach().contiguous(), f32(a2.to_out[0].bias)
            if cfg.cross_attn_norm:
                p.n2w, p.n2b = f32(blk.norm2.weight), f32(blk.norm2.bias)
            else:
                p.n2w = p.n2b = None
            p.w_f1, p.b_f1 = blk.ffn.net[0].proj.weight.detach().contiguous(), f32(blk.ffn.net[0].proj.bias)
            p.w_f2, p.b_f2 = blk.ffn.net[2].weight.detach().contiguous(), f32(blk.ffn.net[2].bias)
            tables.append(f32(blk.scale_shift_table).reshape(6, self.D))
            self.blk.append(p)
        self.fp8_attn = model.attn_dtype == "mxfp8"
        self.fp8_cross = self.fp8_attn and bool(getattr(model, "fp8_cross", False))  # cross-attention under the MXFP8 contract too
        self.fp8 = model.gemm_dtype in ("fp8", "mxfp8")
        self.mx = model.gemm_dtype == "mxfp8"  # MX block scales on both GEMM operands (ce_gemm_mxfp8)
        self.fp8_set = frozenset(getattr(model, "fp8_linears", model.FP8_LINEARS)) if self.fp8 else frozenset()  # which Linears (mixed precision)
        self.fuse_quant = bool(getattr(model, "fp8_fuse_quant", True)) and self.F % 128 == 0  # MX: quantisation fused into the FFN-up epilogue
        self.fuse_attn_quant = self.fuse_quant and bool(getattr(model, "fp8_fuse_attn_quant", True))
        fuse_o = self.mx and self.fuse_attn_quant and self.D % 128 == 0  # MX: both attention kernels emit the out-projections' fp8 operands themselves
        self.fuse_o1, self.fuse_o2 = fuse_o and "o1" in self.fp8_set, fuse_o and "o2" in self.fp8_set  # (only for an out-projection that runs in fp8)
        self.v_transposed = bool(getattr(model, "v_transposed", True))
        if self.fp8:
            if self.D % 256 or self.F % 256:
                raise NotImplementedError("fp8 GEMMs need inner and ffn dims that are multiples of 256")
            for p in self.blk:  # per-output-channel e4m3 copies of the six large weights (the bf16 originals stay)
                for name in sorted(self.fp8_set):
                    w = getattr(p, "w_" + name)  # (MX: the weight operand's scale order, ce_quant_rows_mxfp8_w)
                    setattr(p, "q_" + name, ops.quant_rows_mxfp8(w, w_order=True) if self.mx else ops.quant_rows_fp8(w))
        # K13 for ALL layers as one GEMM per context stream and operand: the per-layer to_k (to_v, add_k_proj, add_v_proj) weights are
        # re-homed, layer after layer, in one [L*D, D] buffer each (the step-invariant projections of 769 context rows are 160 small
        # GEMMs otherwise: 0.5-1.0 PFLOP/s at M = 514 / 1024 against 1.35 for one [M, L*D] product).  K and V apart (round 4): the V
        # half is taken as V^T = W_v . ctx^T - the same GEMM with its operand roles swapped and the bias along rows - which is the
        # operand the LDS-DMA form of the cross-attention kernel wants, at no extra pass.
        self.w_k_t_all = self._fuse([blk.attn2.to_k for blk in model.blocks])
        self.b_k_t_all = torch.cat([f32(blk.attn2.to_k.bias) for blk in model.blocks])
        self.w_v_t_all = self._fuse([blk.attn2.to_v for blk in model.blocks])
        self.b_v_t_all = torch.cat([f32(blk.attn2.to_v.bias) for blk in model.blocks])
        self.all_img = all(p.has_img for p in self.blk)  # (added_kv_proj_dim is one constructor argument: all layers or none)
        if self.all_img:
            self.w_k_i_all = self._fuse([blk.attn2.add_k_proj for blk in model.blocks])
            self.b_k_i_all = torch.cat([f32(blk.attn2.add_k_proj.bias) for blk in model.blocks])
            self.w_v_i_all = self._fuse([blk.attn2.add_v_proj for blk in model.blocks])
            self.b_v_i_all = torch.cat([f32(blk.attn2.add_v_proj.bias) for blk in model.blocks])
        self.cross_vt = bool(getattr(model, "cross_vt", True))
        self._ctx_bufs = {}
        self.tables = torch.stack(tables, 0).contiguous()  # [L, 6, D]
        self.table_out = f32(model.scale_shift_table).reshape(1, 2, self.D)
        self.w_out, self.b_out = _pad_n(model.proj_out.weight.detach().contiguous(), f32(model.proj_out.bias))
        self.ones = torch.ones(self.D, dtype=torch.float32, device=dev)
        self.zeros = torch.zeros(self.D, dtype=torch.float32, device=dev)
        self._rope = {}
        self._ws = {}
        self.ws_generation = 0  # bumped when a workspace is evicted (a shape seen before is then "new" again)
        # the context cache: one entry (key, ctx, keyed tensors) per FORM of the forward = its sample count - the stacked guidance pair and the
        # single sample.  A loop with guidance reuse alternates between the two; with one entry every switch would recompute the projections,
        # and a graph captured on a hit would replay over K tensors whose owner was dropped
        self._ctx_cache = {}
        self.ctx_projections = 0  # context projections computed (cache misses included) since clear_context_cache()
        self._tea_res = None      # TeaCache: the block stack's residual of the last computed step, bf16 [rows, D] (engine-owned)
        self._tea_valid = False   # ... and whether a computed step of THIS edit has written it
        self._tea_prev = None     # measuring only: the second residual buffer (the step before's residual; the two alternate)
        self._tea_sums = None     # measuring only: fp32 [steps, 2], row i = the two distance sums of step i (NaN: nothing measured)
        self._tea_row = 0         # ... and the row the next measured forward writes (set by the loop)
        self._sparse = None       # sparse region edits: the active ids, the sparse workspace and the K / V^T cache of one edit (sparse_begin)
        self._sparse_ran = set()  # ... and the geometries (B, Na, N) a sparse step has run eagerly at on this engine (sparse_is_warm)
        self._tap = None          # tests: a dict here receives copies of intermediates of eager (not captured) forwards ("x_pre_cross0": block 0's stream in front of its cross-attention)

    def _fuse(self, linears) -> torch.Tensor:
        """cat the [out,in] weights into one buffer and re-point the module parameters at its rows."""
        w = torch.cat([l.weight.detach() for l in linears], dim=0).contiguous()
        o = 0
        for l in linears:
            n = l.weight.shape[0]
            l.weight.data = w[o : o + n]
            o += n
        return w

    def _ln_linear(self, ws, x: torch.Tensor, a_row, b_row, p, name: str, out: torch.Tensor, ab_rows: int = 0, ab_stride: int = 0, **kw):
        """LayerNorm (+ affine / AdaLN rows) followed by one of the large projections.  fp8 mode: the LN kernel emits the fp8
        operand and its row scales directly (no bf16 round trip through HBM, no separate quantisation pass).  bf16: x may be a row range of
        the workspace (the normed rows go to the same range of ws.h)."""
        eps = self.cfg.eps
        if name not in self.fp8_set:
            h = ws.h[: x.shape[0]]
            ops.ln_affine(x, a_row, b_row, eps, out=h, ab_rows=ab_rows, ab_stride=ab_stride)
            return ops.gemm(h, getattr(p, "w_" + name), getattr(p, "b_" + name), out=out, **kw)
        aq = ws.a8[:, : x.shape[1]]
        wq, sw = getattr(p, "q_" + name)
        if self.mx:
            ops.ln_affine_mxfp8(x, a_row, b_row, eps, out=aq, scale=ws.s8, ab_rows=ab_rows, ab_stride=ab_stride)
            return ops.gemm_mxfp8(aq, ws.s8, wq, sw, getattr(p, "b_" + name), out=out, **kw)
        ops.ln_affine_fp8(x, a_row, b_row, eps, out=aq, scale=ws.s8, ab_rows=ab_rows, ab_stride=ab_stride)
        return ops.gemm_fp8(aq, ws.s8, wq, sw, getattr(p, "b_" + name), out=out, **kw)

    def _linear(self, ws, a: torch.Tensor, p, name: str, out: torch.Tensor, quantised: bool = False, **kw):
        """One of the six large projections of a block: bf16 GEMM, or (fp8 mode) row-quantise the activations and run the MX GEMM.
        quantised: the producer already wrote the MX operand into ws.a8 / ws.s8 (an attention kernel's fused output)."""
        w, b = getattr(p, "w_" + name), getattr(p, "b_" + name)
        if name not in self.fp8_set:
            assert not quantised, name  # (a bf16 Linear takes bf16 activations: the caller did not ask its producer for the MX operand)
            return ops.gemm(a, w, b, out=out, **kw)
        K = a.shape[1]
        aq = ws.a8[:, :K]
        wq, sw = getattr(p, "q_" + name)
        if self.mx:
            if not quantised:
                ops.quant_rows_mxfp8(a, out=aq, scale=ws.s8)
            return ops.gemm_mxfp8(aq, ws.s8, wq, sw, b, out=out, **kw)
        ops.quant_rows_fp8(a, out=aq, scale=ws.s8)
        return ops.gemm_fp8(aq, ws.s8, wq, sw, b, out=out, **kw)

    def _self_attention_ulysses(self, ws, sp, x, a_row, b_row, p, cs, N: int, Nl: int, B: int = 1):
        """Self-attention with the tokens sharded over sp.world ranks (parallel.py has the layout story); B samples stacked [sample][local
        token] along the rows (B > 1: the blocked receive layout, Nl a multiple of 64).
        The fused q|k|v projection runs as two GEMMs - [k | v] first - so that the k|v exchange (2/3 of the volume) is on
        the wire while the q projection is still computing; q / k are normalised and rotated by the pass that writes the
        all-to-all send layout; the attention kernel and the out-projection read the receive buffers in place."""
        D, H, hd, eps, W = self.D, self.H, self.cfg.attention_head_dim, self.cfg.eps, sp.world
        Dl = D // W
        if "qkv" not in self.fp8_set:
            ops.ln_affine(x, a_row, b_row, eps, out=ws.h, ab_rows=Nl, ab_stride=6 * D)
            lin = lambda lo, hi, out: ops.gemm(ws.h, p.w_qkv[lo:hi], p.b_qkv[lo:hi], out=out)
        else:
            aq = ws.a8[:, :D]
            wq, sw = p.q_qkv
            if self.mx:  # (row slices of the fused weight at multiples of D = whole 128-row scale blocks: 512 (D / 128) bytes per block)
                ops.ln_affine_mxfp8(x, a_row, b_row, eps, out=aq, scale=ws.s8, ab_rows=Nl, ab_stride=6 * D)
                sblk = (D // 128) * 512
                lin = lambda lo, hi, out: ops.gemm_mxfp8(aq, ws.s8, wq[lo:hi], sw[lo // 128 * sblk: hi // 128 * sblk], p.b_qkv[lo:hi], out=out)
            else:
                ops.ln_affine_fp8(x, a_row, b_row, eps, out=aq, scale=ws.s8, ab_rows=Nl, ab_stride=6 * D)
                lin = lambda lo, hi, out: ops.gemm_fp8(aq, ws.s8, wq[lo:hi], sw[lo:hi], p.b_qkv[lo:hi], out=out)
        lin(D, 3 * D, ws.qkv[:, D:])
        ops.rope_scatter(ws.qkv, (D, 2 * D), (p.nk1, None), D, W, cs, hd, eps, out=ws.send_kv)
        _, wait_kv = sp.all_to_all(ws.send_kv, ws.recv_kv, async_op=True)
        lin(0, D, ws.qkv[:, :D])
        ops.rope_scatter(ws.qkv, (0,), (p.nq1,), D, W, cs, hd, eps, out=ws.send_q)
        _, wait_q = sp.all_to_all(ws.send_q, ws.recv_q, async_op=True)
        wait_kv.wait()
        wait_q.wait()
        kv = sp.gathered_view(ws.recv_kv)  # [W*Nl = global token, k | v of this rank's heads]
        if B > 1:  # rows are [source rank][sample][local token]: the blocked forms of the transposer and of the attention kernel
            vt_shape = (Dl, B * ops.vt_columns(N))
            ws.vt_sp = ops.v_transpose_blocked(kv[:, Dl:], H // W, B, Nl, N, out=ws.vt_sp if getattr(ws, "vt_sp", torch.empty(0)).shape == vt_shape else None)
            ops.attention_vt_blocked(sp.gathered_view(ws.recv_q), kv[:, :Dl], ws.vt_sp, H // W, B, Nl, N, out=ws.att_g)
        elif self.v_transposed:  # the LDS-DMA form of the kernel wants V^T: one small transpose pass over this rank's heads
            if getattr(ws, "vt_sp", None) is None or ws.vt_sp.shape != (Dl, ops.vt_columns(N)):
                ws.vt_sp = torch.zeros((Dl, ops.vt_columns(N)), dtype=torch.bfloat16, device=self.dev)
            ops.v_transpose(kv[:N, Dl:], H // W, out=ws.vt_sp)
            ops.attention_vt(sp.gathered_view(ws.recv_q), kv[:N, :Dl], ws.vt_sp, H // W, out=ws.att_g)
        else:
            ops.attention(sp.gathered_view(ws.recv_q), kv[:N, :Dl], kv[:N, Dl:], H // W, out=ws.att_g)
        y, _ = sp.all_to_all(ws.att_g.view(W, B * Nl, Dl), ws.att_seg)  # [head group][local row][Dl]
        if "o1" in self.fp8_set:  # the row quantiser wants plain rows: secondary mode, one gather pass
            ws.att.copy_(sp.merge_heads_reference(y))
            return ws.att
        return y  # K-segmented A operand of the out-projection (a_seg_k of ce_gemm_bf16)

    # -- workspaces --------------------------------------------------------------------
    def _row_buffers(self, M: int):
        """The bf16 buffers every launch sequence over M token rows works in."""
        D = self.D
        e = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=self.dev)
        return SimpleNamespace(x=e(M, D), h=e(M, D), qkv=e(M, 3 * D), att=e(M, D), q2=e(M, D), ffn=e(M, self.F),
                               cols=e(M, self.kpatch), head=e(M, self.w_out.shape[0]))

    def _workspace(self, N: int):
        ws = self._ws.get(N)
        if ws is None:
            D, F, dev = self.D, self.F, self.dev
            e = lambda *s: torch.empty(s, dtype=torch.bfloat16, device=dev)
            ws = self._row_buffers(N)
            if self.fp8:  # activation rows as fp8 + one scale per row (MX: one E8M0 byte per 32 elements, tiled: ops.mx_scale_bytes)
                ws.a8 = torch.empty((N, max(D, F)), dtype=torch.uint8, device=dev)
                ws.s8 = (torch.empty((ops.mx_scale_bytes(N, max(D, F)),), dtype=torch.uint8, device=dev) if self.mx else
                         torch.empty((N,), dtype=torch.float32, device=dev))
                if self.mx and self.fuse_quant and F % 128 == 0:  # the FFN hidden activation as the up-projection's epilogue writes it
                    ws.a8b = torch.empty((N, F), dtype=torch.uint8, device=dev)
                    ws.s8b = torch.empty((ops.mx_scale_bytes(N, F),), dtype=torch.uint8, device=dev)
            if self.fp8_attn:  # MXFP8 q / k (+ E8M0 scale bytes); the V^T tiles depend on the batch split and are sized in forward
                u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
                ws.q8, ws.k8, ws.sq, ws.sk = u8(N, D), u8(N, D), u8(N, D // 32), u8(N, D // 32)
                ws.v8t = ws.sv = None
            sp = self.model._sp
            if sp is not None and sp.sharded:  # Ulysses exchange buffers (chronoedit_amd/parallel.py): N = local rows
                W, Dl = sp.world, D // sp.world
                ws.send_kv, ws.recv_kv = e(W, N, 2, Dl), e(W, N, 2, Dl)
                ws.send_q, ws.recv_q = e(W, N, 1, Dl), e(W, N, 1, Dl)
                ws.att_g, ws.att_seg = e(W * N, Dl), e(W, N, Dl)
            # keep the two most recent shapes resident: a temporal-reasoning edit alternates between its 8-frame and 2-frame shapes, and a
            # hipGraph capture of a shape seen before must find its workspace (nothing may be allocated for the engine under capture)
            if len(self._ws) > 1:
                self.ws_generation += 1  # the oldest shape leaves: a warm-set entry for it is stale
            keep = list(self._ws.items())[-1:]
            self._ws = dict(keep + [(N, ws)])
        return ws

    def _rope_table(self, T, Hp, Wp):
        plain = bool(getattr(self.model, "rope_plain_temporal", False))
        key = (T, Hp, Wp, plain)
        if key not in self._rope:
            c = self.cfg
            if len(self._rope) >= 4:  # a handful of latent shapes per process (8 / 2 frames, + their sharded slices)
                self._rope.pop(next(iter(self._rope)))
            self._rope[key] = rope_cos_sin(c.attention_head_dim, c.rope_max_seq_len, c.rope_temporal_skip_len, T, Hp, Wp,
                                           plain_temporal=plain).to(self.dev)
        return self._rope[key]

    def is_warm(self, B: int, T: int, Hh: int, Ww: int) -> bool:
        """Has a forward of exactly this shape already run through this engine (workspace and RoPE table resident)?  What a hipGraph
        capture without a warm-up step requires (pipeline.GraphedDenoiser)."""
        plain = bool(getattr(self.model, "rope_plain_temporal", False))
        N = T * (Hh // 2) * (Ww // 2)
        return (B * N) in self._ws and (T, Hh // 2, Ww // 2, plain) in self._rope

    # -- K3 + K13: conditioning-side work (step-invariant) -------------------------------
    def _cross_fp8(self) -> bool:
        """Does the cross-attention run under the MXFP8 contract (enable_fp8_attention(cross=True), unsharded)?"""
        m = self.model
        return bool(self.fp8_cross and (m._sp is None or not m._sp.sharded) and getattr(m, "_cfgp", None) is None)

    def _cross_vt_form(self, Tt: int, image_given: bool) -> bool:
        """Does the cross-attention take V^T from the context projections (ce_attention_2seg_vt_bf16)?  ONE predicate for `_context`, which
        builds the operands, and `_share_image`, which may only share a segment in this form."""
        return bool(self.cross_vt and image_given and self.has_image and self.all_img and Tt % 8 == 0 and not self._cross_fp8())

    def _plain_vt_path(self, Tt: int) -> bool:
        """Is this the one launch sequence that can express a shared image segment and a compacted text: plain bf16, unsharded, with the
        transposed-V self- and cross-attention (an image context of this model given)?"""
        m = self.model
        return bool(self._cross_vt_form(Tt, True) and not self.fp8 and not self.fp8_attn and self.v_transposed
                    and (m._sp is None or not m._sp.sharded) and getattr(m, "_cfgp", None) is None)

    def _share_image(self, text: torch.Tensor, image: Optional[torch.Tensor]) -> bool:
        """Does this forward project the image context ONCE for its two samples?  Only when the caller declared the pair's inputs shared
        (model._shared_inputs; never inferred from the tensors) and the launch sequence is the one that can express it: two samples on
        `_plain_vt_path`.  Everything else keeps the stacked sequence, silently."""
        m = self.model
        return bool(m._shared_inputs and m.shared_guidance and image is not None and text.shape[0] == 2 and image.shape[0] == 2
                    and self._plain_vt_path(text.shape[1]))

    def _text_compact(self, text: torch.Tensor, image: Optional[torch.Tensor]):
        """The compacted form of this text context (pipeline.compact_text_context hung it on the tensor where the edit's context was built),
        or None: switched off, a tensor nobody examined or that changed since, nothing to save, or a launch sequence that cannot express it
        (as `_share_image`: `_plain_vt_path`).  Never inferred from the tensor's content here."""
        m = self.model
        info = getattr(text, "_ce_compact", None)
        if info is None or info.text is None or not m.text_compaction or info.version != text._version or info.shape != tuple(text.shape):
            return None
        if image is None or not self._plain_vt_path(text.shape[1]):
            return None
        return info

    def _context(self, text: torch.Tensor, image: Optional[torch.Tensor], share_image: bool = False):
        """text [B, Tt, text_dim], image [B, Ti, image_dim] -> per-layer cross-attention K/V, samples stacked along rows.
        share_image (_share_image): image[0] stands for every sample - the image embedder and the image K / V^T projections run on its rows only.
        A text tensor that carries a compacted form (_text_compact) is projected on its Lc rows per sample instead of Tt: ctx.Tt = Lc, and
        ctx.valid / ctx.w (device arrays that live with the tensor, hence with the cache entry) go to the weighted cross-attention."""
        key = None
        cmp = self._text_compact(text, image)
        if self.model.cache_context:
            # The entry keeps the keyed tensors alive (its third member): an address can then not be handed out again for another
            # edit's conditioning while the entry exists, so (data_ptr, _version, shape) identifies the CONTENT, not just a slot.
            key = (text.data_ptr(), text._version, tuple(text.shape), text.dtype,
                   None if image is None else (image.data_ptr(), image._version, tuple(image.shape), image.dtype), bool(share_image),
                   cmp is not None)
            hit = self._ctx_cache.get(text.shape[0])
            if hit is not None and hit[0] == key:
                return hit[1]
        keyed = (text, image)
        form = text.shape[0]
        self.ctx_projections += 1
        D = self.D
        if cmp is not None:  # rows [0, Lc) of every sample: its real rows, ONE padding row, then rows the kernel masks
            text = cmp.text
        B, Tt = text.shape[0], text.shape[1]
        share_image = bool(share_image and B == 2 and self._cross_vt_form(Tt, image is not None))  # (any other form: stacked, silently)
        Bi = 1 if share_image else B  # samples of image context actually projected
        text = text.to(torch.bfloat16).reshape(B * Tt, -1)
        if text.shape[1] != self.tx_w1.shape[1]:
            tp = torch.zeros((text.shape[0], self.tx_w1.shape[1]), dtype=torch.bfloat16, device=self.dev)
            tp[:, : text.shape[1]] = text
            text = tp
        t1 = ops.gemm(text.contiguous(), self.tx_w1, self.tx_b1, epilogue=ops.EPI_BIAS_GELU)
        enc_t = ops.gemm(t1, self.tx_w2, self.tx_b2)
        enc_i = None
        Ti = 0
        if image is not None:
            if not self.has_image:
                raise ValueError("encoder_hidden_states_image given but the model has no image_embedder (image_dim=None)")
            Ti = image.shape[1]
            if share_image:
                image = image[:1]
            image = image.to(torch.bfloat16).reshape(Bi * Ti, -1).contiguous()
            w, b, eps = self.im_n1
            h = ops.ln_affine(image, w, b, eps)
            if h.shape[1] != self.im_w1.shape[1]:
                hp = torch.zeros((h.shape[0], self.im_w1.shape[1]), dtype=torch.bfloat16, device=self.dev)
                hp[:, : h.shape[1]] = h
                h = hp
            h = ops.gemm(h, self.im_w1, self.im_b1, epilogue=ops.EPI_BIAS_GELU_ERF)
            if h.shape[1] != self.im_w2.shape[1]:
                hp = torch.zeros((h.shape[0], self.im_w2.shape[1]), dtype=torch.bfloat16, device=self.dev)
                hp[:, : h.shape[1]] = h
                h = hp
            h_img = ops.gemm(h, self.im_w2, self.im_b2)
            w, b, eps = self.im_n2
            enc_i = ops.ln_affine(h_img, w, b, eps)
        # K13: per-layer cross-attention K/V of the text and image context, all layers per launch: K row-major [B*len, L*D] (layer li
        # = columns [li D, (li+1) D)), V either row-major the same way or TRANSPOSED [L*D, columns] (layer li = rows [li D, (li+1) D),
        # sample b's keys at columns [b cols, b cols + len)) for ce_attention_2seg_vt_bf16.  The V^T form needs the N axis of its
        # swapped-role GEMM (= key rows of all samples) in multiples of 8 with even per-sample strides: Tt % 8 == 0 (512), and the image
        # context (257 rows) is layer-normed a second time into a copy whose samples are padded to 264 rows (zero rows -> bias-only
        # columns that meet P = 0).
        eps = self.cfg.eps
        hd = self.cfg.attention_head_dim
        L = self.L
        f8 = self._cross_fp8()
        use_vt = self._cross_vt_form(Tt, enc_i is not None)
        k_t_all = ops.gemm(enc_t, self.w_k_t_all, self.b_k_t_all)  # [B*Tt, L*D]
        k_i_all = v_t_all = v_i_all = v1t = v2t = None
        c1 = c2 = 0
        if enc_i is not None and self.all_img:
            k_i_all = ops.gemm(enc_i, self.w_k_i_all, self.b_k_i_all)
        if use_vt:
            c1, c2 = Tt, (Ti + 7) // 8 * 8
            ld1 = ((B - 1) * c1 + (Tt + 63) // 64 * 64 + 7) // 8 * 8
            ld2 = ((Bi - 1) * c2 + (Ti + 63) // 64 * 64 + 7) // 8 * 8
            bufs = self._ctx_bufs.get((B, Bi, Tt, Ti))
            if bufs is None:  # zero-filled once: the padding rows / columns are never written afterwards.  Engine-owned (not per call):
                # a captured step that computes the projections (cache_context off) replays into the same addresses
                if cmp is not None and torch.cuda.is_current_stream_capturing():  # (their size follows the prompt's length)
                    raise RuntimeError(f"no context buffers for {(B, Bi, Tt, Ti)} exist and none can be allocated under a hipGraph capture "
                                       "(prime_context first)")
                z = lambda *sh: torch.zeros(sh, dtype=torch.bfloat16, device=self.dev)
                bufs = SimpleNamespace(enc_i_pad=z(Bi * c2, D), v1t=z(L * D, ld1), v2t=z(L * D, ld2))
                self._ctx_bufs = dict(list(self._ctx_bufs.items())[-1:] + [((B, Bi, Tt, Ti), bufs)])  # the guided pair and the single sample
            v1t, v2t = bufs.v1t, bufs.v2t
            # these engine-owned buffers are about to be rewritten in place, and a cached context of the same shape holds VIEWS into them
            # (its K tensors are its own): whatever was cached is stale from here on - drop it, so a later hit cannot pair the old K with
            # another conditioning's V^T (a call with cache_context off, key None, would otherwise leave the cached key standing)
            # (the other form's entry lives in buffers of another sample count: it stays)
            self._ctx_cache.pop(form, None)
            w, b, eps_i = self.im_n2
            for bi in range(Bi):
                ops.ln_affine(h_img[bi * Ti:(bi + 1) * Ti], w, b, eps_i, out=bufs.enc_i_pad[bi * c2: bi * c2 + Ti])
            ops.gemm(self.w_v_t_all, enc_t, self.b_v_t_all, out=v1t[:, : B * Tt], epilogue=ops.EPI_BIAS_ROW)
            ops.gemm(self.w_v_i_all, bufs.enc_i_pad, self.b_v_i_all, out=v2t[:, : Bi * c2], epilogue=ops.EPI_BIAS_ROW)
        else:
            v_t_all = ops.gemm(enc_t, self.w_v_t_all, self.b_v_t_all)
            if k_i_all is not None:
                v_i_all = ops.gemm(enc_i, self.w_v_i_all, self.b_v_i_all)
        kv = []
        for li, p in enumerate(self.blk if not f8 else ()):
            cols = slice(li * D, (li + 1) * D)
            k_t = k_t_all[:, cols]
            ops.rmsnorm_rope_(k_t, p.nk2, None, hd, eps)
            k_i = None
            if k_i_all is not None:
                k_i = k_i_all[:, cols]
                ops.rmsnorm_rope_(k_i, p.nk_i, None, hd, eps)
            if use_vt:
                kv.append((k_t, v1t[cols], k_i, v2t[cols]))
            else:
                kv.append((k_t, v_t_all[:, cols], k_i, None if v_i_all is None else v_i_all[:, cols]))
        if f8:
            # MXFP8 operands of both segments, per layer: K (RMS-normed, no RoPE) quantised along the head channels, V^T tiles quantised along
            # the keys (ce_rmsnorm_rope_mxfp8 reads the un-normed projection: the bf16 loop above, which norms in place, did not run)
            for li, p in enumerate(self.blk):
                cols = slice(li * D, (li + 1) * D)
                seg_t = ops.rmsnorm_rope_mxfp8(k_t_all[:, cols], p.nk2, None, hd, eps) + ops.v_mxfp8_transpose(v_t_all[:, cols], Tt, B, self.H)
                seg_i = None
                if k_i_all is not None:
                    seg_i = ops.rmsnorm_rope_mxfp8(k_i_all[:, cols], p.nk_i, None, hd, eps) + ops.v_mxfp8_transpose(v_i_all[:, cols], Ti, B, self.H)
                kv.append((seg_t, seg_i))
        assert cmp is None or (use_vt and not f8)
        ctx = SimpleNamespace(kv=kv, Tt=Tt, Ti=Ti, vt=use_vt, c1=c1, c2=c2, f8=f8, img_shared=bool(share_image),
                              valid=None if cmp is None else cmp.valid, w=None if cmp is None else cmp.w)
        if key is not None:
            self._ctx_cache.pop(form, None)  # (re-inserted last: _ctx_key names the newest entry)
            self._ctx_cache[form] = (key, ctx, keyed)
            while len(self._ctx_cache) > 2:  # the pair and the single sample; a third sample count evicts the oldest
                self._ctx_cache.pop(next(iter(self._ctx_cache)))
        return ctx

    @property
    def _ctx_key(self):
        """The key of the newest cache entry, None when nothing is cached."""
        return next(reversed(self._ctx_cache.values()))[0] if self._ctx_cache else None

    def clear_context_cache(self):
        """Drop the cached conditioning-side results of every form (called by the pipeline at the start of every edit)."""
        self._ctx_cache = {}
        self.ctx_projections = 0

    # -- TeaCache (chronoedit_amd/teacache.py) ---------------------------------------------
    def tea_reserve(self, rows: int) -> torch.Tensor:
        """The residual buffer for `rows` token rows (all samples of a forward).  Re-allocated - and its content dropped - when the row
        count changes; never under a hipGraph capture (the compute and the skip graph of a loop share its address):
        pipeline.GraphedDenoiser reserves it in front of every capture."""
        if self._tea_res is None or self._tea_res.shape[0] != rows:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"TeaCache: no residual buffer of {rows} rows exists and none can be allocated under a hipGraph capture")
            self._tea_res = None
            self._tea_res = torch.empty((rows, self.D), dtype=torch.bfloat16, device=self.dev)
            self._tea_valid = False
        return self._tea_res

    def tea_drop(self):
        """Forget the cached residual (a new edit starts); the buffer stays."""
        self._tea_valid = False

    def tea_release(self):
        self._tea_res = self._tea_prev = self._tea_sums = None
        self._tea_valid = False

    def tea_measure_begin(self, steps: int):
        """A measured edit starts: the sums table, nothing of an earlier edit's residual to compare with."""
        self._tea_sums = torch.full((steps, 2), float("nan"), dtype=torch.float32, device=self.dev)
        self._tea_prev = None
        self._tea_row = 0
        self._tea_valid = False

    def tea_measure_end(self) -> torch.Tensor:
        """The sums table on the host (the one device-to-host read of a measured edit); the second residual buffer is given back."""
        sums, self._tea_sums, self._tea_prev = self._tea_sums, None, None
        return sums.cpu()

    def _tea_measure_buffers(self, rows: int):
        """(buffer for this step's saved tokens, previous step's residual or None).  The two buffers alternate: this step's residual is
        written where the residual of two steps ago was, while the previous one is read.  A change of row count drops the previous residual."""
        if self._tea_sums is None:
            raise RuntimeError("TeaCache: a measured step outside a measured edit (pipeline.denoise(teacache_measure=True))")
        prev = self._tea_res if self._tea_valid and self._tea_res is not None and self._tea_res.shape[0] == rows else None
        if prev is None:
            self._tea_prev = None
            return self.tea_reserve(rows), None
        cur = self._tea_prev if self._tea_prev is not None else torch.empty_like(prev)
        self._tea_res, self._tea_prev = cur, prev
        return cur, prev

    def tea_tproj_rows(self, timesteps: torch.Tensor) -> torch.Tensor:
        """bf16 [S, 6*D]: the time projection (K2 of the forward: sinusoid -> time_embedder -> silu -> time_proj) of every timestep, by
        the very launches a step makes - bit-identical to the `tproj` the step computes."""
        ts = timesteps.reshape(-1)
        ts = ts.to(device=self.dev, dtype=torch.float32 if ts.is_floating_point() else torch.int64).contiguous()
        rows = torch.empty((ts.numel(), 6 * self.D), dtype=torch.float32, device=self.dev)
        for i in range(ts.numel()):
            sin = ops.timestep_sinusoid(ts[i : i + 1], self.cfg.freq_dim)
            h1 = ops.gemv(self.te_w1, sin, self.te_b1, flags=2)
            temb = ops.gemv(self.te_w2, h1, self.te_b2, flags=4)
            ops.gemv(self.tp_w, temb, self.tp_b, flags=1 | 4, out=rows[i])
        return rows.to(torch.bfloat16)  # (exact: flag 4 left bf16 values in the fp32 rows)

    # -- sparse region edits (chronoedit_amd/sparse_region.py) -------------------------------
    def sparse_check(self, B: int = 1, N: int = 0):
        """The launch sequences a sparse region edit exists for: the default bf16 path with the transposed-V self-attention, unsharded."""
        m = self.model
        if self.fp8 or self.fp8_attn:
            raise NotImplementedError("sparse region edits with fp8 GEMMs or fp8 attention are not implemented: the cached K / V^T are the "
                                      "bf16 attention kernel's operands")
        if not self.v_transposed:
            raise NotImplementedError("sparse region edits need the transposed-V self-attention (enable_transposed_v): the cache holds V^T")
        if (m._sp is not None and m._sp.sharded) or getattr(m, "_cfgp", None) is not None:
            raise NotImplementedError("sparse region edits with the tokens sharded over ranks or with CFG parallelism are not implemented "
                                      "(the cache is row-local; nothing sharded has been tested with it)")
        if N and ((B * N) % 8 or (B > 1 and N % 2)):
            raise NotImplementedError(f"sparse region edits need the V^T form of the dense step: {B} x {N} token rows are not a multiple of 8 "
                                      "(or an odd count per sample)")

    def sparse_begin(self, ids: torch.Tensor, B: int, T: int, Hh: int, Ww: int):
        """A sparse region edit starts: `ids` (sparse_region.active_tokens: sorted, unique, a multiple of 8 of them, validated HERE, once) are
        the active token rows of every one of the B samples of a forward on latents [.., T, Hh, Ww].  Reserves, outside any capture,
          * the K / V^T cache, [L][B*N, D] and [L][D][vt_columns(B*N)] bf16 - at 720p with a guidance pair 40 x 2 x 14 400 x 5 120 x 2 B =
            11.8 GB; never at the 8-frame shape of a temporal-reasoning edit, whose steps are all "compute";
          * the workspace of the sparse steps (B*Na rows) - here, not in `_ws`, which holds the two most recent dense shapes only;
          * the RoPE table of the active rows, gathered once.
        A second call with the same geometry keeps the buffers (and drops what the cache holds); `sparse_drop` gives everything back."""
        from .sparse_region import validate_ids
        B, T, Hh, Ww = int(B), int(T), int(Hh), int(Ww)
        Hp, Wp = Hh // 2, Ww // 2
        N = T * Hp * Wp
        self.sparse_check(B, N)
        host = validate_ids(ids, N)
        Na = host.numel()
        if Na % 8:
            raise ValueError(f"sparse region: the active rows per sample must be a multiple of 8 (sparse_region.active_tokens pads), got {Na}")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("sparse region: sparse_begin allocates; it cannot run under a hipGraph capture")
        D, L, dev = self.D, self.L, self.dev
        st = self._sparse
        if st is None or (st.B, st.N) != (B, N):
            self._sparse = st = None  # (the old cache goes before the new one comes)
            st = SimpleNamespace(B=B, N=N, k=torch.empty((L, B * N, D), dtype=torch.bfloat16, device=dev),
                                 vt=torch.zeros((L, D, ops.vt_columns(B * N)), dtype=torch.bfloat16, device=dev), Na=0, ws=None)
        if st.Na != Na:
            st.ws = self._row_buffers(B * Na)
        st.T, st.Hh, st.Ww, st.Na = T, Hh, Ww, Na
        st.ids = host.to(device=dev, dtype=torch.int32)
        st.cs = self._rope_table(T, Hp, Wp)[host.to(dev)].contiguous()
        st.valid = False  # no refresh step of THIS edit has filled the cache yet
        self._sparse = st
        return st

    def sparse_drop(self):
        """Forget the active ids and give the cache and the sparse workspace back."""
        self._sparse = None

    def sparse_is_warm(self) -> bool:
        """Has a sparse step of the begun edit's geometry already run eagerly through this engine?  What a hipGraph capture of a sparse step
        without an eager one in front requires (pipeline.GraphedDenoiser), as `is_warm` for the dense forms."""
        st = self._sparse
        return st is not None and (st.B, st.Na, st.N) in self._sparse_ran

    def _sparse_state(self, B: int, T: int, Hh: int, Ww: int):
        st = self._sparse
        if st is None or (st.B, st.T, st.Hh, st.Ww) != (B, T, Hh, Ww):
            raise RuntimeError(f"sparse region: no sparse_begin for {B} samples of latents [.., {T}, {Hh}, {Ww}]"
                               + ("" if st is None else f" (the edit was begun for {(st.B, st.T, st.Hh, st.Ww)})"))
        return st

    def _forward_sparse(self, st, hidden: torch.Tensor, timestep: torch.Tensor, text: torch.Tensor, image: Optional[torch.Tensor]):
        """A "sparse" step: the plain forward's arithmetic on the Na active token rows of every sample.  Per block the fresh K (after norm +
        RoPE) and V^T of the active rows replace their entries in the layer's cache, and the self-attention runs Na queries against all N
        cached keys; everything else is row-local and runs on B*Na rows.  The prediction is written at the active tokens' cells of an output
        that is zero elsewhere (the region blend discards it there).  The guidance pair's shared prefix is not used."""
        cfg, D, H = self.cfg, self.D, self.H
        B, C, T, Hh, Ww = hidden.shape
        hd, eps = cfg.attention_head_dim, cfg.eps
        if not st.valid:
            raise RuntimeError("sparse region: a sparse step needs the K / V^T a refresh step of this edit stored")
        self.sparse_check(B, st.N)
        Na, N, ids, cs, ws = st.Na, st.N, st.ids, st.cs, st.ws
        hidden = hidden.to(torch.bfloat16).contiguous()
        rows = [slice(b * Na, (b + 1) * Na) for b in range(B)]
        for b in range(B):
            ops.sparse_patchify(hidden[b], ids, self.kpatch, out=ws.cols[rows[b]])
        x = ops.gemm(ws.cols, self.w_patch, self.b_patch, out=ws.x)
        _, mod, mod_out, gate_msa, gate_ffn = self._time_tables(timestep, B, B)  # ab_rows / gate_rows = Na
        grow = Na if B > 1 else 0
        # the context in the form the dense steps of this edit use: the same cache entry serves both kinds
        ctx = self._context(text, image, share_image=B == 2 and self._share_image(text, image))
        if ctx.f8:
            raise NotImplementedError("sparse region edits with fp8 cross-attention are not implemented")
        for li, p in enumerate(self.blk):
            # 1. self-attention: q | k | v of the active rows as ONE product; k and v are scattered into the layer's cache, v transposed on
            # the way (measured at 720p, profiles/notes_region_sparse.md: the scatter from row-major V is 1.0 - 1.7 x faster than from the
            # transposed store's V^T, and the fused product replaces two); Nq = Na queries, len = N keys
            ops.ln_affine(x, mod[li, 0, 1], mod[li, 0, 0], eps, out=ws.h, ab_rows=Na, ab_stride=6 * D)
            ops.gemm(ws.h, p.w_qkv, p.b_qkv, out=ws.qkv)
            ops.rmsnorm_rope_(ws.qkv[:, :D], p.nq1, cs, hd, eps, x2=ws.qkv[:, D : 2 * D], w2=p.nk1)
            ops.sparse_scatter_rows_(st.k[li], ws.qkv[:, D : 2 * D], ids, batch=B)
            ops.sparse_scatter_vt_(st.vt[li], ws.qkv[:, 2 * D :], ids, N, batch=B, src_rows=True)
            ops.attention_vt(ws.qkv[:, :D], st.k[li], st.vt[li], H, out=ws.att, batch=B)
            self._linear(ws, ws.att, p, "o1", x, epilogue=ops.EPI_GATE_RES, gate=gate_msa[li], res=x, gate_rows=grow)
            # 2. cross-attention and 3. feed-forward: row-local, the launches the dense step makes with Na rows per sample
            self._cross_queries(ws, x, ws.q2, p, ctx)
            self._cross_attention(ws, ws.q2, ctx, li, B)
            self._linear(ws, ws.att, p, "o2", x, epilogue=ops.EPI_GATE_RES, gate=None, res=x)
            self._ffn(ws, x, p, mod[li, 0, 4], mod[li, 0, 3], gate_ffn[li], Na, grow)
        # K18 on the active rows, then their cells of an output that is zero elsewhere
        self._head_rows(ws, x, mod_out, Na)
        out = torch.zeros((B, cfg.out_channels, T, Hh, Ww), dtype=torch.bfloat16, device=self.dev)
        for b in range(B):
            ops.sparse_unpatchify_(out[b], ws.head[rows[b]], ids)
        if not torch.cuda.is_current_stream_capturing():
            self._sparse_ran.add((st.B, Na, N))
        return out

    # -- the forward (transformer_chronoedit.py:397-476) ---------------------------------
    def forward(self, hidden: torch.Tensor, timestep: torch.Tensor, text: torch.Tensor, image: Optional[torch.Tensor]):
        """hidden [B,C,T,H,W], timestep [B], text [B,Tt,text_dim], image [B,Ti,image_dim] -> [B,Cout,T,H,W] (bf16).

        The B samples' tokens are stacked along the GEMM M axis (weights stream from HBM once for all of them —
        this is how the two classifier-free-guidance passes of pipeline_chronoedit.py:715-735 are batched);
        attention, RoPE and the AdaLN tables stay per sample."""
        cfg, D, H = self.cfg, self.D, self.H
        B, C, T, Hh, Ww = hidden.shape
        if C != cfg.in_channels:
            raise ValueError(f"expected {cfg.in_channels} input channels, got {C}")
        Hp, Wp = Hh // 2, Ww // 2
        N = T * Hp * Wp
        hd = cfg.attention_head_dim
        eps = cfg.eps
        cs = self._rope_table(T, Hp, Wp)  # raises AssertionError for unsupported frame counts (:205)
        # Sparse region edits (per-call mode, set by the denoising loop; None = off: the launch sequence below is exactly the plain forward's).
        # sparse: the forward on the active rows (_forward_sparse).  refresh: the plain forward, which also copies every layer's K (after norm +
        # RoPE) and V^T into the edit's cache - copies only, so its output is the plain forward's bit for bit.
        sparse = self.model._sparse_mode
        sparse_st = None
        if sparse is not None:
            if sparse not in ("refresh", "sparse"):
                raise ValueError(f"unknown sparse region mode {sparse!r}")
            if self.model._tea_mode is not None:
                raise ValueError("sparse region edits and TeaCache exclude each other")
            self.sparse_check(B, N)
            sparse_st = self._sparse_state(B, T, Hh, Ww)
            if text.shape[0] != B or (image is not None and image.shape[0] != B):
                raise ValueError("encoder_hidden_states / encoder_hidden_states_image batch size must match hidden_states")
            if sparse == "sparse":
                return self._forward_sparse(sparse_st, hidden, timestep, text, image)
        sp = self.model._sp
        if sp is not None and sp.sharded:
            if B != 1 and not self.v_transposed:
                raise ValueError("several samples per sequence-parallel forward need the V^T attention path (enable_transposed_v)")
            if self.fp8_attn and not getattr(self, "_warned_fp8_attn_sp", False):
                import warnings
                warnings.warn("enable_fp8_attention() has no effect while the tokens are sharded (Ulysses / CFG parallel): the exchange "
                              "carries bf16 q / k / v and the self-attention runs the bf16 V^T kernel; see attention_path()")
                self._warned_fp8_attn_sp = True
            align = 64 if B > 1 else 1  # B > 1: blocked receive layout, a key tile must not straddle two source ranks' blocks
            Nl = sp.shard(N, align)[0]  # local (zero-padded) token rows
            key = ("sp", T, Hp, Wp, sp.rank, sp.world, Nl)
            if key not in self._rope:
                self._rope[key] = sp.take_rows(cs, N, align).contiguous()
            cs = self._rope[key]
        else:
            sp = None
            Nl = N
        ws = self._workspace(B * Nl)
        hidden = hidden.to(torch.bfloat16).contiguous()
        rows = [slice(b * Nl, (b + 1) * Nl) for b in range(B)]

        # The guidance pair with shared inputs (model._shared_inputs, declared by the denoising loop): the image context is projected once
        # (share_img: every block's cross-attention reads one image segment), and everything in front of block 0's cross-attention - patch
        # embedding, modulation tables, block 0's self-attention half - runs on ONE sample's N rows (share), in `xs`.  xs borrows the head of
        # the FFN hidden buffer, which nothing uses before block 0's FFN: the out-projection of block 0's cross-attention reads it as the residual
        # of BOTH samples (row period N) while it writes the stacked stream ws.x - the fan-out, without a copy.  A skipped TeaCache step has
        # no block 0: it runs as before.
        if text.shape[0] != B or (image is not None and image.shape[0] != B):
            raise ValueError("encoder_hidden_states / encoder_hidden_states_image batch size must match hidden_states")
        share_img = sp is None and B == 2 and self._share_image(text, image)
        share = share_img and N % 8 == 0 and 2 * self.F >= D and self.model._tea_mode != "skip"
        xs = ws.ffn.view(-1)[: N * D].view(N, D) if share else None

        # K1
        if share:
            ops.patchify(hidden[0], self.kpatch, out=ws.cols[rows[0]])
            ops.gemm(ws.cols[rows[0]], self.w_patch, self.b_patch, out=xs)
        elif sp is None:
            for b in range(B):
                ops.patchify(hidden[b], self.kpatch, out=ws.cols[rows[b]])
        else:  # only this rank's token rows (zero rows past the last token: wan_video_new_chronoedit.py:1450-1453)
            for b in range(B):
                ops.patchify(hidden[b], self.kpatch, out=ws.cols[rows[b]], row0=sp.rank * Nl, nrows=Nl)
        if not share:
            ops.gemm(ws.cols, self.w_patch, self.b_patch, out=ws.x)

        # TeaCache (per-call mode, set by the denoising loop; None = off: the launch sequence below is exactly the plain forward's).  compute: the
        # tokens in front of the blocks are saved, and turned into the stack's residual behind them.  skip: that residual is added to
        # this step's tokens and the forward continues at the head (K18): no AdaLN block tables, no context, no block.
        tea = self.model._tea_mode
        if tea is not None:
            if tea not in ("compute", "skip", "measure"):
                raise ValueError(f"unknown TeaCache mode {tea!r}")
            if sp is not None:
                raise NotImplementedError("TeaCache with the tokens sharded over ranks is not implemented")
            if tea == "skip":
                if self._tea_res is None or self._tea_res.shape[0] != B * Nl or not self._tea_valid:
                    raise RuntimeError(f"TeaCache: a skipped step needs the residual of a computed step with the same {B * Nl} token rows")
                ops.tea_apply_(ws.x, self._tea_res)
            else:
                # measure: a computed step whose residual is also compared with the previous step's (below), in the other of two buffers
                tr, tea_prev = self._tea_measure_buffers(B * Nl) if tea == "measure" else (self.tea_reserve(B * Nl), None)
                if share:  # the residual buffer stays [2 N, D]: both samples' tokens in front of the blocks are xs
                    tr[rows[0]].copy_(xs)
                    tr[rows[1]].copy_(xs)
                else:
                    tr.copy_(ws.x)
        skip = tea == "skip"

        # K2; the shared pair has one timestep: one set of tables, stacked twice for the per-sample row strides of the launches behind the fan-out
        mods, mod, mod_out, gate_msa, gate_ffn = self._time_tables(timestep, 1 if share else B, B, blocks=not skip)
        x = ws.x
        if skip:
            return self._head(ws, x, mod_out, sp, B, T, Hh, Ww, N, Nl, rows)

        ctx = self._context(text, image, share_image=share_img)
        grow = Nl if B > 1 else 0

        for li, p in enumerate(self.blk):
            if share and li == 0:
                # block 0 up to its cross-attention on the one shared sample (the B = 1 launches on N rows), then the fan-out: queries shared,
                # text keys per sample, image keys shared, output per sample; the out-projection adds the shared residual to both
                self._block0_shared_prefix(ws, xs, p, mods[0], cs, N, ctx)
                if sparse_st is not None:  # refresh: the one shared sample's K / V^T are both samples'
                    for b in range(B):
                        sparse_st.k[0][rows[b]].copy_(ws.qkv[:N, D : 2 * D])
                        sparse_st.vt[0][:, b * N : (b + 1) * N].copy_(ws.vt[:, :N])
                self._cross_attention(ws, ws.q2[:N], ctx, li, B, share_q=True)
                self._linear(ws, ws.att, p, "o2", x, epilogue=ops.EPI_GATE_RES, gate=None, res=xs, res_rows=N)
                self._ffn(ws, x, p, mod[li, 0, 4], mod[li, 0, 3], gate_ffn[li], Nl, grow)
                continue
            q_o1 = False
            # 1. self-attention
            if sp is None and self.fp8_attn:  # MXFP8: the norm / RoPE pass and a V^T pass write the quantised operands
                self._ln_linear(ws, x, mod[li, 0, 1], mod[li, 0, 0], p, "qkv", ws.qkv, ab_rows=Nl, ab_stride=6 * D)
                ops.rmsnorm_rope_mxfp8(ws.qkv[:, :D], p.nq1, cs, hd, eps, out=ws.q8, scale=ws.sq, post_scale=ops.MXFP8_Q_SCALE)
                ops.rmsnorm_rope_mxfp8(ws.qkv[:, D : 2 * D], p.nk1, cs, hd, eps, out=ws.k8, scale=ws.sk)
                if ws.v8t is None or ws.v8t.shape[0] != B:
                    ws.v8t = ws.sv = None
                ws.v8t, ws.sv = ops.v_mxfp8_transpose(ws.qkv[:, 2 * D :], Nl, B, H, out=ws.v8t, scale=ws.sv)
                if self.fuse_o1:  # the out-projection's MX operand straight from the attention epilogue (no bf16 output, no quantisation pass)
                    ops.attention_mxfp8(ws.q8, ws.sq, ws.k8, ws.sk, ws.v8t, ws.sv, H, batch=B, out8=ws.a8[:, :D], scale8=ws.s8)
                    q_o1 = True
                else:
                    ops.attention_mxfp8(ws.q8, ws.sq, ws.k8, ws.sk, ws.v8t, ws.sv, H, out=ws.att, batch=B)
                att = ws.att
            elif sp is None and self.v_transposed and "qkv" not in self.fp8_set and (B * Nl) % 8 == 0 and (B == 1 or Nl % 2 == 0):
                keep = None if sparse_st is None else (sparse_st.k[li], sparse_st.vt[li])  # refresh
                att = self._self_attention_vt(ws, x, B * Nl, B, p, mod[li, 0, 1], mod[li, 0, 0], cs, keep)
            elif sp is None:  # all samples in one launch (stacked rows)
                self._ln_linear(ws, x, mod[li, 0, 1], mod[li, 0, 0], p, "qkv", ws.qkv, ab_rows=Nl, ab_stride=6 * D)
                ops.rmsnorm_rope_(ws.qkv[:, :D], p.nq1, cs, hd, eps, x2=ws.qkv[:, D : 2 * D], w2=p.nk1)  # q and k, all samples
                ops.attention(ws.qkv[:, :D], ws.qkv[:, D : 2 * D], ws.qkv[:, 2 * D :], H, out=ws.att, batch=B)
                att = ws.att
            else:
                att = self._self_attention_ulysses(ws, sp, x, mod[li, 0, 1], mod[li, 0, 0], p, cs, N, Nl, B)
            self._linear(ws, att, p, "o1", x, quantised=q_o1, epilogue=ops.EPI_GATE_RES, gate=gate_msa[li], res=x, gate_rows=grow)
            if self._tap is not None and li == 0 and not torch.cuda.is_current_stream_capturing():
                self._tap["x_pre_cross0"] = x.clone()
            # 2. cross-attention (text + image segments)
            self._cross_queries(ws, x, ws.q2, p, ctx)
            q_o2 = self._cross_attention(ws, ws.q2, ctx, li, B)
            self._linear(ws, ws.att, p, "o2", x, quantised=q_o2, epilogue=ops.EPI_GATE_RES, gate=None, res=x)
            # 3. feed-forward
            self._ffn(ws, x, p, mod[li, 0, 4], mod[li, 0, 3], gate_ffn[li], Nl, grow)

        if tea is not None:  # the saved tokens become the residual of this (computed) step
            if tea == "measure" and tea_prev is not None:
                ops.tea_store_dist_(x, self._tea_res, tea_prev, self._tea_sums[self._tea_row])
            else:
                ops.tea_store_(x, self._tea_res)
            self._tea_valid = True
        if sparse_st is not None:
            sparse_st.valid = True
        return self._head(ws, x, mod_out, sp, B, T, Hh, Ww, N, Nl, rows)

    def _block0_shared_prefix(self, ws, xs, p, mods0, cs, N: int, ctx):
        """Block 0 from its first LayerNorm to the normed cross-attention queries for ONE sample's N rows (the guidance pair's shared prefix):
        the launches a B = 1 forward makes, on the first N rows of the workspaces; xs [N, D] is updated in place, ws.q2[:N] receives the queries.
        V^T goes into sample 0's columns [0, N) of the stacked pair's buffer.  When N % 64 != 0 the kernel's last key strip also reads columns
        [N, pad64(N)): zeros after the first fill, sample 1's V^T of the previous stacked block from then on.  That is exactly what sample 0 of
        every stacked launch meets (ce_attention_vt_bf16: columns past a sample's keys are finite and meet P = 0), so the result is bit-equal
        to a B = 1 forward's, whose strip holds zeros - as long as those columns are finite, which zeros and projected values are."""
        att = self._self_attention_vt(ws, xs, N, 1, p, mods0[0, 1], mods0[0, 0], cs)
        self._linear(ws, att, p, "o1", xs, epilogue=ops.EPI_GATE_RES, gate=mods0[0, 2], res=xs)
        if self._tap is not None and not torch.cuda.is_current_stream_capturing():
            self._tap["x_pre_cross0"] = xs.clone()
        self._cross_queries(ws, xs, ws.q2[:N], p, ctx)

    # -- the launch groups of a block, each on the rows it is given -------------------------
    def _time_tables(self, timestep: torch.Tensor, n: int, B: int, blocks: bool = True):
        """K2 for the first n samples: sinusoid -> time_embedder (fp32) -> temb (bf16-rounded) -> silu -> time_proj -> AdaLN tables, stacked
        for B samples (n = B, or n = 1: one set of tables stacked B times).  Returns
          mods      per computed sample [L, 6, D]: shift, 1 + scale, gate, ... of every block;
          mod       [L, B, 6, D]: per-sample AdaLN rows (ab_rows / gate_rows = token rows per sample);
          mod_out   [B, 1, 2, D]: the head's shift, 1 + scale;
          gate_msa, gate_ffn   the gate rows of the two GEMM epilogues per layer: stacked [L, B, D], or for B = 1 the rows of mods[0].
        blocks=False (a skipped TeaCache step): mod_out only."""
        D = self.D
        # integer timesteps as in the diffusers pipeline; floating-point ones (sibling stacks) keep their fraction
        timestep = timestep.to(device=self.dev, dtype=torch.float32 if timestep.is_floating_point() else torch.int64).contiguous()
        mods, mods_out = [], []
        for b in range(n):
            sin = ops.timestep_sinusoid(timestep[b : b + 1], self.cfg.freq_dim)
            h1 = ops.gemv(self.te_w1, sin, self.te_b1, flags=2)
            temb = ops.gemv(self.te_w2, h1, self.te_b2, flags=4)
            if blocks:
                tproj = ops.gemv(self.tp_w, temb, self.tp_b, flags=1 | 4)  # [6*D]
                mods.append(ops.modulation(self.tables, tproj.view(6, D), one_mask=0b010010))
            mods_out.append(ops.modulation(self.table_out, temb.view(1, D), one_mask=0b10))
        if n != B:
            mods, mods_out = mods * B, mods_out * B
        mod = torch.stack(mods, dim=1).contiguous() if blocks else None
        mod_out = torch.stack(mods_out, dim=0).contiguous()
        if not blocks:
            return mods, mod, mod_out, None, None
        if B > 1:
            return mods, mod, mod_out, mod[:, :, 2].contiguous(), mod[:, :, 5].contiguous()
        return mods, mod, mod_out, mods[0][:, 2], mods[0][:, 5]

    def _self_attention_vt(self, ws, x, n: int, batch: int, p, a_row, b_row, cs, keep=None):
        """The bf16 V^T self-attention of the first n rows of the workspace (`batch` samples of n / batch rows): LayerNorm with the AdaLN rows,
        q | k as one GEMM, V^T = (h.W_v^T)^T by a GEMM whose epilogue stores the transpose - the attention kernel's V^T operand [D][keys of
        all samples] without a transpose pass; K and V^T tiles both go by LDS-DMA.  keep = (k, vt): the normed K and V^T are also copied
        there (a refresh step's cache).  Returns the attention output rows."""
        D, hd, eps = self.D, self.cfg.attention_head_dim, self.cfg.eps
        h, qkv, att = ws.h[:n], ws.qkv[:n], ws.att[:n]
        if getattr(ws, "vt", None) is None:  # (all rows of the workspace, whichever range comes first)
            ws.vt = torch.zeros((D, ops.vt_columns(ws.x.shape[0])), dtype=torch.bfloat16, device=self.dev)  # padding columns stay zero
        ops.ln_affine(x, a_row, b_row, eps, out=h, ab_rows=n // batch, ab_stride=6 * D)
        ops.gemm(h, p.w_qkv[: 2 * D], p.b_qkv[: 2 * D], out=qkv[:, : 2 * D])
        ops.gemm(h, p.w_qkv[2 * D :], p.b_qkv[2 * D :], out=ws.vt[:, :n], epilogue=ops.EPI_BIAS_T)
        ops.rmsnorm_rope_(qkv[:, :D], p.nq1, cs, hd, eps, x2=qkv[:, D : 2 * D], w2=p.nk1)
        if keep is not None:
            keep[0].copy_(qkv[:, D : 2 * D])
            keep[1][:, :n].copy_(ws.vt[:, :n])
        ops.attention_vt(qkv[:, :D], qkv[:, D : 2 * D], ws.vt, self.H, out=att, batch=batch)
        return att

    def _cross_queries(self, ws, x, q2, p, ctx):
        """The cross-attention queries of the rows of x into q2: norm2 (where the model has one), the projection, the RMS norm - for an
        MXFP8 context into the quantised ws.q8 / ws.sq instead of in place."""
        hd, eps = self.cfg.attention_head_dim, self.cfg.eps
        if p.n2w is not None:
            self._ln_linear(ws, x, p.n2w, p.n2b, p, "q2", q2)
        else:
            self._linear(ws, x, p, "q2", q2)
        if ctx.f8:
            ops.rmsnorm_rope_mxfp8(q2, p.nq2, None, hd, eps, out=ws.q8, scale=ws.sq, post_scale=ops.MXFP8_Q_SCALE)
        else:
            ops.rmsnorm_rope_(q2, p.nq2, None, hd, eps)

    def _cross_attention(self, ws, q, ctx, li: int, batch: int, share_q: bool = False) -> bool:
        """Layer li's cross-attention (text + image segments) of the queries q into ws.att, by the kernel the context's form asks for.
        share_q: q holds ONE sample's queries for all `batch` samples.  Returns whether the output is the out-projection's MX operand in
        ws.a8 / ws.s8 (the fused quantisation of the fp8 mode) instead of bf16 rows in ws.att."""
        D, H, Tt, Ti, fuse = self.D, self.H, ctx.Tt, ctx.Ti, self.fuse_o2
        if ctx.f8:  # MXFP8 (round 5): text segment -> bf16, image segment adds it and emits bf16 or the out-projection's MX operand
            seg_t, seg_i = ctx.kv[li]
            if seg_i is None and fuse:
                ops.attention_mxfp8(ws.q8, ws.sq, *seg_t, H, batch=batch, out8=ws.a8[:, :D], scale8=ws.s8)
            else:
                ops.attention_mxfp8(ws.q8, ws.sq, *seg_t, H, out=ws.att, batch=batch)
                if seg_i is not None and fuse:
                    ops.attention_mxfp8(ws.q8, ws.sq, *seg_i, H, batch=batch, out8=ws.a8[:, :D], scale8=ws.s8, add=ws.att)
                elif seg_i is not None:
                    ops.attention_mxfp8(ws.q8, ws.sq, *seg_i, H, out=ws.att, batch=batch, add=ws.att)
            return fuse
        k_t, v_t, k_i, v_i = ctx.kv[li]
        if ctx.valid is not None:  # compacted text: per-sample valid keys, the padding as one weighted key
            ops.attention_2seg_vt_weighted(q, k_t, v_t, Tt, k_i, v_i, Ti, H, out=ws.att, batch=batch, valid1=ctx.valid, w1=ctx.w,
                                           share_q=share_q, share2=ctx.img_shared, cols1=ctx.c1, cols2=None if ctx.img_shared else ctx.c2)
        elif ctx.vt and fuse:
            ops.attention_2seg_vt(q, k_t, v_t, Tt, k_i, v_i, Ti, H, batch=batch, cols1=ctx.c1, cols2=ctx.c2, out8=ws.a8[:, :D], scale8=ws.s8)
            return True
        elif ctx.img_shared:  # one image segment for all samples
            ops.attention_2seg_vt_shared(q, k_t, v_t, Tt, k_i, v_i, Ti, H, out=ws.att, batch=batch, share_q=share_q, share2=True, cols1=ctx.c1)
        elif ctx.vt:  # both segments' K and V^T tiles by LDS-DMA (v_t / v_i are V^T row blocks of this layer)
            ops.attention_2seg_vt(q, k_t, v_t, Tt, k_i, v_i, Ti, H, out=ws.att, batch=batch, cols1=ctx.c1, cols2=ctx.c2)
        elif k_i is not None:
            ops.attention(q, k_t, v_t, H, out=ws.att, k2=k_i, v2=v_i, batch=batch)
        else:
            ops.attention(q, k_t, v_t, H, out=ws.att, batch=batch)
        return False

    def _ffn(self, ws, x, p, a_row, b_row, gate, ab_rows: int, gate_rows: int):
        """The feed-forward of the rows of x, in place: LayerNorm with the AdaLN rows, up-projection + GELU, gated down-projection + residual."""
        D, eps = self.D, self.cfg.eps
        if self.mx and self.fuse_quant and "f1" in self.fp8_set and "f2" in self.fp8_set:
            # MX: the up-projection's bias + GELU epilogue emits the down-projection's fp8 operand and its block scales directly (a
            # block = 32 consecutive output columns: no row-wide reduction) - no bf16 [N, F] matrix, no quantisation pass
            aq = ws.a8[:, :D]
            ops.ln_affine_mxfp8(x, a_row, b_row, eps, out=aq, scale=ws.s8, ab_rows=ab_rows, ab_stride=6 * D)
            ops.gemm_mxfp8_gelu_quant(aq, ws.s8, *p.q_f1, p.b_f1, out=ws.a8b, scale=ws.s8b)
            ops.gemm_mxfp8(ws.a8b, ws.s8b, *p.q_f2, p.b_f2, out=x, epilogue=ops.EPI_GATE_RES, gate=gate, res=x, gate_rows=gate_rows)
        else:
            self._ln_linear(ws, x, a_row, b_row, p, "f1", ws.ffn, ab_rows=ab_rows, ab_stride=6 * D, epilogue=ops.EPI_BIAS_GELU)
            self._linear(ws, ws.ffn, p, "f2", x, epilogue=ops.EPI_GATE_RES, gate=gate, res=x, gate_rows=gate_rows)

    def _head_rows(self, ws, x, mod_out, ab_rows: int):
        """K18 on the rows of x: the head's LayerNorm with its AdaLN rows and the output projection, into ws.head."""
        ops.ln_affine(x, mod_out[0, 0, 1], mod_out[0, 0, 0], self.cfg.eps, out=ws.h, ab_rows=ab_rows, ab_stride=2 * self.D)
        ops.gemm(ws.h, self.w_out, self.b_out, out=ws.head)

    def _head(self, ws, x, mod_out, sp, B, T, Hh, Ww, N, Nl, rows):
        cfg = self.cfg
        self._head_rows(ws, x, mod_out, Nl)
        out = torch.empty((B, cfg.out_channels, T, Hh, Ww), dtype=torch.bfloat16, device=self.dev)
        if sp is None:
            for b in range(B):
                ops.unpatchify(ws.head[rows[b]], cfg.out_channels, T, Hh, Ww, out=out[b])
        else:
            full = sp.all_gather_rows(ws.head).view(sp.world, B, Nl, -1)  # [source rank][sample][local token]
            for b in range(B):
                ops.unpatchify(full[:, b].reshape(sp.world * Nl, -1)[:N].contiguous(), cfg.out_channels, T, Hh, Ww, out=out[b])
        return out
