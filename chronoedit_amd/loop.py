"""Denoising loop of ChronoEditPipeline.__call__ on the HIP engine
(chronoedit_diffusers/pipeline_chronoedit.py:694-756).

`denoise_step` is one loop iteration — the unit BASELINE.json's "denoising-steps/sec" counts:
cat(latents, condition) -> 1 or 2 DiT forwards -> CFG -> scheduler update.  The latents stay fp32
on the device for the whole trajectory; the CFG combine and the UniPC update are one fused launch.

A step has a KIND (`step_kinds`): `_run_step` is the one place that turns a kind into forwards and a `step_cfg` call, `_step_modes` the one
place that sets the engine's per-forward mode flags for it; `denoise_step` (eager) and `GraphedDenoiser` (captured) both go through them.
What a feature of the loop keeps per edit lives in a state object next to the feature's code (guidance.GuidanceState,
teacache.TeaCacheState, sparse_region.SparseRegionState, auto_region.AutoRegionState, region.RegionState, preview.PreviewDelivery,
tiles.TileState);
`denoise` calls their moments in order.  `chronoedit_amd.pipeline` re-exports every name here.
"""
from __future__ import annotations

import contextlib
import math
from types import SimpleNamespace
from typing import Optional, Sequence

import torch

from . import auto_region as _ar, guidance as _gd, region as _rg, sparse_region as _sr, teacache as _tea
from .scheduler import FlowUniPCMultistepScheduler
from .transformer import ChronoEditTransformer3DModel

_INT_OF_SIZE = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def text_real_lengths(text: torch.Tensor) -> torch.Tensor:
    """text [B, Tt, C] -> int64 [B] (on text's device): per sample, the rows in front of its padding = Tt minus the length of the trailing run
    of rows that equal the LAST row bit for bit (compared as integers: no tolerance, -0 != +0, a NaN equals itself).  The reference
    re-pads every prompt with zero rows (pipeline_chronoedit.py:230-237); any constant padding row is found the same way.  A last row that is
    unlike its predecessor is a run of one: the sample has no padding to speak of."""
    B, Tt = text.shape[0], text.shape[1]
    bits = text.contiguous().view(_INT_OF_SIZE[text.element_size()]).reshape(B, Tt, -1)
    differs = (bits != bits[:, -1:, :]).any(-1)  # [B, Tt]; False at the last row
    idx = torch.arange(1, Tt + 1, device=text.device).expand(B, Tt)
    return torch.where(differs, idx, torch.zeros_like(idx)).amax(1)  # one past the last row that differs from the last row


def text_compaction_plan(real: Sequence[int], Tt: int):
    """real = rows in front of the padding per sample -> (Lc, valid, log2 weights) or None when nothing is saved.  Sample b keeps its real
    rows and ONE padding row that stands for all Tt - real[b] of them (valid = real + 1, weight log2(Tt - real)); a sample whose trailing
    run is a single row keeps everything (valid = Tt, weight 0).  Lc = the largest valid count rounded up to 8 (the transposed-V projection
    wants its columns in multiples of 8 with even per-sample strides).  None unless every sample walks at least one 64-key tile less."""
    valid = [min(int(n) + 1, Tt) for n in real]
    Lc = (max(valid) + 7) // 8 * 8
    if Lc > Tt or (max(valid) + 63) // 64 >= (Tt + 63) // 64:
        return None
    return Lc, valid, [math.log2(Tt - v + 1) for v in valid]


def compact_text_context(text: torch.Tensor):
    """Find the padding of a text context [B, Tt, C] (one device-to-host read) and hang the compacted form on the tensor as
    `text._ce_compact`: rows [0, Lc) of every sample (its real rows, the representative padding row, then rows the kernel masks), the valid
    counts (int32) and log2 weights (fp32) on the device, and the tensor version they were taken at.  The engine picks it up when the SAME
    tensor object reaches a forward (chronoedit_amd/transformer.py `_context`); a tensor without the attribute is never compacted.  Returns text.
    A tensor already examined at its version costs nothing, and that is all a captured step may ask for: the read cannot be captured, so a
    miss while the stream is capturing is a RuntimeError (GraphedDenoiser examines its contexts in its constructor)."""
    if getattr(text, "_ce_compact", None) is not None and text._ce_compact.version == text._version:
        return text
    if text.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("compact_text_context: a text context that has not been examined reached a step under capture")
    info = SimpleNamespace(version=text._version, shape=tuple(text.shape), text=None, valid=None, w=None, Lc=0, real=None)
    if text.dim() == 3 and text.shape[1] > 1 and text.is_floating_point():
        Tt = text.shape[1]
        info.real = [int(n) for n in text_real_lengths(text).tolist()]
        plan = text_compaction_plan(info.real, Tt)
        if plan is not None:
            info.Lc, valid, w = plan
            info.text = text[:, : info.Lc].contiguous()
            info.valid = torch.tensor(valid, dtype=torch.int32, device=text.device)
            info.w = torch.tensor(w, dtype=torch.float32, device=text.device)
    text._ce_compact = info
    return text


def make_cfg_inputs(prompt_embeds, negative_prompt_embeds, image_embeds):
    """[cond | uncond] conditioning stacked along the batch axis; build it ONCE per edit so that the transformer's
    context cache (step-invariant text/image K/V) can recognise the tensors across steps.  The text padding is found here, once
    (`compact_text_context`): the stacked text tensor carries its compacted form to the engine."""
    text2 = compact_text_context(torch.cat([prompt_embeds, negative_prompt_embeds], 0))
    image2 = None if image_embeds is None else torch.cat([image_embeds, image_embeds], 0)
    return text2, image2


@contextlib.contextmanager
def _shared_inputs(transformer):
    """Declare, for the forwards inside, that the two halves of the batch carry the same latents, timestep and image embedding and differ in the
    text context only - what `make_cfg_inputs` and the loops below build.  The engine then runs the pair's common work once
    (ChronoEditTransformer3DModel.enable_shared_guidance); a transformer without the attribute is left alone.  Cleared on the way out: a
    forward from anywhere else never shares."""
    if not hasattr(transformer, "_shared_inputs"):
        yield
        return
    transformer._shared_inputs = True
    try:
        yield
    finally:
        transformer._shared_inputs = None


def _token_sharded(transformer) -> bool:
    sp = getattr(transformer, "_sp", None)
    return sp is not None and sp.sharded


def refuse_sharded(transformer, wording: str):
    """The refusal every feature of the loop that has only been built for replicated, unsharded work shares: NotImplementedError with the
    feature's `wording`, whose {} is where the sharding is named."""
    if getattr(transformer, "_cfgp", None) is not None or _token_sharded(transformer):
        raise NotImplementedError(wording.format("the tokens sharded over ranks or with CFG parallelism"))


def _capturable(transformer) -> bool:
    """Can a step of this transformer be captured into a hipGraph?  Unsharded: yes.  Token-sharded: only when the exchanges run on the
    library-owned RCCL communicator (`enable_sequence_parallel(owned_comm=True)`, parallel.OwnedComm); CFG parallelism (its pairwise
    exchange is a torch.distributed collective) runs eagerly."""
    if getattr(transformer, "_cfgp", None) is not None:
        return False
    if not _token_sharded(transformer):
        return True
    return bool(getattr(transformer._sp, "capturable", False))


def _sharded_batchable(transformer) -> bool:
    """Can a token-sharded (Ulysses) forward take the guidance pair as ONE batch of two?  Yes on the V^T attention path (the
    blocked-layout kernels, chronoedit_amd/parallel.py) - with bf16 or fp8 GEMMs; the sharded self-attention itself is always the
    bf16 kernel (transformer.attention_path()).  The register-staged attention kernel runs the passes in sequence."""
    return bool(getattr(transformer, "v_transposed", False) and getattr(transformer, "sp_batch_cfg", True))


# ---------------------------------------------------------------------------------------------------------------
# One step: its kind, the mode flags of its forwards, the forwards and the scheduler update
# ---------------------------------------------------------------------------------------------------------------
def step_kinds(n_steps: int, tea_plan=None, guidance_plan=None, sparse_plan=None, measure: bool = False) -> list:
    """The kind of every step of an edit - the one list the eager loop and GraphedDenoiser index.  The plans exclude each other: with
    guidance reuse the plan itself ("pair" / "reuse" / "off"), with a sparse region the plan itself ("compute" / "refresh" / "sparse"), with
    TeaCache "compute" / "skip" (measuring: "measure" throughout), otherwise "compute"."""
    if guidance_plan is not None:
        return [str(k) for k in guidance_plan]
    if sparse_plan is not None:
        return [str(k) for k in sparse_plan]
    if tea_plan is not None:
        return ["compute" if c else "skip" for c in tea_plan]
    return ["measure" if measure else "compute"] * int(n_steps)


@contextlib.contextmanager
def _step_modes(transformer, kind: Optional[str], tea: bool = False, row: Optional[int] = None):
    """The engine's per-forward mode flags for a step of this kind, for the forwards inside: `_sparse_mode` for "refresh" / "sparse",
    `_tea_mode` for "skip" / "measure" and - `tea`: the edit has a TeaCache plan - for "compute"; measuring, `row` is the row of the sums
    table this step's forward writes (`engine()._tea_row`).  Back to None on the way out, exceptions included: a forward outside the loop
    runs the whole model.  A step that needs no flag touches none."""
    tea_mode = kind if kind in ("skip", "measure") or (tea and kind == "compute") else None
    sparse_mode = kind if kind in ("refresh", "sparse") else None
    if row is not None:
        transformer.engine()._tea_row = row
    if tea_mode is not None:
        transformer._tea_mode = tea_mode
    if sparse_mode is not None:
        transformer._sparse_mode = sparse_mode
    try:
        yield
    finally:
        if tea_mode is not None:
            transformer._tea_mode = None
        if sparse_mode is not None:
            transformer._sparse_mode = None


def _run_step(transformer, scheduler, latents, condition, timestep, prompt_embeds, negative_prompt_embeds, image_embeds, cfg_inputs,
              guidance_scale: float, batch_cfg: bool, kind: Optional[str] = None, delta=None, delta_measure=None, coef=None, cfgp=None):
    """One step of kind `kind`, eager or under capture: the forwards it runs and the `step_cfg` call that follows.  timestep: a 0-d tensor
    (the loop's `t`, or the graph's staging buffer); coef: an explicit coefficient row (the graph's staging buffer; None: the scheduler's
    own row of this step); cfgp: the transformer's CFG-parallel group (eager only).
    "reuse" and "off", and every kind of an unguided edit, run the conditional sample alone; every other kind (None, "compute", "skip",
    "measure", "pair", "refresh", "sparse") runs the guidance pair - exchanged between ranks (cfgp), as one stacked forward under
    `_shared_inputs` (batch_cfg), or as two passes.  "pair" stores the guidance direction in `delta` (delta_measure = (slot, table, row): into
    that slot of a ring, with the distance sums), "reuse" guides with it; the others are the plain update."""
    latent_model_input = torch.cat([latents.to(torch.bfloat16), condition], dim=1)
    B = latents.shape[0]
    timestep = timestep.expand(B)
    if guidance_scale > 1.0 and negative_prompt_embeds is not None and kind not in ("reuse", "off"):  # do_classifier_free_guidance
        if cfgp is not None:
            # CFG parallelism: this rank's Ulysses group runs ONE of the two passes, the predictions are exchanged pairwise
            text = prompt_embeds if cfgp.branch == 0 else negative_prompt_embeds
            mine = transformer(latent_model_input, timestep, text, image_embeds, return_dict=False)[0]
            noise_pred, noise_uncond = cfgp.exchange(mine)
        elif batch_cfg:
            # the conditional and unconditional passes (pipeline_chronoedit.py:715-735) as ONE forward over 2B samples:
            # identical per-sample arithmetic, but every weight streams from HBM once and the GEMM grids fill the chip
            text2, image2 = cfg_inputs if cfg_inputs is not None else make_cfg_inputs(prompt_embeds, negative_prompt_embeds, image_embeds)
            with _shared_inputs(transformer):  # both halves of the batch: the same latents, timestep and image embedding (built right here)
                out = transformer(torch.cat([latent_model_input, latent_model_input], 0), torch.cat([timestep, timestep], 0),
                                  text2, image2, return_dict=False)[0]
            noise_pred, noise_uncond = out[:B].contiguous(), out[B:].contiguous()
        else:
            noise_pred = transformer(latent_model_input, timestep, prompt_embeds, image_embeds, return_dict=False)[0]
            noise_uncond = transformer(latent_model_input, timestep, negative_prompt_embeds, image_embeds, return_dict=False)[0]
    else:
        compact_text_context(prompt_embeds)  # (examined once per tensor version: later steps, and every captured one, find the attribute)
        noise_pred = transformer(latent_model_input, timestep, prompt_embeds, image_embeds, return_dict=False)[0]
        noise_uncond = None
    extra = {} if coef is None else {"coef": coef}
    if kind in ("pair", "reuse"):
        mode = "reuse" if kind == "reuse" else "store" if delta_measure is None else "measure"
        return scheduler.step_cfg(noise_pred, noise_uncond, guidance_scale, latents, delta=delta, delta_mode=mode, delta_measure=delta_measure, **extra)
    return scheduler.step_cfg(noise_pred, noise_uncond, guidance_scale, latents, **extra)


@torch.no_grad()
def denoise_step(transformer: ChronoEditTransformer3DModel, scheduler: FlowUniPCMultistepScheduler, latents: torch.Tensor,
                 condition: torch.Tensor, t: torch.Tensor, prompt_embeds: torch.Tensor,
                 negative_prompt_embeds: Optional[torch.Tensor], image_embeds: Optional[torch.Tensor],
                 guidance_scale: float, batch_cfg: bool = True, cfg_inputs=None, guidance_kind: Optional[str] = None,
                 delta: Optional[torch.Tensor] = None, delta_measure=None) -> torch.Tensor:
    """latents fp32 [B,16,T,h,w] (updated in place), condition bf16 [B,20,T,h,w]  (pipeline_chronoedit.py:711-739).
    guidance_kind (guidance reuse, chronoedit_amd/guidance.py; needs the bf16 `delta` buffer of the latents' shape): "pair" = the guided
    step as ever, which also stores the guidance direction in `delta` (delta_measure = (slot, table, row): into that slot of a ring, with
    the distance sums); "reuse" = the conditional sample alone, guided by the stored direction; "off" = the conditional sample alone,
    unguided.  None: the plain step.  The eager caller of `_run_step`."""
    if guidance_kind not in (None, "pair", "reuse", "off"):
        raise ValueError(f"denoise_step: guidance_kind {guidance_kind!r} is none of 'pair', 'reuse', 'off'")
    if guidance_kind in ("pair", "reuse") and (delta is None or not (guidance_scale > 1.0 and negative_prompt_embeds is not None)):
        raise ValueError(f"denoise_step: a {guidance_kind!r} step needs a guided edit and its delta buffer")
    batch_cfg = batch_cfg and (not _token_sharded(transformer) or _sharded_batchable(transformer))
    return _run_step(transformer, scheduler, latents, condition, t, prompt_embeds, negative_prompt_embeds, image_embeds, cfg_inputs,
                     guidance_scale, batch_cfg, guidance_kind, delta=delta, delta_measure=delta_measure, cfgp=getattr(transformer, "_cfgp", None))


_WARMUP_STREAMS = {}


def _warmup_stream(dev: torch.device) -> "torch.cuda.Stream":
    """The side stream the un-captured step in front of a capture runs on - one per device for the life of the process (a fresh stream per
    GraphedDenoiser left a 64 MiB split-K scratch registered for each of them: ADVICE r4)."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _WARMUP_STREAMS.get(key)
    if st is None:
        st = _WARMUP_STREAMS[key] = torch.cuda.Stream(device=dev)
    return st


class GraphedDenoiser:
    """One denoising step captured as a hipGraph and replayed per step (north star: "the 50-step / 8-step sampling loops
    are hipGraph-captured").  Everything a step reads lives at fixed device addresses: the fp32 latents (updated in place),
    the condition, the stacked CFG conditioning, the scheduler history, and two small staging buffers that receive the
    step's timestep and UniPC coefficient row (device-to-device copies enqueued in front of the replay - no host sync).
    A new graph is needed when the latent shape changes (temporal-reasoning truncation 8 -> 2 frames).
    `step(i)` raises RuntimeError when the object was built at one step index with keep_warmup_step=True (that step ran eagerly in the
    constructor) and the first `step()` asks for another index: build it at the index it starts from.  Between construction and the last
    `step()` the transformer's modes (fp8, sequence parallelism, cache_context) must not change; other forwards of the same transformer
    are allowed (the lazy capture re-primes its context entry).
    With a TeaCache plan (`tea_plan`, chronoedit_amd/teacache.py: one bool per step of the schedule, True = compute) the computed steps replay
    one graph and the skipped steps a second one, captured lazily at the first skipped step; both address the engine's one residual buffer.
    With a guidance-reuse plan (`guidance_plan`, chronoedit_amd/guidance.py: "pair" / "reuse" / "off" per step, and the loop's `delta` buffer)
    there is one graph per kind of step the plan contains, each captured lazily at the first step of its kind that is replayed; all of them
    address the same latents, scheduler history, staging buffers and delta buffer.  "reuse" and "off" run ONE sample where "pair" runs two: the
    first step of either form on an engine that has not run it yet (`is_warm`) runs eagerly, for real, before that form is captured.
    With a sparse-region plan (`sparse_plan`, chronoedit_amd/sparse_region.py: "compute" / "refresh" / "sparse" per step; the engine's
    `sparse_begin` has been called for this edit) there is likewise one graph per kind, captured lazily; all address the engine's one K / V^T
    cache.  The first sparse step on an engine that has not run a sparse step of this geometry (`sparse_is_warm`) runs eagerly.
    Whichever plan is given is folded into `kinds` (`step_kinds`): the kind of step i is `kinds[i]`, and one graph is kept per kind."""

    def __init__(self, transformer, scheduler, latents, condition, prompt_embeds, negative_prompt_embeds, image_embeds,
                 guidance_scale: float, batch_cfg: bool = True, warm: bool = False, keep_warmup_step: bool = True, tea_plan=None,
                 guidance_plan=None, delta: Optional[torch.Tensor] = None, region=None, sparse_plan=None, tiles=None):
        """warm: this process has already run a step of exactly this shape / guidance form through `transformer` (packed weights,
        workspaces, kernel attributes exist), so no un-captured step is needed in front of the capture; only the step-invariant context
        projections are computed eagerly so that the graph holds the cache HIT (`cache_context`), not the projections.
        Not warm: the un-captured step that triggers the lazy initialisations IS the trajectory's current step (it runs eagerly on the
        live state, `step()` then skips the replay for that index) - a discarded warm-up cost a whole step per new shape: 2 s of a
        temporal-reasoning edit at 28 800 tokens, 12 % of an 8-step edit.  keep_warmup_step=False: run it on saved state and put the
        state back (a caller that wants every `step()` to be a replay: bench.py).
        region: the edit's region.RegionState, or None.  Every kind of step then ends with the region blend, inside its graph; the blend
        reads its sigma from the state's staging float, which `_stage` fills next to the coefficient row.
        tiles: the edit's tiles.TileState, or None.  The latents' samples are then the tiles of one canvas, and every kind of step ends with the
        fusion (two launches), inside its graph."""
        assert latents.dtype == torch.float32 and latents.is_contiguous()
        if not _capturable(transformer):
            # Measured on this stack (ROCm 7.0 / RCCL 2.26 / torch 2.10: tools/rccl_graph_probe.py, profiles/r03_rccl_graph_probe.txt): ONE
            # collective of torch.distributed's "nccl" backend can be captured and replayed, but the process-group watchdog thread keeps
            # polling the event of every Work created under capture - the next capture (or any later poll) kills the process
            # (hipErrorStreamCaptureUnsupported in "global" capture mode, a segmentation fault in "thread_local" / "relaxed"), with
            # synchronous collectives, async_op=True and side-stream fork / join alike.  A sharded loop needs two graphs (8 -> 2 frames), so it
            # runs eagerly on torch's communicator; DESIGN.md section 6 has the measurement of why that costs nothing at the per-rank kernel
            # times of 4 / 8 GPUs.  The way to capture it: the library-owned communicator (`enable_sequence_parallel(owned_comm=True)`).
            raise NotImplementedError("hipGraph capture of a step with torch.distributed exchanges is not usable on this torch / RCCL build: "
                                      "enable_sequence_parallel(owned_comm=True) or run the sharded loop eagerly")
        self.tr, self.sch, self.latents, self.condition = transformer, scheduler, latents, condition
        self.region, self.tiles = region, tiles
        self._ran_eagerly = set()  # sample counts (1: the single sample, 2: the stacked pair) this object has run an eager step of
        self.prompt, self.negative, self.image, self.g, self.batch_cfg = prompt_embeds, negative_prompt_embeds, image_embeds, guidance_scale, batch_cfg
        dev = latents.device
        self.cfg_inputs = None
        self.guided = guidance_scale > 1.0 and negative_prompt_embeds is not None
        # every text context a step of this object will look at is examined here, not under the capture (it reads the lengths back)
        if self.guided and batch_cfg:
            self.cfg_inputs = make_cfg_inputs(prompt_embeds, negative_prompt_embeds, image_embeds)
        elif not self.guided:
            compact_text_context(prompt_embeds)
        self.guidance_plan = None if guidance_plan is None or not self.guided else [str(k) for k in guidance_plan]
        self.delta = delta
        if self.guidance_plan is not None:
            if tea_plan is not None:
                raise ValueError("guidance reuse and TeaCache exclude each other")
            if delta is None or delta.shape != latents.shape or delta.dtype != torch.bfloat16 or not delta.is_contiguous():
                raise ValueError("guidance reuse: the delta buffer must be a contiguous bf16 tensor of the latents' shape")
            if any(k != "pair" for k in self.guidance_plan):
                compact_text_context(prompt_embeds)  # the single-sample steps' context
        self.tea_plan = None if tea_plan is None else [bool(c) for c in tea_plan]
        self.sparse_plan = None if sparse_plan is None else [str(k) for k in sparse_plan]
        if self.sparse_plan is not None:
            if tea_plan is not None or self.guidance_plan is not None:
                raise ValueError("a sparse region plan excludes TeaCache and guidance reuse")
            if region is None:
                raise ValueError("a sparse region plan needs the edit's region")
        if self.tea_plan is not None and self.guided and self.cfg_inputs is None:
            raise NotImplementedError("TeaCache needs the guidance pair as ONE batched forward (one residual buffer covers both samples)")
        self.kinds = step_kinds(len(scheduler.timesteps), self.tea_plan, self.guidance_plan, self.sparse_plan)
        self.t_buf = torch.zeros((), dtype=torch.int64, device=dev)
        self.coef_buf = torch.zeros(10, dtype=torch.float32, device=dev)
        scheduler._ensure_state(latents)
        if scheduler.last_sample is None:
            scheduler.last_sample = torch.zeros_like(latents)
        idx0 = scheduler._step_index
        self._stage(idx0 or 0)
        kind0 = self._kind(idx0 or 0)
        self._caller_warm = bool(warm)
        warm = self._form_warm(kind0)
        self._done_index = None  # the step that already ran eagerly (below); step() does not replay it
        if not warm:
            # lazy initialisations (packed weights, workspaces, function attributes) must not happen under capture: run the CURRENT step
            # eagerly, for real, on a side stream as torch asks of anything that precedes a capture
            saved = None if keep_warmup_step else (latents.clone(), [m.clone() for m in scheduler.model_outputs], scheduler.last_sample.clone())
            self._eager_body(kind0)
            if keep_warmup_step:
                self._done_index = idx0 or 0
            else:
                self.latents.copy_(saved[0])
                for m, sv in zip(scheduler.model_outputs, saved[1]):
                    m.copy_(sv)
                scheduler.last_sample.copy_(saved[2])
        else:
            self._prime_context(kind0)
        # The capture: at once when every step() must be a replay (warm shape, or keep_warmup_step=False); LAZILY - at the first step() that needs a
        # replay - when the constructor already ran the trajectory's current step eagerly: if that was the last step of this shape (truncation lands
        # there, or a callback replaces the latents every step) nothing is ever replayed and a whole capture would be thrown away
        self.graphs = {}  # kind of step -> captured graph
        if self._done_index is None:
            self._capture(kind0)
        scheduler._step_index = idx0  # step_cfg counts on the host, also while being captured

    @property
    def graph(self):
        """The step that runs the whole model on the edit's usual form (with TeaCache: the computed steps; with guidance reuse: "pair")."""
        return self.graphs.get("compute", self.graphs.get("pair"))

    @property
    def skip_graph(self):
        """TeaCache: the skipped steps."""
        return self.graphs.get("skip")

    def _single(self, kind: str) -> bool:
        """Does a step of this kind run the conditional sample alone?"""
        return not self.guided or kind in ("reuse", "off")

    def _n_samples(self, kind: str) -> int:
        return self.latents.shape[0] * (2 if self.cfg_inputs is not None and not self._single(kind) else 1)

    def _form(self, kind: str):
        """What an eager step of this kind warms: the sample count of a dense forward, or the sparse forward."""
        return "sparse" if kind == "sparse" else self._n_samples(kind)

    def _form_warm(self, kind: str) -> bool:
        """May a step of this kind be captured without an eager step of its form in front?  Yes when this object already ran one, or when the
        caller vouches for the edit's shape (`warm`) and the engine holds the workspace of exactly this sample count.  A sparse step: when
        the engine has run one of this edit's geometry."""
        n = self._form(kind)
        if n in self._ran_eagerly:
            return True
        eng = getattr(self.tr, "_engine", None)
        if kind == "sparse":
            return bool(eng is not None and eng.sparse_is_warm())
        return bool(self._caller_warm and eng is not None and hasattr(eng, "is_warm") and eng.is_warm(n, *self.latents.shape[2:]))

    def _prime_context(self, kind: str = "compute"):
        """With `cache_context`: the step-invariant context projections of THIS conditioning, in the form a step of this kind looks up,
        computed eagerly now, so that the capture records the cache hit and not the projections."""
        tr = self.tr
        if hasattr(tr, "prime_context"):  # (without `cache_context` it only reserves the buffers of a compacted text context)
            if self._single(kind):
                if not self.guided or self.guidance_plan is not None:
                    tr.prime_context(self.prompt, self.image)
            elif self.cfg_inputs is not None:
                with _shared_inputs(tr):  # (the entry the captured forward will look up)
                    tr.prime_context(self.cfg_inputs[0], self.cfg_inputs[1])

    def _kind(self, i: int) -> str:
        """The kind of step i: which graph replays it."""
        return self.kinds[i]

    def _capture(self, kind: str = "compute"):
        # The LAZY capture (first replayed step()) runs at an arbitrary later point of the caller's program: another forward of the same
        # transformer in between (another conditioning of the same shape) may have replaced the context-cache entry and the engine-owned
        # context buffers the eager step left, so the entry is re-primed here (a hit costs nothing) - ADVICE r5.  torch.cuda.graph() itself
        # synchronises the device and runs a gc pass: callers that cannot afford that inside their loop build with keep_warmup_step=False
        # (capture in the constructor).
        self._prime_context(kind)
        if self.tea_plan is not None:  # the residual buffer both graphs address exists before either is captured
            self.tr.engine().tea_reserve(self.latents.shape[0] * (2 if self.cfg_inputs is not None else 1) * self._tokens())
        idx = self.sch._step_index
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # (a capture executes nothing: the device state stays what the eager step left)
            self._body(kind)
        self.sch._step_index = idx
        self.graphs[kind] = graph

    def _tokens(self) -> int:
        _, _, T, h, w = self.latents.shape
        return T * (h // 2) * (w // 2)

    def _stage(self, i):
        self.t_buf.copy_(self.sch.timesteps[i])
        self.coef_buf.copy_(self.sch.coef_row(i, self.g, self.latents.device))
        if self.region is not None:
            self.region.stage(i)

    def _body(self, kind: str = "compute"):
        """One step of any kind, captured or eager, under its mode flags: the model and the scheduler update, then, with a region, the blend
        (chronoedit_amd/region.py), or, with tiles, their fusion (chronoedit_amd/tiles.py)."""
        with _step_modes(self.tr, kind, tea=self.tea_plan is not None):
            self._model_step(kind)
            if self.region is not None:
                self.region.blend(self.latents)
            if self.tiles is not None:
                self.tiles.fuse(self.latents)

    def _model_step(self, kind: str = "compute"):
        """The captured caller of `_run_step`: the timestep and the coefficient row come from the staging buffers."""
        _run_step(self.tr, self.sch, self.latents, self.condition, self.t_buf, self.prompt, self.negative, self.image, self.cfg_inputs,
                  self.g, self.cfg_inputs is not None, kind, delta=self.delta, coef=self.coef_buf)

    def _eager_body(self, kind: str):
        """A step of this kind run for real on the warm-up stream, as torch asks of anything that precedes a capture."""
        side = _warmup_stream(self.latents.device)  # ONE long-lived side stream per device: every stream GEMMs run on gets a split-K scratch of its own (ops._gemm_scratch)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._body(kind)
        torch.cuda.current_stream().wait_stream(side)
        self._ran_eagerly.add(self._form(kind))

    def step(self, i: int) -> torch.Tensor:
        if self._done_index is not None:  # the constructor already ran ONE real step (index _done_index) eagerly on the live state
            if i != self._done_index:
                # a caller that re-seeded the latents or starts elsewhere would silently get a trajectory with one extra step
                raise RuntimeError(f"GraphedDenoiser was built at step {self._done_index} (which it ran eagerly, keep_warmup_step=True) but step({i}) "
                                   "was asked first: build it at the step it starts from, or with keep_warmup_step=False")
            self._done_index = None
            self.sch._step_index = i + 1
            return self.latents
        kind = self._kind(i)
        if kind not in self.graphs:
            if not self._form_warm(kind):
                # this form (the single sample after pairs, or the other way round) has not run on this engine yet: its lazy initialisations
                # must not happen under capture, so THIS step runs eagerly, on the live state, as the constructor's first step does
                self._stage(i)
                self.sch._step_index = i
                self._eager_body(kind)
                self.sch._step_index = i + 1
                return self.latents
            self._capture(kind)
        self._stage(i)
        self.graphs[kind].replay()
        self.sch._step_index = i + 1
        return self.latents


# ---------------------------------------------------------------------------------------------------------------
# The loop
# ---------------------------------------------------------------------------------------------------------------
_PREVIEW_SHARDED = "live previews with {} are not implemented (nothing sharded has been tested with them)"


def _first_and_last_frame(x: torch.Tensor) -> torch.Tensor:
    return x[:, :, [0, -1]].contiguous()


@torch.no_grad()
def denoise(transformer, scheduler, latents, condition, prompt_embeds, negative_prompt_embeds, image_embeds,
            num_inference_steps: int, guidance_scale: float = 5.0, enable_temporal_reasoning: bool = False,
            num_temporal_reasoning_steps: int = 0, use_graph: bool = False, on_step_end=None, interrupted=None, graph_warm=None,
            teacache=None, teacache_measure: bool = False, guidance_reuse=None, guidance_measure: Optional[int] = None,
            keep_deltas: bool = False, region=None, sparse_region=None, auto_region=None, start_step: int = 0, start_eps=None,
            preview=None, tiles=None):
    """The whole loop, including the temporal-reasoning truncation 8 -> 2 latent frames (pipeline_chronoedit.py:700-709).
    Per step i, in this order: `interrupted()` -> True skips this and every remaining step (`self.interrupt`, :697-698); at
    i == num_temporal_reasoning_steps the truncation - latents, condition, the scheduler history and every feature's latent-shaped state
    are sliced to the first and last frame, and a graphed loop is rebuilt; each feature's "before step"; the step of kind `kinds[i]`
    (`_run_step` under `_step_modes`, or one GraphedDenoiser replay when `use_graph`); each feature's "after step" - the region blend, the
    auto-region detection; the preview; then `on_step_end(i + start_step, t, latents)` -> replacement latents, a dict with any of latents /
    prompt_embeds / negative_prompt_embeds, or None (the reference's callback_on_step_end hook, :741-749), and, when it replaced
    something, each feature's "replaced" (new conditioning or latents also rebuild a graphed loop).  After the last step each feature's
    "finish": the one read of its table.  graph_warm: a set the caller keeps across edits - shapes already run once in this process skip
    GraphedDenoiser's warm-up step.  With the tokens sharded over ranks (Ulysses) every rank holds the replicated latents and scheduler
    history, so the truncation is a local slice on every rank (the reference all-gathers and re-shards:
    chronoedit_14b_edit_model.py:168-186) and the next forward simply shards the shorter sequence; a step with torch.distributed exchanges
    runs eagerly whatever `use_graph` says.
    start_step = b > 0: the loop runs the TAIL of the schedule, steps b .. n - 1, on latents the caller has brought to sigma[b]
    (`scheduler.set_timesteps(n, begin=b)`: the history starts empty); every plan is made from the tail's arrays, `on_step_end` is told
    i + b.  start_eps: the region blend's eps instead of a copy of the incoming latents - which, behind a warm start, are no longer the
    noise.  start_step=0 is the loop as ever, launch for launch.  With temporal reasoning or a detecting auto_region a ValueError.

    Every feature below is off by default, and the loop is then the plain loop, launch for launch.
    teacache (a teacache.TeaCacheConfig; None: whatever `transformer.enable_teacache()` set) / teacache_measure: teacache.TeaCacheState -
    the compute / skip plan of the edit, or the calibration measurement.
    guidance_reuse (a guidance.GuidanceReuseConfig; None: whatever `transformer.enable_guidance_reuse()` set) / guidance_measure /
    keep_deltas: guidance.GuidanceState - the "pair" / "reuse" / "off" plan and the stored direction, or the measurement of how fast the
    direction moves.
    region (a region.RegionConfig) / start_eps: region.RegionState - the blend behind every step's scheduler update.
    sparse_region (a sparse_region.SparseRegionConfig; None: whatever `transformer.enable_sparse_region()` set; needs a region):
    sparse_region.SparseRegionState - the "compute" / "refresh" / "sparse" plan, the active tokens and the engine's K / V^T cache.
    auto_region (an auto_region.AutoRegion; an explicit `region=` wins): auto_region.AutoRegionState - the detection behind step k that
    turns the edit into a region-limited one, or the per-step measurement.
    preview (a preview.PreviewConfig): preview.PreviewDelivery - per-step RGB estimates, handed to `on_preview`.
    tiles (a tiles.TileState): the latents' samples are the overlapping tiles of one canvas, and `tiles.fuse(latents)` makes them agree behind
    every step's scheduler update (inside the graph of a graphed step); the scheduler's history stays per tile.  It goes with none of the
    features above, nor with temporal reasoning or start_step (ValueError), nor sharded (NotImplementedError).

    Refusals, in the order they are raised (a call that earns two gets the first): start_step with temporal reasoning or a detecting
    auto_region (ValueError); previews, then an auto region, then a region, sharded (NotImplementedError) and what their states refuse;
    `sparse_region=` without a region; a sparse region with TeaCache or guidance reuse; a TeaCache plan with measuring (ValueError each);
    then what GuidanceState.begin, TeaCacheState.begin and SparseRegionState.begin refuse, each in its own documented order."""
    start_step = int(start_step)
    if tiles is not None:
        if start_step or enable_temporal_reasoning or region is not None or auto_region is not None or preview is not None:
            raise ValueError("denoise: tiles go with neither start_step, temporal reasoning, a region, an auto region nor previews")
        from . import tiles as _tl
        refuse_sharded(transformer, _tl.SHARDED)
    if start_step:
        if enable_temporal_reasoning or (auto_region is not None and region is None):
            raise ValueError("denoise: start_step > 0 goes with neither temporal reasoning nor a detecting auto_region (their step indices "
                             "count from the head of the schedule)")
        scheduler.set_timesteps(num_inference_steps, device=latents.device, begin=start_step)
    else:
        scheduler.set_timesteps(num_inference_steps, device=latents.device)
    latents = latents.to(torch.float32).contiguous()
    n_steps = len(scheduler.timesteps)
    pv = None
    if preview is not None:
        refuse_sharded(transformer, _PREVIEW_SHARDED)
        from . import preview as _pv
        pv = _pv.PreviewDelivery(preview, latents.device, [int(v) for v in scheduler.timesteps.tolist()])  # (one read, before the first step)
    auto = _ar.AutoRegionState.begin(transformer, auto_region, region, latents, n_steps, enable_temporal_reasoning, num_temporal_reasoning_steps)
    detecting = auto is not None and auto.detecting
    region_state = None
    if region is not None:
        refuse_sharded(transformer, _rg.SHARDED)
        region_state = _rg.RegionState.begin(region, latents if start_eps is None else start_eps.to(latents.device), scheduler)
    sharded = getattr(transformer, "_cfgp", None) is not None or (_token_sharded(transformer) and not _sharded_batchable(transformer))
    guided = guidance_scale > 1.0 and negative_prompt_embeds is not None
    cfg_inputs = None
    if guided and not sharded:
        cfg_inputs = make_cfg_inputs(prompt_embeds, negative_prompt_embeds, image_embeds)
    if hasattr(transformer, "clear_context_cache"):
        transformer.clear_context_cache()  # a new edit: nothing of the previous edit's conditioning may be reused
    # -- which features the edit asks for, and what excludes what, before anything of them is set up
    tea_cfg = teacache if teacache is not None else getattr(transformer, "_teacache", None)
    measure = bool(teacache_measure or getattr(transformer, "_tea_measure", False))
    sr = sparse_region if sparse_region is not None else getattr(transformer, "_sparse_region", None)
    if sparse_region is not None and region is None and not detecting:
        raise ValueError("sparse_region needs the edit's region (region=): without a mask there are no inactive tokens to leave out")
    if sr is not None and (region is not None or detecting) and (tea_cfg is not None or measure or guidance_reuse is not None or guidance_measure is not None
                                                  or getattr(transformer, "_guidance_reuse", None) is not None):
        raise ValueError("a sparse region plan and TeaCache or guidance reuse (enabled or measuring) exclude each other: their cached "
                         "residual / direction covers all token rows of a step, a sparse step computes the active ones only")
    if measure and tea_cfg is not None:
        raise ValueError("TeaCache: measuring (teacache_measure / calibrate_teacache) and a skip plan (teacache= / enable_teacache) "
                         "exclude each other: disable_teacache() first")
    # -- begin each feature's state (None: the feature is off)
    forced = {int(num_temporal_reasoning_steps)} if enable_temporal_reasoning else set()  # the truncation step: nothing cached at 8 frames fits it
    gs = _gd.GuidanceState.begin(transformer, n_steps, latents.device, guided, guidance_reuse, guidance_measure, keep_deltas, forced,
                                 tea_active=tea_cfg is not None or measure)
    tea = _tea.TeaCacheState.begin(transformer, scheduler.timesteps, tea_cfg, measure, forced)
    sparse = _sr.SparseRegionState.begin(transformer, sr if region is not None or detecting else None, n_steps)
    if tiles is not None and (gs is not None or tea is not None):
        raise ValueError("denoise: tiles go with neither TeaCache nor guidance reuse (enabled or measuring)")
    if sparse is not None and region is not None:
        truncates = enable_temporal_reasoning and 0 <= int(num_temporal_reasoning_steps) < n_steps
        # with reasoning every step up to and including the truncation step is dense: the cache is never built at the 8-frame shape
        dense = set(range(min(int(num_temporal_reasoning_steps), n_steps - 1) + 1)) if enable_temporal_reasoning else set()
        sparse.setup(region_state.w, dense, latents.shape[0] * (2 if cfg_inputs is not None else 1), 2 if truncates else latents.shape[2], *latents.shape[3:])
    if (gs is not None and gs.measuring) or measure:
        use_graph = False  # a measured edit runs eagerly: the table row (and the ring slot) changes per step, and measuring is offline
    if use_graph and not _capturable(transformer):
        use_graph = False  # a step with torch.distributed exchanges runs eagerly (GraphedDenoiser says why); the pipeline default stays use_graph=True

    def plans():
        return dict(tea_plan=None if tea is None else tea.plan, guidance_plan=None if gs is None else gs.plan,
                    sparse_plan=None if sparse is None else sparse.plan)

    kinds = step_kinds(n_steps, measure=measure, **plans())
    graphed = None
    exiting = False
    for i, t in enumerate(scheduler.timesteps):
        if exiting:
            break
        if interrupted is not None and interrupted():
            continue
        if enable_temporal_reasoning and i == num_temporal_reasoning_steps:
            graphed = None  # new latent shape -> new graph
            latents, condition = _first_and_last_frame(latents), _first_and_last_frame(condition)
            for j in range(len(scheduler.model_outputs)):
                mo = scheduler.model_outputs[j]
                if mo is not None and mo.shape[-3] != latents.shape[-3]:
                    scheduler.model_outputs[j] = _first_and_last_frame(mo)
            if scheduler.last_sample is not None and scheduler.last_sample.shape[-3] != latents.shape[-3]:
                scheduler.last_sample = _first_and_last_frame(scheduler.last_sample)
            if region_state is not None and region_state.eps.shape[-3] != latents.shape[-3]:
                region_state.truncate()
            if auto is not None:
                auto.truncated(latents)
        if gs is not None:
            gs.before_step(i, latents)
        if use_graph:
            if graphed is None:
                if scheduler._step_index is None:
                    scheduler._step_index = i
                # engine_generation(): bumped whenever the transformer's engine, its workspaces or a mode that changes the launch sequence
                # is replaced - a recycled id() or a mode switch that keeps the workspace key must not skip the eager warm-up step
                def warm_key():
                    gen = transformer.engine_generation() if hasattr(transformer, "engine_generation") else id(transformer)
                    # (the scheduler object is not part of the key: everything a step reads from it is created eagerly by GraphedDenoiser
                    # before the capture - _ensure_state, the staged timestep / coefficient row - so a fresh scheduler per edit stays warm)
                    # (with guidance reuse: which forms - the stacked pair, the single sample - the rest of the plan runs; GraphedDenoiser
                    # asks the engine per form on top of this)
                    forms = None if gs is None else tuple(sorted({1 if k in ("reuse", "off") else 2 for k in gs.plan[i:]}))
                    return (tuple(latents.shape), guided, gen, tea is not None and tea.plan is not None, forms, tiles is not None,
                            region_state is not None)
                graphed = GraphedDenoiser(transformer, scheduler, latents, condition, prompt_embeds, negative_prompt_embeds,
                                          image_embeds, guidance_scale, batch_cfg=not sharded, warm=graph_warm is not None and warm_key() in graph_warm,
                                          delta=None if gs is None else gs.delta, region=region_state, tiles=tiles, **plans())
                if graph_warm is not None:
                    graph_warm.add(warm_key())  # (taken AFTER the construction: the first step of a process creates the engine)
            latents = graphed.step(i)
        else:
            with _step_modes(transformer, kinds[i], tea=tea is not None and tea.plan is not None, row=i if measure else None):
                latents = _run_step(transformer, scheduler, latents, condition, t, prompt_embeds, negative_prompt_embeds, image_embeds, cfg_inputs,
                                    guidance_scale, not sharded, kinds[i], delta=None if gs is None else gs.delta,
                                    delta_measure=None if gs is None else gs.delta_measure, cfgp=getattr(transformer, "_cfgp", None))
            if tiles is not None:  # (a graphed step fuses inside its graph)
                tiles.fuse(latents)
        if gs is not None:
            gs.after_step(i)
        if pv is not None and preview.lag > 0:
            pv.deliver(i - preview.lag)  # step i is enqueued: the previews of the steps up to i - lag have had that long
        if region_state is not None and not use_graph:  # (a graphed step blends inside its graph)
            region_state.blend(latents, i)
        if auto is not None:
            found = auto.after_step(i, scheduler, latents, sr.margin if sr is not None else 0)
            if found is not None:  # a region was found and accepted: (its state, already blended into step i; the weights on the host)
                region_state, w_cpu = found
                graphed = None  # a region is a different warm shape, and every later step ends with the blend
                if sparse is not None:  # every step up to here ran dense: step k + 1 is the first refresh
                    sparse.setup(w_cpu, set(range(i + 1)), latents.shape[0] * (2 if cfg_inputs is not None else 1), *latents.shape[2:])
                    kinds = step_kinds(n_steps, measure=measure, **plans())
            exiting = auto.exiting
        if pv is not None and _pv.due(i, n_steps, preview.every):
            # kept cells show the source when asked to - and always under a sparse plan, whose steps predict 0 outside the active tokens
            comp = region_state is not None and (preview.composite or (sparse is not None and sparse.plan is not None))
            pv.submit(i, i + start_step, scheduler.model_outputs[-1], region_state.w if comp else None, region_state.z_src if comp else None)
            if preview.lag == 0:
                pv.deliver(i)
        if on_step_end is not None:
            new = on_step_end(i + start_step, t, latents)
            replaced = (isinstance(new, dict) and any(k in new for k in ("latents", "prompt_embeds", "negative_prompt_embeds"))) or \
                (new is not None and not isinstance(new, dict) and new is not latents)
            if sparse is not None and replaced and sparse.replaced(i):
                kinds, graphed = step_kinds(n_steps, measure=measure, **plans()), None  # (the graphed loop holds the plan it was built with)
            if isinstance(new, dict):  # the reference's callback may also replace the conditioning (pipeline_chronoedit.py:747-749)
                if "prompt_embeds" in new or "negative_prompt_embeds" in new:
                    prompt_embeds = new.get("prompt_embeds", prompt_embeds)
                    if negative_prompt_embeds is not None:
                        negative_prompt_embeds = new.get("negative_prompt_embeds", negative_prompt_embeds)
                    if cfg_inputs is not None:
                        cfg_inputs = make_cfg_inputs(prompt_embeds, negative_prompt_embeds, image_embeds)
                    graphed = None  # the graph holds the stacked conditioning it was captured with
                    if gs is not None and gs.replaced(i):
                        kinds = step_kinds(n_steps, measure=measure, **plans())
                new = new.get("latents")
            if new is not None and new is not latents:
                graphed = None  # the graph is tied to the latents' storage
                latents = new.to(torch.float32).contiguous()
    if pv is not None:
        pv.flush()  # everything outstanding, before the loop returns
    if tea is not None:
        tea.finish()
    if gs is not None:
        gs.finish(scheduler.timesteps)
    if auto is not None:
        auto.finish(scheduler.timesteps)
    return latents
