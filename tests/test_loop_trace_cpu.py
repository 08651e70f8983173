"""The control flow of pipeline.denoise, traced on the CPU: which forwards and which scheduler update every step of every kind of edit runs, under
which mode flags, what a callback, an interrupt, the truncation and a warm start change, and which refusal wins where two apply.  The
transformer is a stub that records every forward; the scheduler is the real one with `step_cfg` replaced by a recorder.  The expected traces
are written out below; nothing here needs the built library."""
from types import SimpleNamespace

import pytest
import torch

from chronoedit_amd import guidance, region, sparse_region, teacache
from chronoedit_amd.pipeline import denoise
from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler

STEPS = 5


class StubEngine:
    def __init__(self):
        self._tea_row = None
        self.log = []

    def tea_drop(self):
        self.log.append("tea_drop")

    def tea_measure_begin(self, n):
        self.log.append(("tea_measure_begin", n))

    def tea_measure_end(self):
        self.log.append("tea_measure_end")
        return torch.ones(STEPS, 2)

    def sparse_check(self):
        self.log.append("sparse_check")

    def sparse_begin(self, ids, n_samples, T, h, w):
        self.log.append(("sparse_begin", int(ids.numel()), n_samples, T, h, w))


class StubTransformer:
    """Records (input shape, text shape, _tea_mode, _sparse_mode, _shared_inputs) per forward and returns x[:, :16]."""

    def __init__(self, ratios=None, fail_at=None, sharded=False):
        self.calls, self.texts, self.rows, self.first = [], [], [], []
        self._tea_mode = self._sparse_mode = self._shared_inputs = None
        self._teacache = self._guidance_reuse = None
        self.teacache_report = self.guidance_report = self.sparse_report = self.auto_region_report = "stale"
        self.teacache_measurement = self.guidance_measurement = None
        self.cleared = 0
        self.ratios, self.fail_at = ratios, fail_at
        self._engine = StubEngine()
        if sharded:
            self._sp = SimpleNamespace(sharded=True)

    def engine(self):
        return self._engine

    def teacache_ratios(self, timesteps):
        return list(self.ratios)

    def clear_context_cache(self):
        self.cleared += 1

    def __call__(self, x, timestep, text, image, return_dict=False):
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            self.seen_at_failure = (self._tea_mode, self._sparse_mode, self._shared_inputs)
            raise RuntimeError("boom")
        self.calls.append((tuple(x.shape), tuple(text.shape), self._tea_mode, self._sparse_mode, self._shared_inputs))
        self.texts.append(text)
        self.rows.append(self._engine._tea_row)
        self.first.append(float(x[0, 0, 0, 0, 0]))
        return (x[:, :16],)


class StubScheduler(FlowUniPCMultistepScheduler):
    """`step_cfg` records (step index, v_cond shape, v_uncond given, delta_mode, (slot, row) of delta_measure, coef given) and adds 1 to the
    sample in place; `frames` keeps the frame count of the history the step found (None: no history yet)."""

    def __init__(self):
        super().__init__()
        self.trace, self.frames = [], []

    def step_cfg(self, v_cond, v_uncond, guidance_scale, sample, coef=None, delta=None, delta_mode=None, delta_measure=None):
        if self._step_index is None:
            self._step_index = 0
        self.trace.append((self._step_index, tuple(v_cond.shape), v_uncond is not None, delta_mode,
                           None if delta_measure is None else (delta_measure[0], delta_measure[2]), coef is not None))
        mo, ls = self.model_outputs[-1], self.last_sample
        self.frames.append((None if mo is None else mo.shape[2], None if ls is None else ls.shape[2]))
        self._ensure_state(sample)
        if delta_measure is not None:
            delta_measure[1][delta_measure[2]] = 1.0  # (every sum finite: rel_l2 is 1 wherever the loop says a direction of that age exists)
        sample.add_(1.0)
        self._step_index += 1
        return sample


def inputs():
    g = torch.Generator().manual_seed(0)
    latents = torch.randint(-8, 8, (1, 16, 3, 4, 4), generator=g).to(torch.float32)  # (integers: adding 1 per step is exact)
    condition = torch.randn(1, 20, 3, 4, 4, generator=g).to(torch.bfloat16)
    prompt = torch.randn(1, 8, 16, generator=g).to(torch.bfloat16)
    negative = torch.randn(1, 8, 16, generator=g).to(torch.bfloat16)
    return latents, condition, prompt, negative


def run(tr=None, guidance_scale=5.0, unguided=False, **kw):
    tr = StubTransformer() if tr is None else tr
    sch = StubScheduler()
    latents, condition, prompt, negative = inputs()
    out = denoise(tr, sch, latents, condition, prompt, None if unguided else negative, None, STEPS, guidance_scale=guidance_scale, **kw)
    return tr, sch, out


# one forward of the stacked pair / of one sample, at 3 and at 2 latent frames; (.., _tea_mode, _sparse_mode, _shared_inputs)
PAIR3 = ((2, 36, 3, 4, 4), (2, 8, 16), None, None, True)
PAIR2 = ((2, 36, 2, 4, 4), (2, 8, 16), None, None, True)
ONE3 = ((1, 36, 3, 4, 4), (1, 8, 16), None, None, None)
V3, V2 = (1, 16, 3, 4, 4), (1, 16, 2, 4, 4)


def tea_pair(mode):
    return ((2, 36, 3, 4, 4), (2, 8, 16), mode, None, True)


def test_guided_plain():
    tr, sch, out = run()
    assert tr.calls == [PAIR3, PAIR3, PAIR3, PAIR3, PAIR3]
    assert sch.trace == [(0, V3, True, None, None, False), (1, V3, True, None, None, False), (2, V3, True, None, None, False),
                         (3, V3, True, None, None, False), (4, V3, True, None, None, False)]
    assert tr.cleared == 1 and tr._engine.log == []
    assert tr.guidance_report is None and tr.sparse_report is None and tr.auto_region_report is None
    assert tr.texts[0] is tr.texts[4]  # the stacked conditioning is built once per edit
    assert out.dtype == torch.float32 and torch.equal(out, inputs()[0] + 5.0)
    assert (tr._tea_mode, tr._sparse_mode, tr._shared_inputs) == (None, None, None)


@pytest.mark.parametrize("kw", [dict(unguided=True), dict(guidance_scale=1.0)], ids=["no_negative", "scale_1"])
def test_unguided(kw):
    tr, sch, _ = run(**kw)
    g = kw.get("guidance_scale", 5.0)
    assert tr.calls == [ONE3, ONE3, ONE3, ONE3, ONE3]
    assert sch.trace == [(0, V3, False, None, None, False), (1, V3, False, None, None, False), (2, V3, False, None, None, False),
                         (3, V3, False, None, None, False), (4, V3, False, None, None, False)]
    assert tr.guidance_report is None and g in (1.0, 5.0)


def test_unguided_ignores_guidance_reuse():
    tr, sch, _ = run(unguided=True, guidance_reuse=guidance.GuidanceReuseConfig(pair_every=2))
    assert tr.calls == [ONE3] * 5 and [r[3] for r in sch.trace] == [None] * 5 and tr.guidance_report is None


def test_truncation_at_step_2():
    tr, sch, out = run(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    assert tr.calls == [PAIR3, PAIR3, PAIR2, PAIR2, PAIR2]
    assert [r[1] for r in sch.trace] == [V3, V3, V2, V2, V2]
    assert sch.frames == [(None, None), (3, 3), (2, 2), (2, 2), (2, 2)]  # the history is sliced with the latents, in front of step 2
    assert tuple(out.shape) == V2 and torch.equal(out, inputs()[0][:, :, [0, -1]] + 5.0)


RATIOS = [0.0, 0.1, 0.1, 0.1, 0.1]  # threshold 0.15: every second inner step computes


def test_teacache_plan():
    tr, sch, _ = run(StubTransformer(RATIOS), teacache=teacache.TeaCacheConfig(0.15))
    assert tr.calls == [tea_pair("compute"), tea_pair("skip"), tea_pair("compute"), tea_pair("skip"), tea_pair("compute")]
    assert sch.trace == [(i, V3, True, None, None, False) for i in range(5)]
    assert tr.teacache_report == {"plan": [True, False, True, False, True], "computed": 3, "skipped": 2, "ratios": RATIOS}
    assert tr._engine.log == ["tea_drop"] and tr.rows == [None] * 5 and tr._tea_mode is None


def test_teacache_plan_from_the_transformers_switch_and_forced_truncation_step():
    tr = StubTransformer(RATIOS)
    tr._teacache = teacache.TeaCacheConfig(0.15)
    run(tr, enable_temporal_reasoning=True, num_temporal_reasoning_steps=3)
    assert tr.teacache_report["plan"] == [True, False, True, True, True]  # step 3 would skip: the truncation step computes
    assert [c[2] for c in tr.calls] == ["compute", "skip", "compute", "compute", "compute"]
    assert [c[0][2] for c in tr.calls] == [3, 3, 3, 2, 2]


def test_teacache_measure():
    tr, sch, _ = run(StubTransformer(RATIOS), teacache_measure=True, use_graph=True)  # (a measured edit runs eagerly whatever use_graph says)
    assert tr.calls == [tea_pair("measure")] * 5
    assert tr.rows == [0, 1, 2, 3, 4]
    assert tr._engine.log == [("tea_measure_begin", 5), "tea_measure_end"]
    assert sorted(tr.teacache_measurement) == ["distances", "ratios"]
    assert tr.teacache_measurement["ratios"] == RATIOS and tr.teacache_measurement["distances"] == [1.0] * 5
    assert tr._tea_mode is None


PAIR_STEP = (V3, True, "store", None, False)
REUSE_STEP = (V3, False, "reuse", None, False)
OFF_STEP = (V3, False, None, None, False)


def test_guidance_reuse_pair_every_2():
    tr, sch, _ = run(guidance_reuse=guidance.GuidanceReuseConfig(pair_every=2))
    assert tr.calls == [PAIR3, ONE3, PAIR3, ONE3, PAIR3]
    assert [r[1:] for r in sch.trace] == [PAIR_STEP, REUSE_STEP, PAIR_STEP, REUSE_STEP, PAIR_STEP]
    assert tr.guidance_report == {"plan": ["pair", "reuse", "pair", "reuse", "pair"], "pair": 3, "reuse": 2, "off": 0}


def test_guidance_reuse_interval_with_off_steps():
    tr, sch, _ = run(guidance_reuse=guidance.GuidanceReuseConfig(pair_every=2, interval=(0.0, 0.6)))
    assert tr.calls == [PAIR3, ONE3, PAIR3, ONE3, ONE3]
    assert [r[1:] for r in sch.trace] == [PAIR_STEP, REUSE_STEP, PAIR_STEP, OFF_STEP, OFF_STEP]
    assert tr.guidance_report == {"plan": ["pair", "reuse", "pair", "off", "off"], "pair": 2, "reuse": 1, "off": 2}


def test_guidance_reuse_truncation_step_is_a_pair():
    tr, sch, _ = run(guidance_reuse=guidance.GuidanceReuseConfig(pair_every=3), enable_temporal_reasoning=True, num_temporal_reasoning_steps=1)
    assert tr.guidance_report["plan"] == ["pair", "pair", "reuse", "reuse", "pair"]
    assert [c[0][2] for c in tr.calls] == [3, 2, 2, 2, 2] and [c[0][0] for c in tr.calls] == [2, 2, 1, 1, 2]


def test_guidance_reuse_replans_when_a_callback_replaces_an_embedding():
    new_prompt = torch.full((1, 8, 16), 3.0, dtype=torch.bfloat16)
    tr = StubTransformer()
    reports = []

    def on_step_end(i, t, latents):
        reports.append(list(tr.guidance_report["plan"]))
        return {"prompt_embeds": new_prompt} if i == 1 else None

    _, sch, _ = run(tr, guidance_reuse=guidance.GuidanceReuseConfig(pair_every=3), on_step_end=on_step_end)
    assert reports[0] == reports[1] == ["pair", "reuse", "reuse", "pair", "reuse"]
    assert reports[2] == ["pair", "reuse", "pair", "reuse", "reuse"] == tr.guidance_report["plan"]  # step 2 becomes a pair
    assert tr.guidance_report == {"plan": ["pair", "reuse", "pair", "reuse", "reuse"], "pair": 2, "reuse": 3, "off": 0}
    assert tr.calls == [PAIR3, ONE3, PAIR3, ONE3, ONE3]
    assert [r[3] for r in sch.trace] == ["store", "reuse", "store", "reuse", "reuse"]
    assert torch.equal(tr.texts[2][0], new_prompt[0]) and torch.equal(tr.texts[2][1], inputs()[3][0])  # the new stacked pair
    assert not torch.equal(tr.texts[0][0], new_prompt[0]) and tr.texts[3] is new_prompt


def test_guidance_measure():
    nan = float("nan")
    tr, sch, _ = run(guidance_measure=2, use_graph=True)  # (runs eagerly whatever use_graph says)
    assert tr.calls == [PAIR3] * 5
    assert sch.trace == [(0, V3, True, "measure", (0, 0), False), (1, V3, True, "measure", (1, 1), False), (2, V3, True, "measure", (0, 2), False),
                         (3, V3, True, "measure", (1, 3), False), (4, V3, True, "measure", (0, 4), False)]
    m = tr.guidance_measurement
    assert sorted(m) == ["rel_l2", "timesteps"] and m["timesteps"] == [int(v) for v in sch.timesteps.tolist()]
    assert str(m["rel_l2"]) == str([[nan, nan], [1.0, nan], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0]])  # the ring held 0, 1, 2, 2, 2 directions
    assert tr.guidance_report == {"plan": ["pair"] * 5, "pair": 5, "reuse": 0, "off": 0}


def test_guidance_measure_keeps_the_deltas_and_restarts_the_ring_at_the_truncation():
    nan = float("nan")
    tr, sch, _ = run(guidance_measure=2, keep_deltas=True, enable_temporal_reasoning=True, num_temporal_reasoning_steps=3)
    assert [r[4] for r in sch.trace] == [(0, 0), (1, 1), (0, 2), (0, 3), (1, 4)]
    assert str(tr.guidance_measurement["rel_l2"]) == str([[nan, nan], [1.0, nan], [1.0, 1.0], [nan, nan], [1.0, nan]])
    assert [tuple(d.shape) for d in tr.guidance_measurement["deltas"]] == [V3, V3, V3, V2, V2]


def test_a_callback_that_returns_new_latents():
    seen = []

    def on_step_end(i, t, latents):
        seen.append(i)
        return torch.full((1, 16, 3, 4, 4), 7.0, dtype=torch.float64) if i == 1 else None

    tr, sch, out = run(on_step_end=on_step_end)
    assert seen == [0, 1, 2, 3, 4] and len(tr.calls) == 5
    assert tr.first[2] == 7.0 and tr.first[3] == 8.0  # the next forward sees them (as fp32), and the loop goes on from them
    assert out.dtype == torch.float32 and torch.equal(out, torch.full((1, 16, 3, 4, 4), 10.0))


def test_interrupted_after_step_1():
    state = {"done": 0}
    tr = StubTransformer()

    def on_step_end(i, t, latents):
        state["done"] = i + 1

    _, sch, out = run(tr, on_step_end=on_step_end, interrupted=lambda: state["done"] >= 2)
    assert tr.calls == [PAIR3, PAIR3] and [r[0] for r in sch.trace] == [0, 1]
    assert torch.equal(out, inputs()[0] + 2.0)


def test_start_step_runs_the_tail():
    told = []
    tr, sch, out = run(start_step=2, on_step_end=lambda i, t, latents: told.append((i, int(t))))
    full = FlowUniPCMultistepScheduler()
    full.set_timesteps(STEPS)
    assert tr.calls == [PAIR3, PAIR3, PAIR3] and [r[0] for r in sch.trace] == [0, 1, 2]
    assert told == [(2, int(full.timesteps[2])), (3, int(full.timesteps[3])), (4, int(full.timesteps[4]))]
    assert torch.equal(out, inputs()[0] + 3.0)


def test_start_step_plans_from_the_tail():
    tr, _, _ = run(start_step=2, guidance_reuse=guidance.GuidanceReuseConfig(pair_every=2))
    assert tr.guidance_report["plan"] == ["pair", "reuse", "pair"]


# ---- refusals, in the order the loop raises them ----------------------------------------------------------------------------------------
TEA = teacache.TeaCacheConfig(0.15)
GR = guidance.GuidanceReuseConfig(pair_every=2)
SR = sparse_region.SparseRegionConfig(refresh_every=2, margin=0)


def region_config():
    w = torch.zeros(4, 4)
    w[:2, :2] = 1.0
    return region.RegionConfig(w, torch.zeros(1, 16, 3, 4, 4))


REFUSALS = [
    ("tea_and_measure", dict(teacache=TEA, teacache_measure=True), ValueError, "TeaCache: measuring (teacache_measure / calibrate_teacache) and a skip plan"),
    ("reuse_and_tea", dict(guidance_reuse=GR, teacache=TEA), ValueError, "guidance reuse and TeaCache (enabled or measuring) exclude each other"),
    ("reuse_and_tea_measure", dict(guidance_reuse=GR, teacache_measure=True), ValueError, "guidance reuse and TeaCache (enabled or measuring) exclude each other"),
    ("measure_unguided", dict(guidance_measure=2, unguided=True), ValueError, "guidance_measure needs a guided edit"),
    ("measure_with_plan", dict(guidance_measure=2, guidance_reuse=GR), ValueError, "guidance_measure measures the plain loop (every step a pair)"),
    ("measure_age", dict(guidance_measure=0), ValueError, "guidance_measure: max_age must be in 1.."),
    ("sparse_without_region", dict(sparse_region=SR), ValueError, "sparse_region needs the edit's region (region=)"),
    ("start_step_reasoning", dict(start_step=1, enable_temporal_reasoning=True, num_temporal_reasoning_steps=2), ValueError,
     "denoise: start_step > 0 goes with neither temporal reasoning nor a detecting auto_region"),
    # where two apply: the one named wins
    ("start_step_before_sparse", dict(start_step=1, enable_temporal_reasoning=True, sparse_region=SR), ValueError, "denoise: start_step > 0"),
    ("sparse_before_tea_and_measure", dict(sparse_region=SR, teacache=TEA, teacache_measure=True), ValueError, "sparse_region needs the edit's region"),
    ("tea_and_measure_before_reuse", dict(teacache=TEA, teacache_measure=True, guidance_reuse=GR), ValueError, "TeaCache: measuring"),
    ("tea_and_measure_before_measure_unguided", dict(teacache=TEA, teacache_measure=True, guidance_measure=2, unguided=True), ValueError, "TeaCache: measuring"),
    ("measure_unguided_before_reuse_and_tea", dict(guidance_measure=2, unguided=True, guidance_reuse=GR, teacache=TEA), ValueError,
     "guidance_measure needs a guided edit"),
    ("reuse_and_tea_before_measure_with_plan", dict(guidance_measure=2, guidance_reuse=GR, teacache=TEA), ValueError, "guidance reuse and TeaCache"),
]


@pytest.mark.parametrize("kw,exc,text", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_refusals(kw, exc, text):
    tr = StubTransformer(RATIOS)
    with pytest.raises(exc) as e:
        run(tr, **kw)
    assert str(e.value).startswith(text), str(e.value)
    assert tr.calls == []


def test_sparse_with_region_and_tea_is_refused():
    with pytest.raises(ValueError) as e:
        run(StubTransformer(RATIOS), region=region_config(), sparse_region=SR, teacache=TEA)
    assert str(e.value).startswith("a sparse region plan and TeaCache or guidance reuse (enabled or measuring) exclude each other")


SHARDED = [
    ("teacache", dict(teacache=TEA), "TeaCache with the tokens sharded over ranks or with CFG parallelism is not implemented "
                                     "(the cached residual is row-local; nothing sharded has been tested with it)"),
    ("teacache_measure", dict(teacache_measure=True), "TeaCache with the tokens sharded over ranks or with CFG parallelism is not implemented "
                                                      "(the cached residual is row-local; nothing sharded has been tested with it)"),
    ("guidance_reuse", dict(guidance_reuse=GR), "guidance reuse with the tokens sharded over ranks or with CFG parallelism is not implemented "
                                                "(the stored direction is latent-local; nothing sharded has been tested with it)"),
    ("guidance_measure", dict(guidance_measure=2), "guidance reuse with the tokens sharded over ranks or with CFG parallelism is not implemented "
                                                   "(the stored direction is latent-local; nothing sharded has been tested with it)"),
    ("region", dict(region="a region"), "an edit region with the tokens sharded over ranks or with CFG parallelism is not implemented "
                                        "(the blend runs on replicated latents; nothing sharded has been tested with it)"),
    ("preview", dict(preview="a preview"), "live previews with the tokens sharded over ranks or with CFG parallelism are not implemented "
                                           "(nothing sharded has been tested with them)"),
    # where two apply
    ("preview_before_region", dict(preview="a preview", region="a region"), "live previews with"),
    ("region_before_teacache", dict(region="a region", teacache=TEA), "an edit region with"),
]


@pytest.mark.parametrize("kw,text", [r[1:] for r in SHARDED], ids=[r[0] for r in SHARDED])
def test_sharded_refusals(kw, text):
    tr = StubTransformer(RATIOS, sharded=True)
    with pytest.raises(NotImplementedError) as e:
        run(tr, **kw)
    assert str(e.value) == text if len(text) > 40 else str(e.value).startswith(text), str(e.value)
    assert tr.calls == []


def test_sharded_exclusions_come_before_the_sharded_refusal():
    with pytest.raises(ValueError) as e:
        run(StubTransformer(RATIOS, sharded=True), guidance_reuse=GR, teacache=TEA)
    assert str(e.value).startswith("guidance reuse and TeaCache")
    with pytest.raises(ValueError) as e:
        run(StubTransformer(RATIOS, sharded=True), teacache=TEA, teacache_measure=True)
    assert str(e.value).startswith("TeaCache: measuring")


def test_sharded_plain_loop_runs_two_passes():
    tr, sch, _ = run(StubTransformer(sharded=True))  # (no transposed-V path: the pair cannot be one batch)
    assert tr.calls == [ONE3] * 10 and [r[2] for r in sch.trace] == [True] * 5
    assert all(tr.texts[2 * i] is tr.texts[0] and tr.texts[2 * i + 1] is tr.texts[1] for i in range(5))


# ---- the mode flags never outlive a step -------------------------------------------------------------------------------------------------
def test_flags_are_cleared_when_a_forward_raises_under_a_teacache_plan():
    tr = StubTransformer(RATIOS, fail_at=1)
    with pytest.raises(RuntimeError, match="boom"):
        run(tr, teacache=TEA)
    assert tr.seen_at_failure == ("skip", None, True)
    assert (tr._tea_mode, tr._sparse_mode, tr._shared_inputs) == (None, None, None)


def test_flags_are_cleared_when_a_forward_raises_while_measuring():
    tr = StubTransformer(RATIOS, fail_at=0)
    with pytest.raises(RuntimeError, match="boom"):
        run(tr, teacache_measure=True)
    assert tr.seen_at_failure == ("measure", None, True)
    assert (tr._tea_mode, tr._sparse_mode, tr._shared_inputs) == (None, None, None)


def test_flags_are_cleared_when_a_forward_raises_under_a_sparse_plan():
    tr = StubTransformer(fail_at=0)
    with pytest.raises(RuntimeError, match="boom"):
        run(tr, region=region_config(), sparse_region=SR)
    assert tr.sparse_report["plan"] == ["refresh", "sparse", "refresh", "sparse", "compute"]
    assert tr._engine.log[0] == "sparse_check" and tr._engine.log[1][0] == "sparse_begin"
    assert tr.seen_at_failure == (None, "refresh", True)
    assert (tr._tea_mode, tr._sparse_mode, tr._shared_inputs) == (None, None, None)
