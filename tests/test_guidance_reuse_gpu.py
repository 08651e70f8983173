"""Guidance reuse in the denoising loop (chronoedit_amd/guidance.py, pipeline.denoise / denoise_step / GraphedDenoiser, ChronoEditPipeline).

An all-pair plan is the plain loop bit for bit; an alternating plan is, bit for bit, the loop this file writes out from public pieces
(transformer forwards + ops.cfg_unipc_step_delta in the planned mode); hipGraph replay == eager for every kind of plan; against an fp32
oracle driven by the same plan the latents stay inside the bound tests/test_teacache_gpu.py holds this model and step count to (6e-2: only
the combine differs); state handling (second edit, context cache, refusals, restore); the measuring edit.
Shapes: the tiny model of tests/test_teacache_gpu.py (2 heads x 128, 2 layers, ffn 512), latents 1 x 16 x T x 8 x 12, 6 steps."""
import math
import types

import pytest
import torch

from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
P, R, O = "pair", "reuse", "off"
STEPS, G = 6, 5.0
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
_PARAMS = {}


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cfg(pair_every=2, interval=(0.0, 1.0)):
    from chronoedit_amd.guidance import GuidanceReuseConfig
    return GuidanceReuseConfig(pair_every, interval)


def _model():
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    if "p" not in _PARAMS:
        _PARAMS["p"] = D.make_synthetic_params(DCFG, dtype=BF)
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in _PARAMS["p"].items()})
    return m


def _inputs(T=2, seed=1):
    """bf16-representable (lat0, cond, prompt, negative, img) on the CPU in fp32."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    return r(1, 16, T, 8, 12), r(1, 20, T, 8, 12), r(1, 40, 128), r(1, 40, 128), r(1, 257, 64)


def _dev(inp):
    lat0, cond, pr, ng, img = inp
    return lat0.cuda(), cond.cuda().to(BF), pr.cuda().to(BF), ng.cuda().to(BF), img.cuda().to(BF)


def _run(m, inp, use_graph=False, steps=STEPS, negative=True, **kw):
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    lat0, cond, pr, ng, img = _dev(inp)
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    return denoise(m, sch, lat0, cond, pr, ng if negative else None, img, steps, G, use_graph=use_graph, **kw).clone()


@pytest.fixture(scope="module")
def plain_run():
    """The plain guided loop on the shared inputs (eager; tests/test_pipeline_gpu.py holds graphed == eager)."""
    return _run(_model(), _inputs())


# ----------------------------------------------------------------------------------------------------------------------------------
# the loop does what the plan says
# ----------------------------------------------------------------------------------------------------------------------------------
def test_all_pair_plan_is_bit_identical_to_the_plain_loop(plain_run):
    m = _model()
    for use_graph in (False, True):
        out = _run(m, _inputs(), use_graph=use_graph, guidance_reuse=_cfg(pair_every=1))
        assert m.guidance_report == {"plan": [P] * STEPS, "pair": STEPS, "reuse": 0, "off": 0}
        assert torch.equal(out, plain_run), (use_graph, float((out - plain_run).abs().max()))


def _hand_rolled(m, inp, kinds, steps=STEPS):
    """The loop written out from public pieces: the stacked pair under the shared-input declaration denoise_step uses, or the single
    sample, then ops.cfg_unipc_step_delta in the planned mode (ops.cfg_unipc_step for "off")."""
    from chronoedit_amd import ops
    from chronoedit_amd.pipeline import _shared_inputs, compact_text_context, make_cfg_inputs
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    lat, cond, pr, ng, img = _dev(inp)
    lat = lat.float().contiguous()
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    sch.set_timesteps(steps, device=lat.device)
    m.clear_context_cache()
    text2, image2 = make_cfg_inputs(pr, ng, img)
    compact_text_context(pr)
    x_last, m0, m1 = (torch.zeros_like(lat) for _ in range(3))
    delta = torch.zeros(lat.shape, dtype=BF, device=lat.device)
    for i, t in enumerate(sch.timesteps):
        x_in = torch.cat([lat.to(BF), cond], dim=1)
        ts = t.expand(1)
        coef = sch.coef_row(i, G, lat.device)
        if kinds[i] == P:
            with _shared_inputs(m):
                out = m(torch.cat([x_in, x_in], 0), torch.cat([ts, ts], 0), text2, image2, return_dict=False)[0]
            ops.cfg_unipc_step_delta(out[:1].contiguous(), out[1:].contiguous(), lat, x_last, m0, m1, coef, delta, round_sigma_v=False)
        else:
            c = m(x_in, ts, pr, img, return_dict=False)[0].contiguous()
            if kinds[i] == R:
                ops.cfg_unipc_step_delta(c, None, lat, x_last, m0, m1, coef, delta, round_sigma_v=False)
            else:
                ops.cfg_unipc_step(c, None, lat, x_last, m0, m1, coef, round_sigma_v=False)
    return lat.clone()


@pytest.mark.parametrize("pair_every, interval, kinds", [(2, (0.0, 1.0), [P, R, P, R, P, R]), (3, (0.0, 0.67), [P, R, R, P, R, O])])
def test_planned_loop_equals_the_hand_rolled_loop_and_its_replay(plain_run, pair_every, interval, kinds):
    m = _model()
    cfg = _cfg(pair_every, interval)
    eager = _run(m, _inputs(), guidance_reuse=cfg)
    assert m.guidance_report["plan"] == kinds
    assert (m.guidance_report["pair"], m.guidance_report["reuse"], m.guidance_report["off"]) == (kinds.count(P), kinds.count(R), kinds.count(O))
    want = _hand_rolled(_model(), _inputs(), kinds)
    assert torch.equal(eager, want), float((eager - want).abs().max())
    assert torch.isfinite(eager).all() and not torch.equal(eager, plain_run)  # the plan really left the unconditional sample out
    # hipGraph replay (a cold engine: every form warms up eagerly before it is captured), then a second edit with the shapes warm
    m2 = _model()
    warm = set()
    replay = _run(m2, _inputs(), use_graph=True, guidance_reuse=cfg, graph_warm=warm)
    assert torch.equal(replay, eager), float((replay - eager).abs().max())
    second = _inputs(seed=2)
    eager2 = _run(_model(), second, guidance_reuse=cfg)
    replay2 = _run(m2, second, use_graph=True, guidance_reuse=cfg, graph_warm=warm)
    assert torch.equal(replay2, eager2), float((replay2 - eager2).abs().max())
    assert not torch.equal(replay2, replay)
    # ... and the first edit again on the warm pipeline: nothing of the second edit's direction is seen
    assert torch.equal(_run(m2, _inputs(), use_graph=True, guidance_reuse=cfg, graph_warm=warm), eager)


def test_all_off_equals_the_unguided_call():
    for use_graph in (False, True):
        m = _model()
        off = _run(m, _inputs(), use_graph=use_graph, guidance_reuse=_cfg(2, (0, 0)))
        assert m.guidance_report == {"plan": [O] * STEPS, "pair": 0, "reuse": 0, "off": STEPS}
        unguided = _run(_model(), _inputs(), use_graph=use_graph, negative=False)
        assert torch.equal(off, unguided), (use_graph, float((off - unguided).abs().max()))


def test_temporal_reasoning_forces_a_pair_at_the_truncation():
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2, guidance_reuse=_cfg(3))
    outs = []
    for use_graph in (False, True):
        m = _model()
        outs.append(_run(m, _inputs(T=8), use_graph=use_graph, **kw))
        assert m.guidance_report["plan"] == [P, R, P, R, R, P]
    assert outs[0].shape == (1, 16, 2, 8, 12) and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


def _oracle_loop_with_plan(inp, kinds, steps=STEPS, guidance=G):
    """The reference loop in fp32 (oracle/dit_oracle.py, oracle/unipc_oracle.py) with the same plan and the reuse formula in fp32:
    a pair stores d = c - u; a reuse step takes u' = c - d, v = u' + g d; an off step takes v = c."""
    from oracle.unipc_oracle import UniPCOracle
    p = {k: v.float() for k, v in _PARAMS["p"].items()}
    lat, cond, pr, ng, img = inp
    sch = UniPCOracle()
    sch.set_timesteps(steps, shift=5.0)
    d = None
    with torch.no_grad():
        for i, t in enumerate(sch.timesteps):
            x_in = torch.cat([lat, cond], dim=1)
            ts = t.expand(1)
            c = D.dit_forward(p, DCFG, x_in, ts, pr, img)
            if kinds[i] == P:
                u = D.dit_forward(p, DCFG, x_in, ts, ng, img)
                d = c - u
                v = u + guidance * d
            elif kinds[i] == R:
                u = c - d
                v = u + guidance * d
            else:
                v = c
            lat = sch.step(v, lat)
    return lat.float()


def test_alternating_loop_vs_fp32_oracle_with_the_same_plan(plain_run):
    m = _model()
    out = _run(m, _inputs(), guidance_reuse=_cfg(2))
    kinds = m.guidance_report["plan"]
    assert kinds == [P, R, P, R, P, R]
    ref = _oracle_loop_with_plan(_inputs(), kinds)
    e, moved = rel_l2(out, ref), rel_l2(out, plain_run)
    print(f"guidance reuse p r p r p r: final latents rel-L2 vs the fp32 oracle with the same plan {e:.3e}; vs the plain loop {moved:.3e}")
    assert torch.isfinite(out).all()
    assert e < 6e-2, e
    assert moved > 0


# ----------------------------------------------------------------------------------------------------------------------------------
# state
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_context_projections_are_computed_once_per_form(use_graph):
    m = _model()
    m.cache_context = True
    cached = _run(m, _inputs(), use_graph=use_graph, guidance_reuse=_cfg(2))
    assert m.engine().ctx_projections == 2, m.engine().ctx_projections  # the stacked pair and the single sample: not once per switch
    assert len(m.engine()._ctx_cache) == 2
    _run(m, _inputs(seed=2), use_graph=use_graph, guidance_reuse=_cfg(2))
    assert m.engine().ctx_projections == 2  # a second edit starts again from 0
    m.clear_context_cache()
    assert m.engine().ctx_projections == 0 and m.engine()._ctx_key is None and not m.engine()._ctx_cache
    plain = _model()
    assert torch.equal(cached, _run(plain, _inputs(), guidance_reuse=_cfg(2)))  # (cache_context off: projected every step)
    assert plain.engine().ctx_projections == STEPS


def test_refusals_and_restore(plain_run):
    from chronoedit_amd.teacache import TeaCacheConfig
    m = _model()
    m.enable_guidance_reuse(pair_every=2)
    m.enable_teacache(2.5, (1.0,))
    with pytest.raises(ValueError, match="TeaCache"):
        _run(m, _inputs())
    m.disable_teacache()
    with pytest.raises(ValueError, match="TeaCache"):
        _run(m, _inputs(), teacache=TeaCacheConfig(2.5, (1.0,)))
    with pytest.raises(ValueError, match="TeaCache"):
        _run(m, _inputs(), teacache_measure=True)
    with pytest.raises(ValueError):
        m.enable_guidance_reuse(pair_every=0)
    with pytest.raises(ValueError):
        m.enable_guidance_reuse(interval=(0.5, 0.2))
    moved = _run(m, _inputs(), use_graph=True)  # (the enabled setting, no keyword)
    assert m.guidance_report["plan"] == [P, R, P, R, P, R] and not torch.equal(moved, plain_run)
    # an unguided call ignores the setting: the unguided loop's bits, no report
    unguided = _run(m, _inputs(), negative=False)
    assert m.guidance_report is None
    assert torch.equal(unguided, _run(_model(), _inputs(), negative=False))
    m.disable_guidance_reuse()
    for use_graph in (False, True):
        assert torch.equal(_run(m, _inputs(), use_graph=use_graph), plain_run)
        assert m.guidance_report is None
    # sharded tokens / CFG parallelism: refused before any forward
    m.enable_guidance_reuse()
    m._sp = types.SimpleNamespace(sharded=True, world=2, rank=0, capturable=False)
    with pytest.raises(NotImplementedError, match="guidance reuse"):
        _run(m, _inputs())
    m._sp = None
    m._cfgp = object()
    with pytest.raises(NotImplementedError, match="guidance reuse"):
        _run(m, _inputs())


def test_a_callback_that_replaces_an_embedding_forces_the_next_pair():
    m = _model()
    other = _dev(_inputs(seed=3))[2]
    seen = []

    def on_step_end(i, t, lat):
        seen.append(i)
        return {"prompt_embeds": other} if i == 2 else None

    _run(m, _inputs(), guidance_reuse=_cfg(3), on_step_end=on_step_end)
    assert seen == list(range(STEPS))
    assert m.guidance_report["plan"] == [P, R, R, P, R, R]  # step 3 was a pair anyway: the count restarts there
    m2 = _model()
    _run(m2, _inputs(), guidance_reuse=_cfg(3), on_step_end=lambda i, t, lat: {"prompt_embeds": other} if i == 0 else None)
    assert m2.guidance_report["plan"] == [P, P, R, R, P, R]
    # a callback that replaces the latents keeps the stored direction: the plan stands
    m3 = _model()
    out = _run(m3, _inputs(), guidance_reuse=_cfg(3), on_step_end=lambda i, t, lat: lat.clone())
    assert m3.guidance_report["plan"] == [P, R, R, P, R, R]
    assert torch.equal(out, _run(_model(), _inputs(), guidance_reuse=_cfg(3)))


def test_sequential_guidance_and_bf16_trajectory_run_eagerly():
    """denoise_step with batch_cfg=False: the pair is two forwards, then the store launch; trajectory_dtype = bfloat16 in every mode."""
    from chronoedit_amd.pipeline import denoise_step
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    m = _model()
    lat, cond, pr, ng, img = _dev(_inputs())
    lat = lat.float().contiguous()
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    sch.trajectory_dtype = BF
    sch.set_timesteps(3, device=lat.device)
    delta = torch.zeros(lat.shape, dtype=BF, device=lat.device)
    for i, kind in enumerate([P, R, O]):
        denoise_step(m, sch, lat, cond, sch.timesteps[i], pr, ng, img, G, batch_cfg=False, guidance_kind=kind, delta=delta)
        assert torch.isfinite(lat).all() and torch.equal(lat, lat.to(BF).float()), kind  # bf16 values in fp32 storage
    assert float(delta.float().abs().max()) > 0
    with pytest.raises(ValueError):
        denoise_step(m, sch, lat, cond, sch.timesteps[0], pr, ng, img, G, guidance_kind=R)  # no delta buffer


def test_fp8_gemms_replay_equals_eager():
    m = _model()
    m.enable_fp8_gemms(policy="fast")
    try:
        m.engine()
    except NotImplementedError as e:  # fp8 GEMMs need inner and ffn dims that are multiples of 256
        pytest.skip(str(e))
    outs = [_run(m, _inputs(), use_graph=g, guidance_reuse=_cfg(2)) for g in (False, True)]
    assert m.guidance_report["plan"] == [P, R, P, R, P, R]
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


# ----------------------------------------------------------------------------------------------------------------------------------
# the pipeline's switches and the measuring edit
# ----------------------------------------------------------------------------------------------------------------------------------
def _pipeline(m):
    from oracle import vae_oracle as V
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.vae import AutoencoderKLWan
    vp = V.make_synthetic_params(V.VAEConfig(dim=32, z_dim=16))
    vae = AutoencoderKLWan({k: v.cuda() for k, v in vp.items()}, dim=32, z_dim=16)
    return ChronoEditPipeline(vae=vae, transformer=m, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0))


def test_pipeline_switches_and_measurement():
    pipe = _pipeline(_model())
    m = pipe.transformer
    g = torch.Generator().manual_seed(0)
    image = (torch.rand(1, 3, 64, 96, generator=g) * 2 - 1).cuda().to(BF)
    lat0, _, pr, ng, img = _dev(_inputs())
    kw = dict(image=image, prompt_embeds=pr, negative_prompt_embeds=ng, image_embeds=img, num_frames=5, latents=lat0)

    def edit(**over):
        return pipe.edit_tensors(**dict(kw, latents=lat0.clone(), num_inference_steps=STEPS, guidance_scale=G, output_type="latent"), **over).clone()

    plain = edit()
    assert m.guidance_report is None  # off by default
    assert pipe.enable_guidance_reuse(pair_every=2) is pipe
    reused = edit()
    assert m.guidance_report["plan"] == [P, R, P, R, P, R] and not torch.equal(reused, plain)
    pipe.use_graph = False
    assert torch.equal(edit(), reused)
    pipe.use_graph = True
    pipe.enable_teacache(2.5, (1.0,))
    with pytest.raises(ValueError, match="TeaCache"):
        edit()
    pipe.disable_teacache()
    # measuring: every step a pair, the plain loop's latents, whatever is enabled
    res = pipe.measure_guidance_reuse([dict(kw, latents=lat0.clone())], STEPS, max_age=2, guidance_scale=G, keep_deltas=True)
    assert m._guidance_reuse is not None  # the setting is left as it was
    assert pipe.disable_guidance_reuse() is pipe
    assert torch.equal(edit(), plain)
    assert len(res) == 1
    r = res[0]
    assert torch.equal(r["latents"], plain)
    assert len(r["timesteps"]) == STEPS and len(r["rel_l2"]) == STEPS and len(r["deltas"]) == STEPS
    assert all(d.dtype == BF and tuple(d.shape) == tuple(lat0.shape) for d in r["deltas"])
    for i in range(STEPS):
        assert len(r["rel_l2"][i]) == 2
        for a in (1, 2):
            got = r["rel_l2"][i][a - 1]
            if i < a:
                assert math.isnan(got), (i, a, got)  # no direction of that age exists
                continue
            d_new, d_old = r["deltas"][i].double(), r["deltas"][i - a].double()
            want = math.sqrt(float(((d_new - d_old) ** 2).sum()) / float((d_new ** 2).sum()))
            print(f"measured step {i} age {a}: rel-L2 {got:.6e} (float64 from the kept directions {want:.6e})")
            assert math.isfinite(got) and abs(got - want) <= 1e-5 * want, (i, a, got, want)
    with pytest.raises(ValueError):
        pipe.measure_guidance_reuse([dict(kw, latents=lat0.clone())], STEPS, max_age=5)
