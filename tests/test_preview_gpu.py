"""Live previews in the loop and the pipeline (chronoedit_amd/preview.py, pipeline.denoise(preview=), ChronoEditPipeline.enable_preview).

Everything is bit-equal.  The previews of every step equal a SECOND implementation - an `on_step_end` hook that clones
`scheduler.model_outputs[-1]` and evaluates `preview.rgb_u8_reference` on the CPU - eager and under hipGraph replay; the returned latents
are those of the loop without previews; which steps are previewed, in which order and when; an interrupt; the temporal-reasoning
truncation; an explicit region, an auto region, a sparse plan, TeaCache, a tail of the schedule; refusals; the pipeline's switches and fit.
Shapes: the tiny model of tests/test_region_gpu.py (2 heads x 128, 2 layers, ffn 512), latents 1 x 16 x T x 8 x 12, 6 steps, guidance 5."""
import math
import types

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import preview as pv
from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
STEPS, G = 6, 5.0
H, W = 64, 96
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
_PARAMS = {}
FACTORS = torch.randn(17, 3, generator=torch.Generator().manual_seed(11)) * 0.2  # random, fixed


def _model(plain_rope=False):
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    if "p" not in _PARAMS:
        _PARAMS["p"] = D.make_synthetic_params(DCFG, dtype=BF)
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in _PARAMS["p"].items()})
    if plain_rope:
        m.rope_plain_temporal = True
    return m


def _inputs(T=2, seed=1):
    """bf16-representable (lat0, cond, prompt, negative, img, z_src) on the device."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    lat0, cond, pr, ng, img, z = r(1, 16, T, 8, 12), r(1, 20, T, 8, 12), r(1, 40, 128), r(1, 40, 128), r(1, 257, 64), r(1, 16, T, 8, 12)
    return lat0.cuda(), cond.cuda().to(BF), pr.cuda().to(BF), ng.cuda().to(BF), img.cuda().to(BF), z.cuda()


def _scheduler():
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    return FlowUniPCMultistepScheduler(flow_shift=5.0)


def grey_mask(seed=0):
    """uint8 [64, 96]: random bytes, one latent cell all 0, two all 255, one column of cells a ramp (tests/test_region_gpu.py)."""
    m = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8))
    m[:8, :8], m[8:16, 8:24] = 0, 255
    m[:, 40:48] = torch.linspace(0, 255, H).round().to(torch.uint8)[:, None]
    return m


def _loop(m, inp, options=None, use_graph=False, steps=STEPS, interrupt_behind=None, **kw):
    """`denoise`, with previews when `options` (PreviewConfig keywords) is given -> a namespace: latents, previews (the dicts, in the order
    they arrived), x0 (step -> a clone of the scheduler's x0 slot behind that step, taken in `on_step_end`), events (the order of
    ("step", i) and ("preview", i)), timesteps."""
    from chronoedit_amd.pipeline import denoise
    sch = _scheduler()
    out = types.SimpleNamespace(previews=[], x0={}, events=[], sch=sch)

    def on_preview(d):
        out.previews.append(d)
        out.events.append(("preview", d["step"]))
        return "ignored"

    def on_step_end(i, t, lat):
        out.x0[i] = sch.model_outputs[-1].clone()
        out.events.append(("step", i))

    cfg = None if options is None else pv.PreviewConfig(on_preview, **dict(dict(factors=FACTORS), **options))
    interrupted = None if interrupt_behind is None else (lambda: interrupt_behind in out.x0)
    out.latents = denoise(m, sch, inp[0].clone(), *inp[1:5], steps, G, use_graph=use_graph, on_step_end=on_step_end, interrupted=interrupted,
                          preview=cfg, **kw).clone()
    out.timesteps = [int(v) for v in sch.timesteps.tolist()]
    return out


def _bytes(d):
    assert isinstance(d["image"], Image.Image) and d["image"].mode == "RGB"
    return torch.from_numpy(np.asarray(d["image"]).copy())


def _want(x0, scale=2, frame=-1, w=None, z=None):
    if z is not None and z.shape[2] != x0.shape[2]:
        z = z[:, :, [0, -1]]  # sliced as the latents were
    return pv.rgb_u8_reference(x0.cpu(), FACTORS, scale, frame, None if w is None else w.cpu(), None if z is None else z.cpu())[0]


def _check_all(run, scale=2, frame=-1, w_of=lambda i: None, z=None, steps=None, first=0):
    steps = list(range(first, first + STEPS)) if steps is None else steps
    assert [d["step"] for d in run.previews] == steps, [d["step"] for d in run.previews]
    for d in run.previews:
        i = d["step"]
        w = w_of(i)
        want = _want(run.x0[i], scale, frame, w, z if w is not None else None)
        assert d["image"].size == (12 * scale, 8 * scale)
        assert torch.equal(_bytes(d), want), (i, int((_bytes(d) != want).sum()))
        assert d["timestep"] == run.timesteps[i - first]


@pytest.fixture(scope="module")
def plain():
    return _loop(_model(), _inputs())


@pytest.mark.parametrize("options", [dict(scale=2, lag=1), dict(scale=8, lag=0), dict(scale=1, lag=3), dict(scale=4, lag=1, frame=0)])
def test_every_step_equals_the_callback_reference_eager_and_replayed(plain, options):
    runs = []
    for use_graph in (False, True):
        run = _loop(_model(), _inputs(), options, use_graph=use_graph)
        _check_all(run, options["scale"], options.get("frame", -1))
        assert torch.equal(run.latents, plain.latents), use_graph  # a preview only reads the loop's state
        runs.append(run)
    assert all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(runs[0].previews, runs[1].previews))
    assert not torch.equal(_bytes(runs[0].previews[0]), _bytes(runs[0].previews[-1]))  # the picture moves with the steps
    # when they arrive: step i's preview once step i + lag is enqueued (so before that step's `on_step_end`), the rest before the return
    lag, ev = options["lag"], runs[0].events
    for i in range(STEPS):
        at = ev.index(("preview", i))
        if lag == 0:
            assert at < ev.index(("step", i))
        elif i + lag < STEPS:
            assert ev.index(("step", i + lag - 1)) < at < ev.index(("step", i + lag)), (i, ev)
        else:
            assert at > ev.index(("step", STEPS - 1)), (i, ev)


def test_every_nth_step_the_last_one_and_an_interrupt(plain):
    m = _model()
    for use_graph in (False, True):
        assert [d["step"] for d in _loop(m, _inputs(), dict(every=2), use_graph=use_graph).previews] == [1, 3, 5]
        run = _loop(m, _inputs(), dict(every=4, lag=2), use_graph=use_graph)
        _check_all(run, steps=[3, 5])
        assert torch.equal(run.latents, plain.latents)
        assert [d["step"] for d in _loop(m, _inputs(), dict(every=5), use_graph=use_graph).previews] == [4, 5]
        # interrupted() turns True behind step 2: steps 0..2 ran, and all their previews arrive although no later step is enqueued
        run = _loop(m, _inputs(), dict(lag=2), use_graph=use_graph, interrupt_behind=2)
        assert sorted(run.x0) == [0, 1, 2]
        _check_all(run, steps=[0, 1, 2])


@pytest.mark.parametrize("T, frame", [(8, -1), (8, 1)])
def test_temporal_reasoning_truncation(T, frame):
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    base = _loop(_model(), _inputs(T=T), **kw)
    for use_graph in (False, True):
        run = _loop(_model(), _inputs(T=T), dict(frame=frame), use_graph=use_graph, **kw)
        assert [run.x0[i].shape[2] for i in range(STEPS)] == [T, T, 2, 2, 2, 2]
        _check_all(run, frame=frame)  # frame -1: the last of 8, then the last of 2; frame 1: the second of 8, then the last of 2
        assert torch.equal(run.latents, base.latents)
    with pytest.raises(ValueError, match="frame"):
        _loop(_model(), _inputs(T=T), dict(frame=5), **kw)  # fits the 8 frames, not the 2 behind the truncation


def test_an_explicit_region_composites_the_kept_cells():
    from chronoedit_amd import region
    inp, mask = _inputs(), grey_mask()
    w = region.latent_weights(mask.cuda())
    z = inp[5]
    keep = (w == 0).cpu()
    assert int(keep.sum()) >= 1 and int((w == 1).sum()) >= 1
    src = _want(z, scale=1)  # the projected source latents
    base = _loop(_model(), inp, region=region.RegionConfig(w=w, z_src=z))
    for use_graph in (False, True):
        on = _loop(_model(), inp, dict(scale=1), use_graph=use_graph, region=region.RegionConfig(w=w, z_src=z))
        _check_all(on, scale=1, w_of=lambda i: w, z=z)
        assert all(torch.equal(_bytes(d)[keep], src[keep]) for d in on.previews)  # kept cells show the source
        off = _loop(_model(), inp, dict(scale=1, composite=False), use_graph=use_graph, region=region.RegionConfig(w=w, z_src=z))
        _check_all(off, scale=1)
        assert all(not torch.equal(_bytes(d)[keep], src[keep]) for d in off.previews)
        assert torch.equal(on.latents, base.latents) and torch.equal(off.latents, base.latents)
    _check_all(_loop(_model(), inp, dict(scale=4), use_graph=True, region=region.RegionConfig(w=w, z_src=z)), scale=4, w_of=lambda i: w, z=z)


K = 1
RECT = (slice(2, 4), slice(4, 6))  # latent rows 2..3, columns 4..5: one patch


def _source(x0):
    """z_src with exactly RECT for a region (tests/test_auto_region_gpu.py): x0 + 2 there on the last frame, x0 elsewhere."""
    z = x0.clone()
    z[:, :, -1, RECT[0], RECT[1]] += 2.0
    return z.contiguous()


def test_an_auto_region_is_plain_up_to_the_detection_and_composited_from_it_on(plain):
    from chronoedit_amd import auto_region as ar
    z = _source(plain.x0[K])
    for use_graph in (False, True):
        a = ar.AutoRegion(ar.AutoRegionConfig(K), z)
        m = _model()
        run = _loop(m, _inputs(), {}, use_graph=use_graph, auto_region=a)
        assert a.report["accepted"] and a.report["step"] == K
        w = a.report["w"]
        _check_all(run, w_of=lambda i: w if i >= K else None, z=z)
        # (at step k itself z_src is x0 outside the rectangle by construction; one step on, the kept cells visibly show the source)
        assert not torch.equal(_bytes(run.previews[K + 1]), _want(run.x0[K + 1]))
        b = ar.AutoRegion(ar.AutoRegionConfig(K), z)
        assert torch.equal(run.latents, _loop(_model(), _inputs(), auto_region=b).latents)


def test_a_sparse_plan_composites_even_with_composite_off(plain):
    from chronoedit_amd import auto_region as ar
    from chronoedit_amd.sparse_region import SparseRegionConfig
    z = _source(plain.x0[K])
    cfg = ar.AutoRegionConfig(K, dilate=0, feather=1)
    for use_graph in (False, True):
        a, m = ar.AutoRegion(cfg, z), _model()
        run = _loop(m, _inputs(), dict(composite=False), use_graph=use_graph, auto_region=a, sparse_region=SparseRegionConfig(2, margin=0))
        assert "sparse" in m.sparse_report["plan"] and a.report["accepted"]
        w = a.report["w"]
        _check_all(run, w_of=lambda i: w if i >= K else None, z=z)
        b = ar.AutoRegion(cfg, z)
        assert torch.equal(run.latents, _loop(_model(), _inputs(), auto_region=b, sparse_region=SparseRegionConfig(2, margin=0)).latents)


def test_teacache_skipped_steps_still_preview():
    from chronoedit_amd.teacache import TeaCacheConfig
    sch = _scheduler()
    sch.set_timesteps(STEPS, device="cuda:0")
    ratios = _model().teacache_ratios(sch.timesteps)
    tea = TeaCacheConfig(rel_l1_thresh=2.0 * max(ratios[1:STEPS - 1]), coefficients=(1.0, 0.0))
    base = _loop(_model(), _inputs(), teacache=tea)
    for use_graph in (False, True):
        m = _model()
        run = _loop(m, _inputs(), {}, use_graph=use_graph, teacache=tea)
        assert m.teacache_report["skipped"] >= 1
        _check_all(run)
        assert torch.equal(run.latents, base.latents)


def test_a_tail_of_the_schedule_reports_the_schedules_step_numbers():
    run = _loop(_model(), _inputs(), dict(every=2), start_step=2)
    assert sorted(run.x0) == [2, 3, 4, 5]
    _check_all(run, steps=[3, 5], first=2)  # tail steps 1 and 3: (i + 1) % 2 == 0 counts on the tail, the report on the schedule


def test_refusals():
    m = _model()
    with pytest.raises(ValueError, match="factors"):
        _loop(m, _inputs(), dict(factors=None))
    m._sp = types.SimpleNamespace(sharded=True, world=2, rank=0, capturable=False)
    with pytest.raises(NotImplementedError, match="preview"):
        _loop(m, _inputs(), {})
    m._sp = None
    m._cfgp = object()
    with pytest.raises(NotImplementedError, match="preview"):
        _loop(m, _inputs(), {})


# ----------------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe():
    from transformers import CLIPImageProcessor

    from chronoedit_amd.clip_vision import CLIPVisionModel
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    from chronoedit_amd.vae import AutoencoderKLWan
    from oracle import vae_oracle as V
    dcfg = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320, added_kv_proj_dim=256)
    dp = D.make_synthetic_params(dcfg, dtype=BF)
    vp = V.make_synthetic_params(V.VAEConfig(dim=32, z_dim=16))
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in dp.items()})
    vae = AutoencoderKLWan({k: v.cuda() for k, v in vp.items()}, dim=32, z_dim=16)
    torch.manual_seed(0)
    ie = CLIPVisionModel(hidden_size=320, intermediate_size=640, num_hidden_layers=3, num_attention_heads=4, image_size=56, patch_size=14, device="cuda:0")
    proc = CLIPImageProcessor(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})
    return ChronoEditPipeline(image_encoder=ie, image_processor=proc, transformer=m, vae=vae,
                              scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers"))


IMAGE = Image.fromarray(np.random.default_rng(9).integers(0, 256, (150, 203, 3), dtype=np.uint8))
PSTEPS = 3


def _call_kwargs(batch=1, seed=5, steps=PSTEPS):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=torch.randn(batch, 40, 128, generator=g).to(BF).cuda(), negative_prompt_embeds=torch.randn(batch, 40, 128, generator=g).to(BF).cuda(),
                height=H, width=W, num_frames=5, num_inference_steps=steps, guidance_scale=5.0,
                latents=torch.randn(batch, 16, 2, H // 8, W // 8, generator=g).to(BF).float())


def _call(pipe, kw, output_type="pil", image=IMAGE, **more):
    return pipe(image=image, **dict(kw, latents=kw["latents"].clone(), output_type=output_type), **more).frames


def _frames(frames):
    return np.stack([np.stack([np.asarray(f) for f in sample]) for sample in frames])


def test_pipeline_fit_on_the_loaded_vae(pipe, monkeypatch):
    assert pipe._preview is None and pipe.preview_factors is None
    with pytest.raises(ValueError, match="factors"):
        pipe.enable_preview(lambda d: None)
    seen, real = {}, pipe.preview_fit_tensors
    monkeypatch.setattr(pipe, "preview_fit_tensors", lambda *a, **k: seen.setdefault("zy", real(*a, **k)))
    images = [IMAGE, Image.fromarray(np.random.default_rng(3).integers(0, 256, (80, 120, 3), dtype=np.uint8))]
    factors = pipe.fit_preview_factors(images, height=H, width=W)
    z, y = seen["zy"]
    assert tuple(z.shape) == (2, 16, 1, H // 8, W // 8) and z.dtype == torch.float32 and tuple(y.shape) == (2, 3, H, W)
    assert factors is pipe.preview_factors and factors.dtype == torch.float32 and tuple(factors.shape) == (17, 3) and bool(torch.isfinite(factors).all())
    # the Gram matrix of those very tensors, on the CPU, within the summation bound n * 2^-52 * sum |terms| (tests/test_exact_preview_gpu.py)
    want = pv.gram_reference(z.cpu(), y.cpu(), 0)
    v = torch.cat([z[:, :, 0].cpu(), torch.ones(2, 1, H // 8, W // 8), pv.box_mean_reference(y.cpu())], dim=1).permute(0, 2, 3, 1).reshape(-1, 20).double()
    bound = v.shape[0] * 2.0 ** -52 * (v.abs().T @ v.abs())
    assert bool(((pipe.preview_fit_gram - want).abs() <= bound).all())
    got, report = pv.solve_factors(pipe.preview_fit_gram)
    assert torch.equal(got, factors) and report == pipe.preview_fit_report and set(report) == {"rms", "r2"}
    print("fit report on the synthetic VAE:", report)
    assert pipe.enable_preview(lambda d: None) is pipe and pipe.disable_preview() is pipe  # fitted: enabling needs no factors=
    for bad in (dict(every=0), dict(scale=3), dict(lag=-1), dict(factors=np.zeros((3, 17)))):
        with pytest.raises(ValueError):
            pipe.enable_preview(lambda d: None, **bad)
    assert pipe._preview is None


def test_pipeline_call_delivers_the_images_and_disable_restores_the_plain_call(pipe):
    pipe.preview_factors = None
    kw = _call_kwargs(batch=2, seed=6, steps=5)
    image = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (2, H, W, 3), dtype=np.uint8).astype(np.float32) / 255.0).permute(0, 3, 1, 2)
    embeds = torch.randn(2, 17, 320, generator=torch.Generator().manual_seed(7)).to(BF).cuda()
    plain = _frames(_call(pipe, kw, image=image, image_embeds=embeds))
    got = []
    pipe.enable_preview(got.append, every=2, scale=4, factors=FACTORS)
    try:
        assert np.array_equal(_frames(_call(pipe, kw, image=image, image_embeds=embeds)), plain)  # previews only read
        for b in range(2):
            mine = [d for d in got if d["sample"] == b]
            assert [d["step"] for d in mine] == [1, 3, 4] and len(mine) == math.ceil(5 / 2)
            assert all(d["image"].size == (W // 8 * 4, H // 8 * 4) and d["image"].mode == "RGB" and d["pass"] is None for d in mine)
        assert [d["sample"] for d in got] == [0] * 3 + [1] * 3
        # PIL in; the tensor-level edit honours the setting too
        del got[:]
        _call(pipe, _call_kwargs(steps=5))
        assert [(d["step"], d["sample"], d["pass"]) for d in got] == [(1, 0, None), (3, 0, None), (4, 0, None)]
        del got[:]
        from chronoedit_amd import image_io
        k1 = _call_kwargs(steps=5)
        pipe.edit_tensors(image_io.preprocess_pil(IMAGE, H, W, "cuda:0"), k1["prompt_embeds"], k1["negative_prompt_embeds"],
                          pipe.encode_image(IMAGE).to(BF), num_frames=5, num_inference_steps=5, latents=k1["latents"].clone(), output_type="latent")
        assert [d["step"] for d in got] == [1, 3, 4]
    finally:
        assert pipe.disable_preview() is pipe
    del got[:]
    assert np.array_equal(_frames(_call(pipe, kw, image=image, image_embeds=embeds)), plain) and not got


def test_an_auto_focused_call_tags_its_passes(pipe):
    kw = _call_kwargs()
    pipe.enable_auto_region(detect_step=0)
    try:
        _call(pipe, kw, "latent")
        dmax = float(pipe.auto_region_report["dmax"])
    finally:
        pipe.disable_auto_region()
    # a number threshold just under sqrt(dmax): only the top cell is a seed, a compact region (tests/test_autofocus_gpu.py)
    det = dict(detect_step=0, threshold=math.sqrt(dmax) * (1 - 1e-3), dilate=1, feather=1, max_area=1.0)
    pipe.enable_auto_region(**det).enable_auto_focus(0.0)
    try:
        plain = _frames(_call(pipe, kw))
        assert pipe.focus_report[0]["reason"] == "ok", pipe.focus_report
        got = []
        pipe.enable_preview(got.append, factors=FACTORS, lag=2)
        out = _frames(_call(pipe, kw))
        # the scout leaves behind step 0, its preview delivered at its exit; the focused pass runs the whole schedule on the crop
        assert [(d["pass"], d["step"]) for d in got] == [("scout", 0), ("focus", 0), ("focus", 1), ("focus", 2)]
        assert all(d["image"].size == (W // 8 * 2, H // 8 * 2) and d["sample"] == 0 for d in got)
        assert np.array_equal(out, plain)
    finally:
        pipe.disable_preview().disable_auto_region().disable_auto_focus()
