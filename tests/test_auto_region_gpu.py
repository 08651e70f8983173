"""Automatic edit regions in the loop and the pipeline (chronoedit_amd/auto_region.py, pipeline.denoise(auto_region=), ChronoEditPipeline).

Random source latents have no region, so the inputs are made to have one: the plain loop runs once, x0 = scheduler.model_outputs[-1] is
taken behind step k, and z_src = x0 + 2.0 on a rectangle of last-frame cells, z_src = x0 everywhere else.  The change map is then exactly 0
outside the rectangle and about 4 inside, and both threshold forms give exactly the rectangle as the seed set - checked first, on the CPU
expression.  Everything else is bit-equal (torch.equal): the auto edit equals a SECOND implementation - the plain `denoise` with an
`on_step_end` hook that computes w at step k with the CPU expressions and applies the blend as torch operations from there on - and
hipGraph replay equals eager; a declined edit is the plain loop; an explicit mask wins; temporal reasoning; sparse steps; TeaCache; refusals;
the pipeline's switch, report, paste-back, per-image regions and the measure entry.
Shapes: the tiny model of tests/test_region_gpu.py (2 heads x 128, 2 layers, ffn 512), latents 1 x 16 x T x 8 x 12, 6 steps."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import auto_region as ar
from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
STEPS, G, K = 6, 5.0, 1
H, W = 64, 96
RECT = (slice(2, 4), slice(4, 6))    # latent rows 2..3, columns 4..5: one patch
RECT2 = (slice(4, 8), slice(8, 12))  # the lower right corner: four patches
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
_PARAMS = {}


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
    """bf16-representable (lat0, cond, prompt, negative, img) on the device (`denoise` works in place on fp32 latents: the callers below
    hand it a copy)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    lat0, cond, pr, ng, img = r(1, 16, T, 8, 12), r(1, 20, T, 8, 12), r(1, 40, 128), r(1, 40, 128), r(1, 257, 64)
    return lat0.cuda(), cond.cuda().to(BF), pr.cuda().to(BF), ng.cuda().to(BF), img.cuda().to(BF)


def _scheduler():
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    return FlowUniPCMultistepScheduler(flow_shift=5.0)


def _plain(m, inp, k=None, use_graph=False, **kw):
    """The plain loop -> (latents, x0 behind step k)."""
    from chronoedit_amd.pipeline import denoise
    sch, seen = _scheduler(), {}

    def on_step_end(i, t, lat):
        if i == k:
            seen["x0"] = sch.model_outputs[-1].clone()

    out = denoise(m, sch, inp[0].clone(), *inp[1:], STEPS, G, use_graph=use_graph, on_step_end=None if k is None else on_step_end, **kw).clone()
    return out, seen.get("x0")


def _source(x0, rect=RECT, T=None):
    """z_src with exactly `rect` for a region: x0 + 2 there on the last frame, x0 elsewhere.  T: that many frames, the first and the last
    those of x0 (what the truncation keeps), random ones between."""
    z = x0.clone()
    if rect is not None:
        z[:, :, -1, rect[0], rect[1]] += 2.0
    if T is not None and T != z.shape[2]:
        mid = torch.randn(z.shape[0], z.shape[1], T - 2, *z.shape[3:], generator=torch.Generator().manual_seed(8)).cuda()
        z = torch.cat([z[:, :, :1], mid, z[:, :, -1:]], dim=2)
    return z.contiguous()


def _rect_mask(rect=RECT):
    m = torch.zeros(8, 12, dtype=torch.bool)
    m[rect] = True
    return m


def _auto(m, inp, z, cfg, use_graph=False, **kw):
    """`denoise` with the detector -> (latents, the AutoRegion the loop filled in)."""
    from chronoedit_amd.pipeline import denoise
    a = ar.AutoRegion(cfg, z)
    return denoise(m, _scheduler(), inp[0].clone(), *inp[1:], STEPS, G, use_graph=use_graph, auto_region=a, **kw).clone(), a


def _callback_loop(m, inp, z, cfg, k=K, **kw):
    """The second implementation: the plain loop; behind step k the hook computes w from the scheduler's x0 slot with the CPU expressions,
    and from step k on it applies the blend as torch operations."""
    from chronoedit_amd.pipeline import denoise
    sch = _scheduler()
    state = {"z": z, "e": inp[0].float().clone(), "w": None}

    def on_step_end(i, t, lat):
        if state["z"].shape[2] != lat.shape[2]:  # the truncation: sliced as the latents were
            state["z"], state["e"] = state["z"][:, :, [0, -1]], state["e"][:, :, [0, -1]]
        if i == k:
            _, _, _, w = ar.weights(sch.model_outputs[-1].cpu(), state["z"].cpu(), cfg)
            if ar.decide(w, cfg)[0]:
                state["w"] = w.cuda()
        if state["w"] is None:
            return None
        s = sch.sigmas[i + 1].to(lat.device)
        kk = (1.0 - s) * state["z"] + s * state["e"]
        return state["w"] * lat + (1.0 - state["w"]) * kk

    return denoise(m, sch, inp[0].clone(), *inp[1:], STEPS, G, on_step_end=on_step_end, **kw).clone()


@pytest.fixture()
def captures(monkeypatch):
    """Records the hipGraph captures of the loop."""
    from chronoedit_amd import pipeline
    n, real = [], pipeline.GraphedDenoiser._capture
    monkeypatch.setattr(pipeline.GraphedDenoiser, "_capture", lambda self, kind="compute": (n.append((tuple(self.latents.shape), kind, self.region is not None)), real(self, kind))[1])
    return n


@pytest.fixture(scope="module")
def base():
    """The plain run and x0 behind step K, computed once and left unchanged."""
    out, x0 = _plain(_model(), _inputs(), K)
    return types.SimpleNamespace(plain=out, x0=x0)


CFGS = {"otsu": ar.AutoRegionConfig(K), "number": ar.AutoRegionConfig(K, threshold=1.0, dilate=0, feather=2)}


def test_the_input_has_exactly_the_rectangle_for_a_region(base):
    z = _source(base.x0)
    for name, cfg in CFGS.items():
        d, thr, dmax, w = ar.weights(base.x0.cpu(), z.cpu(), cfg)
        assert torch.equal(d > thr, _rect_mask()), name
        assert bool((d[~_rect_mask()] == 0).all()) and 3.9 < float(dmax) < 4.1
        assert ar.decide(w, cfg)[0], name


@pytest.mark.parametrize("name", list(CFGS))
def test_the_auto_edit_equals_the_callback_loop_and_its_replay(name, base, captures):
    cfg, z, inp = CFGS[name], _source(base.x0), _inputs()
    m = _model()
    eager, a = _auto(m, inp, z, cfg)
    want = _callback_loop(_model(), inp, z, cfg)
    assert torch.equal(eager, want), float((eager - want).abs().max())
    assert torch.isfinite(eager).all() and not torch.equal(eager, base.plain)
    # the report: on the transformer and on the request, with the CPU expression's w and its pixel mask
    rep = m.auto_region_report
    _, thr, dmax, w = ar.weights(base.x0.cpu(), z.cpu(), cfg)
    assert rep is a.report and rep["accepted"] and rep["reason"] == "accepted" and rep["step"] == K
    assert rep["threshold"] == float(thr) and rep["dmax"] == float(dmax) and rep["active_fraction"] == ar.decide(w, cfg)[2]
    assert torch.equal(rep["w"], w) and np.array_equal(np.asarray(rep["mask"]), ar.pixel_mask(w).numpy())
    assert torch.equal(a.mask_u8.cpu(), ar.pixel_mask(w))
    # at the last step the blend's k is z_src: a kept cell holds the source latents, an edited cell something else
    keep = (w == 0).cuda()
    assert bool(keep.any()) and torch.equal(eager[..., keep], z[..., keep]) and not torch.equal(eager[..., ~keep], z[..., ~keep])
    assert not captures
    m2 = _model()
    replay, _ = _auto(m2, inp, z, cfg, use_graph=True)
    assert torch.equal(replay, eager), float((replay - eager).abs().max())
    # at most one graph before the detection (no region) and one per kind of step behind it
    assert len(captures) <= 2 and len(set(captures)) == len(captures) and [c[2] for c in captures] == sorted(c[2] for c in captures), captures
    assert torch.equal(m2.auto_region_report["w"], w)


def test_a_declined_edit_is_the_plain_loop_and_says_why(base):
    inp = _inputs()
    for use_graph in (False, True):
        # z_src == x0: nothing changed anywhere, the threshold is +inf
        m = _model()
        out, a = _auto(m, inp, _source(base.x0, rect=None), CFGS["otsu"], use_graph=use_graph)
        assert torch.equal(out, base.plain), use_graph
        rep = m.auto_region_report
        assert not rep["accepted"] and rep["reason"] == "empty" and rep["threshold"] == float("inf") and rep["dmax"] == 0.0
        assert rep["active_fraction"] == 0.0 and not bool(rep["w"].any()) and a.mask_u8 is None and rep["step"] == K
        # the rectangle with its rim covers 9 of 24 patches: over max_area = 0.25
        m = _model()
        out, a = _auto(m, inp, _source(base.x0), ar.AutoRegionConfig(K, max_area=0.25), use_graph=use_graph)
        assert torch.equal(out, base.plain), use_graph
        rep = m.auto_region_report
        assert not rep["accepted"] and rep["reason"] == "max_area" and rep["active_fraction"] == 9 / 24 and a.mask_u8 is None
    # a detect_step past the last step: nothing is detected, and there is no report
    m = _model()
    out, a = _auto(m, inp, _source(base.x0), ar.AutoRegionConfig(STEPS))
    assert torch.equal(out, base.plain) and m.auto_region_report is None and a.report is None


def test_an_explicit_mask_overrides_the_detector(base):
    from chronoedit_amd import region
    inp, z = _inputs(), _source(base.x0)
    mask = torch.zeros((H, W), dtype=torch.uint8)
    mask[40:64, 0:40] = 255
    explicit = lambda: region.RegionConfig(w=region.latent_weights(mask.cuda()), z_src=z)
    from chronoedit_amd.pipeline import denoise
    want = denoise(_model(), _scheduler(), inp[0].clone(), *inp[1:], STEPS, G, region=explicit()).clone()
    m = _model()
    out, a = _auto(m, inp, z, CFGS["otsu"], region=explicit())
    assert torch.equal(out, want) and m.auto_region_report is None and a.report is None and a.mask_u8 is None
    assert not torch.equal(out, _auto(_model(), inp, z, CFGS["otsu"])[0])


def test_with_temporal_reasoning_the_detection_follows_the_first_two_frame_step(captures):
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    inp = _inputs(T=3)
    make = lambda: _model(plain_rope=True)  # (3 frames need the plain temporal RoPE)
    plain, x0 = _plain(make(), inp, 2, **kw)
    assert x0.shape[2] == 2
    z = _source(x0, T=3)
    cfg = ar.AutoRegionConfig(1)  # in front of the truncation: the detection waits for step 2
    d, thr, _, w = ar.weights(x0.cpu(), z[:, :, [0, -1]].cpu(), cfg)
    assert torch.equal(d > thr, _rect_mask())
    m = make()
    eager, _ = _auto(m, inp, z, cfg, **kw)
    assert m.auto_region_report["step"] == 2 and m.auto_region_report["accepted"] and torch.equal(m.auto_region_report["w"], w)
    want = _callback_loop(make(), inp, z, cfg, k=2, **kw)
    assert eager.shape[2] == 2 and torch.equal(eager, want) and not torch.equal(eager, plain)
    assert not captures
    replay, _ = _auto(make(), inp, z, cfg, use_graph=True, **kw)
    assert torch.equal(replay, eager)
    assert len(captures) <= 3 and len(set(captures)) == len(captures), captures  # 3 frames, 2 frames, 2 frames with the region


# ----------------------------------------------------------------------------------------------------------------------------------
# sparse steps behind the detection
# ----------------------------------------------------------------------------------------------------------------------------------
def S(*a, **kw):
    from chronoedit_amd.sparse_region import SparseRegionConfig
    return SparseRegionConfig(*a, **kw)


SPARSE_CFG = ar.AutoRegionConfig(K, dilate=0, feather=1)  # w > 0 on 4 x 4 cells: 9 patches of 24


def test_sparse_refresh_every_1_is_the_dense_auto_edit(base):
    inp, z = _inputs(), _source(base.x0)
    dense, _ = _auto(_model(), inp, z, SPARSE_CFG)
    for use_graph in (False, True):
        m = _model()
        out, _ = _auto(m, inp, z, SPARSE_CFG, use_graph=use_graph, sparse_region=S(1, margin=0))
        assert torch.equal(out, dense), use_graph
        assert m.sparse_report["plan"] == ["compute"] * STEPS and m.auto_region_report["accepted"]


def test_sparse_plan_kept_cells_replay_second_edit_and_disable(base, captures):
    from chronoedit_amd import sparse_region
    inp, z = _inputs(), _source(base.x0)
    _, _, _, w = ar.weights(base.x0.cpu(), z.cpu(), SPARSE_CFG)
    m = _model()
    eager, _ = _auto(m, inp, z, SPARSE_CFG, sparse_region=S(2, margin=0))
    rep = m.sparse_report
    assert rep["plan"] == ["compute"] * (K + 1) + ["refresh", "sparse"] * 2, rep  # dense through k, the first refresh at k + 1
    ids = sparse_region.active_tokens(w, 2, 0)[0]
    assert rep["active"] == ids.numel() == 24 and rep["tokens"] == 48 and torch.equal(m.engine()._sparse.ids.cpu().long(), ids)
    keep = (w == 0).cuda()
    assert torch.isfinite(eager).all() and torch.equal(eager[..., keep], z[..., keep]) and not torch.equal(eager[..., ~keep], z[..., ~keep])
    assert not torch.equal(eager, _auto(_model(), inp, z, SPARSE_CFG)[0])  # sparse steps are another computation than dense ones
    assert not captures
    replay, _ = _auto(_model(), inp, z, SPARSE_CFG, use_graph=True, sparse_region=S(2, margin=0))
    assert torch.equal(replay, eager), float((replay - eager).abs().max())
    assert len(set(captures)) == len(captures) and len(captures) <= 3, captures  # compute in front; refresh and sparse behind
    assert [c[1] for c in captures if not c[2]] in ([], ["compute"]) and {c[1] for c in captures if c[2]} <= {"refresh", "sparse"}, captures
    # the sparse margin counts in the decision: 20 of 24 patches with margin 1 is over max_area
    m3 = _model()
    out, _ = _auto(m3, inp, z, SPARSE_CFG, sparse_region=S(2, margin=1))
    assert torch.equal(out, base.plain) and m3.auto_region_report["reason"] == "max_area" and m3.auto_region_report["active_fraction"] == 20 / 24
    assert m3.sparse_report is None
    # the transformer-level switches; a second edit on the same engine detects its own region
    m.enable_sparse_region(2, margin=0)
    assert m.enable_auto_region(K, dilate=0, feather=1) is m
    z2 = _source(base.x0, RECT2)
    second, a2 = _auto(m, inp, z2, None, use_graph=True)
    _, _, _, w2 = ar.weights(base.x0.cpu(), z2.cpu(), SPARSE_CFG)
    assert torch.equal(a2.report["w"], w2) and not torch.equal(w2, w)
    assert torch.equal(m.engine()._sparse.ids.cpu().long(), sparse_region.active_tokens(w2, 2, 0)[0])
    assert torch.equal(second, _auto(_model(), inp, z2, SPARSE_CFG, sparse_region=S(2, margin=0))[0])
    keep2 = (w2 == 0).cuda()
    assert torch.equal(second[..., keep2], z2[..., keep2])
    # switched off: the plain loop again, and no report
    assert m.disable_auto_region() is m
    out, a3 = _auto(m, inp, z2, None, use_graph=True)
    assert torch.equal(out, base.plain) and m.auto_region_report is None and a3.report is None and m.sparse_report is None


def test_teacache_composes_as_with_an_explicit_region():
    from chronoedit_amd.teacache import TeaCacheConfig
    inp, cfg = _inputs(), CFGS["otsu"]
    sch = _scheduler()
    sch.set_timesteps(STEPS, device="cuda:0")
    ratios = _model().teacache_ratios(sch.timesteps)
    # the identity polynomial, at a threshold the first inner step's distance stays below: at least that step is skipped
    kw = dict(teacache=TeaCacheConfig(rel_l1_thresh=2.0 * max(ratios[1:STEPS - 1]), coefficients=(1.0, 0.0)))
    plain, x0 = _plain(_model(), inp, K, **kw)
    z = _source(x0)  # (TeaCache moves step K's estimate: the region is built on ITS x0)
    d, thr, _, _ = ar.weights(x0.cpu(), z.cpu(), cfg)
    assert torch.equal(d > thr, _rect_mask())
    m = _model()
    eager, _ = _auto(m, inp, z, cfg, **kw)
    assert m.teacache_report["skipped"] >= 1 and m.auto_region_report["accepted"]
    want = _callback_loop(_model(), inp, z, cfg, **kw)
    assert torch.equal(eager, want) and not torch.equal(eager, plain)


def test_refusals(base):
    from chronoedit_amd.guidance import GuidanceReuseConfig
    from chronoedit_amd.teacache import TeaCacheConfig
    inp, z, cfg = _inputs(), _source(base.x0), CFGS["otsu"]
    m = _model()
    m._sp = types.SimpleNamespace(sharded=True, world=2, rank=0, capturable=False)
    with pytest.raises(NotImplementedError, match="edit region"):
        _auto(m, inp, z, cfg)
    m._sp, m._cfgp = None, object()
    with pytest.raises(NotImplementedError, match="edit region"):
        _auto(m, inp, z, cfg)
    for kw in (dict(teacache=TeaCacheConfig(rel_l1_thresh=0.1, coefficients=(1.0, 0.0))), dict(guidance_reuse=GuidanceReuseConfig(pair_every=2))):
        with pytest.raises(ValueError):
            _auto(_model(), inp, z, cfg, sparse_region=S(2), **kw)
    with pytest.raises(ValueError, match="shape"):
        _auto(_model(), inp, z[:, :, :1], cfg)
    with pytest.raises(ValueError):
        _model().enable_auto_region(1, dilate=5, feather=4)


# ----------------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------------------------
def frames_array(frames):
    return np.stack([np.stack([np.asarray(f) for f in sample]) for sample in frames])


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


def _call_kwargs(batch=1, seed=5):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=torch.randn(batch, 40, 128, generator=g).to(BF).cuda(), negative_prompt_embeds=torch.randn(batch, 40, 128, generator=g).to(BF).cuda(),
                height=H, width=W, num_frames=5, num_inference_steps=3, guidance_scale=5.0, latents=torch.randn(batch, 16, 2, H // 8, W // 8, generator=g).to(BF).float())


# On synthetic weights the change map is noise; Otsu's threshold still splits it (some cell lies above it, some cell below: 0 < w0 < N), so
# with no dilation and no feather the mask holds both 0 and 255, and max_area = 1 accepts whatever it is.
PIPE_OPTIONS = dict(detect_step=0, dilate=0, feather=0, max_area=1.0)


def test_pipeline_pil_in_pil_out_keeps_the_source_where_the_reported_mask_is_0(pipe):
    image = Image.fromarray(np.random.default_rng(9).integers(0, 256, size=(70, 90, 3), dtype=np.uint8))
    source = np.asarray(image.convert("RGB").resize((W, H), Image.LANCZOS))
    kw = _call_kwargs()
    call = lambda output_type="pil": pipe(image=image, **dict(kw, latents=kw["latents"].clone(), output_type=output_type)).frames
    try:
        plain, plain_lat = frames_array(call()), call("latent")
        assert pipe.auto_region_report is None
        assert pipe.enable_auto_region(**PIPE_OPTIONS) is pipe
        frames = frames_array(call())
        rep = pipe.auto_region_report
        assert rep is pipe.transformer.auto_region_report and rep["accepted"] and rep["step"] == 0
        mask = np.asarray(rep["mask"])
        assert rep["mask"].mode == "L" and mask.shape == (H, W) and set(np.unique(mask)) == {0, 255}
        keep = mask == 0
        for f in range(frames.shape[1]):
            assert np.array_equal(frames[0, f][keep], source[keep]), f  # the resized source's bytes, exactly, in every returned frame
        assert not np.array_equal(frames[0, -1][~keep], source[~keep]) and not np.array_equal(plain[0, -1][keep], source[keep])
        auto_lat = call("latent")
        assert not torch.equal(auto_lat, plain_lat)
        # composite=False: the latent-space blend alone
        pipe.enable_auto_region(**dict(PIPE_OPTIONS, composite=False))
        loose = frames_array(call())
        assert int((loose[0][:, keep] != source[keep][None]).sum()) >= 1 and torch.equal(call("latent"), auto_lat)
        # the reported mask, handed back as an explicit region: accepted, it wins, and there is no report
        pipe.set_edit_region(rep["mask"])
        again = frames_array(call())
        assert pipe.auto_region_report is None and pipe.transformer.auto_region_report is None
        for f in range(again.shape[1]):
            assert np.array_equal(again[0, f][keep], source[keep]), f
        pipe.clear_edit_region()
        # a region nobody accepts: the plain frames, bit for bit, and the report says why
        pipe.enable_auto_region(**dict(PIPE_OPTIONS, max_area=1e-3))
        assert np.array_equal(frames_array(call()), plain) and pipe.auto_region_report["reason"] == "max_area"
        assert pipe.disable_auto_region() is pipe
        assert np.array_equal(frames_array(call()), plain) and torch.equal(call("latent"), plain_lat) and pipe.auto_region_report is None
    finally:
        pipe.disable_auto_region()
        pipe.clear_edit_region()


def test_pipeline_gives_each_image_of_a_batch_its_own_region(pipe):
    rgb = np.stack([np.random.default_rng(s).integers(0, 256, size=(H, W, 3), dtype=np.uint8) for s in (11, 12)])
    image = torch.from_numpy(rgb.astype(np.float32) / 255.0).permute(0, 3, 1, 2)  # [2, 3, H, W] in [0, 1]
    kw = _call_kwargs(batch=2, seed=6)
    embeds = torch.randn(2, 17, 320, generator=torch.Generator().manual_seed(7)).to(BF).cuda()
    try:
        pipe.enable_auto_region(**PIPE_OPTIONS)
        frames = frames_array(pipe(image=image, image_embeds=embeds, **dict(kw, output_type="pil")).frames)
        reps = pipe.auto_region_report
        assert isinstance(reps, list) and len(reps) == 2 and all(r["accepted"] for r in reps)
        masks = [np.asarray(r["mask"]) for r in reps]
        assert not np.array_equal(masks[0], masks[1])
        for b in range(2):
            keep = masks[b] == 0
            assert keep.any() and not keep.all()
            for f in range(frames.shape[1]):
                assert np.array_equal(frames[b, f][keep], rgb[b][keep]), (b, f)
    finally:
        pipe.disable_auto_region()


def test_measure_auto_region_leaves_the_plain_latents_and_returns_a_row_per_step(pipe):
    image = Image.fromarray(np.random.default_rng(9).integers(0, 256, size=(70, 90, 3), dtype=np.uint8))
    kw = _call_kwargs()
    plain_lat = pipe(image=image, **dict(kw, latents=kw["latents"].clone(), output_type="latent")).frames
    edit = dict(image=image, **{k: v for k, v in kw.items() if k not in ("num_inference_steps", "guidance_scale")})
    for options in (dict(), dict(threshold=0.5)):
        res = pipe.measure_auto_region([dict(edit, latents=kw["latents"].clone())], 3, guidance_scale=5.0, **options)
        assert len(res) == 1 and torch.equal(res[0]["latents"], plain_lat)
        rows = res[0]["steps"]
        assert [r["step"] for r in rows] == [0, 1, 2] and len(res[0]["timesteps"]) == 3 and rows[-1]["iou"] == 1.0
        assert all(0.0 <= r["iou"] <= 1.0 and 0.0 <= r["active_fraction"] <= 1.0 and r["threshold"] > 0 for r in rows)
        if options:
            assert all(r["threshold"] == 0.25 for r in rows)
    assert pipe.transformer._auto_region is None and pipe.auto_region_report is None
