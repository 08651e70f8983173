"""Region-limited edits in the loop and the pipeline (chronoedit_amd/region.py, pipeline.denoise / GraphedDenoiser, ChronoEditPipeline).

Everything is bit-equal (torch.equal): an all-255 mask is the plain loop; an all-0 mask ends on z_src; a grey mask equals a SECOND
implementation - the plain `denoise` with an `on_step_end` callback that applies the torch expression and returns the latents - eager,
and hipGraph replay equals eager; the same with the temporal-reasoning truncation, a bf16 trajectory, TeaCache and guidance reuse (a
callback that replaces the latents changes neither's plan - both are functions of the schedule alone - so all four are held to the
callback loop); refusals; the pipeline's switch, paste-back and per-image masks.
Shapes: the tiny model of tests/test_guidance_reuse_gpu.py (2 heads x 128, 2 layers, ffn 512), latents 1 x 16 x T x 8 x 12, 6 steps."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
STEPS, G = 6, 5.0
H, W = 64, 96
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
_PARAMS = {}


def _model(plain_rope=False):
    """plain_rope: temporal RoPE indices 0..T-1 for any frame count (the DiffSynth call path's spelling); the default takes 2 or 8 frames only."""
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
    """bf16-representable (lat0, cond, prompt, negative, img, z_src) on the CPU in fp32."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    return r(1, 16, T, 8, 12), r(1, 20, T, 8, 12), r(1, 40, 128), r(1, 40, 128), r(1, 257, 64), r(1, 16, T, 8, 12)


def _dev(inp):
    lat0, cond, pr, ng, img, z = inp
    return lat0.cuda(), cond.cuda().to(BF), pr.cuda().to(BF), ng.cuda().to(BF), img.cuda().to(BF), z.cuda()


def grey_mask(seed=0):
    """uint8 [64, 96]: random bytes, one latent cell all 0, one all 255, one column of cells a ramp."""
    m = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8))
    m[:8, :8], m[8:16, 8:24] = 0, 255
    m[:, 40:48] = torch.linspace(0, 255, H).round().to(torch.uint8)[:, None]
    return m


def _config(mask_u8, z_src):
    from chronoedit_amd import region
    return region.RegionConfig(w=region.latent_weights(mask_u8.cuda()), z_src=z_src)


def _scheduler(bf16=False):
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    if bf16:
        sch.trajectory_dtype = BF
    return sch


def _run(m, inp, mask=None, use_graph=False, bf16=False, **kw):
    """`denoise` with the native region (mask given) or without."""
    from chronoedit_amd.pipeline import denoise
    lat0, cond, pr, ng, img, z = _dev(inp)
    region = None if mask is None else _config(mask, z)
    return denoise(m, _scheduler(bf16), lat0, cond, pr, ng, img, STEPS, G, use_graph=use_graph, region=region, **kw).clone()


def _callback_loop(m, inp, mask, bf16=False, **kw):
    """The second implementation: the plain loop, and the blend as torch operations in the public `on_step_end` hook."""
    from chronoedit_amd import region
    from chronoedit_amd.pipeline import denoise
    lat0, cond, pr, ng, img, z = _dev(inp)
    w = region.latent_weights(mask).cuda()  # (the CPU expression)
    sch = _scheduler(bf16)
    state = {"z": z, "e": lat0.float().clone()}

    def on_step_end(i, t, lat):
        if state["z"].shape[2] != lat.shape[2]:  # the truncation: sliced as the latents were
            state["z"], state["e"] = state["z"][:, :, [0, -1]], state["e"][:, :, [0, -1]]
        s = sch.sigmas[i + 1].to(lat.device)  # a device float
        k = (1.0 - s) * state["z"] + s * state["e"]
        out = w * lat + (1.0 - w) * k
        return out.to(BF).float() if bf16 else out

    return denoise(m, sch, lat0, cond, pr, ng, img, STEPS, G, on_step_end=on_step_end, **kw).clone()


@pytest.fixture()
def captures(monkeypatch):
    """Counts the hipGraph captures of the loop."""
    from chronoedit_amd import pipeline
    n, real = [], pipeline.GraphedDenoiser._capture
    monkeypatch.setattr(pipeline.GraphedDenoiser, "_capture", lambda self, kind="compute": (n.append((tuple(self.latents.shape), kind)), real(self, kind))[1])
    return n


@pytest.fixture(scope="module")
def plain_run():
    return _run(_model(), _inputs())


def test_all_255_mask_is_the_plain_loop(plain_run):
    mask = torch.full((H, W), 255, dtype=torch.uint8)
    m = _model()
    for use_graph in (False, True):
        out = _run(m, _inputs(), mask, use_graph=use_graph)
        assert torch.equal(out, plain_run), (use_graph, float((out - plain_run).abs().max()))


def test_all_0_mask_ends_on_the_source_latents():
    mask = torch.zeros((H, W), dtype=torch.uint8)
    m = _model()
    z = _inputs()[5].cuda()
    for use_graph in (False, True):
        out = _run(m, _inputs(), mask, use_graph=use_graph)
        assert torch.equal(out, z), (use_graph, float((out - z).abs().max()))


def test_grey_mask_equals_the_callback_loop_and_its_replay(plain_run, captures):
    mask = grey_mask()
    eager = _run(_model(), _inputs(), mask)
    want = _callback_loop(_model(), _inputs(), mask)
    assert torch.equal(eager, want), float((eager - want).abs().max())
    assert torch.isfinite(eager).all() and not torch.equal(eager, plain_run)
    # at the last step k == z_src: a kept cell holds the source latents, an edited cell something else
    z = _inputs()[5].cuda()
    assert torch.equal(eager[..., 0, 0], z[..., 0, 0]) and not torch.equal(eager[..., 1, 1], z[..., 1, 1])
    m2, warm = _model(), set()
    assert not captures
    replay = _run(m2, _inputs(), mask, use_graph=True, graph_warm=warm)
    assert torch.equal(replay, eager), float((replay - eager).abs().max())
    assert len(captures) <= 1, captures  # one kind of step: one graph serves every step, whatever its sigma
    # a second edit on the warm engine, another mask and other inputs; then the plain loop again: the region leaves nothing behind
    second, mask2 = _inputs(seed=2), grey_mask(seed=5)
    assert torch.equal(_run(m2, second, mask2, use_graph=True, graph_warm=warm), _run(_model(), second, mask2))
    assert torch.equal(_run(m2, _inputs(), use_graph=True, graph_warm=warm), plain_run)
    assert any(k[-1] for k in warm) and any(not k[-1] for k in warm)  # with and without a region are two warm shapes


VARIANTS = {
    # 3 latent frames truncated to 2 at step 2 (3 frames need the plain temporal RoPE), and the product's 8 -> 2 under the default RoPE
    "temporal-reasoning": dict(T=3, plain_rope=True, kw=dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2), graphs=2),
    "temporal-reasoning-8-frames": dict(T=8, kw=dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2), graphs=2),
    "bf16-trajectory": dict(T=2, bf16=True, kw={}, graphs=1),
    "teacache": dict(T=2, kw="teacache", graphs=2),
    "guidance-reuse": dict(T=2, kw="guidance", graphs=2),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variants_equal_the_callback_loop_and_their_replay(name, captures):
    v = VARIANTS[name]
    make = lambda: _model(plain_rope=v.get("plain_rope", False))
    kw = v["kw"]
    if kw == "teacache":
        from chronoedit_amd.teacache import TeaCacheConfig
        # the identity polynomial, at a threshold the first inner step's distance stays below: at least that step is skipped
        sch = _scheduler()
        sch.set_timesteps(STEPS, device="cuda:0")
        ratios = make().teacache_ratios(sch.timesteps)
        kw = dict(teacache=TeaCacheConfig(rel_l1_thresh=2.0 * max(ratios[1:STEPS - 1]), coefficients=(1.0, 0.0)))
    elif kw == "guidance":
        from chronoedit_amd.guidance import GuidanceReuseConfig
        kw = dict(guidance_reuse=GuidanceReuseConfig(pair_every=2))
    bf16 = v.get("bf16", False)
    inp, mask = _inputs(T=v["T"]), grey_mask(seed=3)
    m = make()
    eager = _run(m, inp, mask, bf16=bf16, **kw)
    if name == "teacache":
        assert m.teacache_report["skipped"] >= 1, m.teacache_report
    if name == "guidance-reuse":
        assert m.guidance_report["reuse"] >= 1, m.guidance_report
    plan = (getattr(m, "teacache_report", None) or {}).get("plan"), (getattr(m, "guidance_report", None) or {}).get("plan")
    m1 = make()
    want = _callback_loop(m1, inp, mask, bf16=bf16, **kw)
    # the callback's replaced latents change neither plan (both are made from the schedule before the first step)
    assert plan == ((getattr(m1, "teacache_report", None) or {}).get("plan"), (getattr(m1, "guidance_report", None) or {}).get("plan"))
    assert torch.equal(eager, want), (name, float((eager - want).abs().max()))
    assert eager.shape[2] == 2 and torch.isfinite(eager).all()
    if bf16:
        assert torch.equal(eager, eager.to(BF).float())
    assert not torch.equal(eager, _run(make(), inp, bf16=bf16, **kw))  # the region moved the result
    assert not captures
    replay = _run(make(), inp, mask, use_graph=True, bf16=bf16, **kw)
    assert torch.equal(replay, eager), (name, float((replay - eager).abs().max()))
    assert len(captures) <= v["graphs"] and len(set(captures)) == len(captures), captures  # one graph per kind of step (and latent shape)


def test_a_callback_that_replaces_the_latents_is_taken_as_it_is():
    """The replaced latents enter the next step unblended; that step's blend then runs on what it produced - eager and graphed alike."""
    mask, outs = grey_mask(), []
    for use_graph in (False, True):
        seen = []

        def on_step_end(i, t, lat):
            seen.append(lat.clone())
            return lat * 0.5 if i == 2 else None

        outs.append(_run(_model(), _inputs(), mask, use_graph=use_graph, on_step_end=on_step_end))
        assert len(seen) == STEPS
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0], _run(_model(), _inputs(), mask))


def test_sharded_and_cfg_parallel_transformers_are_refused():
    m = _model()
    m._sp = types.SimpleNamespace(sharded=True, world=2, rank=0, capturable=False)
    with pytest.raises(NotImplementedError, match="edit region"):
        _run(m, _inputs(), grey_mask())
    m._sp = None
    m._cfgp = object()
    with pytest.raises(NotImplementedError, match="edit region"):
        _run(m, _inputs(), grey_mask())


# ----------------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------------------------
def random_rgb(size, seed=0):
    w, h = size
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def frames_array(frames):
    return np.stack([np.stack([np.asarray(f) for f in sample]) for sample in frames])


def pipeline_mask(seed=0):
    """A 0 rectangle, a 255 rectangle, a ramp, noise elsewhere."""
    m = np.random.default_rng(seed).integers(1, 255, size=(H, W), dtype=np.uint8)
    m[4:30, 10:50] = 0
    m[36:60, 20:70] = 255
    m[:, 80:96] = np.linspace(0, 255, 16).round().astype(np.uint8)[None, :]
    return m


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
                height=H, width=W, num_frames=5, num_inference_steps=3, guidance_scale=5.0, latents=torch.randn(batch, 16, 2, H // 8, W // 8, generator=g).to(BF).float())  # (`__call__` takes the latents as bf16 values)


def test_pipeline_keeps_the_source_pixels_where_the_mask_is_0(pipe):
    image = Image.fromarray(random_rgb((90, 70), 9))
    source = np.asarray(image.convert("RGB").resize((W, H), Image.LANCZOS))
    mask = pipeline_mask()
    keep = mask == 0
    kw = _call_kwargs()
    call = lambda output_type="pil": pipe(image=image, **dict(kw, latents=kw["latents"].clone(), output_type=output_type)).frames
    # no region set: the state every later `clear_edit_region()` must restore
    plain = frames_array(call())
    plain_lat = call(output_type="latent")
    assert pipe.set_edit_region(Image.fromarray(mask)) is pipe
    out = {}
    for flag in (True, False):  # the device image path on and off
        pipe.enable_device_image_io(flag)
        out[flag] = frames_array(call())
    pipe.enable_device_image_io(True)
    frames = out[True]
    assert frames.shape == (1, 5, H, W, 3) and np.array_equal(out[True], out[False])
    for f in range(frames.shape[1]):
        assert np.array_equal(frames[0, f][keep], source[keep]), f  # the resized source's bytes, exactly, in every returned frame
    assert not np.array_equal(frames[0, -1][mask == 255], source[mask == 255])  # ... and an edit where the mask says so
    assert not np.array_equal(plain[0, -1][keep], source[keep])
    # the latent-space blend alone: the frames differ from the source there
    pipe.set_edit_region(mask, composite=False)  # (a numpy array this time)
    loose = frames_array(call())
    assert int((loose[0][:, keep] != source[keep][None]).sum()) >= 1
    assert not np.array_equal(loose, plain)
    # "latent": the blended latents - those of the tensor-level edit with the same mask
    lat = call(output_type="latent")
    from chronoedit_amd import image_io
    img = image_io.preprocess_pil(image, H, W, "cuda:0")
    want = pipe.edit_tensors(img, kw["prompt_embeds"], kw["negative_prompt_embeds"], pipe.encode_image(image).to(BF), num_frames=5,
                             num_inference_steps=3, guidance_scale=5.0, latents=kw["latents"].clone(), output_type="latent",
                             region_mask=torch.from_numpy(mask))
    assert lat.dtype == torch.float32 and torch.equal(lat, want) and not torch.equal(lat, plain_lat)
    # the tensor-level paste-back: a new fp32 video whose kept pixels are the source tensor's values
    video = pipe.edit_tensors(img, kw["prompt_embeds"], kw["negative_prompt_embeds"], pipe.encode_image(image).to(BF), num_frames=5,
                              num_inference_steps=3, guidance_scale=5.0, latents=kw["latents"].clone(), region_mask=torch.from_numpy(mask))
    assert video.dtype == torch.float32 and tuple(video.shape) == (1, 3, 5, H, W)
    k5 = torch.from_numpy(keep).cuda().expand(1, 3, 5, H, W)
    assert torch.equal(video[k5], img.float().unsqueeze(2).expand(1, 3, 5, H, W)[k5])
    # cleared: the first run's bits again
    assert pipe.clear_edit_region() is pipe
    assert np.array_equal(frames_array(call()), plain) and torch.equal(call(output_type="latent"), plain_lat)


def test_pipeline_gives_each_image_its_own_mask(pipe):
    """Two images as one tensor (`check_inputs` takes a tensor or ONE PIL image), two masks, "pil" out."""
    rgb = np.stack([random_rgb((W, H), 11), random_rgb((W, H), 12)])
    image = torch.from_numpy(rgb.astype(np.float32) / 255.0).permute(0, 3, 1, 2)  # [2, 3, H, W] in [0, 1]
    masks = [pipeline_mask(1), np.ascontiguousarray(pipeline_mask(2)[::-1, ::-1])]
    kw = _call_kwargs(batch=2, seed=6)
    g = torch.Generator().manual_seed(7)
    embeds = torch.randn(2, 17, 320, generator=g).to(BF).cuda()
    call = lambda: frames_array(pipe(image=image, image_embeds=embeds, **dict(kw, latents=kw["latents"].clone(), output_type="pil")).frames)
    try:
        pipe.set_edit_region(masks)
        frames = call()
        assert frames.shape == (2, 5, H, W, 3)
        for b in range(2):
            keep = masks[b] == 0
            for f in range(5):
                assert np.array_equal(frames[b, f][keep], rgb[b][keep]), (b, f)
            other = (masks[1 - b] == 0) & (masks[b] == 255)  # kept by the OTHER mask only: edited here
            assert other.any() and not np.array_equal(frames[b, -1][other], rgb[b][other]), b
        pipe.set_edit_region(masks[:1] * 3)
        with pytest.raises(ValueError, match="masks"):
            call()
        pipe.set_edit_region(np.zeros((H, W + 8), dtype=np.uint8))
        with pytest.raises(ValueError):
            call()
        pipe.set_edit_region(masks[0])  # ONE mask: every image's
        frames = call()
        for b in range(2):
            assert np.array_equal(frames[b, 0][masks[0] == 0], rgb[b][masks[0] == 0]), b
    finally:
        pipe.clear_edit_region()
