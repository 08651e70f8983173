"""Auto-focused edits through `ChronoEditPipeline.__call__`: the scout finds the region on the whole photo, the focused pass edits its crop and
pastes it back at the photo's size - bit for bit the explicit-mask focused call (cold start), a second implementation built from the
public pieces (warm start), or the plain auto-region call (fallbacks)."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import autofocus, focus, region

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H = 96, 64
BF = torch.bfloat16
STEPS, K = 3, 0  # the detection follows step 0: the warm start's tail is steps 1 and 2
CONTEXT = 0.0
FLOW_SHIFT = 5.0


@pytest.fixture(scope="module")
def pipe():
    from transformers import CLIPImageProcessor

    from chronoedit_amd.clip_vision import CLIPVisionModel
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    from chronoedit_amd.vae import AutoencoderKLWan
    from oracle import dit_oracle as D
    from oracle import vae_oracle as V
    dcfg = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320, added_kv_proj_dim=256)
    dp = D.make_synthetic_params(dcfg, dtype=BF)
    vp = V.make_synthetic_params(V.VAEConfig(dim=32, z_dim=16))
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320,
                                     added_kv_proj_dim=256, device=DEV)
    m.load_synthetic_({k: v.cuda() for k, v in dp.items()})
    vae = AutoencoderKLWan({k: v.cuda() for k, v in vp.items()}, dim=32, z_dim=16)
    torch.manual_seed(0)
    ie = CLIPVisionModel(hidden_size=320, intermediate_size=640, num_hidden_layers=3, num_attention_heads=4, image_size=56, patch_size=14, device=DEV)
    proc = CLIPImageProcessor(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})
    return ChronoEditPipeline(image_encoder=ie, image_processor=proc, transformer=m, vae=vae,
                              scheduler=FlowUniPCMultistepScheduler(flow_shift=FLOW_SHIFT, sigma_grid="diffusers"))


IMAGE = Image.fromarray(np.random.default_rng(9).integers(0, 256, (150, 203, 3), dtype=np.uint8))


def inputs(n=1, frames=5, steps=STEPS, seed=5):
    g = torch.Generator().manual_seed(seed)
    T = (frames - 1) // 4 + 1
    return dict(prompt_embeds=torch.randn(n, 40, 128, generator=g).to(BF).cuda(), negative_prompt_embeds=torch.randn(n, 40, 128, generator=g).to(BF).cuda(),
                height=H, width=W, num_frames=frames, num_inference_steps=steps, guidance_scale=5.0,
                latents=torch.randn(n, 16, T, H // 8, W // 8, generator=g).to(BF).float())


def call(pipe, image, kw, output_type="pil", **more):
    return pipe(image=image, **dict(kw, latents=kw["latents"].clone(), output_type=output_type), **more).frames


def arrays(sample):
    return np.stack([np.asarray(f) for f in sample])


@pytest.fixture(scope="module")
def dmax(pipe):
    """Random weights scatter Otsu's seeds over the grid.  The same inputs give the same bits, so a number threshold just under sqrt(dmax) of
    one auto-region call leaves only the top cell as the seed of the next ones: a compact region, through the public interface."""
    pipe.enable_auto_region(detect_step=K)
    try:
        call(pipe, IMAGE, inputs(), "latent")
        return float(pipe.auto_region_report["dmax"])
    finally:
        pipe.disable_auto_region()


def detector(dmax, **over):
    return dict(dict(detect_step=K, threshold=math.sqrt(dmax) * (1 - 1e-3), dilate=1, feather=1, max_area=1.0), **over)


def auto_region_call(pipe, kw, det, output_type="pil", **more):
    pipe.enable_auto_region(**det)
    try:
        return call(pipe, IMAGE, kw, output_type, **more), pipe.auto_region_report
    finally:
        pipe.disable_auto_region()


def auto_focused(pipe, kw, det, warm=False, context=CONTEXT, output_type="pil", image=IMAGE, **more):
    pipe.enable_auto_region(**det).enable_auto_focus(context, warm_start=warm)
    try:
        out = call(pipe, image, kw, output_type, **more)
        return out, pipe.focus_report, pipe.auto_region_report
    finally:
        pipe.disable_auto_region().disable_auto_focus()


def explicit_focused(pipe, kw, mask, composite=True, context=CONTEXT, **more):
    assert pipe._auto_focus is None
    pipe.set_edit_region(mask, composite=composite).enable_region_focus(context)
    try:
        return call(pipe, IMAGE, kw, "pil", **more), pipe.focus_report
    finally:
        pipe.clear_edit_region().disable_region_focus()


def check_accepted(report, warm=False, context=CONTEXT):
    """The precondition of the tests below: the detection gave a region worth cropping to."""
    rep = report[0]
    assert rep["reason"] == "ok" and rep["box"] != (0, 0) + IMAGE.size, rep
    assert rep["source_size"] == IMAGE.size and rep["edit_size"] == (W, H) and rep["start_step"] == (K + 1 if warm else 0)
    assert rep["mask"].mode == "L" and rep["mask"].size == IMAGE.size
    assert rep["detect"]["accepted"] and rep["detect"]["step"] == K
    assert rep["mask"].tobytes() == rep["detect"]["mask"].resize(IMAGE.size, Image.BILINEAR).tobytes()  # the lift is PIL's
    mask = torch.from_numpy(np.array(rep["mask"]))
    assert {k: rep[k] for k in ("box", "reason", "source_size", "edit_size", "scale", "mask_fraction_of_box")} == \
        focus.plan(IMAGE.size, rep["mask"], H, W, context) == autofocus.plan(mask, (W, H), context)
    assert 0.0 < rep["mask_fraction_of_box"] <= 1.0
    return rep


@pytest.mark.parametrize("use_graph", [True, False])
def test_cold_start_equals_the_explicit_focused_call(pipe, dmax, use_graph):
    kw, det = inputs(), detector(dmax)
    pipe.use_graph = use_graph
    try:
        got, report, detect = auto_focused(pipe, kw, det)
        rep = check_accepted(report)
        assert detect is rep["detect"]
        want, want_report = explicit_focused(pipe, kw, rep["mask"], composite=True)
    finally:
        pipe.use_graph = True
    assert want_report[0] == {k: v for k, v in rep.items() if k not in ("mask", "detect", "start_step")}
    frames = arrays(got[0])
    assert frames.shape == (5, IMAGE.size[1], IMAGE.size[0], 3) and np.array_equal(frames, arrays(want[0]))  # the photo's size
    # the kept area is the photo: its own bytes wherever the photo-size mask is 0
    keep, src = np.array(rep["mask"]) == 0, np.array(IMAGE)
    assert keep.any() and not keep.all()
    for f in frames:
        assert np.array_equal(f[keep], src[keep])
    assert not np.array_equal(frames[-1][~keep], src[~keep])


def test_cold_start_with_sparse_steps_and_composite_off(pipe, dmax):
    kw, det = inputs(), detector(dmax, composite=False)
    pipe.enable_sparse_region(refresh_every=2, margin=0)
    try:
        got, report, _ = auto_focused(pipe, kw, det, context=1.0)  # (the largest box the photo holds: the region leaves tokens inactive)
        rep = check_accepted(report, context=1.0)
        sparse = pipe.transformer.sparse_report
        want, _ = explicit_focused(pipe, kw, rep["mask"], composite=False, context=1.0)
        assert pipe.transformer.sparse_report == sparse and sparse is not None and "sparse" in sparse["plan"], sparse
    finally:
        pipe.disable_sparse_region()
    frames, src = arrays(got[0]), np.array(IMAGE)
    assert np.array_equal(frames, arrays(want[0]))
    l, t, r, b = rep["box"]
    outside = np.ones(src.shape[:2], bool)
    outside[t:b, l:r] = False
    assert np.array_equal(frames[-1][outside], src[outside])  # composite off: the whole box is replaced, nothing else


def warm_second_implementation(pipe, kw, det, context=CONTEXT):
    """The warm start from public pieces: a scout that copies the estimate behind step K and interrupts, the CPU expression of the mix, the
    region edit of the crop through `denoise(start_step=K + 1, start_eps=)`, PIL's paste."""
    from chronoedit_amd.pipeline import decode_latents, denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    grabbed = {}

    def scout_end(p, i, t, tensors):
        if i == K:
            grabbed["x0"] = p.scheduler.model_outputs[-1].clone()
            p._interrupt = True
        return {}

    _, detect = auto_region_call(pipe, kw, det, "latent", callback_on_step_end=scout_end)
    assert detect["accepted"] and detect["step"] == K
    mask_src = detect["mask"].resize(IMAGE.size, Image.BILINEAR)
    mask_u8 = torch.from_numpy(np.array(mask_src))
    box, reason = focus.focus_box(focus.mask_bbox(mask_u8), IMAGE.size, (W, H), context)
    assert reason == "ok"
    crop, m_edit = focus.host_inputs(IMAGE, mask_u8, box, W, H)
    img = pipe.preprocess_image(crop, H, W).to(device=DEV, dtype=BF)
    image_embeds = pipe.encode_image(crop, DEV).to(BF)
    noise, condition = pipe.prepare_latents(img, 1, 16, H, W, kw["num_frames"], BF, DEV, None, kw["latents"].clone())
    eps = noise.float()
    full = FlowUniPCMultistepScheduler(flow_shift=FLOW_SHIFT, sigma_grid="diffusers")
    full.set_timesteps(kw["num_inference_steps"])
    tabs = autofocus.restart_tables(box, IMAGE.size, (H // 8, W // 8))
    lat0 = autofocus.restart(grabbed["x0"].cpu(), eps.cpu(), tabs, float(full.sigmas[K + 1])).to(DEV)
    cfg = region.RegionConfig(w=region.latent_weights(m_edit.to(DEV)), z_src=region.static_source_latents(pipe.vae, img, kw["num_frames"]))
    seen = []
    out = denoise(pipe.transformer, pipe.scheduler, lat0, condition, kw["prompt_embeds"], kw["negative_prompt_embeds"], image_embeds,
                  kw["num_inference_steps"], kw["guidance_scale"], use_graph=pipe.use_graph, graph_warm=pipe._graph_warm, region=cfg,
                  start_step=K + 1, start_eps=eps, on_step_end=lambda i, t, lat: seen.append(i))
    assert seen == list(range(K + 1, kw["num_inference_steps"]))
    frames = pipe.postprocess_video(decode_latents(pipe.vae, out), "pil")[0]
    return arrays(focus.host_paste(IMAGE, frames, mask_u8, box)), box


@pytest.mark.parametrize("use_graph", [True, False])
def test_warm_start_equals_the_second_implementation(pipe, dmax, use_graph):
    kw, det = inputs(), detector(dmax)
    pipe.use_graph = use_graph
    try:
        steps = []
        got, report, _ = auto_focused(pipe, kw, det, warm=True, callback_on_step_end=lambda p, i, t, tensors: steps.append(i) or {})
        rep = check_accepted(report, warm=True)
        want, box = warm_second_implementation(pipe, kw, det)
    finally:
        pipe.use_graph = True
    assert steps == list(range(K + 1)) + list(range(K + 1, STEPS))  # the scout's steps, then the tail
    assert box == rep["box"]
    frames = arrays(got[0])
    assert frames.shape == want.shape and np.array_equal(frames, want)
    cold = arrays(auto_focused(pipe, kw, det)[0][0])
    assert not np.array_equal(frames, cold)  # another trajectory than the cold start's
    keep = np.array(rep["mask"]) == 0
    assert np.array_equal(frames[-1][keep], np.array(IMAGE)[keep])


@pytest.mark.parametrize("why", ["empty", "max_area", "whole"])
def test_fallbacks_are_the_auto_region_call(pipe, dmax, why):
    kw = inputs()
    det = {"empty": detector(dmax, threshold=math.sqrt(dmax) * 1.01), "max_area": detector(dmax, max_area=0.01),
           "whole": detector(dmax, threshold=0.0)}[why]  # (a threshold of 0: every cell is a seed, the region is the photo)
    for warm in (False, True):
        got, report, detect = auto_focused(pipe, kw, det, warm=warm)
        want, want_detect = auto_region_call(pipe, kw, det)
        assert got[0][0].size == (W, H) and np.array_equal(arrays(got[0]), arrays(want[0]))  # edit-size frames, bit for bit
        if why == "whole":
            assert detect["accepted"] and report[0]["reason"] == "whole" and report[0]["box"] == (0, 0) + IMAGE.size
        else:
            assert not detect["accepted"] and detect["reason"] == why and report[0]["reason"] == "declined"
        assert report[0]["detect"] is detect and detect["reason"] == want_detect["reason"] and detect["threshold"] == want_detect["threshold"]
    lat = auto_focused(pipe, kw, det, output_type="latent")[0]
    assert torch.equal(lat, auto_region_call(pipe, kw, det, "latent")[0])


def test_the_host_form_agrees(pipe, dmax):
    kw, det = inputs(), detector(dmax)
    on_device = [arrays(auto_focused(pipe, kw, det, warm=warm)[0][0]) for warm in (False, True)]
    pipe.enable_device_image_io(False)
    try:
        on_host = []
        for warm in (False, True):
            got, report, _ = auto_focused(pipe, kw, det, warm=warm)
            check_accepted(report, warm)
            on_host.append(arrays(got[0]))
    finally:
        pipe.enable_device_image_io(True)
    assert all(np.array_equal(h, d) for h, d in zip(on_host, on_device))


def test_an_explicit_mask_overrides_auto_focus(pipe, dmax):
    kw, det = inputs(), detector(dmax)
    mask = Image.new("L", (W, H), 0)
    mask.paste(255, (8, 8, 56, 40))
    pipe.set_edit_region(mask)
    try:
        got, report, detect = auto_focused(pipe, kw, det, warm=True)
        want = call(pipe, IMAGE, kw)
    finally:
        pipe.clear_edit_region()
    assert report is None and detect is None  # neither the scout nor the detector ran
    assert got[0][0].size == (W, H) and np.array_equal(arrays(got[0]), arrays(want[0]))


def test_refusals(pipe, dmax):
    det = detector(dmax)
    with pytest.raises(NotImplementedError, match="one photo"):
        auto_focused(pipe, inputs(n=2), det, image=[IMAGE, IMAGE])
    with pytest.raises(NotImplementedError, match="one photo"):
        auto_focused(pipe, inputs(n=2), det)  # two prompts
    kw2 = inputs(n=2)
    kw2.update(prompt_embeds=kw2["prompt_embeds"][:1], negative_prompt_embeds=kw2["negative_prompt_embeds"][:1])
    with pytest.raises(NotImplementedError, match="one photo"):
        auto_focused(pipe, kw2, det, num_videos_per_prompt=2)
    with pytest.raises(NotImplementedError, match="temporal reasoning"):
        auto_focused(pipe, inputs(frames=29), det, enable_temporal_reasoning=True, num_temporal_reasoning_steps=1)
    for image in (np.asarray(IMAGE, dtype=np.float32) / 255.0, torch.rand(1, 3, H, W)):
        with pytest.raises(ValueError, match="PIL"):
            auto_focused(pipe, inputs(), det, image=image, image_embeds=torch.zeros(1, 17, 320, dtype=BF, device=DEV))
    # without the detector the switch is inert: the plain call
    kw = inputs()
    pipe.enable_auto_focus()
    try:
        alone = call(pipe, IMAGE, kw)
        assert pipe.focus_report is None
    finally:
        pipe.disable_auto_focus()
    assert np.array_equal(arrays(alone[0]), arrays(call(pipe, IMAGE, kw)[0]))


def test_disabling_restores_the_auto_region_call(pipe, dmax):
    kw, det = inputs(), detector(dmax)
    want, _ = auto_region_call(pipe, kw, det)
    pipe.enable_auto_focus(warm_start=True).disable_auto_focus()
    got, detect = auto_region_call(pipe, kw, det)
    assert pipe.focus_report is None and detect["accepted"]
    assert got[0][0].size == (W, H) and np.array_equal(arrays(got[0]), arrays(want[0]))
