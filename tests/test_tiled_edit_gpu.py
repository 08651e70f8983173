"""Tiled edits through `ChronoEditPipeline.__call__` (`enable_tiled_edit`): a 150 x 90 photo as a 2 x 2 plan of 96 x 64 tiles, byte for byte
what a second implementation from public pieces gives.

The second implementation: the padded canvas's tile crops through the ordinary pre-processing, CLIP and `pipeline.prepare_latents`; the
tiles' latents cut from the same canvas noise on the CPU (`tiles.reference_scatter`); the public loop `pipeline.denoise` on the batch of
tiles, eagerly, with an `on_step_end` hook that replaces the latents by `tiles.reference_fuse` + `reference_scatter` on the CPU behind every
step; `pipeline.decode_latents`, the host's byte conversion, `tiles.reference_blend` and the crop.  (`__call__` on a LIST of images runs its
samples one after the other, each through all of its steps, so no callback of it can make the samples agree step by step: the batched
loop is the public piece that steps the tiles together.)"""
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import tiles

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H = 96, 64
BF = torch.bfloat16
PHOTO = Image.fromarray(np.random.default_rng(11).integers(0, 256, (90, 150, 3), dtype=np.uint8))
PLAN = tiles.plan(PHOTO.size, H, W)


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
                              scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers"))


def inputs(canvas=PLAN.canvas, frames=5, steps=3, seed=5, guidance_scale=5.0):
    g = torch.Generator().manual_seed(seed)
    T = (frames - 1) // 4 + 1
    return dict(prompt_embeds=torch.randn(1, 40, 128, generator=g).to(BF).cuda(), negative_prompt_embeds=torch.randn(1, 40, 128, generator=g).to(BF).cuda(),
                height=H, width=W, num_frames=frames, num_inference_steps=steps, guidance_scale=guidance_scale,
                latents=torch.randn(1, 16, T, canvas[1] // 8, canvas[0] // 8, generator=g).to(BF).float())


def call(pipe, image, kw, output_type="pil", **more):
    return pipe(image=image, **dict(kw, latents=None if kw.get("latents") is None else kw["latents"].clone(), output_type=output_type), **more).frames


def frames_of(out):
    """`frames` of a "pil" call with one sample -> uint8 [F, H, W, 3]."""
    assert len(out) == 1
    return np.stack([np.asarray(f) for f in out[0]])


def tiled(pipe, image, kw, output_type="pil", graph=True, **switch):
    pipe.enable_tiled_edit(**switch)
    pipe.use_graph = graph
    try:
        return call(pipe, image, kw, output_type), pipe.tile_report
    finally:
        pipe.disable_tiled_edit()
        pipe.use_graph = True


def second(pipe, image, kw, clip="tile", p=PLAN):
    """The second implementation -> (frames uint8 [F, H, W, 3], the canvas latents fp32 [1, 16, T, ch, cw] on the CPU)."""
    from chronoedit_amd.pipeline import decode_latents, denoise, prepare_latents
    crops = tiles.tile_images(image.convert("RGB"), p)
    n = len(crops)
    xs, ys, th, tw, ch, cw = p.cells
    img = pipe.preprocess_image(crops, H, W).to(device=DEV, dtype=BF)
    lat0 = tiles.reference_scatter(kw["latents"][0], xs, ys, th, tw).to(DEV)
    _, condition = prepare_latents(pipe.vae, img, kw["num_frames"], latents=lat0)
    embeds = pipe.encode_image(crops, DEV) if clip == "tile" else pipe.encode_image(image.convert("RGB"), DEV).repeat(n, 1, 1)
    last = {}

    def fuse(i, t, lat):
        last["canvas"] = tiles.reference_fuse(lat.cpu(), xs, ys, ch, cw)
        return tiles.reference_scatter(last["canvas"], xs, ys, th, tw).to(DEV)

    guided = kw["guidance_scale"] > 1
    lat = denoise(pipe.transformer, pipe.scheduler, lat0, condition, kw["prompt_embeds"].repeat(n, 1, 1),
                  kw["negative_prompt_embeds"].repeat(n, 1, 1) if guided else None, embeds.to(BF), kw["num_inference_steps"], kw["guidance_scale"],
                  use_graph=False, on_step_end=fuse)
    assert torch.equal(tiles.reference_fuse(lat.cpu(), xs, ys, ch, cw), last["canvas"])  # (identical tiles return themselves)
    video = decode_latents(pipe.vae, lat)
    u8 = np.stack([np.stack([np.asarray(f) for f in sample]) for sample in pipe.postprocess_video(video, output_type="pil")])
    return tiles.reference_blend(torch.from_numpy(u8), p.xs, p.ys, p.target).numpy(), last["canvas"][None]


@pytest.fixture(scope="module")
def reference(pipe):
    """The second implementation's results, computed once per guidance scale and shared (never written to)."""
    return {g: second(pipe, PHOTO, inputs(guidance_scale=g)) for g in (5.0, 1.0)}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("g", [5.0, 1.0])
def test_tiled_call_equals_the_second_implementation(pipe, reference, g, graph):
    out, report = tiled(pipe, PHOTO, inputs(guidance_scale=g), graph=graph)
    got = frames_of(out)
    assert got.shape == (5, 90, 150, 3) and out[0][0].size == PHOTO.size  # the TARGET's size
    assert np.array_equal(got, reference[g][0])
    assert report == dict(PLAN.report, reason="tiled") and report["count"] == 4 and report["canvas"] == (160, 96)
    assert len(np.unique(got)) > 1  # (not a flat picture: the equality says something)
    if graph:  # a second call replays from the first step on (the shape is warm): still the same bytes
        assert np.array_equal(frames_of(tiled(pipe, PHOTO, inputs(guidance_scale=g))[0]), reference[g][0])


def test_latent_output_is_the_fused_canvas(pipe, reference):
    out, _ = tiled(pipe, PHOTO, inputs(), output_type="latent")
    assert tuple(out.shape) == (1, 16, 2, 12, 20) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), reference[5.0][1])


def test_latent_output_follows_latents_a_callback_returns_last(pipe):
    """A callback that replaces the latents behind the LAST step: the returned canvas is their fusion, not the canvas of the step's own."""
    kw = inputs()
    xs, ys, th, tw, ch, cw = PLAN.cells
    mine = torch.randn(4, 16, 2, th, tw, generator=torch.Generator().manual_seed(8))

    def cb(p, i, t, tensors):
        assert tuple(tensors["latents"].shape) == tuple(mine.shape)
        return {"latents": mine.to(DEV)} if i == kw["num_inference_steps"] - 1 else {}

    pipe.enable_tiled_edit()
    try:
        out = call(pipe, PHOTO, kw, "latent", callback_on_step_end=cb)
    finally:
        pipe.disable_tiled_edit()
    assert torch.equal(out.cpu()[0], tiles.reference_fuse(mine, xs, ys, ch, cw))


def test_host_path_gives_the_same_bytes(pipe, reference):
    pipe.enable_device_image_io(False)
    try:
        out, _ = tiled(pipe, PHOTO, inputs())
    finally:
        pipe.enable_device_image_io(True)
    assert np.array_equal(frames_of(out), reference[5.0][0])


def test_np_and_pt_carry_the_bytes(pipe, reference):
    out, _ = tiled(pipe, PHOTO, inputs(), output_type="np")
    assert out.shape == (1, 5, 90, 150, 3) and np.array_equal(out[0], reference[5.0][0].astype(np.float32) / 255.0)
    out, _ = tiled(pipe, PHOTO, inputs(), output_type="pt")
    assert tuple(out.shape) == (1, 5, 3, 90, 150) and np.array_equal(out[0].permute(0, 2, 3, 1).numpy(), reference[5.0][0].astype(np.float32) / 255.0)


def test_clip_photo_repeats_the_whole_image_s_row(pipe, reference):
    kw = inputs()
    out, _ = tiled(pipe, PHOTO, kw, clip="photo")
    want, _ = second(pipe, PHOTO, kw, clip="photo")
    assert np.array_equal(frames_of(out), want) and not np.array_equal(want, reference[5.0][0])


def test_a_resized_target_device_and_host_agree(pipe):
    kw = inputs(canvas=(192, 112))
    out, report = tiled(pipe, PHOTO, kw, size=(185, 110))
    assert report["target"] == (185, 110) and report["canvas"] == (192, 112) and out[0][0].size == (185, 110)
    p = tiles.plan(PHOTO.size, H, W, size=(185, 110))
    want, _ = second(pipe, PHOTO.resize((185, 110), Image.LANCZOS), kw, p=p)
    assert np.array_equal(frames_of(out), want)
    pipe.enable_device_image_io(False)
    try:
        assert np.array_equal(frames_of(tiled(pipe, PHOTO, kw, size=(185, 110))[0]), want)
    finally:
        pipe.enable_device_image_io(True)


def test_single_and_disabled_are_the_plain_call(pipe):
    kw = inputs(canvas=(W, H))
    plain = frames_of(call(pipe, PHOTO, kw))
    out, report = tiled(pipe, PHOTO, kw, size=(W, H))
    assert report["reason"] == "single" and report["count"] == 1 and np.array_equal(frames_of(out), plain) and report["frames"] == (W, H)
    pipe.enable_tiled_edit().disable_tiled_edit()
    assert np.array_equal(frames_of(call(pipe, PHOTO, kw)), plain) and pipe.tile_report is None


def test_a_generator_draws_one_canvas(pipe):
    kw = dict(inputs(), latents=None)
    out, _ = tiled(pipe, PHOTO, dict(kw, generator=torch.Generator().manual_seed(3)), output_type="latent")
    noise = torch.randn((1, 16, 2, 12, 20), generator=torch.Generator().manual_seed(3), dtype=BF)
    want, _ = tiled(pipe, PHOTO, dict(kw, latents=noise.float()), output_type="latent")
    assert torch.equal(out, want)
    with pytest.raises(ValueError, match="canvas shape"):
        tiled(pipe, PHOTO, dict(kw, latents=torch.zeros(4, 16, 2, 8, 12)))


def test_refusals(pipe):
    kw = inputs()
    switches = [(lambda: pipe.enable_teacache(0.1), pipe.disable_teacache, NotImplementedError),
                (lambda: pipe.enable_guidance_reuse(2), pipe.disable_guidance_reuse, NotImplementedError),
                (lambda: pipe.enable_preview(print, factors=torch.zeros(17, 3)), pipe.disable_preview, NotImplementedError),
                (lambda: pipe.enable_auto_region(1), pipe.disable_auto_region, ValueError),
                (lambda: pipe.set_edit_region(np.ones((90, 150), np.uint8)), pipe.clear_edit_region, ValueError),
                (lambda: pipe.enable_auto_focus(), pipe.disable_auto_focus, ValueError)]
    for on, off, exc in switches:
        on()
        try:
            with pytest.raises(exc, match="enable_tiled_edit"):
                tiled(pipe, PHOTO, kw)
        finally:
            off()
    calls = [(dict(image=[PHOTO, PHOTO]), NotImplementedError), (dict(num_videos_per_prompt=2), NotImplementedError),
             (dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=1), NotImplementedError), (dict(offload_model=True), NotImplementedError),
             (dict(image=np.zeros((90, 150, 3), np.float32)), ValueError), (dict(image={"background": PHOTO, "composite": PHOTO}), ValueError)]
    for more, exc in calls:
        pipe.enable_tiled_edit()
        try:
            with pytest.raises(exc, match="enable_tiled_edit"):
                pipe(**dict(dict(kw, image=PHOTO), **more))
        finally:
            pipe.disable_tiled_edit()
    pipe.enable_tiled_edit()
    try:
        with pytest.raises(ValueError, match="enable_tiled_edit"):
            pipe.enable_detail_lift()
    finally:
        pipe.disable_tiled_edit()
    with pytest.raises(ValueError, match="max_tiles = 2"):
        tiled(pipe, PHOTO, kw, max_tiles=2)
    assert np.array_equal(frames_of(call(pipe, PHOTO, inputs(canvas=(W, H)))), frames_of(call(pipe, PHOTO, inputs(canvas=(W, H)))))  # the pipe still works
