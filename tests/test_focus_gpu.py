"""Focused region edits through `ChronoEditPipeline.__call__`: crop to the mask, edit the crop, paste back at the source's size - bit for bit
what an independent second implementation gives: the plain region call on `image.crop(box)`, then PIL's resize and paste."""
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import focus, sparse_region

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H = 96, 64
BF = torch.bfloat16


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


def photo(size=(203, 150), seed=9):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8))


def blob(size, rows, cols, seed=3):
    """An "L" mask of the photo's size: random greys over the blob, 255 in its core, 0 elsewhere."""
    m = np.zeros((size[1], size[0]), np.uint8)
    m[rows[0]:rows[1], cols[0]:cols[1]] = np.random.default_rng(seed).integers(1, 256, (rows[1] - rows[0], cols[1] - cols[0]), dtype=np.uint8)
    m[rows[0] + 4:rows[1] - 4, cols[0] + 4:cols[1] - 4] = 255
    return Image.fromarray(m)


IMAGE = photo()
MASK = blob(IMAGE.size, (8, 58), (130, 196))  # near the top right corner: the box is shifted into the image, scale 126 / 96
SMALL = blob(IMAGE.size, (100, 120), (20, 50))  # with context 1: 24 x 16 pixels of the crop, so that most tokens stay inactive


def inputs(n=1, frames=5, steps=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    T = (frames - 1) // 4 + 1
    return dict(prompt_embeds=torch.randn(n, 40, 128, generator=g).to(BF).cuda(), negative_prompt_embeds=torch.randn(n, 40, 128, generator=g).to(BF).cuda(),
                height=H, width=W, num_frames=frames, num_inference_steps=steps, guidance_scale=5.0,
                latents=torch.randn(n, 16, T, H // 8, W // 8, generator=g).to(BF).float())


def call(pipe, image, kw, output_type="pil", **more):
    return pipe(image=image, **dict(kw, latents=kw["latents"].clone(), output_type=output_type), **more).frames


def arrays(frames):
    return [np.stack([np.asarray(f) for f in sample]) for sample in frames]


def focused(pipe, image, mask, kw, context=0.25, composite=True, output_type="pil", **more):
    pipe.enable_region_focus(context).set_edit_region(mask, composite=composite)
    try:
        out = call(pipe, image, kw, output_type, **more)
        return out, pipe.focus_report
    finally:
        pipe.disable_region_focus().clear_edit_region()


def second_implementation(pipe, image, mask, boxes, kw, paste_mask=True, **more):
    """The plain region call on the crops (no composite), then per frame PIL's resize to the box and paste into a copy of the photo."""
    images, masks = (image, mask) if isinstance(image, list) else ([image], [mask])
    crops = [im.crop(box) for im, box in zip(images, boxes)]
    cmasks = [m.crop(box) for m, box in zip(masks, boxes)]
    assert pipe._region_focus is None
    pipe.set_edit_region(cmasks if isinstance(image, list) else cmasks[0], composite=False)
    try:
        frames = call(pipe, crops if isinstance(image, list) else crops[0], kw, "pil", **more)
    finally:
        pipe.clear_edit_region()
    out = []
    for sample, im, cm, (l, t, r, b) in zip(frames, images, cmasks, boxes):
        pasted = []
        for f in sample:
            assert f.size == (W, H)
            o = im.copy()
            o.paste(f.resize((r - l, b - t), Image.LANCZOS), (l, t), cm if paste_mask else None)
            pasted.append(o)
        out.append(pasted)
    return arrays(out)


def assert_focused_equals_second(pipe, image, mask, kw, context=0.25, **more):
    got, report = focused(pipe, image, mask, kw, context, **more)
    boxes = [r["box"] for r in report]
    want = second_implementation(pipe, image, mask, boxes, kw, **more)
    got = arrays(got)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    return got, report


@pytest.mark.parametrize("use_graph", [True, False])
def test_focused_call_equals_the_second_implementation(pipe, use_graph):
    kw = inputs()
    pipe.use_graph = use_graph
    try:
        got, report = assert_focused_equals_second(pipe, IMAGE, MASK, kw)
    finally:
        pipe.use_graph = True
    rep = report[0]
    bbox = focus.mask_bbox(torch.from_numpy(np.array(MASK)))
    assert bbox == (130, 8, 196, 58)
    assert (rep["box"], rep["reason"]) == focus.focus_box(bbox, IMAGE.size, (W, H), 0.25) == ((77, 0, 203, 84), "ok")
    assert rep == focus.plan(IMAGE.size, MASK, H, W, 0.25) and rep["scale"] == 126 / 96 and rep["source_size"] == IMAGE.size
    frames = got[0]
    assert frames.shape == (5, IMAGE.size[1], IMAGE.size[0], 3)  # the SOURCE's size
    keep, src = np.array(MASK) == 0, np.array(IMAGE)
    for f in range(5):
        assert np.array_equal(frames[f][keep], src[keep]), f  # the photo's own bytes wherever the source-size mask is 0
    assert not np.array_equal(frames[-1][~keep], src[~keep])


def test_focused_sparse_edit(pipe):
    kw = inputs()
    pipe.enable_sparse_region(refresh_every=2)
    try:
        got, report = assert_focused_equals_second(pipe, IMAGE, SMALL, kw, context=1.0)
        rep = pipe.transformer.sparse_report  # (of the second implementation's call; the focused one is compared bit for bit)
        assert rep["plan"] == ["refresh", "sparse"] and sparse_region.PAD <= rep["active"] < rep["tokens"] == 48, rep
        focused(pipe, IMAGE, SMALL, kw, context=1.0)
        assert pipe.transformer.sparse_report == rep
    finally:
        pipe.disable_sparse_region()
    assert report[0]["reason"] == "ok" and report[0]["scale"] == 1.25


@pytest.mark.parametrize("reasoning_steps,n_frames", [(1, 5), (2, 29)])
def test_focused_edit_with_temporal_reasoning(pipe, reasoning_steps, n_frames):
    """8 latent frames: truncated to 2 behind step 1 (5 frames come back), or kept to the end (the reasoning frames come back as well)."""
    kw = inputs(frames=29)
    more = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=reasoning_steps)
    got, _ = assert_focused_equals_second(pipe, IMAGE, MASK, kw, **more)
    assert got[0].shape[0] == len(call(pipe, IMAGE, kw, "pil", **more)[0]) == n_frames
    keep = np.array(MASK) == 0
    assert all(np.array_equal(f[keep], np.array(IMAGE)[keep]) for f in got[0])  # every returned frame is pasted


def test_two_images_two_masks_two_boxes(pipe):
    other = photo((150, 180), seed=11)
    other_mask = blob(other.size, (120, 170), (10, 60), seed=4)
    kw = inputs(n=2)
    got, report = assert_focused_equals_second(pipe, [IMAGE, other], [MASK, other_mask], kw)
    assert report[0]["box"] != report[1]["box"] and [r["source_size"] for r in report] == [IMAGE.size, other.size]
    assert got[0].shape[1:3] == (150, 203) and got[1].shape[1:3] == (180, 150)
    for frames, im, m in zip(got, (IMAGE, other), (MASK, other_mask)):
        keep = np.array(m) == 0
        assert np.array_equal(frames[-1][keep], np.array(im)[keep])
    # frames of two sizes do not fit one array
    pipe.enable_region_focus().set_edit_region([MASK, other_mask])
    try:
        with pytest.raises(ValueError, match="one size"):
            call(pipe, [IMAGE, other], kw, "np")
    finally:
        pipe.disable_region_focus().clear_edit_region()


def test_fit_and_empty_still_return_source_size_frames(pipe):
    kw = inputs()
    tall = blob(IMAGE.size, (5, 145), (90, 112))  # higher than the largest 3:2 box the photo holds (203 x 135)
    got, report = assert_focused_equals_second(pipe, IMAGE, tall, kw)
    assert report[0]["reason"] == "fit" and report[0]["box"] == (0, 0, 203, 150) and got[0].shape == (5, 150, 203, 3)
    empty = Image.new("L", IMAGE.size, 0)
    got, report = focused(pipe, IMAGE, empty, kw)
    assert report[0]["reason"] == "empty" and report[0]["box"] == (0, 0, 203, 150) and report[0]["mask_fraction_of_box"] == 0.0
    frames = arrays(got)[0]
    assert frames.shape == (5, 150, 203, 3) and all(np.array_equal(f, np.array(IMAGE)) for f in frames)  # nothing is marked: the photo


def test_composite_false_replaces_the_whole_box(pipe):
    kw = inputs()
    got, report = focused(pipe, IMAGE, MASK, kw, composite=False)
    l, t, r, b = box = report[0]["box"]
    want = second_implementation(pipe, IMAGE, MASK, [box], kw, paste_mask=False)
    frames, src = arrays(got)[0], np.array(IMAGE)
    assert np.array_equal(frames, want[0])
    outside = np.ones(src.shape[:2], bool)
    outside[t:b, l:r] = False
    keep_in_box = (np.array(MASK) == 0) & ~outside
    assert np.array_equal(frames[-1][outside], src[outside]) and not np.array_equal(frames[-1][keep_in_box], src[keep_in_box])


def test_np_and_pt_carry_the_pil_bytes(pipe):
    kw = inputs()
    pil = arrays(focused(pipe, IMAGE, MASK, kw)[0])[0]
    as_np = focused(pipe, IMAGE, MASK, kw, output_type="np")[0]
    assert as_np.dtype == np.float32 and as_np.shape == (1, 5, 150, 203, 3) and np.array_equal(as_np[0], pil.astype(np.float32) / 255.0)
    as_pt = focused(pipe, IMAGE, MASK, kw, output_type="pt")[0]
    assert as_pt.dtype == torch.float32 and tuple(as_pt.shape) == (1, 5, 3, 150, 203)
    assert np.array_equal(as_pt[0].permute(0, 2, 3, 1).numpy(), as_np[0])
    # "latent": the crop's latents, nothing pasted - those of the second implementation's call
    lat = focused(pipe, IMAGE, MASK, kw, output_type="latent")[0]
    box = focus.plan(IMAGE.size, MASK, H, W)["box"]
    pipe.set_edit_region(MASK.crop(box), composite=False)
    try:
        want = call(pipe, IMAGE.crop(box), kw, "latent")
    finally:
        pipe.clear_edit_region()
    assert lat.shape == kw["latents"].shape and torch.equal(lat, want)


def test_array_and_tensor_images_are_refused(pipe):
    kw = inputs()
    for image in (np.asarray(IMAGE, dtype=np.float32) / 255.0, torch.rand(1, 3, H, W)):
        pipe.enable_region_focus().set_edit_region(MASK)
        try:
            with pytest.raises(ValueError, match="PIL"):
                call(pipe, image, kw, "pil", image_embeds=torch.zeros(1, 17, 320, dtype=BF, device=DEV))
        finally:
            pipe.disable_region_focus().clear_edit_region()


def test_focus_without_a_mask_is_the_plain_call(pipe):
    kw = inputs()
    plain, plain_lat = arrays(call(pipe, IMAGE, kw))[0], call(pipe, IMAGE, kw, "latent")
    pipe.enable_region_focus()
    try:
        frames, lat = arrays(call(pipe, IMAGE, kw))[0], call(pipe, IMAGE, kw, "latent")
        assert pipe.focus_report is None
    finally:
        pipe.disable_region_focus()
    assert frames.shape == (5, H, W, 3) and np.array_equal(frames, plain) and torch.equal(lat, plain_lat)


def test_the_host_path_gives_the_same_frames(pipe):
    kw = inputs()
    on_device = arrays(focused(pipe, IMAGE, MASK, kw)[0])[0]
    pipe.enable_device_image_io(False)
    try:
        on_host = arrays(focused(pipe, IMAGE, MASK, kw)[0])[0]
        host_box = focused(pipe, IMAGE, MASK, kw, composite=False)[0]
    finally:
        pipe.enable_device_image_io(True)
    assert np.array_equal(on_host, on_device)
    assert np.array_equal(arrays(host_box)[0], arrays(focused(pipe, IMAGE, MASK, kw, composite=False)[0])[0])
