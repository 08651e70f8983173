"""The detail lift through `ChronoEditPipeline.__call__`: whole-image edits come back at the photo's size, byte for byte what a second
implementation built from public pieces gives - the plain call's "pil" frames, PIL's own Lanczos of the photo and of the frames, and
`lift.reference` on the CPU.  (The synthetic VAE decodes noise: the gate is near 1 and the frames near the Lanczos upsample; what is
checked here is the wiring, the definition is checked in test_lift_cpu.py and test_exact_lift_gpu.py.)"""
import math

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import lift

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


IMAGE = photo()


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


def lifted(pipe, image, kw, output_type="pil", lift_kw=None, **more):
    pipe.enable_detail_lift(**(lift_kw or {}))
    try:
        out = call(pipe, image, kw, output_type, **more)
        return out, pipe.lift_report
    finally:
        pipe.disable_detail_lift()


def second_implementation(plain, images, cfg=None):
    """Per sample: the plain call's PIL frames, PIL's Lanczos of the photo (to the edit's size) and of the frames (to the photo's), and
    lift.reference on the CPU."""
    cfg = cfg or lift.LiftConfig()
    t = lambda im: torch.from_numpy(np.array(im, dtype=np.uint8))
    out = []
    for sample, im in zip(plain, images):
        assert all(f.size == (W, H) for f in sample)
        P, L = t(im), t(im.resize((W, H), Image.LANCZOS))
        E = torch.stack([t(f) for f in sample])
        U = None if cfg.gate is None else torch.stack([t(f.resize(im.size, Image.LANCZOS)) for f in sample])
        out.append(lift.reference(P, L, E, U, cfg).numpy())
    return out


def check_report(report, sizes, applied=True, reason="ok"):
    assert len(report) == len(sizes)
    for rep, size in zip(report, sizes):
        assert set(rep) == {"size", "edit_size", "applied", "reason", "fallback_fraction"}
        assert (rep["size"], rep["edit_size"], rep["applied"], rep["reason"]) == (size, (W, H), applied, reason)
        assert (rep["fallback_fraction"] is None) if not applied else 0.0 <= rep["fallback_fraction"] <= 1.0


@pytest.mark.parametrize("use_graph", [True, False])
def test_lifted_call_equals_the_second_implementation(pipe, use_graph):
    kw = inputs()
    pipe.use_graph = use_graph
    try:
        plain = call(pipe, IMAGE, kw)
        assert pipe.lift_report is None
        got, report = lifted(pipe, IMAGE, kw)
    finally:
        pipe.use_graph = True
    want = second_implementation(plain, [IMAGE])
    got = arrays(got)
    assert got[0].shape == (5, 150, 203, 3) and np.array_equal(got[0], want[0])  # the PHOTO's size
    check_report(report, [IMAGE.size])
    # the gate's mean is the reference's
    cells = lift.coefficients_reference(torch.from_numpy(np.array(IMAGE.resize((W, H), Image.LANCZOS))),
                                        torch.from_numpy(arrays(plain)[0]), lift.LiftConfig())
    assert abs(report[0]["fallback_fraction"] - float(cells[..., 6].double().mean())) < 1e-9
    # other settings reach the passes: no gate (and no Lanczos pass), another radius and gain
    for lift_kw in (dict(gate=None), dict(radius=2, eps=4.0, gate=(1.0, 100.0), max_gain=2.0)):
        got, report = lifted(pipe, IMAGE, kw, lift_kw=lift_kw)
        assert np.array_equal(arrays(got)[0], second_implementation(plain, [IMAGE], lift.LiftConfig(**lift_kw))[0])
        if lift_kw.get("gate", 0) is None:
            assert report[0]["fallback_fraction"] == 0.0


def test_two_images_of_two_sizes(pipe):
    other = photo((150, 180), seed=11)
    kw = inputs(n=2)
    plain = call(pipe, [IMAGE, other], kw)
    got, report = lifted(pipe, [IMAGE, other], kw)
    want = second_implementation(plain, [IMAGE, other])
    got = arrays(got)
    assert got[0].shape[1:3] == (150, 203) and got[1].shape[1:3] == (180, 150)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    check_report(report, [IMAGE.size, other.size])
    pipe.enable_detail_lift()
    try:
        with pytest.raises(ValueError, match="one size"):
            call(pipe, [IMAGE, other], kw, "np")
    finally:
        pipe.disable_detail_lift()


def test_region_composite_keeps_the_photo_beyond_the_masks_neighbourhood(pipe):
    kw = inputs()
    r = 2
    mask = np.zeros((H, W), np.uint8)
    mask[40:56, 8:24] = 255
    pipe.set_edit_region(Image.fromarray(mask), composite=True)
    try:
        plain = call(pipe, IMAGE, kw)
        got, report = lifted(pipe, IMAGE, kw, lift_kw=dict(radius=r))
    finally:
        pipe.clear_edit_region()
    got = arrays(got)[0]
    assert np.array_equal(got, second_implementation(plain, [IMAGE], lift.LiftConfig(radius=r))[0])
    check_report(report, [IMAGE.size])
    # the edit-size frames carry the resized photo's bytes where the mask is 0: beyond 3 r + 1 cells of it the lifted pixel is the photo's
    ix0, ix1, _, iy0, iy1, _ = (t.numpy().astype(np.int64) for t in lift.tables(IMAGE.size, (H, W)))
    m = 3 * r + 1
    far = ((iy1 < 40 - m) | (iy0 >= 56 + m))[:, None] | ((ix1 < 8 - m) | (ix0 >= 24 + m))[None, :]
    src = np.array(IMAGE)
    assert far.mean() > 0.5
    for f in got:
        assert np.array_equal(f[far], src[far])
    assert not np.array_equal(got[-1][~far], src[~far])


def test_temporal_reasoning_lifts_every_returned_frame(pipe):
    kw = inputs(frames=29)
    more = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    plain = call(pipe, IMAGE, kw, **more)
    got, report = lifted(pipe, IMAGE, kw, **more)
    got = arrays(got)[0]
    assert len(plain[0]) == 29 and got.shape == (29, 150, 203, 3)
    assert np.array_equal(got, second_implementation(plain, [IMAGE])[0])
    check_report(report, [IMAGE.size])


def test_auto_focus_declined_is_lifted_and_accepted_is_the_focused_call(pipe):
    kw = inputs()
    pipe.enable_auto_region(detect_step=0)
    try:
        call(pipe, IMAGE, kw, "latent")
        dmax = float(pipe.auto_region_report["dmax"])
    finally:
        pipe.disable_auto_region()
    det = dict(detect_step=0, threshold=math.sqrt(dmax) * (1 - 1e-3), dilate=1, feather=1, max_area=1.0)  # one seed cell: a compact region
    # declined (the region may cover 1 % of the image at most): the auto-region call, lifted
    pipe.enable_auto_region(**dict(det, max_area=0.01)).enable_auto_focus(0.0)
    try:
        plain = call(pipe, IMAGE, kw)
        assert pipe.focus_report[0]["reason"] == "declined" and plain[0][0].size == (W, H)
        got, report = lifted(pipe, IMAGE, kw)
        assert pipe.focus_report[0]["reason"] == "declined"
    finally:
        pipe.disable_auto_region().disable_auto_focus()
    got = arrays(got)[0]
    assert got.shape == (5, 150, 203, 3) and np.array_equal(got, second_implementation(plain, [IMAGE])[0])
    check_report(report, [IMAGE.size])
    # accepted: the focused call, bit for bit; the lift stands back
    pipe.enable_auto_region(**det).enable_auto_focus(0.0)
    try:
        focused = call(pipe, IMAGE, kw)
        assert pipe.focus_report[0]["reason"] == "ok" and focused[0][0].size == IMAGE.size
        got, report = lifted(pipe, IMAGE, kw)
        assert pipe.focus_report[0]["reason"] == "ok"
    finally:
        pipe.disable_auto_region().disable_auto_focus()
    assert np.array_equal(arrays(got)[0], arrays(focused)[0])
    check_report(report, [IMAGE.size], applied=False, reason="focus")


def test_an_explicit_focus_wins(pipe):
    kw = inputs()
    mask = np.zeros((150, 203), np.uint8)
    mask[8:58, 130:196] = 255
    pipe.enable_region_focus().set_edit_region(Image.fromarray(mask))
    try:
        focused = call(pipe, IMAGE, kw)
        got, report = lifted(pipe, IMAGE, kw)
    finally:
        pipe.disable_region_focus().clear_edit_region()
    assert np.array_equal(arrays(got)[0], arrays(focused)[0])
    check_report(report, [IMAGE.size], applied=False, reason="focus")


def test_np_and_pt_carry_the_pil_bytes_and_latent_is_untouched(pipe):
    kw = inputs()
    pil = arrays(lifted(pipe, IMAGE, kw)[0])[0]
    as_np, report = lifted(pipe, IMAGE, kw, "np")
    assert as_np.dtype == np.float32 and as_np.shape == (1, 5, 150, 203, 3) and np.array_equal(as_np[0], pil.astype(np.float32) / 255.0)
    check_report(report, [IMAGE.size])
    as_pt = lifted(pipe, IMAGE, kw, "pt")[0]
    assert as_pt.dtype == torch.float32 and tuple(as_pt.shape) == (1, 5, 3, 150, 203)
    assert np.array_equal(as_pt[0].permute(0, 2, 3, 1).numpy(), as_np[0])
    lat, report = lifted(pipe, IMAGE, kw, "latent")
    assert report is None and torch.equal(lat, call(pipe, IMAGE, kw, "latent"))


def test_array_and_tensor_images_are_refused(pipe):
    kw = inputs()
    for image in (np.asarray(IMAGE, dtype=np.float32) / 255.0, torch.rand(1, 3, H, W)):
        pipe.enable_detail_lift()
        try:
            with pytest.raises(ValueError, match="PIL"):
                call(pipe, image, kw, "pil", image_embeds=torch.zeros(1, 17, 320, dtype=BF, device=DEV))
        finally:
            pipe.disable_detail_lift()


def test_a_photo_of_the_edits_size_is_the_plain_call(pipe):
    kw = inputs()
    small = photo((W, H), seed=3)
    for output_type in ("pil", "np"):
        plain = call(pipe, small, kw, output_type)
        got, report = lifted(pipe, small, kw, output_type)
        if output_type == "pil":
            assert np.array_equal(arrays(got)[0], arrays(plain)[0])
        else:
            assert np.array_equal(got, plain)
        check_report(report, [(W, H)], applied=False, reason="same")
    # next to a larger photo: that sample's plain frames, the other one lifted
    kw2 = inputs(n=2)
    plain = call(pipe, [small, IMAGE], kw2)
    got, report = lifted(pipe, [small, IMAGE], kw2)
    got = arrays(got)
    assert np.array_equal(got[0], arrays(plain)[0]) and np.array_equal(got[1], second_implementation(plain[1:], [IMAGE])[0])
    assert [(r["applied"], r["reason"]) for r in report] == [(False, "same"), (True, "ok")]


def test_disabling_restores_the_plain_call(pipe):
    kw = inputs()
    plain = arrays(call(pipe, IMAGE, kw))[0]
    pipe.enable_detail_lift().disable_detail_lift()
    frames = arrays(call(pipe, IMAGE, kw))[0]
    assert pipe.lift_report is None and frames.shape == (5, H, W, 3) and np.array_equal(frames, plain)


def test_the_host_form_gives_the_same_frames(pipe):
    kw = inputs()
    on_device, dev_report = lifted(pipe, IMAGE, kw)
    pipe.enable_device_image_io(False)
    try:
        on_host, host_report = lifted(pipe, IMAGE, kw)
        no_gate = lifted(pipe, IMAGE, kw, lift_kw=dict(gate=None))[0]
    finally:
        pipe.enable_device_image_io(True)
    assert np.array_equal(arrays(on_host)[0], arrays(on_device)[0])
    assert abs(host_report[0]["fallback_fraction"] - dev_report[0]["fallback_fraction"]) < 1e-9
    assert np.array_equal(arrays(no_gate)[0], arrays(lifted(pipe, IMAGE, kw, lift_kw=dict(gate=None))[0])[0])
