"""The detail lift inside focus boxes through `ChronoEditPipeline.__call__` (`enable_detail_lift(focus=True)`), on the tiny synthetic
pipeline of tests/test_lift_gpu.py: a 406 x 300 photo and a mask of about 150 x 100 pixels, so that the box holds 2.75 photo pixels per edit
pixel.  Every case is byte-equal to a second implementation from public pieces: the plain region call on `image.crop(box)` with the mask's
crop (its "pil" frames are E), PIL's Lanczos for L and U, `lift.reference` on the CPU, PIL's `paste` through the photo-size mask.  (The
synthetic VAE decodes noise: the gate is near 1 and the lifted box near the upsample; what is checked here is the wiring - the definition
is checked in tests/test_boxlift_cpu.py, the fused pass in tests/test_exact_boxlift_gpu.py.)"""
import math

import numpy as np
import pytest
import test_lift_gpu as T
import torch
from PIL import Image
from test_lift_gpu import pipe  # noqa: F401  (fixture)
from test_sketch_gpu import draw

from chronoedit_amd import boxlift, lift

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
assert (W, H) == (96, 64)
PHOTO = T.photo((406, 300), seed=21)
REPORT_KEYS = {"size", "edit_size", "applied", "reason", "fallback_fraction", "box", "scale"}


def blob(size, rows, cols, seed=3):
    """An "L" mask of the photo's size: random greys over the blob, 255 in its core, 0 elsewhere."""
    m = np.zeros((size[1], size[0]), np.uint8)
    m[rows[0]:rows[1], cols[0]:cols[1]] = np.random.default_rng(seed).integers(1, 256, (rows[1] - rows[0], cols[1] - cols[0]), dtype=np.uint8)
    m[rows[0] + 8:rows[1] - 8, cols[0] + 8:cols[1] - 8] = 255
    return Image.fromarray(m)


MASK = blob(PHOTO.size, (60, 160), (200, 350))  # 150 x 100, towards the right edge: the box is shifted into the photo
BOX = (142, 22, 406, 198)  # 264 x 176: scale 2.75


def t(im):
    return torch.from_numpy(np.array(im, dtype=np.uint8))


def repeated(kw, rows):
    idx = torch.tensor(rows)
    return dict(kw, **{k: kw[k].index_select(0, idx.to(kw[k].device)) for k in ("prompt_embeds", "negative_prompt_embeds", "latents")})


def lifted(pipe, image, kw, output_type="pil", focus=True, **lift_kw):  # noqa: F811
    """One call with the lift on -> (frames, lift_report, focus_report); whatever focuses the call is the caller's switch."""
    pipe.enable_detail_lift(focus=focus, **lift_kw)
    try:
        out = T.call(pipe, image, kw, output_type)
        return out, pipe.lift_report, pipe.focus_report
    finally:
        pipe.disable_detail_lift()


def region_focused(pipe, image, mask, kw, output_type="pil", composite=True, lift_on=True, focus=True, **lift_kw):  # noqa: F811
    pipe.enable_region_focus(0.25).set_edit_region(mask, composite=composite)
    try:
        if lift_on:
            return lifted(pipe, image, kw, output_type, focus, **lift_kw)
        return T.call(pipe, image, kw, output_type), pipe.lift_report, pipe.focus_report
    finally:
        pipe.disable_region_focus().clear_edit_region()


def crop_frames(pipe, images, masks, boxes, kw):  # noqa: F811
    """E per crop: the plain region call (no composite, no focus, no lift) on the crops with the masks' crops -> per crop its PIL frames."""
    assert pipe._region_focus is None and pipe._detail_lift is None and pipe._sketch_region is None and pipe._auto_focus is None
    crops = [im.crop(box) for im, box in zip(images, boxes)]
    cmasks = [m.crop(box) for m, box in zip(masks, boxes)]
    pipe.set_edit_region(cmasks if len(crops) > 1 else cmasks[0], composite=False)
    try:
        frames = T.call(pipe, crops if len(crops) > 1 else crops[0], kw)
    finally:
        pipe.clear_edit_region()
    assert all(f.size == (W, H) for sample in frames for f in sample)
    return frames


def second_implementation(source, images, masks, boxes, frames, cfg=None, paste_mask=True):
    """One canvas: per crop, in order, L and U by PIL's Lanczos, lift.reference on the crop of the image the VAE saw, PIL's paste into the
    source through the photo-size mask -> (uint8 [F, SH, SW, 3], per crop the mean of g)."""
    cfg = cfg or lift.LiftConfig()
    canvases = [source.convert("RGB").copy() for _ in frames[0]]
    means = []
    for im, m, (l, tt, r, b), sample in zip(images, masks, boxes, frames):
        P, L = t(im.crop((l, tt, r, b))), t(im.crop((l, tt, r, b)).resize((W, H), Image.LANCZOS))
        E = torch.stack([t(f) for f in sample])
        U = None if cfg.gate is None else torch.stack([t(f.resize((r - l, b - tt), Image.LANCZOS)) for f in sample])
        Q, coef = lift.reference(P, L, E, U, cfg, return_coef=True)
        means.append(float(coef[..., 6].double().mean()))
        for f, canvas in enumerate(canvases):
            canvas.paste(Image.fromarray(Q[f].numpy()), (l, tt), m.crop((l, tt, r, b)) if paste_mask else None)
    return np.stack([np.asarray(c) for c in canvases]), means


def check_report(report, boxes, means=None, reason="ok"):
    assert len(report) == len(boxes)
    for i, (rep, (l, tt, r, b)) in enumerate(zip(report, boxes)):
        assert set(rep) == REPORT_KEYS
        assert (rep["size"], rep["edit_size"], rep["box"], rep["scale"]) == ((r - l, b - tt), (W, H), (l, tt, r, b), (r - l) / W)
        assert (rep["applied"], rep["reason"]) == (reason == "ok", reason)
        if reason != "ok":
            assert rep["fallback_fraction"] is None
        elif means is not None:
            assert abs(rep["fallback_fraction"] - means[i]) < 1e-9


@pytest.fixture(scope="module")
def explicit(pipe):  # noqa: F811
    """The shared reference of the explicit-mask cases: E of the crop, computed once."""
    kw = T.inputs()
    return kw, crop_frames(pipe, [PHOTO], [MASK], [BOX], kw)


@pytest.mark.parametrize("use_graph,composite,lift_kw", [(True, True, {}), (False, True, {}), (True, False, {}), (True, True, dict(gate=None)),
                                                         (True, True, dict(radius=2, eps=4.0, gate=(1.0, 100.0), max_gain=2.0))],
                         ids=["replayed", "eager", "whole-box", "no-gate", "other-settings"])
def test_an_explicit_mask_equals_the_second_implementation(pipe, explicit, use_graph, composite, lift_kw):  # noqa: F811
    kw, frames = explicit
    pipe.use_graph = use_graph
    try:
        got, report, freport = region_focused(pipe, PHOTO, MASK, kw, composite=composite, **lift_kw)
    finally:
        pipe.use_graph = True
    assert freport[0]["box"] == BOX and freport[0]["reason"] == "ok" and freport[0]["scale"] == 2.75  # the box is larger than the edit
    want, means = second_implementation(PHOTO, [PHOTO], [MASK], [BOX], frames, lift.LiftConfig(**lift_kw), paste_mask=composite)
    got = T.arrays(got)[0]
    assert got.shape == (5, 300, 406, 3) and np.array_equal(got, want)
    check_report(report, [BOX], means)
    if lift_kw.get("gate", 0) is None:
        assert report[0]["fallback_fraction"] == 0.0
    src = np.array(PHOTO)
    keep = np.array(MASK) == 0
    if composite:
        assert all(np.array_equal(f[keep], src[keep]) for f in got)  # the photo's bytes wherever the mask is 0
    else:
        outside = np.ones(src.shape[:2], bool)
        outside[BOX[1]:BOX[3], BOX[0]:BOX[2]] = False
        assert all(np.array_equal(f[outside], src[outside]) for f in got) and not np.array_equal(got[-1][~outside & keep], src[~outside & keep])


def test_focus_false_is_todays_focused_call_and_focus_true_is_not(pipe, explicit):  # noqa: F811
    kw, _ = explicit
    today, none_report, _ = region_focused(pipe, PHOTO, MASK, kw, lift_on=False)
    assert none_report is None
    off, report, _ = region_focused(pipe, PHOTO, MASK, kw, focus=False)
    assert np.array_equal(T.arrays(off)[0], T.arrays(today)[0])
    T.check_report(report, [PHOTO.size], applied=False, reason="focus")  # today's five keys, today's size
    on, _, _ = region_focused(pipe, PHOTO, MASK, kw, gate=None)  # (the synthetic VAE's noise opens the default gate: the lifted box is then the upsample)
    assert not np.array_equal(T.arrays(on)[0], T.arrays(today)[0])


def test_the_host_path_gives_the_same_bytes(pipe, explicit):  # noqa: F811
    kw, _ = explicit
    on_device, dev_report, _ = region_focused(pipe, PHOTO, MASK, kw)
    pipe.enable_device_image_io(False)
    try:
        on_host, host_report, _ = region_focused(pipe, PHOTO, MASK, kw)
        no_gate, _, _ = region_focused(pipe, PHOTO, MASK, kw, gate=None)
    finally:
        pipe.enable_device_image_io(True)
    assert np.array_equal(T.arrays(on_host)[0], T.arrays(on_device)[0])
    assert abs(host_report[0]["fallback_fraction"] - dev_report[0]["fallback_fraction"]) < 1e-9
    assert {k: v for k, v in host_report[0].items() if k != "fallback_fraction"} == {k: v for k, v in dev_report[0].items() if k != "fallback_fraction"}
    assert np.array_equal(T.arrays(no_gate)[0], T.arrays(region_focused(pipe, PHOTO, MASK, kw, gate=None)[0])[0])


def test_np_and_pt_carry_the_pil_bytes(pipe, explicit):  # noqa: F811
    kw, _ = explicit
    pil = T.arrays(region_focused(pipe, PHOTO, MASK, kw)[0])[0]
    as_np, report, _ = region_focused(pipe, PHOTO, MASK, kw, "np")
    assert as_np.dtype == np.float32 and as_np.shape == (1, 5, 300, 406, 3) and np.array_equal(as_np[0], pil.astype(np.float32) / 255.0)
    check_report(report, [BOX])
    as_pt = region_focused(pipe, PHOTO, MASK, kw, "pt")[0]
    assert as_pt.dtype == torch.float32 and tuple(as_pt.shape) == (1, 5, 3, 300, 406)
    assert np.array_equal(as_pt[0].permute(0, 2, 3, 1).numpy(), as_np[0])
    lat, report, _ = region_focused(pipe, PHOTO, MASK, kw, "latent")
    assert report is None and lat.shape[1] == 16


def test_two_photos_of_two_sizes(pipe):  # noqa: F811
    other = T.photo((300, 380), seed=11)
    other_mask = blob(other.size, (200, 330), (30, 120), seed=4)
    kw = T.inputs(n=2)
    got, report, freport = region_focused(pipe, [PHOTO, other], [MASK, other_mask], kw)
    boxes = [r["box"] for r in freport]
    assert boxes[0] == BOX and boxes[1] != BOX and all(r["reason"] == "ok" and r["scale"] > 1.5 for r in freport)
    frames = crop_frames(pipe, [PHOTO, other], [MASK, other_mask], boxes, kw)
    got = T.arrays(got)
    assert got[0].shape[1:3] == (300, 406) and got[1].shape[1:3] == (380, 300)
    means = []
    for i, (im, m) in enumerate(((PHOTO, MASK), (other, other_mask))):
        want, mean = second_implementation(im, [im], [m], [boxes[i]], [frames[i]])
        assert np.array_equal(got[i], want)
        means += mean
    check_report(report, boxes, means)
    pipe.enable_region_focus(0.25).set_edit_region([MASK, other_mask])
    try:
        pipe.enable_detail_lift(focus=True)
        with pytest.raises(ValueError, match="one size"):  # focus's rule
            T.call(pipe, [PHOTO, other], kw, "np")
    finally:
        pipe.disable_detail_lift().disable_region_focus().clear_edit_region()


def test_a_box_of_the_edits_size_is_todays_paste(pipe):  # noqa: F811
    small_mask = blob(T.IMAGE.size, (20, 50), (120, 160))  # 40 x 30 in a 203 x 150 photo: the box is raised to 96 x 64, nothing more
    kw = T.inputs()
    today, _, freport = region_focused(pipe, T.IMAGE, small_mask, kw, lift_on=False)
    box = freport[0]["box"]
    assert (box[2] - box[0], box[3] - box[1]) == (W, H) and freport[0]["scale"] == 1.0
    got, report, _ = region_focused(pipe, T.IMAGE, small_mask, kw)
    assert np.array_equal(T.arrays(got)[0], T.arrays(today)[0])
    check_report(report, [box], reason="same")


def test_an_accepted_auto_focus(pipe):  # noqa: F811
    kw = T.inputs()
    pipe.enable_auto_region(detect_step=0)
    try:
        T.call(pipe, PHOTO, kw, "latent")
        dmax = float(pipe.auto_region_report["dmax"])
    finally:
        pipe.disable_auto_region()
    det = dict(detect_step=0, threshold=math.sqrt(dmax) * (1 - 1e-3), dilate=1, feather=1, max_area=1.0)  # one seed cell: a compact region
    pipe.enable_auto_region(**det).enable_auto_focus(0.25)
    try:
        got, report, freport = lifted(pipe, PHOTO, kw)
    finally:
        pipe.disable_auto_region().disable_auto_focus()
    rep = freport[0]
    assert rep["reason"] == "ok" and rep["scale"] > 1.0 and rep["mask"].size == PHOTO.size, rep
    frames = crop_frames(pipe, [PHOTO], [rep["mask"]], [rep["box"]], kw)
    want, means = second_implementation(PHOTO, [PHOTO], [rep["mask"]], [rep["box"]], frames)
    assert np.array_equal(T.arrays(got)[0], want)
    check_report(report, [rep["box"]], means)


STROKES = [(200, 60, 350, 70), (200, 60, 210, 160), (340, 100, 350, 160)]  # about 150 x 100
SKETCH = {"background": PHOTO, "composite": draw(PHOTO, STROKES, faint=5)}  # a lossy composite: it differs from the photo everywhere
NW, SE = (20, 20, 50, 40), (356, 250, 386, 280)
TWO = {"background": PHOTO, "composite": draw(PHOTO, [NW, SE], faint=5)}


def sketched(pipe, value, kw, lift_kw=None, **switch):  # noqa: F811
    pipe.enable_sketch_region(**dict(dict(grow=3, feather=4, threshold=5), **switch))
    try:
        got, report, _ = lifted(pipe, value, kw, **(lift_kw or {}))
        return got, report, pipe.sketch_report
    finally:
        pipe.disable_sketch_region()


def test_a_sketch_edit_lifts_the_composite_and_pastes_into_the_background(pipe):  # noqa: F811
    kw = T.inputs()
    cfg = lift.LiftConfig(gate=(1.0, 100.0))  # a gate that stays half open on the synthetic VAE's noise: P and U both show in the bytes
    got, report, sreport = sketched(pipe, SKETCH, kw, dict(gate=cfg.gate))
    rep = sreport[0]
    box, mask = rep["box"], rep["mask"]
    assert rep["reason"] == "ok" and rep["scale"] > 2.0
    bg, cp = SKETCH["background"], SKETCH["composite"]
    frames = crop_frames(pipe, [cp], [mask], [box], kw)
    want, means = second_implementation(bg, [cp], [mask], [box], frames, cfg)  # P from the composite, the paste into the background
    got = T.arrays(got)[0]
    assert np.array_equal(got, want)
    check_report(report, [box], means)
    keep = np.array(mask) == 0
    assert all(np.array_equal(f[keep], np.array(bg)[keep]) for f in got)
    assert 0.0 < report[0]["fallback_fraction"] < 1.0
    assert not np.array_equal(want, second_implementation(bg, [bg], [mask], [box], frames, cfg)[0])  # (P from the background would show)


def test_two_crops_chain_into_one_photo_with_one_gate_read(pipe, monkeypatch):  # noqa: F811
    kw = T.inputs()
    reads = []
    real = boxlift.gate_means
    monkeypatch.setattr(boxlift, "gate_means", lambda means: reads.append(len(means)) or real(means))
    got, report, sreport = sketched(pipe, TWO, kw, max_crops=2)
    assert reads == [2]  # one read per call, for both crops
    rep = sreport[0]
    assert rep["crops_reason"] == "crops" and len(rep["crops"]) == 2
    boxes, masks = [c["box"] for c in rep["crops"]], [c["mask"] for c in rep["crops"]]
    assert all(1.0 < c["scale"] < 1.5 for c in rep["crops"])
    bg, cp = TWO["background"], TWO["composite"]
    frames = crop_frames(pipe, [cp, cp], masks, boxes, repeated(kw, [0, 0]))
    want, means = second_implementation(bg, [cp, cp], masks, boxes, frames)
    got = T.arrays(got)
    assert len(got) == 1 and got[0].shape == (5, 300, 406, 3) and np.array_equal(got[0], want)
    check_report(report, boxes, means)
    nowhere = (np.array(masks[0]) == 0) & (np.array(masks[1]) == 0)
    assert all(np.array_equal(f[nowhere], np.array(bg)[nowhere]) for f in got[0])
    # and the single explicit call reads once as well
    del reads[:]
    region_focused(pipe, PHOTO, MASK, kw)
    assert reads == [1]


def test_two_layers_with_a_prompt_each(pipe):  # noqa: F811
    """`layer_prompts=True`: each layer's crop is lifted from ITS composite (the layer alone over the background) and its prompt row."""
    import layers_values as V
    ls = [V.layer(PHOTO.size, [NW], photo=PHOTO), V.layer(PHOTO.size, [SE], photo=PHOTO)]
    two = T.inputs(n=2)
    kw = dict(two, latents=two["latents"][:1].clone())  # two prompt rows, ONE noise row
    cfg = lift.LiftConfig(gate=(1.0, 100.0))
    got, report, sreport = sketched(pipe, {"background": PHOTO, "layers": ls}, kw, dict(gate=cfg.gate), threshold=0, strokes="layers", layer_prompts=True)
    crops = sreport[0]["crops"]
    assert [c["layer"] for c in crops] == [0, 1]
    boxes, masks = [c["box"] for c in crops], [c["mask"] for c in crops]
    composites = [V.pil_composite(PHOTO, [ly]) for ly in ls]
    frames = crop_frames(pipe, composites, masks, boxes, dict(two, latents=kw["latents"].repeat(2, 1, 1, 1, 1)))
    want, means = second_implementation(PHOTO, composites, masks, boxes, frames, cfg)
    got = T.arrays(got)
    assert len(got) == 1 and np.array_equal(got[0], want)
    check_report(report, boxes, means)
