"""The mask-aware detail lift through `ChronoEditPipeline.__call__` (`enable_detail_lift(focus=True, mask_aware=True)`), on
tests/test_focus_lift_gpu.py's 406 x 300 photo with its 150 x 100 mask.  Every case is byte-equal to a second implementation from public
pieces: the plain region call on `image.crop(box)` with the mask's crop (its "pil" frames are E), PIL's Lanczos for L and U, PIL's bilinear
resize of the mask's crop for the weight plane, rimlift's two stages, `lift.gate_reference` and `lift.apply_reference` on the CPU, PIL's
`paste` through the photo-size mask.  (The synthetic VAE decodes noise: the default gate is near 1; the wiring is what is checked here - the
definition is checked in tests/test_rimlift_cpu.py, the passes in tests/test_exact_rimlift_gpu.py.)"""
import math

import numpy as np
import pytest
import test_focus_lift_gpu as FL
import test_lift_gpu as T
import torch
from PIL import Image
from test_focus_lift_gpu import explicit  # noqa: F401  (fixture: E of the crop, computed once)
from test_lift_gpu import pipe  # noqa: F401  (fixture)

from chronoedit_amd import boxlift, lift, rimlift

pytestmark = pytest.mark.gpu

W, H = FL.W, FL.H
PHOTO, MASK, BOX = FL.PHOTO, FL.MASK, FL.BOX
HALF = (1.0, 100.0)  # a gate that stays half open on the synthetic VAE's noise: the fitted maps and U both show in the bytes
t = FL.t


def second_implementation(source, images, masks, boxes, frames, cfg=None):
    """FL.second_implementation with the two masked stages: per crop, in order, the weight plane by PIL's bilinear resize of the mask's crop,
    rimlift's fit and smoothing, lift's gate and apply, PIL's paste -> (uint8 [F, SH, SW, 3], per crop the mean of g)."""
    cfg = cfg or lift.LiftConfig()
    canvases = [source.convert("RGB").copy() for _ in frames[0]]
    means = []
    for im, m, (l, tt, r, b), sample in zip(images, masks, boxes, frames):
        P, L = t(im.crop((l, tt, r, b))), t(im.crop((l, tt, r, b)).resize((W, H), Image.LANCZOS))
        M = t(m.convert("L").crop((l, tt, r, b)).resize((W, H), Image.BILINEAR))
        E = torch.stack([t(f) for f in sample])
        coef, R = rimlift.smooth_reference(L, E, rimlift.fit_reference(L, E, M, cfg), M, cfg)
        U = None
        if cfg.gate is not None:
            coef[..., 6] = lift.gate_reference(R, cfg)
            U = torch.stack([t(f.resize((r - l, b - tt), Image.LANCZOS)) for f in sample])
        Q = lift.apply_reference(P, coef, lift.tables((r - l, b - tt), (H, W)), U)
        means.append(float(coef[..., 6].double().mean()))
        for f, canvas in enumerate(canvases):
            canvas.paste(Image.fromarray(Q[f].numpy()), (l, tt), m.crop((l, tt, r, b)))
    return np.stack([np.asarray(c) for c in canvases]), means


def check_report(report, boxes, means=None, reason="ok", mask_aware=True):
    """FL.check_report's entries plus "mask_aware"."""
    assert all(set(rep) == FL.REPORT_KEYS | {"mask_aware"} and rep["mask_aware"] is mask_aware for rep in report)
    FL.check_report([{k: v for k, v in rep.items() if k != "mask_aware"} for rep in report], boxes, means, reason)


@pytest.mark.parametrize("use_graph,lift_kw", [(True, dict(gate=HALF)), (False, dict(gate=HALF)), (True, {}), (True, dict(gate=None, radius=2))],
                         ids=["replayed", "eager", "default-gate", "no-gate"])
def test_an_explicit_mask_equals_the_second_implementation(pipe, explicit, use_graph, lift_kw):  # noqa: F811
    kw, frames = explicit
    pipe.use_graph = use_graph
    try:
        got, report, freport = FL.region_focused(pipe, PHOTO, MASK, kw, mask_aware=True, **lift_kw)
    finally:
        pipe.use_graph = True
    assert freport[0]["box"] == BOX
    cfg = lift.LiftConfig(**lift_kw)
    want, means = second_implementation(PHOTO, [PHOTO], [MASK], [BOX], frames, cfg)
    got = T.arrays(got)[0]
    assert got.shape == (5, 300, 406, 3) and np.array_equal(got, want)
    check_report(report, [BOX], means)
    keep = np.array(MASK) == 0
    assert all(np.array_equal(f[keep], np.array(PHOTO)[keep]) for f in got)  # the photo's bytes wherever the mask is 0
    if "gate" in lift_kw:  # (under the default gate the synthetic VAE's noise makes both the upsample)
        assert not np.array_equal(want, FL.second_implementation(PHOTO, [PHOTO], [MASK], [BOX], frames, cfg)[0])  # the masked fit shows


def test_mask_aware_false_is_the_call_as_it_was(pipe, explicit):  # noqa: F811
    kw, frames = explicit
    for lift_kw in ({}, {"mask_aware": False}):
        got, report, _ = FL.region_focused(pipe, PHOTO, MASK, kw, gate=HALF, **lift_kw)
        want, means = FL.second_implementation(PHOTO, [PHOTO], [MASK], [BOX], frames, lift.LiftConfig(gate=HALF))  # the plain fit
        assert np.array_equal(T.arrays(got)[0], want)
        FL.check_report(report, [BOX], means)  # today's seven keys: no "mask_aware"
    pipe.enable_detail_lift(focus=True, mask_aware=True)
    pipe.enable_detail_lift(focus=True)  # every call sets it anew
    assert pipe._detail_lift_mask_aware is False
    pipe.disable_detail_lift()


def test_the_host_path_gives_the_same_bytes(pipe, explicit):  # noqa: F811
    kw, frames = explicit
    pipe.enable_device_image_io(False)
    try:
        on_host, host_report, _ = FL.region_focused(pipe, PHOTO, MASK, kw, mask_aware=True, gate=HALF)
    finally:
        pipe.enable_device_image_io(True)
    want, means = second_implementation(PHOTO, [PHOTO], [MASK], [BOX], frames, lift.LiftConfig(gate=HALF))
    assert np.array_equal(T.arrays(on_host)[0], want)
    check_report(host_report, [BOX], means)


def test_whole_boxes_and_boxes_of_the_edits_size_keep_todays_path(pipe, explicit):  # noqa: F811
    kw, frames = explicit
    got, report, _ = FL.region_focused(pipe, PHOTO, MASK, kw, composite=False, mask_aware=True, gate=HALF)
    want, means = FL.second_implementation(PHOTO, [PHOTO], [MASK], [BOX], frames, lift.LiftConfig(gate=HALF), paste_mask=False)
    assert np.array_equal(T.arrays(got)[0], want)
    check_report(report, [BOX], means, mask_aware=False)
    small_mask = FL.blob(T.IMAGE.size, (20, 50), (120, 160))  # the box is raised to 96 x 64, the edit's size
    kw1 = T.inputs()
    today, _, freport = FL.region_focused(pipe, T.IMAGE, small_mask, kw1, lift_on=False)
    box = freport[0]["box"]
    assert (box[2] - box[0], box[3] - box[1]) == (W, H)
    got, report, _ = FL.region_focused(pipe, T.IMAGE, small_mask, kw1, mask_aware=True)
    assert np.array_equal(T.arrays(got)[0], T.arrays(today)[0])
    check_report(report, [box], reason="same", mask_aware=False)


def test_a_sketch_edit(pipe):  # noqa: F811
    kw = T.inputs()
    cfg = lift.LiftConfig(gate=HALF)
    got, report, sreport = FL.sketched(pipe, FL.SKETCH, kw, dict(gate=cfg.gate, mask_aware=True))
    rep = sreport[0]
    box, mask = rep["box"], rep["mask"]
    bg, cp = FL.SKETCH["background"], FL.SKETCH["composite"]
    frames = FL.crop_frames(pipe, [cp], [mask], [box], kw)
    want, means = second_implementation(bg, [cp], [mask], [box], frames, cfg)  # P from the composite, the paste into the background
    got = T.arrays(got)[0]
    assert np.array_equal(got, want)
    check_report(report, [box], means)
    assert not np.array_equal(want, FL.second_implementation(bg, [cp], [mask], [box], frames, cfg)[0])


def test_two_crops_chain_into_one_photo_with_one_gate_read(pipe, monkeypatch):  # noqa: F811
    kw = T.inputs()
    reads = []
    real = boxlift.gate_means
    monkeypatch.setattr(boxlift, "gate_means", lambda means: reads.append(len(means)) or real(means))
    cfg = lift.LiftConfig(gate=HALF)
    got, report, sreport = FL.sketched(pipe, FL.TWO, kw, dict(gate=cfg.gate, mask_aware=True), max_crops=2)
    assert reads == [2]  # still one read per call, for both crops
    rep = sreport[0]
    assert rep["crops_reason"] == "crops" and len(rep["crops"]) == 2
    boxes, masks = [c["box"] for c in rep["crops"]], [c["mask"] for c in rep["crops"]]
    bg, cp = FL.TWO["background"], FL.TWO["composite"]
    frames = FL.crop_frames(pipe, [cp, cp], masks, boxes, FL.repeated(kw, [0, 0]))
    want, means = second_implementation(bg, [cp, cp], masks, boxes, frames, cfg)
    got = T.arrays(got)
    assert len(got) == 1 and np.array_equal(got[0], want)
    check_report(report, boxes, means)


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
        got, report, freport = FL.lifted(pipe, PHOTO, kw, gate=HALF, mask_aware=True)
    finally:
        pipe.disable_auto_region().disable_auto_focus()
    rep = freport[0]
    assert rep["reason"] == "ok" and rep["scale"] > 1.0, rep
    frames = FL.crop_frames(pipe, [PHOTO], [rep["mask"]], [rep["box"]], kw)
    want, means = second_implementation(PHOTO, [PHOTO], [rep["mask"]], [rep["box"]], frames, lift.LiftConfig(gate=HALF))
    assert np.array_equal(T.arrays(got)[0], want)
    check_report(report, [rep["box"]], means)
