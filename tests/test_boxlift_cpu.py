"""Guided detail lift inside focus boxes, host side (chronoedit_amd/boxlift.py): the entry point in the header and the signature table, the
switch, the definition against "lift.reference on the crop, then PIL's paste" on odd boxes, what follows from the arithmetic (an identity
edit returns the paste source, mask == 0 keeps it, mask == 255 with g == 1 gives the upsample), and the quality of the lift inside a box of
a synthetic photo against the plain paste of the Lanczos upsample.  No GPU."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

from chronoedit_amd import boxlift, hiplib, lift
from test_lift_cpu import EDITS, synthetic_photo

ENTRY_POINTS = ("ce_boxlift_apply_paste_u8",)


def test_the_c_abi_declares_the_boxlift_entry_point():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_boxlift_")] == list(ENTRY_POINTS) == list(boxlift.ENTRY_POINTS)
    assert [n for n in hiplib.SIGNATURES if n.startswith("ce_boxlift_")] == list(ENTRY_POINTS)
    assert "ce_boxlift.hip" in hiplib.SOURCES


def test_the_switch_round_trips_focus():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline()
    assert pipe._detail_lift is None and pipe._detail_lift_focus is False
    assert pipe.enable_detail_lift()._detail_lift == lift.LiftConfig() and pipe._detail_lift_focus is False  # today's call
    assert pipe.enable_detail_lift(focus=True) is pipe and pipe._detail_lift == lift.LiftConfig() and pipe._detail_lift_focus is True
    assert pipe.enable_detail_lift(radius=2, eps=9.0, gate=None, max_gain=4.0, focus=True)._detail_lift == lift.LiftConfig(2, 9.0, None, 4.0)
    assert pipe._detail_lift_focus is True
    assert pipe.enable_detail_lift()._detail_lift_focus is False  # every call sets it anew
    with pytest.raises(ValueError):
        pipe.enable_detail_lift(focus=1)
    pipe.enable_detail_lift(focus=True)
    assert pipe.disable_detail_lift() is pipe and pipe._detail_lift is None and pipe._detail_lift_focus is False


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def _rand_u8(rng, *shape):
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def _img(t):
    return Image.fromarray(t.numpy())


def _t(im):
    return torch.from_numpy(np.array(im, dtype=np.uint8))


def _stack(frames):
    return torch.stack([_t(f) for f in frames])


W, H = 19, 13


def _crop_L(photo, box):
    return _t(photo.crop(box).resize((W, H), Image.LANCZOS))


def _second(source, crops, cfg):
    """lift.reference on the crop, then PIL's paste - written out once more, crop by crop."""
    frames = [source.copy() for _ in crops[0][2]]
    for photo, L, E, mask, box in crops:
        l, t, r, b = box
        P = _t(photo)[t:b, l:r].contiguous()
        U = None if cfg.gate is None else _stack([f.resize((r - l, b - t), Image.LANCZOS) for f in E])
        Q = lift.reference(P, L, _stack(E), U, cfg)
        for f, canvas in enumerate(frames):
            canvas.paste(_img(Q[f]), (l, t), None if mask is None else _img(mask).crop(box))
    return _stack(frames)


@pytest.mark.parametrize("gate", [(4.0, 12.0), None])
@pytest.mark.parametrize("masked", [True, False])
def test_the_definition_is_the_lift_on_the_crop_then_pils_paste(gate, masked):
    rng = np.random.default_rng(0)
    SW, SH = 71, 53
    photo, source = _img(_rand_u8(rng, SH, SW, 3)), _img(_rand_u8(rng, SH, SW, 3))
    cfg = lift.LiftConfig(radius=2, gate=gate)
    crops = []
    for box in ((3, 5, 44, 33), (37, 20, 71, 53)):  # 41 x 28 and 34 x 33: odd, overlapping, the second at the photo's corner
        L = _crop_L(photo, box)
        E = [_img((L.int() + torch.from_numpy(rng.integers(-20, 21, (H, W, 3)))).clamp(0, 255).to(torch.uint8)) for _ in range(2)]
        crops.append((photo, L, E, _rand_u8(rng, SH, SW) if masked else None, box))
    got, means = boxlift.reference(source, crops, cfg)
    assert torch.equal(_stack(got), _second(source, crops, cfg))
    for (_, L, E, _, _), v in zip(crops, means):
        assert abs(float(v) - float(lift.coefficients_reference(L, _stack(E), cfg)[..., 6].double().mean())) < 1e-12
    assert not torch.equal(_stack(got)[0], _t(source))


def test_an_identity_edit_returns_the_paste_source():
    rng = np.random.default_rng(1)
    photo = _img(_rand_u8(rng, 53, 71, 3))
    box = (9, 7, 60, 42)
    L = _crop_L(photo, box)
    mask = _rand_u8(rng, 53, 71)
    for m in (mask, None):
        got, means = boxlift.reference(photo, [(photo, L, [_img(L), _img(L)], m, box)], lift.LiftConfig())
        assert all(torch.equal(_t(f), _t(photo)) for f in got) and float(means[0]) == 0.0


def test_mask_zero_keeps_the_paste_source_and_a_full_gate_under_mask_255_gives_the_upsample():
    rng = np.random.default_rng(2)
    SW, SH = 71, 53
    photo, source = _img(_rand_u8(rng, SH, SW, 3)), _img(_rand_u8(rng, SH, SW, 3))
    box = (9, 7, 60, 42)
    l, t, r, b = box
    L = _crop_L(photo, box)
    E = [_img(_rand_u8(rng, H, W, 3))]  # noise against the source: no affine map explains it
    mask = torch.zeros(SH, SW, dtype=torch.uint8)
    mask[12:30, 20:50] = 255
    mask[30:36, 20:50] = _rand_u8(rng, 6, 30)
    cfg = lift.LiftConfig(radius=2, gate=(0.0, 2.0 ** -9))  # any residual at all opens the gate completely
    got, means = boxlift.reference(source, [(photo, L, E, mask, box)], cfg)
    got = _t(got[0])
    assert torch.equal(got[mask == 0], _t(source)[mask == 0])
    assert float(means[0]) == 1.0
    U = torch.zeros(SH, SW, 3, dtype=torch.uint8)
    U[t:b, l:r] = _t(E[0].resize((r - l, b - t), Image.LANCZOS))
    assert torch.equal(got[mask == 255], U[mask == 255]) and not torch.equal(got[mask == 255], _t(source)[mask == 255])


def test_a_box_of_the_edits_size_is_the_plain_paste():
    rng = np.random.default_rng(3)
    photo = _img(_rand_u8(rng, 53, 71, 3))
    box = (9, 7, 9 + W, 7 + H)
    E = [_img(_rand_u8(rng, H, W, 3))]
    mask = _rand_u8(rng, 53, 71)
    got, means = boxlift.reference(photo, [(photo, _crop_L(photo, box), E, mask, box)], lift.LiftConfig())
    want = photo.copy()
    want.paste(E[0], box[:2], _img(mask).crop(box))
    assert means == [None] and torch.equal(_t(got[0]), _t(want))


def test_the_report_entry():
    from chronoedit_amd.focus import FocusPlan
    plan = FocusPlan(None, {"box": (3, 5, 44, 33), "scale": 41 / 19})
    e = boxlift.report_entry(plan, (W, H), "ok")
    assert e == {"size": (41, 28), "edit_size": (W, H), "applied": True, "reason": "ok", "fallback_fraction": None, "box": (3, 5, 44, 33), "scale": 41 / 19}
    assert boxlift.report_entry(plan, (W, H), "same")["applied"] is False


# ---- quality: the lift inside a box against the plain paste, measured against the edit applied to the photo itself -------------------
SW_Q, SH_Q = 768, 512
BOX_Q = (203, 121, 587, 377)  # 384 x 256: scale 4 against the 96 x 64 edit
EW, EH = 96, 64


@pytest.fixture(scope="module")
def quality():
    P = synthetic_photo(seed=0, W=SW_Q, H=SH_Q)
    photo = Image.fromarray(P)
    l, t, r, b = BOX_Q
    assert (r - l) / EW == 4.0 and (b - t) / EH == 4.0
    yy, xx = np.mgrid[0:SH_Q, 0:SW_Q]  # an ellipse with radii 120 / 80 at the box's centre (pixel centres inside it), feathered
    ell = ((xx + 0.5 - (l + r) / 2) / 120.0) ** 2 + ((yy + 0.5 - (t + b) / 2) / 80.0) ** 2 <= 1
    mask = Image.fromarray((ell * 255).astype(np.uint8)).filter(ImageFilter.BoxBlur(6))
    L = np.asarray(photo.crop(BOX_Q).resize((EW, EH), Image.LANCZOS))
    mask_edit = np.asarray(mask.crop(BOX_Q).resize((EW, EH), Image.BILINEAR)).astype(np.float64)[..., None] / 255.0
    return P, photo, mask, L, mask_edit


@pytest.mark.parametrize("blended", [False, True])
@pytest.mark.parametrize("name", list(EDITS))
def test_the_lift_inside_a_box_beats_the_pasted_upsample(quality, name, blended):
    """rms in bytes over mask > 0 against the edit applied to the photo's own pixels and pasted through the same mask, lift / upsample /
    ratio.  E = T(L) on the whole crop: affine colour map 0.32 / 16.1 / 50, gamma 0.7 2.70 / 15.7 / 5.8, inversion 1.13 / 17.3 / 15,
    vignette 0.95 / 16.3 / 17.  E blended with the edit-size mask (what a region edit's latent blend leaves: the feathered rim, where
    the fit window straddles the mask's edge, is the stated weakness): 3.09 / 16.2 / 5.3, 5.17 / 15.9 / 3.1, 15.6 / 19.7 / 1.26,
    3.00 / 16.4 / 5.5."""
    P, photo, mask, L, mask_edit = quality
    l, t, r, b = BOX_Q
    T = EDITS[name]
    byte = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    Lf = L.astype(np.float64)
    E = byte(Lf + mask_edit * (T(Lf) - Lf)) if blended else byte(T(Lf))
    truth = photo.copy()
    truth.paste(Image.fromarray(byte(T(P[t:b, l:r].astype(np.float64)))), (l, t), mask.crop(BOX_Q))  # (the vignette is the crop's own)
    plain = photo.copy()
    plain.paste(Image.fromarray(E).resize((r - l, b - t), Image.LANCZOS), (l, t), mask.crop(BOX_Q))
    got, means = boxlift.reference(photo, [(photo, torch.from_numpy(L.copy()), [Image.fromarray(E)], _t(mask), BOX_Q)], lift.LiftConfig())
    got, truth, plain, m = np.asarray(got[0]), np.asarray(truth).astype(np.float64), np.asarray(plain), np.asarray(mask)
    on = m > 0
    rms = lambda a: float(np.sqrt(((a.astype(np.float64) - truth)[on] ** 2).mean()))
    print(f"{name}{' (blended)' if blended else ''}: lift {rms(got):.3f}, upsample {rms(plain):.3f}, ratio {rms(plain) / rms(got):.2f}, "
          f"fallback {float(means[0]):.3f}")
    assert np.array_equal(got[~on], P[~on])  # the photo's bytes wherever the mask is 0
    if blended:
        assert rms(got) <= rms(plain)
    else:
        assert rms(got) <= rms(plain) / 4
