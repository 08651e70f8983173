"""The mask-aware detail lift, host side (chronoedit_amd/rimlift.py): the two entry points in the header and the signature table, the switch,
what follows from the definition's arithmetic (a zero plane, an identity edit, mask == 0, the clamp of b, sums at their extremes against
exact rationals), and the quality on test_boxlift_cpu's fixture: the frames blended by the edit-size mask - what every region edit
produces - lifted with and without the weights, against the plain paste of the Lanczos upsample.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import boxlift, hiplib, lift, rimlift
from test_boxlift_cpu import BOX_Q, EDITS, quality  # noqa: F401  (the fixture: the photo, the box, the feathered ellipse)

ENTRY_POINTS = ("ce_rimlift_fit_q16", "ce_rimlift_smooth_f32")


def test_the_c_abi_declares_the_rimlift_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_rimlift_")] == list(ENTRY_POINTS) == list(rimlift.ENTRY_POINTS)
    assert [n for n in hiplib.SIGNATURES if n.startswith("ce_rimlift_")] == list(ENTRY_POINTS)
    assert "ce_rimlift.hip" in hiplib.SOURCES


def test_the_switch_round_trips_mask_aware():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline()
    assert pipe._detail_lift_mask_aware is False
    assert pipe.enable_detail_lift(focus=True)._detail_lift_mask_aware is False  # today's call
    assert pipe.enable_detail_lift(focus=True, mask_aware=True) is pipe and pipe._detail_lift_mask_aware is True and pipe._detail_lift_focus is True
    assert pipe._detail_lift == lift.LiftConfig()  # beside the configuration, not inside it
    assert pipe.enable_detail_lift(focus=True)._detail_lift_mask_aware is False  # every call sets it anew
    for bad in ({"mask_aware": True}, {"mask_aware": True, "focus": False}, {"focus": True, "mask_aware": 1}, {"focus": True, "mask_aware": None}):
        with pytest.raises(ValueError):
            pipe.enable_detail_lift(**bad)
    pipe.enable_detail_lift(focus=True, mask_aware=True)
    assert pipe.disable_detail_lift() is pipe and pipe._detail_lift is None and pipe._detail_lift_mask_aware is False


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def _rand_u8(rng, *shape):
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def _img(t):
    return Image.fromarray(t.numpy())


def _t(im):
    return torch.from_numpy(np.array(im, dtype=np.uint8))


W, H = 19, 13


def test_a_zero_plane_gives_zero_cells_and_the_change_as_the_residual():
    rng = np.random.default_rng(0)
    L, E = _rand_u8(rng, H, W, 3), _rand_u8(rng, 2, H, W, 3)
    M = torch.zeros(H, W, dtype=torch.uint8)
    cfg = lift.LiftConfig(radius=2)
    AB = rimlift.fit_reference(L, E, M, cfg)
    coef, R = rimlift.smooth_reference(L, E, AB, M, cfg)
    assert not bool(AB.any()) and not bool(coef.any())
    assert torch.equal(R, (E.int() - L.int()).abs().amax(dim=3) * 256)


@pytest.mark.parametrize("gate", [(4.0, 12.0), None])
def test_an_identity_edit_returns_the_paste_source(gate):
    rng = np.random.default_rng(1)
    photo = _img(_rand_u8(rng, 53, 71, 3))
    box = (9, 7, 60, 42)
    L = _t(photo.crop(box).resize((W, H), Image.LANCZOS))
    mask = _rand_u8(rng, 53, 71)
    cfg = lift.LiftConfig(radius=2, gate=gate)
    M = boxlift.weight_plane(mask, box, W, H)
    assert not bool(rimlift.fit_reference(L, torch.stack([L, L]), M, cfg).any())  # a = b = 0
    got, means = boxlift.reference(photo, [(photo, L, [_img(L), _img(L)], mask, box)], cfg, mask_aware=True)
    assert all(torch.equal(_t(f), _t(photo)) for f in got) and float(means[0]) == 0.0


def test_the_definition_is_the_masked_stages_on_the_crop_then_pils_paste_and_mask_zero_keeps_the_source():
    rng = np.random.default_rng(2)
    SW, SH = 71, 53
    photo, source = _img(_rand_u8(rng, SH, SW, 3)), _img(_rand_u8(rng, SH, SW, 3))
    box = (9, 7, 60, 42)
    l, t, r, b = box
    L = _t(photo.crop(box).resize((W, H), Image.LANCZOS))
    mask = torch.zeros(SH, SW, dtype=torch.uint8)
    mask[12:30, 20:50] = 255
    mask[30:36, 20:50] = _rand_u8(rng, 6, 30)
    w = boxlift.weight_plane(mask, box, W, H).double()[..., None] / 255.0  # an affine edit, tapered by the weights: the gate stays below 1
    E = [_img((L.double() + w * (s * L.double() + o)).round().clamp(0, 255).to(torch.uint8)) for s, o in ((-0.3, 40.0), (0.2, -25.0))]
    cfg = lift.LiftConfig(radius=2)
    got, means = boxlift.reference(source, [(photo, L, E, mask, box)], cfg, mask_aware=True)
    got = torch.stack([_t(f) for f in got])
    # the second implementation: PIL's own expression for the plane, the stages one by one, lift's apply, PIL's paste
    M = _t(_img(mask).crop(box).resize((W, H), Image.BILINEAR))
    assert torch.equal(M, boxlift.weight_plane(mask, box, W, H))
    Et = torch.stack([_t(f) for f in E])
    coef, R = rimlift.smooth_reference(L, Et, rimlift.fit_reference(L, Et, M, cfg), M, cfg)
    coef[..., 6] = lift.gate_reference(R, cfg)
    U = torch.stack([_t(f.resize((r - l, b - t), Image.LANCZOS)) for f in E])
    Q = lift.apply_reference(_t(photo)[t:b, l:r].contiguous(), coef, lift.tables((r - l, b - t), (H, W)), U)
    for f in range(2):
        want = source.copy()
        want.paste(_img(Q[f]), (l, t), _img(mask).crop(box))
        assert torch.equal(got[f], _t(want))
    assert abs(float(means[0]) - float(coef[..., 6].double().mean())) < 1e-12
    assert torch.equal(got[:, mask == 0], _t(source)[mask == 0][None].expand(2, -1, -1))  # every pixel whose photo-size mask is 0 is the paste source's
    plain, _ = boxlift.reference(source, [(photo, L, E, mask, box)], cfg)
    assert not torch.equal(got[0], _t(plain[0]))  # (the switch does something)
    # without a mask there is no taper to undo: the plain path, byte for byte
    a, _ = boxlift.reference(source, [(photo, L, E, None, box)], cfg, mask_aware=True)
    b_, _ = boxlift.reference(source, [(photo, L, E, None, box)], cfg)
    assert all(torch.equal(_t(x), _t(y)) for x, y in zip(a, b_))


@pytest.mark.parametrize("sign", [1, -1])
def test_b_stays_in_int32_under_a_weight_of_one_and_a_change_of_255(sign):
    L = torch.full((H, W, 3), 0 if sign > 0 else 255, dtype=torch.uint8)
    E = (255 - L)[None].contiguous()
    M = torch.ones(H, W, dtype=torch.uint8)
    AB = rimlift.fit_reference(L, E, M, lift.LiftConfig(radius=2))
    assert int(AB[..., 3:].abs().max()) <= 4096 * 65536
    if sign > 0:  # I = 0: a has nothing to explain, b = 255 d / m = 65025 is clamped
        assert bool((AB[..., 3:] == 4096 * 65536).all())


def _exact_cell(L, E, M, y, x, c, cfg):
    """The normal equations of one cell in exact rationals -> (a*, T_q, T_qI, T_md) with a* before the clamp."""
    r = cfg.radius
    Hh, Ww = M.shape
    q = qI = qII = md = mId = 0
    for yy in range(max(y - r, 0), min(y + r, Hh - 1) + 1):
        for xx in range(max(x - r, 0), min(x + r, Ww - 1) + 1):
            m, I = int(M[yy, xx]), int(L[yy, xx, c])
            d = int(E[0, yy, xx, c]) - I
            q, qI, qII, md, mId = q + m * m, qI + m * m * I, qII + m * m * I * I, md + m * d, mId + m * I * d
    a = Fraction(255 * (q * mId - qI * md), q * qII - qI * qI + cfg.eps_q * q * q)
    return a, q, qI, md, qII


@pytest.mark.parametrize("data", ["all", "mixed"])
def test_sums_at_their_extremes_agree_with_exact_rationals(data):
    """m = 255 and r = 16 on 40 x 40: "all" has I = 255, d = -255 everywhere; "mixed" has I in {0, 255} and E = 255 - I, d = +-255.  The
    roundings the definition states: a is an fp32 (relative 2^-24, doubled for the double operations under it), b is an fp32 computed from
    that a (|a| moves by an ulp: 255 times that in b), and A, B are rounded to integers."""
    rng = np.random.default_rng(5)
    n = 40
    if data == "all":
        L = torch.full((n, n, 3), 255, dtype=torch.uint8)
    else:
        L = torch.from_numpy(rng.integers(0, 2, (n, n, 3)).astype(np.uint8) * 255)
    E = (255 - L)[None].contiguous()
    M = torch.full((n, n), 255, dtype=torch.uint8)
    cfg = lift.LiftConfig(radius=16, eps=0.2)
    AB = rimlift.fit_reference(L, E, M, cfg)
    seen = 0
    for y, x, c in ((0, 0, 0), (20, 20, 1), (39, 17, 2), (16, 23, 0)):
        a, q, qI, md, qII = _exact_cell(L, E, M, y, x, c, cfg)
        if (y, x) == (20, 20):
            assert q == 1089 * 255 ** 2 and q < 2 ** 31 <= qI and (data == "mixed" or qII == 1089 * 255 ** 4)  # the window is whole: 32 bits overflow
        a = min(max(a, Fraction(-8)), Fraction(8))
        b = min(max((255 * md - a * qI) / q, Fraction(-4096)), Fraction(4096))
        ulp = Fraction(1, 2 ** 23)
        A, B = int(AB[0, y, x, c]), int(AB[0, y, x, 3 + c])
        assert abs(A - 65536 * a) <= Fraction(1, 2) + 65536 * abs(a) * ulp, (y, x, c, A, float(65536 * a))
        assert abs(B - 65536 * b) <= Fraction(1, 2) + 65536 * (abs(b) + 255 * abs(a)) * ulp, (y, x, c, B, float(65536 * b))
        seen += int(A != 0 or B != 0)
    assert seen  # (the cells say something)
    if data == "all":  # a flat source under full weight: d = -255 is all offset
        assert bool((AB[..., :3].abs() <= 1).all()) and bool(((AB[..., 3:] + 255 * 65536).abs() <= 16).all())


# ---- quality: on test_boxlift_cpu's fixture ---------------------------------------------------------------------------------------
def _measure(quality, name, weights):
    """weights: None (E = T(L) on the whole crop), or the taper float64 [EH, EW, 1] the frames are blended with -> (rms of the plain lift,
    of the masked lift, of the pasted upsample - in bytes over mask > 0 against the edit applied to the photo itself and pasted through
    the same mask -, the two gate means, whether mask == 0 kept the photo's bytes)."""
    P, photo, mask, L, _ = quality
    l, t, r, b = BOX_Q
    T = EDITS[name]
    byte = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    Lf = L.astype(np.float64)
    E = byte(T(Lf)) if weights is None else byte(Lf + weights * (T(Lf) - Lf))
    truth = photo.copy()
    truth.paste(Image.fromarray(byte(T(P[t:b, l:r].astype(np.float64)))), (l, t), mask.crop(BOX_Q))
    plain = photo.copy()
    plain.paste(Image.fromarray(E).resize((r - l, b - t), Image.LANCZOS), (l, t), mask.crop(BOX_Q))
    crop = [(photo, torch.from_numpy(L.copy()), [Image.fromarray(E)], _t(mask), BOX_Q)]
    unmasked, g0 = boxlift.reference(photo, crop, lift.LiftConfig())
    masked, g1 = boxlift.reference(photo, crop, lift.LiftConfig(), mask_aware=True)
    truth, m = np.asarray(truth).astype(np.float64), np.asarray(mask)
    on = m > 0
    rms = lambda a: float(np.sqrt(((np.asarray(a).astype(np.float64) - truth)[on] ** 2).mean()))
    kept = np.array_equal(np.asarray(masked[0])[~on], P[~on])
    return rms(unmasked[0]), rms(masked[0]), rms(plain), float(g0[0]), float(g1[0]), kept


@pytest.mark.parametrize("name", list(EDITS))
def test_the_masked_lift_recovers_the_whole_crop_quality_on_blended_frames(quality, name):
    """rms in bytes over mask > 0, lift / masked lift / upsample (fallback fractions of the two lifts).  Frames blended by the edit-size
    mask - what every region edit produces: affine 3.09 / 0.33 / 16.2, gamma 5.17 / 2.68 / 15.9, inversion 15.6 / 1.15 / 19.7, vignette
    3.00 / 1.35 / 16.4.  E = T(L) on the whole crop (no taper in the frames: the weights only shape the window) is printed beside it."""
    whole = _measure(quality, name, None)
    print(f"{name} (whole crop): lift {whole[0]:.3f}, masked lift {whole[1]:.3f}, upsample {whole[2]:.3f}, fallback {whole[3]:.3f} / {whole[4]:.3f}")
    lifted, masked, plain, g0, g1, kept = _measure(quality, name, quality[4])
    print(f"{name} (blended): lift {lifted:.3f}, masked lift {masked:.3f}, upsample {plain:.3f}, ratio {plain / masked:.2f}, fallback {g0:.3f} / {g1:.3f}")
    assert kept  # the photo's bytes wherever the mask is 0
    assert masked <= plain / 4  # the bar the whole-crop column meets without a mask
    assert masked <= lifted


@pytest.mark.parametrize("name", list(EDITS))
def test_a_mismatched_taper_falls_back_and_never_does_worse_than_the_plain_paste(quality, name):
    """The frames are blended with the 8 x 8 box mean of the plane, upsampled by nearest - the latent weights, not the mask the fit is told:
    lift / masked lift / upsample.  Only the floor is asserted: the gate hands what the tapered model misfits to the upsample."""
    w = quality[4][..., 0]
    eh, ew = w.shape
    coarse = w.reshape(eh // 8, 8, ew // 8, 8).mean(axis=(1, 3))
    lifted, masked, plain, g0, g1, kept = _measure(quality, name, np.repeat(np.repeat(coarse, 8, axis=0), 8, axis=1)[..., None])
    print(f"{name} (mismatched taper): lift {lifted:.3f}, masked lift {masked:.3f}, upsample {plain:.3f}, fallback {g0:.3f} / {g1:.3f}")
    assert kept
    assert masked <= plain
