"""Guided detail lift, host side (chronoedit_amd/lift.py): the entry points in the header and the signature table, the config's validation,
the box sums and axis tables against brute force and exact rationals, the three guarantees of the arithmetic on `lift.reference`, and the
quality of the lift on a synthetic photo against the plain Lanczos upsample.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import hiplib
from chronoedit_amd import lift

ENTRY_POINTS = ("ce_lift_fit_q16", "ce_lift_smooth_f32", "ce_lift_gate_f32", "ce_lift_apply_u8")


def test_the_c_abi_declares_the_lift_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_lift_")] == list(ENTRY_POINTS)
    assert "ce_lift.hip" in hiplib.SOURCES


def test_config_defaults_and_validation():
    c = lift.LiftConfig()
    assert (c.radius, c.eps, c.gate, c.max_gain, c.eps_q) == (4, 26.0, (4.0, 12.0), 8.0, 26)
    c = lift.LiftConfig(radius=16, eps=0.2, gate=None, max_gain=1)
    assert (c.radius, c.eps_q, c.gate, c.max_gain) == (16, 1, None, 1.0)
    assert lift.LiftConfig(eps=2.5).eps_q == 2 and lift.LiftConfig(eps=3.5).eps_q == 4  # rint: halves to even
    assert lift.LiftConfig(gate=[0, 1]).gate == (0.0, 1.0)
    bad = [dict(radius=0), dict(radius=17), dict(radius=4.0), dict(radius=True), dict(eps=0), dict(eps=-1.0), dict(eps=float("nan")),
           dict(eps=float("inf")), dict(eps="1"), dict(gate=(4.0,)), dict(gate=(4.0, 4.0)), dict(gate=(5.0, 4.0)), dict(gate=(-1.0, 4.0)),
           dict(gate=(0.0, float("inf"))), dict(gate=(0.0, float("nan"))), dict(gate=4.0), dict(max_gain=0.5), dict(max_gain=8.5),
           dict(max_gain=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            lift.LiftConfig(**kw)


def test_the_pipeline_switch():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline()
    assert pipe._detail_lift is None and pipe.lift_report is None
    assert pipe.enable_detail_lift() is pipe and pipe._detail_lift == lift.LiftConfig()
    assert pipe.enable_detail_lift(radius=2, eps=9.0, gate=None, max_gain=4.0)._detail_lift == lift.LiftConfig(2, 9.0, None, 4.0)
    with pytest.raises(ValueError):
        pipe.enable_detail_lift(radius=0)
    assert pipe.disable_detail_lift() is pipe and pipe._detail_lift is None


@pytest.mark.parametrize("r", [1, 3, 16])
def test_box_sums_against_brute_force(r):
    H, W = 7, 9
    x = torch.from_numpy(np.random.default_rng(r).integers(-1000, 1000, (2, H, W)))
    got, n = lift.box_sum(x, r), lift.box_count(H, W, r)
    assert got.dtype == torch.int64 and n.dtype == torch.int64
    for y in range(H):
        for xx in range(W):
            ys, xs = range(max(y - r, 0), min(y + r, H - 1) + 1), range(max(xx - r, 0), min(xx + r, W - 1) + 1)
            assert int(n[y, xx]) == len(ys) * len(xs)
            for k in range(2):
                assert int(got[k, y, xx]) == sum(int(x[k, a, b]) for a in ys for b in xs)
    if r == 16:  # the window holds the whole image
        assert bool((n == H * W).all()) and bool((got == x.sum((1, 2), keepdim=True)).all())


@pytest.mark.parametrize("n,n_out", [(19, 53), (24, 96), (96, 24)])
def test_axis_tables_against_exact_rationals(n, n_out):
    i0, i1, t = lift.axis_table(n_out, n)
    assert (i0.dtype, i1.dtype, t.dtype) == (torch.int32, torch.int32, torch.float32) and len(i0) == len(i1) == len(t) == n_out
    for o in range(n_out):
        u = (Fraction(o) + Fraction(1, 2)) * Fraction(n, n_out) - Fraction(1, 2)
        u = min(max(u, Fraction(0)), Fraction(n - 1))
        a = int(u // 1)
        assert (int(i0[o]), int(i1[o])) == (a, min(a + 1, n - 1)) and float(t[o]) == float(np.float32(float(u - a)))
    assert 0.0 <= float(t.min()) and float(t.max()) < 1.0
    same = lift.axis_table(n, n)  # the identity
    assert same[0].tolist() == list(range(n)) and not bool(same[2].any())


def _rand_u8(rng, *shape):
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def _pil_resize(a, size):
    return torch.from_numpy(np.array(Image.fromarray(a.numpy()).resize(size, Image.LANCZOS)))


def test_an_identity_edit_returns_the_photo():
    rng = np.random.default_rng(0)
    P = _rand_u8(rng, 37, 53, 3)
    L = _pil_resize(P, (19, 13))
    E = torch.stack([L, L])
    U = _rand_u8(rng, 2, 37, 53, 3)  # whatever the fallback plane holds: g is 0
    for cfg in (lift.LiftConfig(), lift.LiftConfig(radius=1, gate=(0.0, 1.0)), lift.LiftConfig(radius=16, gate=None)):
        out, coef = lift.reference(P, L, E, U, cfg, return_coef=True)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 37, 53, 3)
        assert torch.equal(out, torch.stack([P, P])) and not bool(coef.any())


def test_a_replaced_rectangle_is_the_upsample_in_its_core_and_the_photo_away_from_it():
    rng = np.random.default_rng(1)
    H, W, SH, SW, r = 64, 96, 256, 384, 4
    P = _rand_u8(rng, SH, SW, 3)
    L = _pil_resize(P, (W, H))
    top, left, rh, rw = 20, 30, 24, 36
    E = L.clone()
    E[top:top + rh, left:left + rw] = _rand_u8(rng, rh, rw, 3)
    U = _pil_resize(E, (SW, SH))
    cfg = lift.LiftConfig(radius=r)
    out, coef = lift.reference(P, L, E[None], U[None], cfg, return_coef=True)
    out = out[0]
    ix0, ix1, _, iy0, iy1, _ = lift.tables((SW, SH), (H, W))
    m = 3 * r + 1
    # the photo's own bytes: every pixel whose four corners lie more than 3 r + 1 cells from the rectangle
    far_y = (iy1.long() < top - m) | (iy0.long() >= top + rh + m)
    far_x = (ix1.long() < left - m) | (ix0.long() >= left + rw + m)
    far = far_y.view(-1, 1) | far_x.view(1, -1)
    assert int(far.sum()) > SH * SW // 3 and torch.equal(out[far], P[far])
    # U's bytes: every pixel whose four corners all have g == 1 - and the rectangle's core does
    g = coef[0, :, :, 6]
    one = g == 1.0
    assert bool(one[top + 2 * r:top + rh - 2 * r, left + 2 * r:left + rw - 2 * r].all())
    ya, yb, xa, xb = iy0.long().view(-1, 1), iy1.long().view(-1, 1), ix0.long().view(1, -1), ix1.long().view(1, -1)
    core = one[ya, xa] & one[ya, xb] & one[yb, xa] & one[yb, xb]
    assert int(core.sum()) > 16 * (rh - 4 * r) * (rw - 4 * r) // 2 and torch.equal(out[core], U[core])
    assert not torch.equal(out, P) and not torch.equal(out, U)


def test_without_a_gate_nothing_falls_back():
    rng = np.random.default_rng(2)
    P = _rand_u8(rng, 37, 53, 3)
    L = _pil_resize(P, (19, 13))
    E = _rand_u8(rng, 1, 13, 19, 3)
    cfg = lift.LiftConfig(radius=2, gate=None)
    out, coef = lift.reference(P, L, E, None, cfg, return_coef=True)  # no U needed
    assert not bool(coef[..., 6:].any()) and bool(coef[..., :6].any())
    U = _rand_u8(rng, 1, 37, 53, 3)
    assert torch.equal(out, lift.reference(P, L, E, U, cfg))  # and a U that is passed is not read
    with pytest.raises(ValueError):
        lift.reference(P, L, E, None, lift.LiftConfig(radius=2))
    gated = lift.reference(P, L, E, U, lift.LiftConfig(radius=2, gate=(0.0, 1.0)))
    assert not torch.equal(gated, out)


def test_the_stages_keep_their_ranges():
    """Random frames against a random source: |A| <= 65536 max_gain, R <= 255 * 256, g in [0, 1], and the statistics stay far below 2^53."""
    rng = np.random.default_rng(3)
    L, E = _rand_u8(rng, 13, 19, 3), _rand_u8(rng, 2, 13, 19, 3)
    E[1] = torch.where(L < 128, torch.tensor(255, dtype=torch.uint8), torch.tensor(0, dtype=torch.uint8))  # d = +-(255 - I) or -I: steep maps
    for cfg in (lift.LiftConfig(radius=1, eps=1.0, max_gain=2.0), lift.LiftConfig(radius=16)):
        AB = lift.fit_reference(L, E, cfg)
        assert AB.dtype == torch.int32 and tuple(AB.shape) == (2, 13, 19, 6) and int(AB[..., :3].abs().max()) <= int(65536 * cfg.max_gain)
        coef, R = lift.smooth_reference(L, E, AB, cfg)
        assert R.dtype == torch.int32 and 0 <= int(R.min()) and int(R.max()) <= 255 * 256
        g = lift.gate_reference(R, cfg)
        assert 0.0 <= float(g.min()) and float(g.max()) <= 1.0
    assert int(lift.fit_reference(L, E, lift.LiftConfig(radius=1, eps=1.0, max_gain=2.0))[..., :3].abs().max()) == 131072  # the clamp is hit


# ---- quality: the lift against the plain Lanczos upsample, measured against the edit applied to the photo itself ---------------------
def synthetic_photo(seed=0, W=384, H=256):
    """Per colour a smooth sinusoid (period 100 px), +-35 square-wave stripes (period 20 px) along a diagonal, normal grain of sigma 12, six
    random rectangles of 8..40 px with an offset in +-60; rounded and clipped to bytes."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((H, W, 3))
    for c in range(3):
        img[..., c] = 128 + 60 * np.sin(2 * np.pi * (x + 0.5 * y) / 100.0 + c) + 35 * np.sign(np.sin(2 * np.pi * (x + y) / 20.0 + 0.7 * c))
    img += rng.normal(0, 12, img.shape)
    for _ in range(6):
        h, w = rng.integers(8, 41, 2)
        t, l = rng.integers(0, H - h), rng.integers(0, W - w)
        img[t:t + h, l:l + w] += rng.uniform(-60, 60, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _vignette(a):
    h, w = a.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    r2 = ((x + 0.5) / w - 0.5) ** 2 + ((y + 0.5) / h - 0.5) ** 2
    return a * (1 - 1.2 * r2)[..., None]


EDITS = {
    "affine colour map": lambda a: a * np.array([1.1, 0.9, 0.8]) + np.array([10.0, -5.0, 20.0]),
    "gamma 0.7": lambda a: 255.0 * (a / 255.0) ** 0.7,
    "inversion": lambda a: 255.0 - a,
    "vignette": _vignette,
}


@pytest.fixture(scope="module")
def quality_photo():
    P = synthetic_photo()
    return P, np.asarray(Image.fromarray(P).resize((96, 64), Image.LANCZOS))


@pytest.mark.parametrize("name", list(EDITS))
def test_the_lift_beats_the_lanczos_upsample_four_times(quality_photo, name):
    """Measured with lift.reference (defaults; rms in bytes, lift / Lanczos upsample / ratio): affine colour map 0.43 / 17.8 / 41,
    gamma 0.7 2.78 / 17.4 / 6.3, inversion 1.25 / 19.1 / 15, vignette 2.11 / 15.5 / 7.3."""
    P, L = quality_photo
    T = EDITS[name]
    byte = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    E, truth = byte(T(L.astype(np.float64))), byte(T(P.astype(np.float64))).astype(np.float64)
    U = np.asarray(Image.fromarray(E).resize((384, 256), Image.LANCZOS))
    out = lift.reference(torch.from_numpy(P), torch.from_numpy(L.copy()), torch.from_numpy(E)[None], torch.from_numpy(U.copy())[None])[0].numpy()
    rms = lambda a: float(np.sqrt(((a.astype(np.float64) - truth) ** 2).mean()))
    print(f"{name}: lift {rms(out):.3f}, upsample {rms(U):.3f}, ratio {rms(U) / rms(out):.2f}")
    assert rms(out) <= rms(U) / 4
