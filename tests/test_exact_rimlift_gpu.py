"""The two passes of csrc/ce_rimlift.hip against their stages of chronoedit_amd/rimlift.py (CPU torch), bit for bit: shapes around the 16-cell
tile, one and three frames, radius 1 / 4 / 16 (windows larger than the image included), weight planes that are all 0, all 255, one non-zero
cell, a vertical ramp, random, and all 1 under d = +-255 (the clamp of b), m = I = 255 under d = +-255 at r = 16 on 40 x 40 (where 32-bit sums
overflow), a flat source (den is the eps term alone), slopes at both clamps, garbage in every output beforehand, the same bits on a second
run, the return codes, and the whole chain - fit, smooth, ce_lift_gate_f32, ce_boxlift_apply_paste_u8 - against
`boxlift.reference(mask_aware=True)` on one odd box."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import boxlift, lift, rimlift
from exact_util import assert_exact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def u8(rng, *shape):
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def frames(kind, rng, F, H, W):
    """(L uint8 [H, W, 3], E uint8 [F, H, W, 3]) of one data recipe."""
    if kind == "random":
        return u8(rng, H, W, 3), u8(rng, F, H, W, 3)
    if kind == "flat":  # a source without variance: den = eps_q T_q^2
        return torch.full((H, W, 3), 77, dtype=torch.uint8), u8(rng, F, H, W, 3)
    if kind == "extreme":  # d = +-255 everywhere: I in {0, 255}, E = 255 - I
        L = torch.from_numpy(rng.integers(0, 2, (H, W, 3)).astype(np.uint8) * 255)
        return L, (255 - L)[None].repeat(F, 1, 1, 1).contiguous()
    if kind == "white":  # I = 255, d = -255 everywhere: every product at its largest
        L = torch.full((H, W, 3), 255, dtype=torch.uint8)
        return L, torch.zeros(F, H, W, 3, dtype=torch.uint8)
    if kind == "steep":  # I in 118..138, E = 128 +- 12 (I - 128): d = E - I has the slopes 11 and -13, beyond both clamps; the sign alternates
        L = torch.from_numpy(rng.integers(118, 139, (H, W, 3), dtype=np.uint8))
        s = torch.tensor([12.0, -12.0, 12.0, -12.0, 12.0, -12.0, 12.0, -12.0, 12.0])[:3 * F].view(F, 1, 1, 3)
        return L, ((L.float() - 128.0) * s + 128.0).to(torch.uint8).contiguous()
    raise KeyError(kind)


def plane(kind, rng, H, W):
    if kind == "zero":
        return torch.zeros(H, W, dtype=torch.uint8)
    if kind == "full":
        return torch.full((H, W), 255, dtype=torch.uint8)
    if kind == "ones":
        return torch.ones(H, W, dtype=torch.uint8)
    if kind == "single":
        M = torch.zeros(H, W, dtype=torch.uint8)
        M[H // 2, W // 3] = 200
        return M
    if kind == "ramp":  # vertical: 0 in the first row, 255 in the last
        rows = torch.linspace(0, 255, H).round().to(torch.uint8) if H > 1 else torch.tensor([255], dtype=torch.uint8)
        return rows.view(H, 1).repeat(1, W).contiguous()
    if kind == "random":
        return u8(rng, H, W)
    raise KeyError(kind)


CASES = [  # (H, W, F, radius, data, plane, max_gain, eps)
    (1, 1, 1, 1, "random", "full", 8.0, 26.0),
    (1, 37, 3, 4, "random", "random", 8.0, 26.0),
    (37, 1, 1, 16, "random", "ramp", 8.0, 26.0),
    (15, 17, 3, 1, "random", "single", 8.0, 26.0),
    (15, 17, 3, 4, "flat", "random", 8.0, 26.0),
    (16, 16, 1, 4, "random", "zero", 8.0, 26.0),
    (16, 16, 3, 16, "random", "random", 4.0, 1.0),
    (17, 33, 3, 16, "steep", "full", 2.0, 1.0),
    (17, 33, 1, 1, "steep", "random", 8.0, 1.0),
    (17, 33, 1, 4, "extreme", "ones", 8.0, 26.0),
    (40, 40, 1, 16, "extreme", "full", 8.0, 0.2),
    (40, 40, 1, 16, "white", "full", 8.0, float(1 << 30)),
    (40, 40, 3, 4, "random", "ramp", 8.0, 26.0),
]


@pytest.fixture(scope="module")
def ops():
    from chronoedit_amd import ops
    return ops


def run_stages(ops, L, E, M, cfg, rng):
    """Both passes, each into a buffer full of garbage."""
    Ld, Ed, Md = L.to(DEV), E.to(DEV), M.to(DEV)
    F, H, W = E.shape[:3]
    AB = ops.rimlift_fit_q16(Ld, Ed, Md, cfg.radius, cfg.eps_q, cfg.max_gain,
                             out=torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (F, H, W, 6)).astype(np.int32)).to(DEV))
    coef, R = ops.rimlift_smooth(Ld, Ed, Md, AB, cfg.radius, coef=torch.full((F, H, W, 8), float("nan"), device=DEV),
                                 R=torch.full((F, H, W), -7, dtype=torch.int32, device=DEV))
    return AB, coef, R


@pytest.mark.parametrize("H,W,F,r,data,weights,max_gain,eps", CASES)
def test_both_passes_equal_their_stages(ops, H, W, F, r, data, weights, max_gain, eps):
    rng = np.random.default_rng(zlib.crc32(repr((H, W, F, r, data, weights)).encode()))
    cfg = lift.LiftConfig(r, eps, (4.0, 12.0), max_gain)
    L, E = frames(data, rng, F, H, W)
    M = plane(weights, rng, H, W)
    wAB = rimlift.fit_reference(L, E, M, cfg)
    wcoef, wR = rimlift.smooth_reference(L, E, wAB, M, cfg)
    # what the data is there for
    A, B = wAB[..., :3], wAB[..., 3:]
    if weights == "zero":
        assert not bool(wAB.any()) and not bool(wcoef.any()) and torch.equal(wR, (E.int() - L.int()).abs().amax(dim=3) * 256)
    if (data, weights) == ("steep", "full"):
        assert int(A.max()) == int(65536 * max_gain) and int(A.min()) == -int(65536 * max_gain)
    if data == "flat":
        assert int(A.abs().max()) <= 1  # (the two products of num round on their own: a is 0 up to that)
    if weights == "ones":
        assert int(B.max()) == 4096 * 65536 and int(B.min()) >= -4096 * 65536 and set(torch.unique(E.int() - L.int()).tolist()) == {-255, 255}
    if weights == "full" and r == 16 and (H, W) == (40, 40):
        q = lift.box_sum(M.long() ** 2 * L.long().permute(2, 0, 1), r)
        assert int(q.max()) >= 2 ** 31  # the sums of the window overflow 32 bits
    if weights == "single":
        assert int((wcoef[..., :6] != 0).any(dim=-1).sum()) <= F * (2 * r + 1) ** 2
    # the device, pass by pass: the smoothing from the device's own fit
    AB, coef, R = run_stages(ops, L, E, M, cfg, rng)
    assert torch.equal(AB.cpu(), wAB), f"fit: {int((AB.cpu() != wAB).sum())} of {wAB.numel()} differ"
    assert_exact(coef.cpu(), wcoef, "smooth")
    assert torch.equal(R.cpu(), wR)
    # ... and from any int32 at all in AB (the sums of m B are 64-bit whatever B holds)
    junk = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (F, H, W, 6)).astype(np.int32))
    jcoef, jR = rimlift.smooth_reference(L, E, junk, M, cfg)
    gcoef, gR = ops.rimlift_smooth(L.to(DEV), E.to(DEV), M.to(DEV), junk.to(DEV), r)
    assert_exact(gcoef.cpu(), jcoef, "smooth of random AB")
    assert torch.equal(gR.cpu(), jR)
    # the same bits on a second run
    AB2, coef2, R2 = run_stages(ops, L, E, M, cfg, rng)
    assert torch.equal(AB2, AB) and torch.equal(R2, R) and torch.equal(coef2.view(torch.int32), coef.view(torch.int32))
    # the three grid passes through rimlift.device_coefficients
    cells = rimlift.device_coefficients(L.to(DEV), E.to(DEV), M.to(DEV), cfg)
    assert_exact(cells.cpu(), rimlift.coefficients_reference(L, E, M, cfg), "cells")


def test_the_chain_equals_the_definition_on_an_odd_box(ops):
    """fit -> smooth -> ce_lift_gate_f32 -> ce_boxlift_apply_paste_u8 against boxlift.reference(mask_aware=True): a 41 x 28 box of a 71 x 53
    photo, a 19 x 13 edit, frames that carry an affine edit tapered by the weights and one of noise."""
    rng = np.random.default_rng(7)
    SW, SH, W, H = 71, 53, 19, 13
    photo, source = Image.fromarray(u8(rng, SH, SW, 3).numpy()), Image.fromarray(u8(rng, SH, SW, 3).numpy())
    box = (3, 5, 44, 33)
    l, t, r, b = box
    mask = torch.zeros(SH, SW, dtype=torch.uint8)
    mask[8:30, 6:40] = u8(rng, 22, 34)
    mask[12:24, 12:34] = 255
    tt = lambda im: torch.from_numpy(np.array(im, dtype=np.uint8))
    L = tt(photo.crop(box).resize((W, H), Image.LANCZOS))
    M = boxlift.weight_plane(mask, box, W, H)
    w = M.double()[..., None] / 255.0
    E = torch.stack([(L.double() + w * (-0.3 * L.double() + 40.0)).round().clamp(0, 255).to(torch.uint8), u8(rng, H, W, 3)])
    cfg = lift.LiftConfig(radius=2, gate=(1.0, 100.0))
    frames_pil = [Image.fromarray(f.numpy()) for f in E]
    want, means = boxlift.reference(source, [(photo, L, frames_pil, mask, box)], cfg, mask_aware=True)
    want = torch.stack([tt(f) for f in want])
    coef = rimlift.device_coefficients(L.to(DEV), E.to(DEV), M.to(DEV), cfg)
    U = torch.stack([tt(f.resize((r - l, b - t), Image.LANCZOS)) for f in frames_pil]).to(DEV)
    canvas = tt(source).to(DEV).unsqueeze(0).repeat(2, 1, 1, 1)
    tabs = lift.tables((r - l, b - t), (H, W), DEV)
    ops.boxlift_apply_paste_u8(tt(photo).to(DEV), coef, tabs, U, mask.to(DEV), canvas, l, t, r - l, b - t)
    assert torch.equal(canvas.cpu(), want), f"{int((canvas.cpu() != want).sum())} of {want.numel()} bytes differ"
    assert abs(float(coef[..., 6].double().mean()) - float(means[0])) < 1e-12
    plain, _ = boxlift.reference(source, [(photo, L, frames_pil, mask, box)], cfg)
    assert not torch.equal(want[0], tt(plain[0]))  # (the masked fit shows in the bytes)


def test_return_codes():
    from chronoedit_amd import hiplib
    lib = hiplib.load()
    H, W, F = 8, 8, 1
    L = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    E = torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV)
    M = torch.zeros(H, W, dtype=torch.uint8, device=DEV)
    AB = torch.zeros(F * H * W * 6 + 1, dtype=torch.int32, device=DEV)
    coef = torch.zeros(F * H * W * 8 + 4, dtype=torch.float32, device=DEV)
    R = torch.zeros(F * H * W + 1, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fit = lambda **k: lib.ce_rimlift_fit_q16(k.get("L", p(L)), k.get("E", p(E)), k.get("M", p(M)), k.get("AB", p(AB)), k.get("F", F), k.get("H", H),
                                             k.get("W", W), k.get("r", 4), k.get("eps", 26), k.get("mg", 8.0), st)
    assert fit() == 0
    assert [fit(L=None), fit(E=None), fit(M=None), fit(AB=None), fit(F=0), fit(F=65536), fit(H=0), fit(W=0), fit(r=0), fit(r=17), fit(eps=0),
            fit(mg=0.5), fit(mg=9.0), fit(mg=float("nan"))] == [-1] * 14
    assert fit(H=1 << 28) == -2 and fit(AB=p(AB, 2)) == -3
    smooth = lambda **k: lib.ce_rimlift_smooth_f32(k.get("L", p(L)), p(E), k.get("M", p(M)), k.get("AB", p(AB)), k.get("coef", p(coef)), k.get("R", p(R)),
                                                   k.get("F", F), k.get("H", H), W, k.get("r", 4), st)
    assert smooth() == 0
    assert [smooth(L=None), smooth(M=None), smooth(AB=None), smooth(coef=None), smooth(R=None), smooth(F=0), smooth(H=0), smooth(r=0),
            smooth(r=17)] == [-1] * 9
    assert smooth(H=1 << 28) == -2 and smooth(coef=p(coef, 4)) == -3 and smooth(R=p(R, 1)) == -3 and smooth(AB=p(AB, 2)) == -3
    torch.cuda.synchronize()
