"""The four passes of csrc/ce_lift.hip against their stages of `lift.reference` (CPU torch), bit for bit: odd sizes and non-integer ratios on
the byte-by-byte path, the 16-byte path, identity tables, one and three frames, radius 1 / 4 / 16, flat sources, changes of +-255, slopes at
both clamps, gates that are 0 / 1 / mixed, no fallback plane, garbage and unaligned outputs, more groups than one launch round holds, the
return codes, and the same bits on a second run."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from chronoedit_amd import lift
from exact_util import assert_exact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = {"odd": ((13, 19), (37, 53)), "aligned": ((16, 24), (64, 96)), "identity": ((16, 24), (16, 24))}  # (H, W) -> (SH, SW)


def u8(rng, *shape):
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def frames(kind, rng, F, H, W):
    """(L uint8 [H, W, 3], E uint8 [F, H, W, 3]) of one data recipe."""
    if kind == "random":
        return u8(rng, H, W, 3), u8(rng, F, H, W, 3)
    if kind == "flat":  # a source without variance: den = eps_q n^2, a = 0 up to the regulariser
        L = torch.full((H, W, 3), 77, dtype=torch.uint8)
        return L, u8(rng, F, H, W, 3)
    if kind == "extreme":  # d = +-255 everywhere: I in {0, 255}, E = 255 - I
        L = torch.from_numpy(rng.integers(0, 2, (H, W, 3)).astype(np.uint8) * 255)
        return L, (255 - L)[None].repeat(F, 1, 1, 1).contiguous()
    if kind == "steep":  # I in 118..138, E = 128 +- 12 (I - 128): d = E - I has the slopes 11 and -13, beyond both clamps; the sign alternates
        L = torch.from_numpy(rng.integers(118, 139, (H, W, 3), dtype=np.uint8))
        s = torch.tensor([12.0, -12.0, 12.0, -12.0, 12.0, -12.0, 12.0, -12.0, 12.0])[:3 * F].view(F, 1, 1, 3)
        return L, ((L.float() - 128.0) * s + 128.0).to(torch.uint8).contiguous()
    if kind == "mixed":  # E == L but for one rectangle of noise: g runs from 0 to 1
        L = u8(rng, H, W, 3)
        E = L[None].repeat(F, 1, 1, 1).contiguous()
        E[:, H // 4:H // 4 + 6, W // 4:W // 4 + 8] = u8(rng, F, 6, 8, 3)
        return L, E
    raise KeyError(kind)


CASES = [  # (shape, F, radius, data, gate, max_gain, eps)
    ("odd", 1, 1, "mixed", (4.0, 12.0), 8.0, 26.0),
    ("odd", 3, 4, "random", (4.0, 12.0), 8.0, 26.0),
    ("odd", 3, 16, "steep", (0.0, 300.0), 2.0, 1.0),
    ("odd", 1, 4, "flat", None, 8.0, 26.0),
    ("aligned", 3, 4, "random", (4.0, 12.0), 8.0, 26.0),
    ("aligned", 1, 16, "extreme", (4.0, 12.0), 8.0, 0.2),
    ("aligned", 3, 1, "mixed", (0.5, 0.75), 1.0, 26.0),
    ("aligned", 1, 4, "steep", None, 8.0, 1.0),
    ("identity", 3, 4, "random", (4.0, 12.0), 8.0, 26.0),
    ("identity", 1, 1, "mixed", (4.0, 12.0), 8.0, 26.0),
]


@pytest.fixture(scope="module")
def ops():
    from chronoedit_amd import ops
    return ops


def run_stages(ops, L, E, cfg):
    Ld, Ed = L.to(DEV), E.to(DEV)
    AB = ops.lift_fit_q16(Ld, Ed, cfg.radius, cfg.eps_q, cfg.max_gain)
    coef, R = ops.lift_smooth(Ld, Ed, AB, cfg.radius, coef=torch.full((*E.shape[:3], 8), float("nan"), device=DEV),
                              R=torch.full(tuple(E.shape[:3]), -7, dtype=torch.int32, device=DEV))
    smooth = coef.clone()
    if cfg.gate is not None:
        ops.lift_gate(R, coef, cfg.radius, *cfg.gate)
    return AB, smooth, R, coef


@pytest.mark.parametrize("shape,F,r,data,gate,max_gain,eps", CASES)
def test_every_stage_equals_the_reference(ops, shape, F, r, data, gate, max_gain, eps):
    (H, W), (SH, SW) = SHAPES[shape]
    rng = np.random.default_rng(zlib.crc32(repr((shape, F, r, data)).encode()))
    cfg = lift.LiftConfig(r, eps, gate, max_gain)
    L, E = frames(data, rng, F, H, W)
    P, U = u8(rng, SH, SW, 3), u8(rng, F, SH, SW, 3)
    # the definition, stage by stage
    wAB = lift.fit_reference(L, E, cfg)
    wcoef, wR = lift.smooth_reference(L, E, wAB, cfg)
    wsmooth = wcoef.clone()
    if gate is not None:
        wcoef[..., 6] = lift.gate_reference(wR, cfg)
    tabs = lift.tables((SW, SH), (H, W))
    want = lift.apply_reference(P, wcoef, tabs, U if gate is not None else None)
    assert torch.equal(want, lift.reference(P, L, E, U, cfg))
    # what the data is there for
    A = wAB[..., :3]
    if data == "steep":
        assert int(A.max()) == int(65536 * max_gain) and int(A.min()) == -int(65536 * max_gain)
    if data == "flat":
        assert not bool(A.any())
    if data == "extreme":
        assert set(torch.unique(E.int() - L.int()).tolist()) == {-255, 255}
    if data == "mixed":
        g = wcoef[..., 6]
        assert bool((g == 0).any()) and bool((g == 1).any()) and bool(((g > 0) & (g < 1)).any())
    # the device, stage by stage, each from the device's own previous stage
    AB, smooth, R, coef = run_stages(ops, L, E, cfg)
    assert torch.equal(AB.cpu(), wAB), f"fit: {int((AB.cpu() != wAB).sum())} of {wAB.numel()} differ"
    assert_exact(smooth.cpu(), wsmooth, "smooth")
    assert torch.equal(R.cpu(), wR)
    assert_exact(coef.cpu(), wcoef, "gate")
    dtabs = tuple(t.to(DEV) for t in tabs)
    Pd, Ud = P.to(DEV), U.to(DEV) if gate is not None else None
    garbage = torch.from_numpy(rng.integers(0, 256, (F, SH, SW, 3), dtype=np.uint8)).to(DEV)
    got = ops.lift_apply_u8(Pd, coef, dtabs, Ud, out=garbage)
    assert torch.equal(got.cpu(), want), f"apply: {int((got.cpu() != want).sum())} of {want.numel()} bytes differ"
    # an unaligned output base takes the byte-by-byte path: the same bytes, and nothing outside them is touched
    buf = torch.full((F * SH * SW * 3 + 2,), 201, dtype=torch.uint8, device=DEV)
    odd = buf[1:-1].view(F, SH, SW, 3)
    ops.lift_apply_u8(Pd, coef, dtabs, Ud, out=odd)
    assert torch.equal(odd.cpu(), want) and int(buf[0]) == 201 and int(buf[-1]) == 201
    # the same bits on a second run, and through lift.lift
    AB2, smooth2, R2, coef2 = run_stages(ops, L, E, cfg)
    assert torch.equal(AB2, AB) and torch.equal(R2, R) and torch.equal(coef2.view(torch.int32), coef.view(torch.int32))
    both, frac = lift.lift(Pd, L.to(DEV), E.to(DEV), Ud, cfg)
    assert torch.equal(both.cpu(), want) and torch.equal(ops.lift_apply_u8(Pd, coef, dtabs, Ud), got)
    assert abs(float(frac) - float(wcoef[..., 6].double().mean())) < 1e-12


def test_the_gate_at_its_ends_and_the_fallback_plane(ops):
    """g all 0: U is never read (a NaN-free proof: the result equals the call without U); g all 1: the result is U."""
    rng = np.random.default_rng(11)
    (H, W), (SH, SW) = SHAPES["aligned"]
    L, E = frames("random", rng, 3, H, W)
    P, U = u8(rng, SH, SW, 3), u8(rng, 3, SH, SW, 3)
    tabs = tuple(t.to(DEV) for t in lift.tables((SW, SH), (H, W)))
    for gate, full in (((200.0, 300.0), 0.0), ((0.0, 2.0 ** -9), 1.0)):
        cfg = lift.LiftConfig(4, 26.0, gate, 8.0)
        _, _, R, coef = run_stages(ops, L, E, cfg)
        assert int(R.min()) > 0 and bool((coef[..., 6] == full).all())
        got = ops.lift_apply_u8(P.to(DEV), coef, tabs, U.to(DEV)).cpu()
        assert torch.equal(got, lift.reference(P, L, E, U, cfg))
        if full == 0.0:
            assert torch.equal(got, ops.lift_apply_u8(P.to(DEV), coef, tabs, None).cpu())
        else:
            assert torch.equal(got, U)


def test_more_groups_than_one_round_of_the_launch(ops):
    """64 frames leave each frame 32 workgroups = 131072 pixels per round: a 400 x 400 photo takes two rounds.  The cells are random
    numbers, not a fit: slopes, offsets and gates of every sign and size, bytes that clamp at both ends."""
    F, H, W, SH, SW = 64, 5, 7, 400, 400
    g = torch.Generator().manual_seed(4)
    coef = torch.randn(F, H, W, 8, generator=g) * torch.tensor([1.0, 1.0, 1.0, 120.0, 120.0, 120.0, 1.0, 0.0])
    coef[::2, ..., 6] = 0.0  # every other frame reads no U
    rng = np.random.default_rng(4)
    P, U = u8(rng, SH, SW, 3), u8(rng, F, SH, SW, 3)
    tabs = lift.tables((SW, SH), (H, W))
    want = lift.apply_reference(P, coef, tabs, U)
    assert int((want == 0).sum()) > 1000 and int((want == 255).sum()) > 1000
    got = ops.lift_apply_u8(P.to(DEV), coef.to(DEV), tuple(t.to(DEV) for t in tabs), U.to(DEV))
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).sum())} of {want.numel()} bytes differ"


def test_return_codes():
    from chronoedit_amd import hiplib
    lib = hiplib.load()
    H, W, SH, SW, F = 8, 8, 16, 16, 1
    L = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    E = torch.zeros(F, H, W, 3, dtype=torch.uint8, device=DEV)
    AB = torch.zeros(F * H * W * 6 + 1, dtype=torch.int32, device=DEV)
    coef = torch.zeros(F * H * W * 8 + 4, dtype=torch.float32, device=DEV)
    R = torch.zeros(F * H * W + 1, dtype=torch.int32, device=DEV)
    P = torch.zeros(SH, SW, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(F, SH, SW, 3, dtype=torch.uint8, device=DEV)
    ti, tf = torch.zeros(17, dtype=torch.int32, device=DEV), torch.zeros(17, dtype=torch.float32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fit = lambda **k: lib.ce_lift_fit_q16(k.get("L", p(L)), p(E), k.get("AB", p(AB)), k.get("F", F), k.get("H", H), W, k.get("r", 4), k.get("eps", 26),
                                          k.get("mg", 8.0), st)
    assert fit() == 0
    assert [fit(L=None), fit(F=0), fit(F=65536), fit(r=0), fit(r=17), fit(eps=0), fit(mg=0.5), fit(mg=9.0), fit(mg=float("nan"))] == [-1] * 9
    assert fit(H=1 << 28) == -2 and fit(AB=p(AB, 2)) == -3
    smooth = lambda **k: lib.ce_lift_smooth_f32(p(L), p(E), p(AB), k.get("coef", p(coef)), k.get("R", p(R)), F, k.get("H", H), W, k.get("r", 4), st)
    assert smooth() == 0
    assert [smooth(coef=None), smooth(R=None), smooth(r=0), smooth(r=17)] == [-1] * 4
    assert smooth(H=1 << 28) == -2 and smooth(coef=p(coef, 4)) == -3 and smooth(R=p(R, 1)) == -3
    gate = lambda **k: lib.ce_lift_gate_f32(k.get("R", p(R)), k.get("coef", p(coef)), F, k.get("H", H), W, k.get("r", 4), k.get("t0", 4.0), k.get("t1", 12.0), st)
    assert gate() == 0
    assert [gate(R=None), gate(r=17), gate(t0=-1.0), gate(t0=12.0), gate(t1=float("inf")), gate(t0=float("nan"))] == [-1] * 6
    assert gate(H=1 << 28) == -2 and gate(coef=p(coef, 8)) == -3 and gate(R=p(R, 2)) == -3
    apply = lambda **k: lib.ce_lift_apply_u8(k.get("P", p(P)), None, k.get("coef", p(coef)), k.get("ix0", p(ti)), p(ti), p(tf), p(ti), p(ti), p(tf),
                                             k.get("out", p(out)), k.get("F", F), k.get("SH", SH), SW, k.get("H", H), W, st)
    assert apply() == 0
    assert [apply(P=None), apply(out=None), apply(out=p(P)), apply(F=0), apply(F=65536), apply(SH=0), apply(H=0)] == [-1] * 7
    assert apply(SH=1 << 27) == -2 and apply(H=1 << 24) == -2 and apply(coef=p(coef, 4)) == -3 and apply(ix0=p(ti, 2)) == -3
    torch.cuda.synchronize()
