"""ce_boxlift_apply_paste_u8 (csrc/ce_boxlift.hip) against its definition, bit for bit: `lift.apply_reference` on the crop of the photo, then
PIL's own `paste` through the photo-size mask.  The canvas starts as garbage, every buffer lies between guard bytes that must stay as
they were, every canvas byte outside the box must be unchanged, and a second run gives the same bits.  Box widths 1 / 3 / 4 / 17 / 37 and
heights 1 / 2 / 9, a row's first byte on every residue mod 16, photo widths that are and are not multiples of 4, the whole photo as the
box, grids of 1 x 1, 2 x 3 and 8 x 12 cells at non-integer scales, one and three frames, no mask / all 0 / all 255 / random bytes with runs
of 0 and 255 longer than a wave's 512 pixels, no fallback plane or one with the gate planted 0 / 1 / mixed, slopes at both clamps and a NaN
cell, buffers at odd addresses, and the return codes."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import lift

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, SENTINEL = 64, 0xA5


class Guarded:
    """A device buffer of `nbytes` at byte offset `off` behind GUARD sentinel bytes, and as many behind it."""

    def __init__(self, host: torch.Tensor, off: int = 0):
        raw = host.contiguous().view(-1).view(torch.uint8)
        self.n, self.off = raw.numel(), off
        self.buf = torch.full((GUARD + off + self.n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.buf[GUARD + off:GUARD + off + self.n] = raw.to(DEV)
        self.dtype, self.shape = host.dtype, tuple(host.shape)

    @property
    def t(self) -> torch.Tensor:
        return self.buf[GUARD + self.off:GUARD + self.off + self.n].view(self.dtype).view(self.shape)

    def intact(self) -> bool:
        return bool((self.buf[:GUARD + self.off] == SENTINEL).all()) and bool((self.buf[GUARD + self.off + self.n:] == SENTINEL).all())


def u8(rng, *shape):
    return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))


def make_coef(rng, F, H, W, gate):
    """Random cells, not a fit: slopes, offsets of every sign, bytes that clamp at both ends; slopes at both clamps; the gate planted."""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    coef = torch.randn(F, H, W, 8, generator=g) * torch.tensor([1.0, 1.0, 1.0, 120.0, 120.0, 120.0, 0.0, 0.0])
    coef[0, 0, 0, 0:3] = torch.tensor([8.0, -8.0, 8.0])  # |a| = max_gain
    coef[-1, -1, -1, 0:3] = torch.tensor([-8.0, 8.0, -8.0])
    if gate == "one":
        coef[..., 6] = 1.0
    elif gate == "mixed":
        gg = torch.rand(F, H, W, generator=g)
        coef[..., 6] = torch.where(gg < 0.4, torch.zeros(()), torch.where(gg > 0.8, torch.ones(()), gg))
    return coef.contiguous()


def long_runs_mask(rng, SH, SW):
    """Random bytes with runs of 0 and of 255 of 600 pixels - more than the 64 x 8 pixels one wave covers - and shorter ones."""
    m = u8(rng, SH * SW)
    p = 0
    while p < m.numel():
        kind, n = int(rng.integers(4)), int(rng.integers(1, 40))
        if kind == 0:
            m[p:p + n] = 0
        elif kind == 1:
            m[p:p + n] = 255
        p += n + int(rng.integers(1, 40))
    for start, v in ((SW // 7, 0), (SW + 11, 255), (2 * SW + 5, 0)):
        if start + 600 <= m.numel():
            m[start:start + 600] = v
    return m.view(SH, SW)


def expected(canvas, P, U, coef, mask, box, grid):
    """The definition: apply_reference on the crop, PIL's paste into every frame of the canvas."""
    l, t, r, b = box
    Q = lift.apply_reference(P[t:b, l:r].contiguous(), coef, lift.tables((r - l, b - t), grid), U)
    out = []
    for f in range(canvas.shape[0]):
        c = Image.fromarray(canvas[f].numpy())
        c.paste(Image.fromarray(Q[f].numpy()), (l, t), None if mask is None else Image.fromarray(mask.numpy()).crop(box))
        out.append(torch.from_numpy(np.array(c)))
    return torch.stack(out)


def run_case(ops, seed, src, box, grid, F, mask_kind, u_kind, offs=(0, 0, 0, 0), nan_cell=False):
    rng = np.random.default_rng(seed)
    SH, SW = src
    l, t, r, b = box
    bw, bh = r - l, b - t
    H, W = grid
    P, garbage = u8(rng, SH, SW, 3), u8(rng, F, SH, SW, 3)
    coef = make_coef(rng, F, H, W, {"none": "zero", "g0": "zero"}.get(u_kind, u_kind))
    if nan_cell:
        coef[0, H // 2, W // 2, :] = float("nan")
    U = None if u_kind == "none" else u8(rng, F, bh, bw, 3)
    mask = {"none": lambda: None, "zero": lambda: torch.zeros(SH, SW, dtype=torch.uint8), "full": lambda: torch.full((SH, SW), 255, dtype=torch.uint8),
            "random": lambda: long_runs_mask(rng, SH, SW)}[mask_kind]()
    want = expected(garbage, P, U, coef, mask, box, grid)
    tabs = lift.tables((bw, bh), grid)
    results = []
    for _ in range(2):  # the same bits twice, from the same garbage
        gc, gp = Guarded(garbage, offs[0]), Guarded(P, offs[1])
        gu = None if U is None else Guarded(U, offs[2])
        gm = None if mask is None else Guarded(mask, offs[3])
        gcoef, gtabs = Guarded(coef), [Guarded(x) for x in tabs]
        ops.boxlift_apply_paste_u8(gp.t, gcoef.t, tuple(x.t for x in gtabs), None if gu is None else gu.t, None if gm is None else gm.t, gc.t, l, t, bw, bh)
        torch.cuda.synchronize()
        got = gc.t.cpu()
        assert all(x.intact() for x in [gc, gp, gcoef] + gtabs + [x for x in (gu, gm) if x is not None]), "a guard byte changed"
        assert torch.equal(gp.t.cpu(), P) and torch.equal(gcoef.t.cpu().view(torch.int32), coef.view(torch.int32))
        results.append(got)
    got = results[0]
    assert torch.equal(results[1], got), "two runs differ"
    outside = torch.ones(SH, SW, dtype=torch.bool)
    outside[t:b, l:r] = False
    assert torch.equal(got[:, outside], garbage[:, outside]), "a byte outside the box changed"
    diff = int((got != want).sum())
    assert diff == 0, f"{diff} of {bw * bh * 3 * F} bytes of the box differ"
    return SimpleNamespace(got=got, garbage=garbage, want=want, U=U, mask=mask)


@pytest.fixture(scope="module")
def ops():
    from chronoedit_amd import ops
    return ops


GRIDS = [(1, 1), (2, 3), (8, 12)]
MASKS = ["none", "random", "full", "zero"]
US = ["none", "g0", "one", "mixed"]
SIZES = [(bw, bh) for bw in (1, 3, 4, 17, 37) for bh in (1, 2, 9)]


@pytest.mark.parametrize("i", range(len(SIZES)))
def test_box_sizes_grids_masks_and_fallbacks(ops, i):
    """Every box size, with the grid, the frame count, the mask, the fallback plane and the photo's width taken in turn."""
    bw, bh = SIZES[i]
    SW = 52 if i % 2 else 53  # a multiple of 4, and none
    SH = 23
    l, t = 5 + i % 7, 3 + i % 5
    grid = GRIDS[(i + i // 3) % 3]
    assert (bw % grid[1] or bh % grid[0]) or grid == (1, 1)  # (a non-integer scale on some axis, but for the one cell)
    c = run_case(ops, 100 + i, (SH, SW), (l, t, l + bw, t + bh), grid, 1 + 2 * (i % 2), MASKS[i % 4], US[(i // 2) % 4], nan_cell=i % 4 == 1)
    if MASKS[i % 4] == "zero":
        assert torch.equal(c.got, c.garbage)  # nothing was written: the canvas keeps its garbage


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("u_kind", US)
def test_every_mask_with_every_fallback(ops, mask_kind, u_kind):
    c = run_case(ops, 7, (31, 61), (9, 4, 46, 13), (8, 12), 3, mask_kind, u_kind, nan_cell=True)
    assert torch.equal(c.got, c.garbage) == (mask_kind == "zero")


@pytest.mark.parametrize("SW", [60, 61])
def test_a_rows_first_byte_on_every_residue_mod_16(ops, SW):
    seen = set()
    for left in range(16):
        gc = Guarded(torch.zeros(1, dtype=torch.uint8))
        base = gc.t.data_ptr()  # (the allocator hands out the same alignment for every buffer of the run: checked below)
        assert base % 16 == 0
        for y in range(3):
            seen.add((base + ((2 + y) * SW + left) * 3) % 16)
        run_case(ops, 200 + left, (9, SW), (left, 2, left + 37, 5), (2, 3), 1, "random" if left % 2 else "none", "mixed")
    assert seen == set(range(16))


@pytest.mark.parametrize("offs", [(1, 0, 0, 0), (2, 3, 1, 1), (3, 3, 2, 3), (0, 1, 3, 2)])
def test_buffers_at_odd_addresses(ops, offs):
    """canvas, P, U and the mask each at its own phase: dword access where a plane allows it, bytes where it does not - the same bytes."""
    run_case(ops, 300 + sum(offs), (14, 45), (3, 2, 40, 11), (2, 3), 3, "random", "mixed", offs=offs)


@pytest.mark.parametrize("src", [(9, 40), (7, 37)])
def test_the_whole_photo_as_the_box(ops, src):
    SH, SW = src
    run_case(ops, 400 + SW, src, (0, 0, SW, SH), (2, 3), 3, "random", "mixed")
    run_case(ops, 401 + SW, src, (0, 0, SW, SH), (8, 12), 1, "none", "none")


def test_mask_runs_longer_than_a_waves_span(ops):
    """Rows of 1301 pixels: runs of 600 pixels of 0 and of 255 put whole waves (64 lanes x 8 pixels) under m == 0 and under m == 255."""
    SH, SW = 4, 1301
    c = run_case(ops, 500, (SH, SW), (2, 0, SW - 1, SH), (8, 12), 3, "random", "mixed")
    flat = c.mask.view(-1)
    assert bool((flat[SW // 7:SW // 7 + 600] == 0).all()) and bool((flat[SW + 11:SW + 611] == 255).all()) and bool((flat[2 * SW + 5:2 * SW + 605] == 0).all())
    assert not torch.equal(c.got, c.garbage)


def test_a_full_gate_gives_the_fallback_plane_and_none_ignores_it(ops):
    SH, SW, box, grid, F = 12, 41, (2, 1, 39, 10), (2, 3), 1
    c = run_case(ops, 600, (SH, SW), box, grid, F, "full", "one")
    assert torch.equal(c.got[:, 1:10, 2:39], c.U)  # g == 1 under m == 255: the plane's bytes
    a = run_case(ops, 601, (SH, SW), box, grid, F, "full", "g0")
    b = run_case(ops, 601, (SH, SW), box, grid, F, "full", "none")
    assert torch.equal(a.got[:, 1:10, 2:39], b.got[:, 1:10, 2:39])  # g == 0 everywhere: the plane changes nothing


def test_return_codes():
    from chronoedit_amd import hiplib
    lib = hiplib.load()
    F, SH, SW, H, W = 2, 16, 20, 4, 4
    bw, bh = 8, 8
    canvas = torch.zeros(F, SH, SW, 3, dtype=torch.uint8, device=DEV)
    P = torch.zeros(SH, SW, 3, dtype=torch.uint8, device=DEV)
    U = torch.zeros(F, bh, bw, 3, dtype=torch.uint8, device=DEV)
    mask = torch.zeros(SH, SW, dtype=torch.uint8, device=DEV)
    coef = torch.zeros(F * H * W * 8 + 4, dtype=torch.float32, device=DEV)
    ti, tf = torch.zeros(17, dtype=torch.int32, device=DEV), torch.zeros(17, dtype=torch.float32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**k):
        return lib.ce_boxlift_apply_paste_u8(k.get("P", p(P)), k.get("U", p(U)), k.get("coef", p(coef)), k.get("ix0", p(ti)), p(ti), p(tf), p(ti), p(ti),
                                             k.get("ty", p(tf)), k.get("mask", p(mask)), k.get("canvas", p(canvas)), k.get("F", F), k.get("SH", SH), SW,
                                             k.get("left", 2), k.get("top", 3), k.get("bw", bw), k.get("bh", bh), k.get("H", H), W, st)

    assert call() == 0 and call(U=None, mask=None) == 0
    assert [call(P=None), call(canvas=None), call(coef=None), call(ix0=None), call(F=0), call(F=65536), call(bw=0), call(bh=0), call(H=0)] == [-1] * 9
    # a box that leaves the image
    assert [call(left=-1), call(top=-1), call(left=SW - bw + 1), call(top=SH - bh + 1), call(bw=SW), call(bh=SH)] == [-1] * 6
    assert call(left=SW - bw, top=SH - bh) == 0  # the corner itself lies inside
    # images of 2^31 bytes or more
    assert call(SH=1 << 27) == -2 and call(H=1 << 24) == -2
    # misaligned cells and tables
    assert call(coef=p(coef, 4)) == -3 and call(coef=p(coef, 8)) == -3 and call(ix0=p(ti, 2)) == -3 and call(ty=p(tf, 1)) == -3
    # P, U or the mask sharing a byte with the canvas
    assert [call(P=p(canvas)), call(U=p(canvas)), call(mask=p(canvas)), call(P=p(canvas, 3)), call(mask=p(canvas, F * SH * SW * 3 - 1))] == [-1] * 5
    torch.cuda.synchronize()
    assert not bool(canvas.any())  # (zero cells on a zero photo, a zero mask: nothing was written by the calls that ran)
