"""The three passes of csrc/ce_tiles.hip against chronoedit_amd/tiles.py (CPU torch), bit for bit.

Shapes: tiles of 12 x 8 cells (96 x 64 px) and 16 x 8 cells (128 x 64 px); plans 1 x 1, 2 x 2, 3 x 1 with a triple-covered strip and 1 x 2 from
the planner, plus one grid given by hand (16-wide tiles at 0, 4, 8: a triple cover whose origins are multiples of 4); 1 and 2 latent frames.
The latent passes move four cells per lane where tile width, canvas width and every x origin are multiples of 4 and the bases are 16-byte
aligned (the 2 x 2, 1 x 2 and hand-made grids), one cell per lane otherwise (the planner's 3 x 1 grids, whose origins are 0, 4, 10 and
0, 6, 14 cells, and every grid again from a base that is 4 bytes off); the byte pass stores dwords where a frame's bytes are a multiple of 4
and the base is aligned, bytes otherwise (a 150 x 90 target; odd bases).  NaN and infinite cells, garbage in every output, guards around
every output, the same bits twice, the return codes."""
import ctypes

import numpy as np
import pytest
import torch

from chronoedit_amd import tiles

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 16


def _px_grid(tile, canvas, overlap=0.25):
    p = tiles.plan(canvas, tile[1], tile[0], overlap=overlap)
    return p.xs, p.ys, tile, p.canvas


GRIDS = {  # name -> (xs, ys in px, (TW, TH), (CW, CH))
    "96 1x1": _px_grid((96, 64), (96, 64)),
    "96 2x2": _px_grid((96, 64), (160, 96)),
    "96 3x1 triple": _px_grid((96, 64), (176, 64)),
    "96 1x2": _px_grid((96, 64), (96, 96)),
    "128 1x1": _px_grid((128, 64), (128, 64)),
    "128 2x2": _px_grid((128, 64), (192, 96)),
    "128 3x1 triple": _px_grid((128, 64), (240, 64)),
    "128 1x2": _px_grid((128, 64), (128, 96)),
    "128 3x1 by hand": ((0, 32, 64), (0,), (128, 64), (192, 64)),
}


def test_the_grids_are_what_the_docstring_says():
    assert GRIDS["96 2x2"][:2] == ((0, 64), (0, 32)) and GRIDS["96 3x1 triple"][:2] == ((0, 32, 80), (0,)) and GRIDS["96 1x2"][:2] == ((0,), (0, 32))
    assert GRIDS["128 2x2"][:2] == ((0, 64), (0, 32)) and GRIDS["128 3x1 triple"][:2] == ((0, 48, 112), (0,))
    for name in ("96 3x1 triple", "128 3x1 triple", "128 3x1 by hand"):
        xs, _, (TW, _), (CW, _) = GRIDS[name]
        assert max(sum(1 for x in xs if x <= X < x + TW) for X in range(CW)) == 3


def _cells(grid):
    xs, ys, (TW, TH), (CW, CH) = grid
    return tuple(x // 8 for x in xs), tuple(y // 8 for y in ys), TH // 8, TW // 8, CH // 8, CW // 8


def _guarded(numel, dtype, fill, offset=0):
    """A flat device buffer of `numel` elements behind `offset` extra elements, with GUARD elements of `fill` on either side -> (whole, view)."""
    whole = torch.full((GUARD + offset + numel + GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD + offset:GUARD + offset + numel]


def _guards_intact(whole, numel, fill, offset=0):
    w = whole.cpu()
    return bool((w[:GUARD + offset] == fill).all() and (w[GUARD + offset + numel:] == fill).all())


def _same_bits(got, want):
    """fp32 tensors: the same bits, where the reference is a NaN any NaN (the payload of a computed NaN is the processor's business)."""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]))


def _latent_tiles(grid, T, seed):
    xs, ys, th, tw, ch, cw = _cells(grid)
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(len(xs) * len(ys), 16, T, th, tw, generator=g)
    t[0, 0, 0, 0, 0], t[0, 1, 0, 1, 1], t[-1, 2, -1, -1, -1], t[-1, 3, 0, 0, 0] = float("nan"), float("inf"), float("-inf"), float("nan")
    t[0, 4, 0, :, -1], t[-1, 5, 0, :, 0], t[0, 6], t[0, 7, 0, 2, 2] = float("inf"), float("-inf"), -0.0, 1e-42
    return t, (xs, ys, th, tw, ch, cw)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "4 bytes off"])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("name", list(GRIDS))
def test_fuse_and_scatter_equal_the_reference(name, T, offset):
    from chronoedit_amd import ops
    t, (xs, ys, th, tw, ch, cw) = _latent_tiles(GRIDS[name], T, seed=len(name) + T)
    want = tiles.reference_fuse(t, xs, ys, ch, cw)
    n_c = want.numel()
    src_whole, src = _guarded(t.numel(), torch.float32, 7.0, offset)
    src.copy_(t.reshape(-1))
    whole, flat = _guarded(n_c, torch.float32, -12345.0, offset)
    canvas = flat.view(want.shape)
    for _ in range(2):  # twice: the same bits
        flat.fill_(float("nan"))  # garbage in the output
        assert ops.tiles_fuse(src.view(t.shape), canvas, xs, ys) is canvas
        assert _same_bits(canvas, want)
    assert _guards_intact(whole, n_c, -12345.0, offset) and torch.equal(src.cpu().view(torch.int32), t.reshape(-1).view(torch.int32))
    # canvas -> tiles: a copy, NaN payloads included
    back = tiles.reference_scatter(want, xs, ys, th, tw)
    out_whole, out = _guarded(t.numel(), torch.float32, 4321.0, offset)
    for _ in range(2):
        out.fill_(-1.0)
        ops.tiles_scatter(canvas, out.view(t.shape), xs, ys)
        assert _same_bits(out.view(t.shape), back)
    assert torch.equal(out.cpu().view(torch.int32), canvas_bits_scattered(canvas, xs, ys, th, tw))
    assert _guards_intact(out_whole, t.numel(), 4321.0, offset) and _guards_intact(whole, n_c, -12345.0, offset)
    del src_whole


def canvas_bits_scattered(canvas, xs, ys, th, tw):
    """The device canvas's own bits, cut on the host: the scatter is a copy, whatever the bits are."""
    return tiles.reference_scatter(canvas.cpu().view(torch.int32), xs, ys, th, tw).reshape(-1)


def test_fuse_keeps_single_cells_and_identical_tiles():
    from chronoedit_amd import ops
    xs, ys, th, tw, ch, cw = _cells(GRIDS["96 2x2"])
    canvas = torch.randn(16, 2, ch, cw, generator=torch.Generator().manual_seed(4))
    canvas[0, 0, 0, 0], canvas[1, 1, 5, 9] = -0.0, float("inf")
    same = tiles.reference_scatter(canvas, xs, ys, th, tw).to(DEV)
    out = torch.empty(canvas.shape, device=DEV)
    ops.tiles_fuse(same, out, xs, ys)
    assert torch.equal(out.cpu().view(torch.int32), canvas.view(torch.int32))  # identical tiles return themselves, bit for bit
    t = torch.randn(4, 16, 2, th, tw, generator=torch.Generator().manual_seed(5))
    ops.tiles_fuse(t.to(DEV), out, xs, ys)
    assert torch.equal(out.cpu()[..., :ys[1], :xs[1]], t[0][..., :ys[1], :xs[1]])  # the corner under tile 0 alone
    assert torch.equal(out.cpu()[..., ys[0] + th:, xs[0] + tw:], t[3][..., th - (ch - th):, tw - (cw - tw):])  # ... and under tile 3 alone


def test_tile_state_fuse_is_fuse_then_scatter():
    p = tiles.plan((150, 90), 64, 96)
    st = tiles.TileState(p, 16, 2, DEV)
    t = torch.randn(st.latent_shape, generator=torch.Generator().manual_seed(6))
    lat = t.to(DEV)
    assert st.fuse(lat) is lat
    xs, ys, th, tw, ch, cw = p.cells
    want = tiles.reference_fuse(t, xs, ys, ch, cw)
    assert torch.equal(st.canvas.cpu(), want) and torch.equal(lat.cpu(), tiles.reference_scatter(want, xs, ys, th, tw))
    noise = torch.randn(1, 16, 2, ch, cw, generator=torch.Generator().manual_seed(7))
    assert torch.equal(st.cut(noise.to(DEV)).cpu(), tiles.reference_scatter(noise[0], xs, ys, th, tw))


TARGETS = {"96 2x2": [(160, 96), (150, 90), (149, 95)], "128 2x2": [(192, 96), (181, 83)]}


@pytest.mark.parametrize("offset", [0, 1, 3], ids=["aligned", "odd base", "base + 3"])
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("name", list(GRIDS))
def test_blend_equals_the_reference(name, F, offset):
    from chronoedit_amd import ops
    xs, ys, (TW, TH), canvas = GRIDS[name]
    fr = torch.from_numpy(np.random.default_rng(len(name) + F).integers(0, 256, (len(xs) * len(ys), F, TH, TW, 3), dtype=np.uint8))
    fr[0, 0, :3], fr[-1, -1, -3:] = 255, 0
    dev = fr.to(DEV)
    for target in TARGETS.get(name, [canvas]):
        want = tiles.reference_blend(fr, xs, ys, target)
        whole, flat = _guarded(want.numel(), torch.uint8, 0xA5, offset)
        out = flat.view(want.shape)
        for _ in range(2):
            flat.fill_(0x5A)
            assert ops.tiles_blend_u8(dev, xs, ys, target, out=out) is out
            assert torch.equal(out.cpu(), want)
        assert _guards_intact(whole, want.numel(), 0xA5, offset)
    assert torch.equal(ops.tiles_blend_u8(dev, xs, ys, canvas).cpu(), tiles.reference_blend(fr, xs, ys, canvas))  # (an output of its own)


def test_return_codes():
    from chronoedit_amd import ops
    lib = ops.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    t = torch.zeros(4, 16, 1, 8, 12, device=DEV)
    c = torch.zeros(16, 1, 12, 20, device=DEV)
    fuse = lambda tp, cp, nx=2, ny=2, ox=ints(0, 8), oy=ints(0, 4), planes=16, th=8, tw=12, ch=12, cw=20, f=lib.ce_tiles_fuse_f32: \
        f(tp, cp, nx, ny, ox, oy, planes, th, tw, ch, cw, stream)
    tp, cp = t.data_ptr(), c.data_ptr()
    for f in (lib.ce_tiles_fuse_f32, lambda a, b, *r: lib.ce_tiles_scatter_f32(b, a, *r)):
        assert fuse(tp, cp, f=f) == 0
        assert fuse(None, cp, f=f) == -1 and fuse(tp, None, f=f) == -1 and fuse(tp, tp, f=f) == -1 and fuse(tp, cp, planes=0, f=f) == -1
        assert fuse(tp, cp, ox=None, f=f) == -1 and fuse(tp, cp, oy=None, f=f) == -1
        assert fuse(tp, cp, ox=ints(0, 4), f=f) == -1  # the last tile does not end at the canvas's edge
        assert fuse(tp, cp, ox=ints(4, 8), f=f) == -1  # the first does not start at 0
        assert fuse(tp, cp, ox=ints(8, 0), f=f) == -1  # not increasing
        assert fuse(tp, cp, nx=2, ox=ints(0, 13), cw=25, f=f) == -1  # a gap between neighbours
        assert fuse(tp, cp, nx=0, f=f) == -1 and fuse(tp, cp, ny=17, f=f) == -1
        assert fuse(tp, cp, nx=3, ny=6, ox=ints(0, 4, 8), oy=ints(0, 1, 2, 3, 4, 5), ch=13, f=f) == -1  # 18 tiles
        assert fuse(tp, cp, ch=8, f=f) == -1  # a canvas the y origins do not span
        assert fuse(tp + 2, cp, f=f) == -3 and fuse(tp, cp + 1, f=f) == -3
        assert fuse(tp, cp, planes=1 << 24, f=f) == -2
    fr = torch.zeros(4, 1, 64, 96, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, 96, 160, 3, dtype=torch.uint8, device=DEV)
    blend = lambda fp, op, nx=2, ny=2, ox=ints(0, 64), oy=ints(0, 32), F=1, TH=64, TW=96, H=96, W=160: \
        lib.ce_tiles_blend_u8(fp, op, nx, ny, ox, oy, F, TH, TW, H, W, stream)
    fp, op = fr.data_ptr(), out.data_ptr()
    assert blend(fp, op) == 0 and blend(fp, op, H=90, W=150) == 0
    assert blend(None, op) == -1 and blend(fp, None) == -1 and blend(fp, fp) == -1 and blend(fp, op, F=0) == -1 and blend(fp, op, F=65536) == -1
    assert blend(fp, op, W=161) == -1 and blend(fp, op, H=97) == -1 and blend(fp, op, H=0) == -1  # a target outside the canvas
    assert blend(fp, op, ox=ints(0, 97)) == -1 and blend(fp, op, ox=ints(64, 0)) == -1 and blend(fp, op, nx=17) == -1 and blend(fp, op, ox=None) == -1
    torch.cuda.synchronize()
    with pytest.raises(ops.HipKernelError, match="ce_tiles_fuse_f32 failed: bad argument"):
        ops.tiles_fuse(t, c, (0, 4), (0, 4))
    with pytest.raises(ValueError, match="4 tiles"):
        ops.tiles_fuse(t[:3], c, (0, 8), (0, 4))
    with pytest.raises(TypeError):
        ops.tiles_scatter(c.double(), t, (0, 8), (0, 4))
