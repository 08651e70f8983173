"""The three passes of csrc/ce_sketch.hip, and the whole mask built on the device, against `sketch.reference` and its stages on the CPU:
bit-equal, no tolerance."""
import numpy as np
import pytest
import torch

from chronoedit_amd import ops, sketch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (SW, SH): widths that are no multiple of 4 or 16, one-pixel axes, columns longer than a segment of the vertical pass (32 rows) - on its
# byte path with masked columns (11 x 1100) and on its dword path (12 x 1100) -, and rows longer than one
# workgroup's run of the horizontal pass (4096 bytes: 4100 x 3, and 9000 x 2 with a run that has a neighbour on either side)
SIZES = [(7, 9), (53, 37), (130, 41), (1, 17), (17, 1), (1100, 11), (11, 1100), (12, 1100), (4100, 3), (9000, 2)]
LONG = 1100


def radii_for(size, large):
    """0, 1, 7 everywhere; `large` where an axis is long (a window over several tiles and halos); on 7 x 9 one larger than the image."""
    out = [0, 1, 7]
    if max(size) >= LONG:
        out.append(large)
    if size == (7, 9):
        out.append(20 if large == 300 else 12)
    return out


def marked(size, seed, extra=0.0):
    """A 0 / 255 plane uint8 [SH, SW] with all four corners, a pixel on every edge and a few interior pixels set (extra: that share more)."""
    SW, SH = size
    rng = np.random.default_rng(seed)
    m = np.zeros((SH, SW), np.uint8)
    for y, x in ((0, 0), (0, SW - 1), (SH - 1, 0), (SH - 1, SW - 1), (0, SW // 2), (SH - 1, SW // 3), (SH // 2, 0), (SH // 3, SW - 1)):
        m[y, x] = 255
    m[rng.integers(0, SH, 3), rng.integers(0, SW, 3)] = 255
    if extra:
        m[rng.random((SH, SW)) < extra] = 255
    return torch.from_numpy(m)


def sparse(size, seed):
    """A 0 / 255 plane with three set pixels only: most windows stay empty, whatever the radius."""
    SW, SH = size
    rng = np.random.default_rng(seed)
    m = np.zeros((SH, SW), np.uint8)
    m[rng.integers(0, SH, 3), rng.integers(0, SW, 3)] = 255
    return torch.from_numpy(m)


def run_pass(fn, plane_cpu, axis, radius):
    """The device pass into an `out` full of garbage, twice: the same bits, and the result on the host."""
    dev = plane_cpu.to(DEV)
    out = torch.full_like(dev, 0x5A)
    got = fn(dev, axis, radius, out=out)
    assert got.data_ptr() == out.data_ptr()
    again = fn(dev, axis, radius, out=torch.full_like(dev, 0xA5))
    assert torch.equal(got, again)
    assert torch.equal(dev.cpu(), plane_cpu)  # the input is untouched
    return got.cpu()


@pytest.mark.parametrize("size", SIZES)
def test_dilate_equals_the_cpu_stage(size):
    for radius in radii_for(size, 300):
        for axis in (0, 1):
            for plane in (marked(size, 1), sparse(size, 2), torch.zeros(size[1], size[0], dtype=torch.uint8)):
                want = sketch.dilate(plane, radius, axis)
                got = run_pass(ops.sketch_dilate_u8, plane, axis, radius)
                assert torch.equal(got, want), (size, radius, axis, int((got != want).sum()))
    # the window is clipped, not wrapped: one pixel in a corner marks radius + 1 pixels along the axis and nothing else
    SW, SH = size
    one = torch.zeros(SH, SW, dtype=torch.uint8)
    one[SH - 1, SW - 1] = 255
    got = run_pass(ops.sketch_dilate_u8, one, 0, 7)
    assert int((got == 255).sum()) == min(8, SW) and bool((got[SH - 1, max(SW - 8, 0):] == 255).all())
    got = run_pass(ops.sketch_dilate_u8, one, 1, 7)
    assert int((got == 255).sum()) == min(8, SH) and bool((got[max(SH - 8, 0):, SW - 1] == 255).all())


@pytest.mark.parametrize("size", SIZES)
def test_box_equals_the_cpu_stage(size):
    SW, SH = size
    grey = torch.from_numpy(np.random.default_rng(SW * 31 + SH).integers(0, 256, (SH, SW), dtype=np.uint8))
    for radius in radii_for(size, 150):
        for axis in (0, 1):
            for plane in (grey, marked(size, 3, extra=0.3), torch.full((SH, SW), 255, dtype=torch.uint8)):
                want = sketch.box(plane, radius, axis)
                got = run_pass(ops.sketch_box_u8, plane, axis, radius)
                assert torch.equal(got, want), (size, radius, axis, int((got != want).sum()))
    assert torch.equal(run_pass(ops.sketch_box_u8, grey, 0, 0), grey) and torch.equal(run_pass(ops.sketch_box_u8, grey, 1, 0), grey)
    full = torch.full((SH, SW), 255, dtype=torch.uint8)  # the replicated edges: a full plane stays full at every radius
    assert torch.equal(run_pass(ops.sketch_box_u8, full, 0, 7), full) and torch.equal(run_pass(ops.sketch_box_u8, full, 1, 7), full)


def pair(size, seed, threshold):
    """background, composite uint8 [SH, SW, 3]: mostly equal; the first pixels carry, channel by channel, a difference of exactly
    `threshold` (not changed) and of threshold + 1 (changed) in both directions, and of 255 in both directions - the top left corner is
    the first of these probes, so it is NOT changed (the passes see that corner set through `marked`) -; the other three corners and a
    pixel on the bottom and the right edge are changed; the rest differs by at most `threshold`."""
    SW, SH = size
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    step = np.minimum(rng.integers(0, threshold + 1, bg.shape), 127)
    cp = np.where(bg >= 128, bg - step, bg + step).astype(np.uint8)
    expect = {}
    flat_bg, flat_cp = bg.reshape(-1, 3), cp.reshape(-1, 3)
    k = 0
    for c in range(3):
        for delta, is_changed in ((threshold, False), (threshold + 1, True), (255, True)):
            for sign in (1, -1):
                if k >= SW * SH - 1:
                    break
                base = 0 if sign > 0 else 255
                flat_bg[k] = 100
                flat_cp[k] = 100
                flat_bg[k, c], flat_cp[k, c] = base, base + sign * delta
                expect[k] = is_changed
                k += 1
    for y, x in ((0, SW - 1), (SH - 1, 0), (SH - 1, SW - 1), (SH - 1, SW // 2), (SH // 2, SW - 1)):
        if y * SW + x >= k:
            bg[y, x], cp[y, x] = 0, 255
            expect[y * SW + x] = True
    return torch.from_numpy(bg), torch.from_numpy(cp), expect


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("threshold", [0, 5, 254])
def test_changed_equals_the_cpu_stage(size, threshold):
    SW, SH = size
    bg, cp, expect = pair(size, SW + 7 * SH + threshold, threshold)
    want = sketch.changed(bg, cp, threshold)
    for k, is_changed in expect.items():  # the threshold's two sides, every channel taking the maximum in turn, 255 in both directions
        assert int(want.reshape(-1)[k]) == (255 if is_changed else 0), (k, is_changed)
    assert set(np.unique(want.numpy()).tolist()) <= {0, 255}
    b, c = bg.to(DEV), cp.to(DEV)
    out = torch.full((SH, SW), 0x5A, dtype=torch.uint8, device=DEV)
    got = ops.sketch_changed_u8(b, c, threshold, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu(), want)
    assert torch.equal(ops.sketch_changed_u8(b, c, threshold).cpu(), want)  # the same bits twice
    assert torch.equal(ops.sketch_changed_u8(c, b, threshold).cpu(), want)  # |a - b| is symmetric
    # bases that are not 16-byte aligned: byte by byte, the same bytes
    ub = torch.empty(SH * SW * 3 + 1, dtype=torch.uint8, device=DEV)
    uc, uo = torch.empty_like(ub), torch.full((SH * SW + 1,), 0x5A, dtype=torch.uint8, device=DEV)
    ub[1:].copy_(b.reshape(-1)), uc[1:].copy_(c.reshape(-1))
    got = ops.sketch_changed_u8(ub[1:].view(SH, SW, 3), uc[1:].view(SH, SW, 3), threshold, out=uo[1:].view(SH, SW))
    assert torch.equal(got.cpu(), want) and int(uo[0]) == 0x5A


@pytest.mark.parametrize("size", SIZES)
def test_the_whole_mask_equals_the_reference(size):
    bg, cp, _ = pair(size, 5, 3)
    b, c = bg.to(DEV), cp.to(DEV)
    combos = [(g, f) for g in (0, 1, 7) for f in (0, 1, 7)]
    if max(size) >= LONG:
        combos.append((150, 150))  # R = 300, feather 150
    if size == (7, 9):
        combos.append((8, 12))  # R = 20, feather 12: both windows larger than the image
    for grow, feather in combos:
        want = sketch.stages(bg, cp, grow, feather, 3)
        got = sketch.stages(b, c, grow, feather, 3)
        for name, g, w in zip(("changed", "grown", "mask"), got, want):
            assert g.is_cuda and torch.equal(g.cpu(), w), (size, grow, feather, name)
        assert torch.equal(sketch.mask(b, c, grow, feather, 3).cpu(), sketch.reference(bg, cp, grow, feather, 3))
        assert int(want[2].max()) == 255  # (not two empty planes)


@pytest.mark.parametrize("size", [(64, 8), (8, 64), (67, 5), (4200, 2), (6, 2100)])
def test_the_largest_radii_the_passes_admit(size):
    """Radius 4096 for the dilation and 1024 for the box mean, on both axes: the horizontal pass then asks for its largest LDS (13 scan
    rounds, 52 KiB), the vertical pass for its longest segment and halo; most windows hold the whole line."""
    SW, SH = size
    grey = torch.from_numpy(np.random.default_rng(SW + SH).integers(0, 256, (SH, SW), dtype=np.uint8))
    for axis in (0, 1):
        for plane in (marked(size, 6), sparse(size, 7)):
            for radius in (4096, 4095, 1500):
                got = run_pass(ops.sketch_dilate_u8, plane, axis, radius)
                assert torch.equal(got, sketch.dilate(plane, radius, axis)), (size, axis, radius)
        for plane in (grey, marked(size, 8, extra=0.3)):
            for radius in (1024, 1023, 600):
                got = run_pass(ops.sketch_box_u8, plane, axis, radius)
                assert torch.equal(got, sketch.box(plane, radius, axis)), (size, axis, radius)
    bg, cp, _ = pair(size, 9, 0)
    want = sketch.reference(bg, cp, 4096 - 1024, 1024, 0)
    assert torch.equal(sketch.mask(bg.to(DEV), cp.to(DEV), 4096 - 1024, 1024, 0).cpu(), want) and int(want.max()) == 255


@pytest.mark.parametrize("size", [(11, 1100), (12, 1100), (130, 41), (8, 200)])
def test_both_sides_of_the_vertical_pass_threshold(size):
    """Radius 63 sums a segment's first window row by row, radius 64 from the per-segment sums in the scratch; also windows that end inside
    the image's last, short segment, and a scratch of the caller's with garbage in it."""
    SW, SH = size
    grey = torch.from_numpy(np.random.default_rng(SW * SH).integers(0, 256, (SH, SW), dtype=np.uint8))
    for radius in (63, 64, 65, 95, 96, 97, 128):
        for plane, fn, ref in ((marked(size, 1), ops.sketch_dilate_u8, sketch.dilate), (sparse(size, 2), ops.sketch_dilate_u8, sketch.dilate),
                               (grey, ops.sketch_box_u8, sketch.box)):
            assert torch.equal(run_pass(fn, plane, 1, radius), ref(plane, radius, 1)), (size, radius, fn.__name__)
            need = ops.sketch_scratch_bytes(SH, SW, 1, radius)
            assert (need > 0) == (radius >= 64) and ops.sketch_scratch_bytes(SH, SW, 0, radius) == 0
            if need:
                scratch = torch.full((need + 8,), 0xEE, dtype=torch.uint8, device=DEV)
                assert torch.equal(fn(plane.to(DEV), 1, radius, scratch=scratch[:need]).cpu(), ref(plane, radius, 1))
                assert scratch[need:].tolist() == [0xEE] * 8  # nothing written past it
                with pytest.raises(ops.HipKernelError):
                    fn(plane.to(DEV), 1, radius, scratch=scratch[:need - 2])


def test_unaligned_planes_take_the_byte_paths():
    """A plane whose base is not 4-byte aligned (W % 4 == 0 notwithstanding): the same bytes, and nothing written in front of it."""
    SW, SH = 64, 300
    plane = marked((SW, SH), 4, extra=0.2)
    for fn, ref, radius in ((ops.sketch_dilate_u8, sketch.dilate, 9), (ops.sketch_box_u8, sketch.box, 9), (ops.sketch_dilate_u8, sketch.dilate, 70),
                            (ops.sketch_box_u8, sketch.box, 70)):
        for axis in (0, 1):
            src = torch.empty(SH * SW + 1, dtype=torch.uint8, device=DEV)
            src[1:].copy_(plane.reshape(-1).to(DEV))
            dst = torch.full((SH * SW + 3,), 0x5A, dtype=torch.uint8, device=DEV)
            got = fn(src[1:].view(SH, SW), axis, radius, out=dst[3:].view(SH, SW))
            assert torch.equal(got.cpu(), ref(plane, radius, axis)) and dst[:3].tolist() == [0x5A] * 3


def test_refusals():
    x = torch.zeros(4, 8, dtype=torch.uint8, device=DEV)
    for fn, too_large in ((ops.sketch_dilate_u8, 4097), (ops.sketch_box_u8, 1025)):
        with pytest.raises(ops.HipKernelError):
            fn(x, 0, too_large)
        with pytest.raises(ops.HipKernelError):
            fn(x, 0, -1)
        with pytest.raises(ValueError):
            fn(x, 2, 1)
        with pytest.raises(ValueError):
            fn(x[:, ::2], 0, 1)
    rgb = torch.zeros(4, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.sketch_changed_u8(rgb, rgb[:2])
    with pytest.raises(ValueError):
        ops.sketch_changed_u8(rgb, rgb.clone(), 255)
