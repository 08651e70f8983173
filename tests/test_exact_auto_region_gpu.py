"""The four passes of csrc/ce_region_auto.hip against their CPU torch expressions (chronoedit_amd/auto_region.py): bit-equal, no tolerance.
The CPU expressions themselves are held to brute-force loops in tests/test_auto_region_cpu.py."""
import pytest
import torch

from chronoedit_amd import auto_region as ar

pytestmark = pytest.mark.gpu


def _same(a, b):
    """torch.equal with NaNs in the same places."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _pair(shape, seed, offset=0):
    """Two fp32 tensors of `shape` on the CPU and their device copies, the latter `offset` elements into a larger allocation."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        t = torch.randn(*shape, generator=g)
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda:0")
        dv = buf[offset:offset + t.numel()].view(shape)
        dv.copy_(t)
        out += [t, dv]
    return out[0], out[2], out[1], out[3]


# (1, 16, 2, 8, 12) and (2, 16, 3, 6, 10): planes of 96 and 60 cells - four cells per lane when every pointer is 16-byte aligned; a base
# pointer one element off and a plane that is no multiple of 4 take the cell-per-lane kernel
@pytest.mark.parametrize("shape, frame, offset", [((1, 16, 2, 8, 12), -1, 0), ((1, 16, 2, 8, 12), 0, 1), ((2, 16, 3, 6, 10), 1, 0),
                                                  ((2, 16, 3, 6, 10), 2, 1), ((2, 16, 3, 6, 10), -1, 0), ((3, 5, 2, 3, 5), 1, 0),
                                                  ((1, 16, 1, 34, 32), 0, 0)])
def test_change_map(shape, frame, offset):
    from chronoedit_amd import ops
    x0, z, x0d, zd = _pair(shape, seed=len(shape) + shape[-1] + offset, offset=offset)
    assert x0d.data_ptr() % 16 == 4 * offset
    d = ops.auto_region_change(x0d, zd, frame)
    want = ar.change_map(x0, z, frame)
    assert d.dtype == torch.float32 and tuple(d.shape) == shape[-2:] and torch.equal(d.cpu(), want)
    # the output offset by one element too, and a NaN: it stays one, in its own cell only
    x0d[0, 1, frame, 1, 2] = float("nan")
    x0[0, 1, frame, 1, 2] = float("nan")
    buf = torch.zeros(d.numel() + 4, dtype=torch.float32, device="cuda:0")
    out = buf[1:1 + d.numel()].view(d.shape)
    ops.auto_region_change(x0d, zd, frame, out=out)
    assert _same(out.cpu(), ar.change_map(x0, z, frame)) and int(torch.isnan(out).sum()) == 1
    assert float(buf[0]) == 0.0 and bool((buf[1 + d.numel():] == 0).all())


def _otsu_maps():
    g = torch.Generator().manual_seed(1)
    two = torch.rand(8, 12, generator=g) * 0.05
    two[2:5, 3:7] += 3.0 + torch.rand(3, 4, generator=g)
    big = torch.rand(90, 160, generator=g) ** 3
    big[20:50, 40:100] += 2.0
    ties = (torch.arange(90 * 160) % 7).float().view(90, 160)  # seven equal spikes
    nan = big.clone()
    nan[::7, ::5] = float("nan")
    return {"8x12": two, "90x160": big, "90x160-spikes": ties, "90x160-nan": nan, "8x12-constant": torch.full((8, 12), 0.75),
            "8x12-zero": torch.zeros(8, 12), "90x160-one-cell": torch.zeros(90, 160).index_put((torch.tensor(3), torch.tensor(5)), torch.tensor(1e-3)),
            "8x12-all-nan": torch.full((8, 12), float("nan")), "8x12-inf": two.clone().index_put((torch.tensor(0), torch.tensor(0)), torch.tensor(float("inf")))}


@pytest.mark.parametrize("name", list(_otsu_maps()))
def test_otsu(name):
    from chronoedit_amd import ops
    d = _otsu_maps()[name]
    for floor in (0.0, 0.4):
        thr, dmax = ops.auto_region_otsu(d.cuda(), floor)
        want_thr, want_dmax = ar.otsu_threshold(d, floor)
        assert thr.dtype == torch.float32 and torch.equal(thr.cpu(), want_thr), (name, floor, float(thr), float(want_thr))
        assert torch.equal(dmax.cpu(), want_dmax), (name, float(dmax), float(want_dmax))


@pytest.mark.parametrize("dilate, feather", [(0, 0), (1, 1), (0, 8), (3, 5)])
def test_ramp(dilate, feather):
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(dilate * 10 + feather)
    maps = {"sparse": torch.rand(8, 12, generator=g), "empty": torch.zeros(8, 12), "all": torch.ones(8, 12)}
    corners = torch.zeros(8, 12)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = corners[3, 11] = 1.0
    corners[4, 4] = float("nan")
    maps["corners"] = corners
    for name, d in maps.items():
        thr = torch.tensor([0.93])
        w = ops.auto_region_ramp(d.cuda(), thr.cuda(), dilate, feather)
        want = ar.ramp_weights(d, thr, dilate, feather)
        assert w.dtype == torch.float32 and torch.equal(w.cpu(), want), (name, dilate, feather)
    # a threshold of +inf: nothing
    assert not bool(ops.auto_region_ramp(maps["all"].cuda(), torch.tensor([float("inf")]).cuda(), dilate, feather).any())
    with pytest.raises(ValueError):
        ops.auto_region_ramp(maps["all"].cuda(), torch.tensor([0.5]).cuda(), 5, 4)


def test_pixel_mask():
    from chronoedit_amd import ops
    w = torch.rand(8, 12, generator=torch.Generator().manual_seed(4))
    w[0, :6] = torch.tensor([0.0, 1.0, 0.5, 1.0 / 3.0, 2.0 / 3.0, 0.1])  # 127.5 rounds to 128: half to even
    want = ar.pixel_mask(w)
    m = ops.auto_region_mask_u8(w.cuda())
    assert m.dtype == torch.uint8 and tuple(m.shape) == (64, 96) and torch.equal(m.cpu(), want)
    # a mask one byte into its allocation: the byte-store kernel, and nothing written around it
    buf = torch.full((64 * 96 + 16,), 7, dtype=torch.uint8, device="cuda:0")
    out = buf[1:1 + 64 * 96].view(64, 96)
    ops.auto_region_mask_u8(w.cuda(), out=out)
    assert torch.equal(out.cpu(), want) and int(buf[0]) == 7 and bool((buf[1 + 64 * 96:] == 7).all())


def test_the_passes_chain_like_the_cpu_expressions():
    """auto_region.detect (four launches, one read) against auto_region.weights on the CPU, under both threshold forms."""
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(1, 16, 2, 8, 12, generator=g)
    z = x0.clone()
    z[:, :, -1, 2:4, 4:6] += 2.0
    for cfg in (ar.AutoRegionConfig(1), ar.AutoRegionConfig(1, threshold=1.0, dilate=0, feather=3)):
        d, thr, dmax, want = ar.weights(x0, z, cfg)
        rect = torch.zeros(8, 12, dtype=torch.bool)
        rect[2:4, 4:6] = True
        assert torch.equal(d > thr, rect)  # the input has exactly this region, under either threshold
        w, mask, w_cpu, thr_d, dmax_d = ar.detect(x0.cuda(), z.cuda(), cfg)
        assert torch.equal(w.cpu(), want) and torch.equal(w_cpu, want) and torch.equal(mask.cpu(), ar.pixel_mask(want))
        assert thr_d == float(thr) and dmax_d == float(dmax) and 3.9 < dmax_d < 4.1
