"""The device passes of csrc/ce_components.hip bit for bit against `components.reference` (numpy on row runs, itself checked against scipy in
tests/test_components_cpu.py): roots, sums, keep and the counters, on planes placed where the kernels can go wrong - one short of, exactly
and one past the tile on each axis, 2 x 2 and 3 x 3 tiles plus an odd remainder, the serpentine, the comb and the spiral crossing every
tile border, a component whose root lies in the last tile, one random 1024 x 1024 plane - with garbage in every output and scratch buffer,
byte planes at odd addresses, and a second run.  Then the automatic region's two passes against their torch expressions."""
import components_shapes as S
import numpy as np
import pytest
import torch

from chronoedit_amd import auto_region as ar
from chronoedit_amd import components, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = components.TILE
SIZES = [(TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (TH - 1, 2 * TW + 1), (2 * TH + 1, TW - 1), (2 * TH, 2 * TW), (2 * TH + 5, 2 * TW + 7),
         (3 * TH + 3, 3 * TW + 13)]


def unaligned(t: torch.Tensor, offset: int) -> torch.Tensor:
    """A copy of the byte plane t on the device whose first byte lies `offset` past an allocation's start."""
    base = torch.full((t.numel() + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    v = base[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == offset % 4 and v.is_contiguous()
    return v


def garbage_i32(H, W):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (H, W), dtype=torch.int64, device=DEV).to(torch.int32)


def reference(plane: np.ndarray, weight=None):
    r = components.roots(torch.from_numpy(plane))
    return r, components.sums(r, None if weight is None else torch.from_numpy(weight))


def device_roots_and_sums(plane: np.ndarray, weight=None, offset=0):
    H, W = plane.shape
    p = unaligned(torch.from_numpy(plane), offset)
    w = None if weight is None else unaligned(torch.from_numpy(weight), (offset + 1) % 4)
    r = components.roots(p, garbage_i32(H, W))
    return p, r, components.sums(r, w, garbage_i32(H, W))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_roots_and_sums_on_every_shape_around_the_tile(size):
    H, W = size
    cases = dict(S.adversarial(H, W, seed=H + W), last_tile=S.root_in_last_tile(H, W, TH, TW))
    for k, (name, plane) in enumerate(cases.items()):
        want_r, want_s = reference(plane)
        _, r, s = device_roots_and_sums(plane, offset=k % 4)
        assert r.dtype == torch.int32 and torch.equal(r.cpu(), want_r), (name, int((r.cpu() != want_r).sum()))
        assert torch.equal(s.cpu(), want_s), name
    last = components.roots(torch.from_numpy(cases["last_tile"])).numpy()
    assert last.max() // W >= (H - 1) // TH * TH and last.max() % W >= (W - 1) // TW * TW  # (the root does lie in the last tile)


@pytest.fixture(scope="module")
def big():
    plane, weight = S.noise(1024, 1024, 0.4, 7), S.noise(1024, 1024, 0.5, 8)
    r = components.roots(torch.from_numpy(plane))
    return plane, weight, r, components.sums(r), components.sums(r, torch.from_numpy(weight))


def test_a_random_megapixel_plane_a_weight_plane_and_a_second_run(big):
    plane, weight, want_r, want_s, want_sw = big
    p, r, s = device_roots_and_sums(plane)
    assert torch.equal(r.cpu(), want_r) and torch.equal(s.cpu(), want_s)
    _, r2, sw = device_roots_and_sums(plane, weight, offset=3)
    assert torch.equal(r2.cpu(), want_r) and torch.equal(sw.cpu(), want_sw) and not torch.equal(want_sw, want_s)
    for frac in (4, 0.01):
        want_o, want_stats = components.keep(torch.from_numpy(plane), want_r, want_sw, frac)
        scratch = torch.randint(0, 256, (components.scratch_bytes(1024, 1024) + 4,), dtype=torch.uint8, device=DEV)
        out = torch.full((1024, 1024), 0x5A, dtype=torch.uint8, device=DEV)
        o, stats = components.filter(p, frac, torch.from_numpy(weight).to(DEV), scratch, out)
        assert o is out and torch.equal(o.cpu(), want_o) and torch.equal(stats.cpu(), want_stats), frac
        assert want_stats[0] >= 1 and want_stats[1] >= 1
        o2, stats2 = components.filter(p, frac, torch.from_numpy(weight).to(DEV))  # the same bits on a second run, scratch made by the call
        assert torch.equal(o2, o) and torch.equal(stats2, stats)


def three_blobs():
    """Components of 3, 10 and 40 pixels, each across a tile border: a diagonal through a tile corner, a row run across a vertical border,
    a column across a horizontal one."""
    p = np.zeros((2 * TH + 6, 2 * TW + 12), np.uint8)
    for k in range(3):
        p[TH - 1 + k, TW - 1 + k] = 9
    p[TH + 8, TW - 4:TW + 6] = 255
    p[TH - 20:TH + 20, TW + 36] = 1
    return p


@pytest.mark.parametrize("mw, kept", [(9, (10, 40)), (10, (10, 40)), (11, (40,)), (3, (3, 10, 40)), (41, ()),
                                       (0.25, (10, 40)),      # 1 / 4 of 40 = 10 exactly: kept
                                       (0.26, (40,)),         # 13 / 50 of 40 = 10.4 -> 11
                                       (0.075, (3, 10, 40)),  # 3 / 40 of 40 = 3 exactly
                                       (0.076, (10, 40))])    # 19 / 250 of 40 = 3.04 -> 4
def test_keep_at_the_threshold_and_the_counters(mw, kept):
    p = three_blobs()
    H, W = p.shape
    want_o, want_stats = components.reference(torch.from_numpy(p), mw)
    sizes = {3: 9, 10: 255, 40: 1}
    assert np.array_equal(want_o.numpy(), np.where(np.isin(p, [sizes[n] for n in kept]), p, 0))
    assert want_stats.tolist() == [len(kept), 3 - len(kept), sum(n for n in sizes if n not in kept), 40]
    dp, r, s = device_roots_and_sums(p, offset=1)
    o, stats = components.keep(dp, r, s, mw, unaligned(torch.full((H, W), 77, dtype=torch.uint8), 3), garbage_i32(1, 4).view(4))
    assert torch.equal(o.cpu(), want_o) and torch.equal(stats.cpu(), want_stats)


def test_refusals():
    p = torch.from_numpy(three_blobs()).to(DEV)
    H, W = p.shape
    odd = torch.empty(4 * H * W + 4, dtype=torch.uint8, device=DEV)[1:4 * H * W + 1]
    with pytest.raises((ops.HipKernelError, RuntimeError, ValueError)):
        ops.components_roots_i32(p, odd.view(torch.int32).view(H, W))  # (torch itself refuses the misaligned view)
    r = components.roots(p)
    with pytest.raises(ValueError):
        components.filter(p, 0)
    with pytest.raises(ValueError):
        components.filter(p, 3, scratch=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        components.sums(r, torch.zeros(H, W, dtype=torch.uint8))  # a weight plane on another device
    with pytest.raises(ValueError):
        ops.components_keep_u8(p, r, components.sums(r), 0, 3, 3)  # a fraction of 1


@pytest.mark.parametrize("grid", [(1, 1), (7, 13), (45, 80)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_auto_region_seed_and_masked_passes(grid):
    h, w = grid
    g = torch.Generator().manual_seed(h)
    d = torch.rand(h, w, generator=g)
    d.view(-1)[::5] = 0.5  # cells AT the threshold: no seeds
    if h * w > 3:
        d.view(-1)[3] = float("nan")
    thr = torch.tensor([0.5])
    seeds = ar.seed_plane(d.to(DEV), thr.to(DEV))
    want = (d > 0.5).to(torch.uint8) * 255
    assert seeds.dtype == torch.uint8 and torch.equal(seeds.cpu(), want) and torch.equal(ar.seed_plane(d, thr), want)
    kept = (torch.rand(h, w, generator=g) < 0.5).to(torch.uint8) * 3
    dk = ar.masked_map(d.to(DEV), kept.to(DEV))
    want_dk = torch.where(kept != 0, d, torch.tensor(-1.0))
    assert torch.equal(dk.cpu().view(torch.int32), want_dk.view(torch.int32)) and torch.equal(ar.masked_map(d, kept).view(torch.int32), want_dk.view(torch.int32))
    for mw in (2, 0.3):
        got, stats = ar.kept_map(d.to(DEV), thr.to(DEV), mw)
        ref, ref_stats = ar.kept_map(d, thr, mw)
        assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32)) and torch.equal(stats.cpu(), ref_stats)
        assert torch.equal(ar.ramp_weights(got, thr.to(DEV), 1, 1).cpu(), ar.ramp_weights(ref, thr, 1, 1))
