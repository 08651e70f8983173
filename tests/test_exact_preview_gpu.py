"""The two device passes of the live previews (csrc/ce_preview.hip) against their CPU contracts (chronoedit_amd/preview.py).

ce_preview_rgb_u8 is bit-equal to `rgb_u8_reference` - no tolerance - over both store paths (8 x 12 cells: dword stores; 5 x 7: odd rows,
byte stores), one and two samples, one and three latent frames, every scale, with and without the region composite, with a NaN and two
infinite cells, into a buffer pre-filled with garbage.  Random normal data rarely lands a byte on a rounding tie, so a second set of cases
runs on data built to tell the orders of operations apart: there the same map summed in the reverse channel order, or interpolated
vertically first, differs from the reference in the bytes - and the kernel does not.
ce_preview_gram_f64 is exact on dyadic data (torch.equal to `gram_reference`, y as fp32 and as bf16), gives the same bits twice, and on
random data stays within the derived bound |got - want| <= n * 2^-52 * sum |terms| per entry (n cells: two float64 sums of n exact
products, each within (n - 1) * 2^-53 * sum |terms| of the true value to first order)."""
import numpy as np
import pytest
import torch

from chronoedit_amd import preview as pv

pytestmark = pytest.mark.gpu


def _case(h, w, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, 16, T, h, w, generator=g)
    z = torch.randn(B, 16, T, h, w, generator=g)
    f = torch.randn(17, 3, generator=g) * 0.25
    wt = torch.rand(h, w, generator=g)
    wt[0, :3], wt[1, :3] = 0.0, 1.0  # kept cells, edited cells, greys elsewhere
    for t in range(T):  # special cells in every frame, away from each other
        x0[0, 3, t, h - 1, w - 1] = float("nan")
        x0[B - 1, 5, t, 2, 4] = float("inf")
        x0[0, 7, t, 3, 1] = float("-inf")
    return x0, z, f, wt


@pytest.mark.parametrize("hw", [(8, 12), (5, 7)])
@pytest.mark.parametrize("B, T, frame", [(1, 1, 0), (2, 3, 0), (2, 3, -1), (1, 3, 1)])
def test_rgb_u8_is_bit_equal_to_the_reference(hw, B, T, frame):
    from chronoedit_amd import ops
    h, w = hw
    x0, z, f, wt = _case(h, w, B, T, seed=10 * h + B + T)
    dx0, dz, df, dw = x0.cuda(), z.cuda(), f.cuda(), wt.cuda()
    for scale in (1, 2, 4, 8):
        for comp in (False, True):
            kw = dict(w=wt, z_src=z) if comp else {}
            want = pv.rgb_u8_reference(x0, f, scale, frame, **kw)
            out = torch.full((B, h * scale, w * scale, 3), 77, dtype=torch.uint8, device="cuda")  # garbage: every byte is overwritten
            got = ops.preview_rgb_u8(dx0, df, scale, frame, dw if comp else None, dz if comp else None, out=out)
            assert got.data_ptr() == out.data_ptr()
            bad = (got.cpu() != want).nonzero()
            assert bad.numel() == 0, (scale, comp, bad[:4].tolist())


def _cancelling(h, w, scale, seed=0):
    """Data on which the order of the fp32 operations shows in the BYTES: channel 0 carries 4096 * r(y) * c(x) with r, c alternating between
    1 and -(2 scale - 1), so that the bilinear taps at t = 1 / (2 scale) cancel to the size of the other channels' random values - the
    rounding errors of the large terms, which depend on the order, are then a good part of a byte's step."""
    g = torch.Generator().manual_seed(seed)
    x0, f = torch.randn(2, 16, 1, h, w, generator=g), torch.randn(17, 3, generator=g) * 0.25
    r = torch.where(torch.arange(h) % 2 == 0, 1.0, -(2.0 * scale - 1))
    c = torch.where(torch.arange(w) % 2 == 0, 1.0, -(2.0 * scale - 1))
    x0[:, 0] += 4096.0 * (r[:, None] * c[None, :])
    f[0] = torch.tensor([1.0, -0.5, 0.25])
    return x0, f


@pytest.mark.parametrize("hw", [(8, 12), (5, 7)])
@pytest.mark.parametrize("scale", [2, 4, 8])
def test_rgb_u8_on_data_that_tells_the_orders_of_operations_apart(hw, scale):
    from chronoedit_amd import ops
    x0, f = _cancelling(*hw, scale)
    want = pv.rgb_u8_reference(x0, f, scale)
    # the sensitivity of the check: the same map with the channel sum reversed, or interpolated vertically first, differs somewhere
    assert not torch.equal(pv.rgb_u8_reference(x0, f, scale, order=range(15, -1, -1)), want)
    assert not torch.equal(pv.rgb_u8_reference(x0, f, scale, vertical_first=True), want)
    assert 0.05 < float(((want > 0) & (want < 255)).float().mean())  # (not everything is clamped)
    got = ops.preview_rgb_u8(x0.cuda(), f.cuda(), scale).cpu()
    assert torch.equal(got, want), int((got != want).sum())


def test_rgb_u8_into_an_unaligned_buffer_and_its_refusals():
    from chronoedit_amd import ops
    x0, z, f, wt = _case(8, 12, 1, 1, seed=3)
    want = pv.rgb_u8_reference(x0, f, 2)
    store = torch.zeros(8 * 2 * 12 * 2 * 3 + 8, dtype=torch.uint8, device="cuda")
    out = store[1:1 + want.numel()].view(1, 16, 24, 3)  # one byte off a dword: the byte-store path
    ops.preview_rgb_u8(x0.cuda(), f.cuda(), 2, out=out)
    assert torch.equal(out.cpu(), want) and int(store[0]) == 0 and int(store[1 + want.numel():].sum()) == 0
    with pytest.raises(ValueError):
        ops.preview_rgb_u8(x0.cuda(), f.cuda(), 3)
    with pytest.raises(ValueError):
        ops.preview_rgb_u8(x0.cuda(), f.cuda(), 2, frame=1)
    with pytest.raises(ValueError):
        ops.preview_rgb_u8(x0.cuda(), f.cuda(), 2, w=wt.cuda())
    with pytest.raises(ValueError):
        ops.preview_rgb_u8(x0.cuda()[:, :8].contiguous(), f.cuda(), 2)
    lib = ops.lib()
    p = lambda t: ops._ptr(t)
    dx, df = x0.cuda(), f.cuda()
    assert lib.ce_preview_rgb_u8(p(dx), p(None), p(None), p(df), p(out), 1, 8, 1, 0, 8, 12, 2, ops._stream()) == -1  # C != 16
    assert lib.ce_preview_rgb_u8(p(dx), p(None), p(None), p(df), p(out), 1, 16, 1, 0, 8, 12, 3, ops._stream()) == -1  # scale
    assert lib.ce_preview_rgb_u8(p(dx), p(dx), p(None), p(df), p(out), 1, 16, 1, 0, 8, 12, 2, ops._stream()) == -1  # z_src without w
    assert lib.ce_preview_rgb_u8(ops.ctypes.c_void_p(dx.data_ptr() + 2), p(None), p(None), p(df), p(out), 1, 16, 1, 0, 8, 12, 2, ops._stream()) == -3
    assert lib.ce_preview_rgb_u8(p(dx), p(None), p(None), p(df), p(out), 1, 16, 1, 0, 1 << 13, 1 << 13, 2, ops._stream()) == -2


def _dyadic(seed=0, B=2, T=1, h=8, w=12):
    rng = np.random.default_rng(seed)
    z = torch.from_numpy(rng.integers(-4, 5, size=(B, 16, T, h, w)).astype(np.float32))
    f = torch.from_numpy((rng.choice([-1, 1], size=(17, 3)) * rng.integers(1, 9, size=(17, 3)) / 8.0).astype(np.float32))
    y = pv.project_reference(z, f, T - 1).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)
    y = y + torch.from_numpy(rng.integers(-2, 3, size=tuple(y.shape)).astype(np.float32)) * 0.25  # the pixels of a cell differ
    return z, f, y.contiguous()


@pytest.mark.parametrize("B, T, h, w", [(2, 1, 8, 12), (1, 3, 5, 7), (3, 1, 9, 11)])
def test_gram_is_exact_on_dyadic_data_and_the_same_twice(B, T, h, w):
    from chronoedit_amd import ops
    z, f, y = _dyadic(1, B, T, h, w)
    for yy in (y, y.to(torch.bfloat16)):  # (rounded to bf16 the pixels are still dyadic)
        want = pv.gram_reference(z, yy, -1)
        got = ops.preview_gram(z.cuda(), yy.cuda(), -1)
        again = ops.preview_gram(z.cuda(), yy.cuda(), -1)
        assert got.dtype == torch.float64 and torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
        assert torch.equal(got, again)
    # a scratch of one workgroup's size: another summation tree, the same exact sums
    small = torch.empty(210 * 8, dtype=torch.uint8, device="cuda")
    assert torch.equal(ops.preview_gram(z.cuda(), y.cuda(), -1, scratch=small).cpu(), pv.gram_reference(z, y, -1))
    with pytest.raises(ops.HipKernelError):
        ops.preview_gram(z.cuda(), y.cuda(), -1, scratch=small[:-8])


def test_planted_factors_come_back_from_the_device_gram():
    from chronoedit_amd import ops
    rng = np.random.default_rng(4)
    z = torch.from_numpy(rng.integers(-4, 5, size=(2, 16, 1, 8, 12)).astype(np.float32))
    f = torch.from_numpy((rng.choice([-1, 1], size=(17, 3)) * rng.integers(1, 9, size=(17, 3)) / 8.0).astype(np.float32))
    y = pv.project_reference(z, f, 0).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3).contiguous()
    got, report = pv.solve_factors(ops.preview_gram(z.cuda(), y.cuda(), 0).cpu())
    assert torch.equal(got, f) and max(report["rms"]) < 1e-6


def test_gram_on_random_data_is_within_the_derived_bound():
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(7)
    B, h, w = 2, 24, 40  # 1920 cells: 30 rounds of 64 over several workgroups
    z = torch.randn(B, 16, 1, h, w, generator=g)
    for y in (torch.randn(B, 3, 8 * h, 8 * w, generator=g), torch.randn(B, 3, 8 * h, 8 * w, generator=g).to(torch.bfloat16)):
        want = pv.gram_reference(z, y)
        v = torch.cat([z[:, :, 0], torch.ones(B, 1, h, w), pv.box_mean_reference(y)], dim=1).permute(0, 2, 3, 1).reshape(-1, 20).double()
        n = v.shape[0]
        bound = n * 2.0 ** -52 * (v.abs().T @ v.abs())  # per entry: n * 2^-52 * sum over the cells of |v_i v_j|
        got = ops.preview_gram(z.cuda(), y.cuda()).cpu()
        err = (got - want).abs()
        print("gram: max |got - want| / bound =", float((err / bound).max()))
        assert bool((err <= bound).all()), float((err / bound).max())
        assert torch.equal(got, got.T) and float(got[16, 16]) == n
