"""Live previews, host side (chronoedit_amd/preview.py): the config's validation, the two entry points in the header and the signature
table, properties of the CPU contract `rgb_u8_reference`, and `solve_factors` recovering a planted map.  No GPU."""
import numpy as np
import pytest
import torch

from chronoedit_amd import hiplib
from chronoedit_amd import preview as pv

ENTRY_POINTS = ("ce_preview_rgb_u8", "ce_preview_gram_f64")


def test_config_defaults_and_validation():
    cb = lambda d: None
    c = pv.PreviewConfig(cb)
    assert (c.every, c.scale, c.frame, c.composite, c.lag, c.factors) == (1, 2, -1, True, 1, None)
    c = pv.PreviewConfig(cb, every=3, scale=8, frame=0, composite=False, lag=0, factors=np.zeros((17, 3)))
    assert c.factors.dtype == torch.float32 and tuple(c.factors.shape) == (17, 3) and c.lag == 0
    bad = [dict(on_preview=None), dict(every=0), dict(every=1.5), dict(every=True), dict(scale=3), dict(scale=16), dict(scale=2.0),
           dict(frame=0.5), dict(composite=1), dict(lag=-1), dict(lag=1.0), dict(factors=np.zeros((16, 3))),
           dict(factors=np.full((17, 3), np.nan)), dict(factors=np.full((17, 3), np.inf))]
    for kw in bad:
        with pytest.raises(ValueError):
            pv.PreviewConfig(**dict(dict(on_preview=cb), **kw))


def test_which_steps_are_previewed():
    assert [i for i in range(6) if pv.due(i, 6, 1)] == [0, 1, 2, 3, 4, 5]
    assert [i for i in range(6) if pv.due(i, 6, 2)] == [1, 3, 5]
    assert [i for i in range(6) if pv.due(i, 6, 4)] == [3, 5]
    assert [i for i in range(6) if pv.due(i, 6, 7)] == [5]


def test_the_c_abi_declares_the_two_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_preview_")] == list(ENTRY_POINTS)
    assert "ce_preview.hip" in hiplib.SOURCES


def _data(seed=0, shape=(2, 16, 3, 5, 7)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g), torch.randn(17, 3, generator=g) * 0.3


def test_scale_1_is_the_projection_alone():
    x0, f = _data()
    for frame in (0, -1):
        got = pv.rgb_u8_reference(x0, f, 1, frame)
        p = pv.project_reference(x0, f, frame)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 5, 7, 3)
        assert torch.equal(got, pv.byte_reference(p).permute(0, 2, 3, 1))
    # the projection itself, against a float64 evaluation
    p64 = torch.einsum("bkhw,kc->bchw", x0[:, :, -1].double(), f[:16].double()) + f[16].double().view(1, 3, 1, 1)
    assert float((pv.project_reference(x0, f) - p64).abs().max()) < 1e-5


def test_zero_factors_give_128_everywhere_and_the_clamps_are_hit():
    x0, _ = _data(1)
    for scale in (1, 2, 4, 8):
        out = pv.rgb_u8_reference(x0, torch.zeros(17, 3), scale)
        assert tuple(out.shape) == (2, 5 * scale, 7 * scale, 3) and bool((out == 128).all())  # 127.5 -> 128: the only exact tie
    f = torch.zeros(17, 3)
    f[16] = torch.tensor([5.0, -5.0, 1.0])
    out = pv.rgb_u8_reference(x0, f, 2)
    assert bool((out[..., 0] == 255).all()) and bool((out[..., 1] == 0).all()) and bool((out[..., 2] == 255).all())
    f[16] = torch.tensor([-1.0, 0.0, 0.5])
    out = pv.rgb_u8_reference(x0, f, 4)
    assert bool((out[..., 0] == 0).all()) and bool((out[..., 1] == 128).all()) and bool((out[..., 2] == 191).all())  # rint(191.25)
    # the byte: NaN -> 0, +inf -> 255, -inf -> 0, the tie 127.5 -> 128 and 128.5 -> 128 (half to even)
    v = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, 1.0, -1.0, 129.0 / 255.0 - 1.0 + 2.0 ** -24])
    assert pv.byte_reference(v)[:6].tolist() == [0, 255, 0, 128, 255, 0]
    # an infinite interior cell at scale 1: its own pixel takes it with weight 1 (255); the pixels left of and above it take it with
    # weight 0, and 0 * inf is a NaN (0), as the expression says
    cells = torch.zeros(1, 16, 1, 4, 4)
    cells[0, 0, 0, 2, 2] = float("inf")
    f = torch.zeros(17, 3)
    f[0] = 1.0
    out = pv.rgb_u8_reference(cells, f, 1)[0, :, :, 0]
    assert int(out[2, 2]) == 255 and int(out[2, 1]) == 0 and int(out[1, 2]) == 0 and int(out[1, 1]) == 0 and int(out[3, 3]) == 128


def test_the_composite_shows_the_source_where_w_is_0():
    x0, f = _data(2)
    z = torch.randn(2, 16, 3, 5, 7, generator=torch.Generator().manual_seed(9))
    w = torch.zeros(5, 7)
    w[2:, 3:] = 1.0
    w[1, 1] = 0.25
    got = pv.rgb_u8_reference(x0, f, 1, -1, w, z)
    src, plain = pv.rgb_u8_reference(z, f, 1), pv.rgb_u8_reference(x0, f, 1)
    assert torch.equal(got[:, 0, :], src[:, 0, :]) and torch.equal(got[:, 2:, 3:], plain[:, 2:, 3:])
    assert not torch.equal(got, src) and not torch.equal(got, plain)
    with pytest.raises(ValueError):
        pv.rgb_u8_reference(x0, f, 1, -1, w, None)
    with pytest.raises(ValueError):
        pv.rgb_u8_reference(x0, f, 3)


def planted(seed):
    """Dyadic data: z integers in [-4, 4], a planted map whose 17 x 3 entries are nonzero multiples of 1/8 in [-1, 1], y = the map."""
    rng = np.random.default_rng(seed)
    z = torch.from_numpy(rng.integers(-4, 5, size=(2, 16, 1, 8, 12)).astype(np.float32))
    f = torch.from_numpy((rng.choice([-1, 1], size=(17, 3)) * rng.integers(1, 9, size=(17, 3)) / 8.0).astype(np.float32))
    cells = pv.project_reference(z, f, 0)  # exact: every product and partial sum is a multiple of 1/8 far below 2^24
    y = cells.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3).contiguous()
    return z, f, y


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_solve_factors_recovers_a_planted_map_exactly(seed):
    z, f, y = planted(seed)
    G = pv.gram_reference(z, y, 0)
    assert G.dtype == torch.float64 and tuple(G.shape) == (20, 20) and torch.equal(G, G.T) and float(G[16, 16]) == 2 * 8 * 12
    # the Gram matrix is exact: the same in exact integer arithmetic (everything scaled by 8)
    v = torch.cat([z[:, :, 0], torch.ones(2, 1, 8, 12), pv.project_reference(z, f, 0)], dim=1).permute(0, 2, 3, 1).reshape(-1, 20)
    vi = (v.double() * 8).to(torch.int64)
    assert torch.equal((G * 64).to(torch.int64), vi.T @ vi) and torch.equal(G * 64, (vi.T @ vi).double())
    got, report = pv.solve_factors(G)
    assert got.dtype == torch.float32 and torch.equal(got, f), float((got - f).abs().max())
    assert set(report) == {"rms", "r2"} and len(report["rms"]) == 3 and len(report["r2"]) == 3
    assert max(report["rms"]) < 1e-6 and min(report["r2"]) > 1 - 1e-9


def test_the_fit_report_tells_a_poor_fit():
    g = torch.Generator().manual_seed(5)
    z = torch.randn(1, 16, 1, 8, 12, generator=g)
    y = torch.randn(1, 3, 64, 96, generator=g)  # unrelated to z: nothing to explain
    f, report = pv.solve_factors(pv.gram_reference(z, y))
    assert tuple(f.shape) == (17, 3) and all(r2 < 0.5 for r2 in report["r2"]) and all(r > 0.05 for r in report["rms"])
    with pytest.raises(ValueError):
        pv.solve_factors(np.zeros((17, 17)))
