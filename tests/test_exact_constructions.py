"""The exact-test constructions of tests/exact_util.py, checked on the CPU (no GPU): the integer GEMM / conv data keeps every fp32 sum
exact at the largest K the GPU tests use, the needle inputs have one winner per row, head and sample with the required margin (and every
forbidden key would win if read), the MX fp8 operands round-trip through the quantisation contract, and assert_exact names a single
changed element wherever it sits."""
import pytest
import torch

from exact_util import (BF, MIN_MARGIN_NATS, assert_exact, bf16_rne, edge_keys, int_rows, int_vector, linear_f64, mx_operand,
                        needle_k, needle_margins, needle_q, winners_for)
from test_mxfp8_gemm_gpu import _contract, _deq


@pytest.mark.parametrize("recipe", ["gemm", "gelu", "conv"])
def test_integer_data_sums_exactly_in_fp32(recipe):
    """fp32 CPU matmul == fp64, element for element, at the largest K (GEMM 13824; the conv's 27 taps x 384 channels = 10368)."""
    g = torch.Generator().manual_seed(5)
    if recipe == "gemm":
        K, a, w, bias = 13824, None, None, None
        a, w, bias = int_rows(64, K, g), int_rows(48, K, g), int_vector(48, g)
    elif recipe == "gelu":
        K = 5120
        a, w, bias = int_rows(64, K, g, emin=-5, emax=-4), int_rows(48, K, g, emin=-6, emax=-5), int_vector(48, g, lo=-32, hi=32, e=-4)
    else:
        K = 27 * 384
        a, w, bias = int_rows(64, K, g, emin=-1, emax=-1), int_rows(48, K, g), int_vector(48, g)
    exact = linear_f64(a, w, bias)
    f32 = a.float() @ w.float().t() + bias
    assert torch.equal(f32.double(), exact)
    assert exact.abs().max().item() > 256 * 2 ** -8  # (the sums need more bits than bf16 holds: rounding, ties included, happens)
    bf = bf16_rne(exact)
    assert not torch.equal(bf.float().double(), exact)


def test_needle_margins_at_the_step_shape():
    """7200 keys, 3 stacked samples, 2 heads: every query row's winner leads every other key of its sample by >= 22 nats, and every key
    of the other samples, and every key flagged invalid, beats the winner by >= 22 nats (rows: the edge winners and a random subset)."""
    n, B, H = 7200, 3, 2
    g = torch.Generator().manual_seed(9)
    extra = 64
    ks = [needle_k(n, H, sample=b) for b in range(B)] + [needle_k(extra, H, sample=0, invalid=torch.ones(extra, dtype=torch.bool))]
    k = torch.cat(ks).to(BF)
    for b in range(B):
        win = winners_for(n, n, H, g, must=edge_keys(n))
        rows = torch.cat([torch.arange(64), torch.randperm(n - 192, generator=g)[:256] + 64, torch.arange(n - 128, n)])
        q = needle_q(win[rows], sample=b, batch=B).to(BF)
        assert torch.equal(q.float().double(), needle_q(win[rows], sample=b, batch=B))  # exact in bf16
        forb = torch.ones(k.shape[0], dtype=torch.bool)
        forb[b * n:(b + 1) * n] = False
        lead, fl = needle_margins(q, k, H, win[rows] + b * n, forb)
        assert lead.min().item() >= MIN_MARGIN_NATS, lead.min()
        assert fl.min().item() >= MIN_MARGIN_NATS, fl.min()
    assert set(edge_keys(n)) <= set(win[:, 0].tolist()) and {0, 63, 64, 127, 128, n - 1} <= set(edge_keys(n))


def test_needle_winners_differ_per_head():
    g = torch.Generator().manual_seed(1)
    win = winners_for(300, 257, 4, g, must=edge_keys(257))
    for h in range(1, 4):
        assert (win[:, h] != win[:, 0]).float().mean() > 0.5
    assert set(range(256, 257)) <= set(win[-len(edge_keys(257)):, 0].tolist())


def test_mx_operands_round_trip_through_the_contract():
    g = torch.Generator().manual_seed(0)
    for M, K in ((129, 256), (7, 13824)):
        x = mx_operand(M, K, g)
        s, q = _contract(x)
        assert torch.equal(_deq(q, s), x.float())
        assert (s == 1).any()  # an all-zero block / row: scale byte 1 (2^-126)
        amax = x.float().view(M, -1, 32).abs().amax(-1)
        mant = amax / torch.exp2(torch.floor(torch.log2(amax.clamp(min=1e-30))))
        assert ((mant > 1.75) & (amax > 0)).any()  # the non-saturating scale's +1 branch


@pytest.mark.parametrize("pos", ["first", "middle", "last"])
def test_assert_exact_names_a_single_changed_element(pos):
    want = (torch.randn(37, 41) * 3).to(BF)
    idx = {"first": (0, 0), "middle": (18, 20), "last": (36, 40)}[pos]
    got = want.clone()
    got.view(torch.int16)[idx] += 1  # the next bf16 value away from zero: one ulp
    assert got[idx] != want[idx]
    assert_exact(want.clone(), want, "identical")
    with pytest.raises(AssertionError) as e:
        assert_exact(got, want, "probe")
    msg = str(e.value)
    assert "1 of 1517 elements differ" in msg and f"{idx}: got" in msg, msg
    with pytest.raises(AssertionError):
        assert_exact(got, want, "probe", ulps=0)
    assert_exact(got, want, "one ulp", ulps=1)
