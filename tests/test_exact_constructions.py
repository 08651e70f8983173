"""The exact-test constructions of tests/exact_util.py, checked on the CPU (no GPU): the integer GEMM / conv data keeps every fp32 sum
exact at the largest K the GPU tests use, the needle inputs have one winner per row, head and sample with the required margin (and every
forbidden key would win if read), the MX fp8 operands round-trip through the quantisation contract, and assert_exact names a single
changed element wherever it sits.

The row / scheduler / softmax recipes (`unit_rows`, `rope_table`, `unipc_state`, `tie_targets`, ...): fp32 evaluation in a scrambled order
equals the fp64 answer bit for bit (exactness), the asserted share of results needs a real bf16 rounding, and the reference evaluated with
one deliberately wrong index differs from the right one in every affected row (sensitivity: the data can see that bug).

The MXFP8 attention cases (`mx_case`, every launch of tests/test_exact_attention_mxfp8_gpu.py): the bytes hold the intended values and the
quantisation contract keeps them, the margins hold, the contract oracle returns the closed form under both offset schedules, and every entry
of `MX_MISTAKES` is seen by the cases it applies to - and by one case at least.

The fp8 producers and GEMM tails (every launch of tests/test_exact_fp8_producers_gpu.py): the per-row restatement is exact on power-of-two rows,
`mx_contract` equals the contracts in use, sums are exact in fp32, GELU inputs lie in the saturated set (or span the bend), scale bytes differ
between neighbouring blocks, the split-K plan returns the expected cuts on 256 compute units, and every entry of `FP8_MISTAKES` changes the
expected output of the launch it belongs to.

The self-attention sums cases (`SUM_CASES`, every launch of tests/test_exact_attention_sums_gpu.py): the closed form equals the fp64 softmax on
the packed buffers, tie sets score exactly 0 with the losers TIE_GAP below, the stair's step premise holds per kernel family, an fp32 online
softmax returns the expected bits under both offset schedules, and every entry of `SUM_MISTAKES` is seen."""
import math

import pytest
import torch

import exact_util as X
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


# ------------------------------------------------------------------------------------------------------------------------------------
# row kernels, scheduler step, softmaxes
# ------------------------------------------------------------------------------------------------------------------------------------
ROW_DS = (8, 264, 520, 5112, 5120)


def _scrambled_sum(t32: torch.Tensor, gen) -> torch.Tensor:
    """Row sums of fp32 [M, D] taken sequentially in a random order (another association than torch's own reduction)."""
    acc = torch.zeros(t32.shape[0], dtype=torch.float32)
    for j in torch.randperm(t32.shape[1], generator=gen).tolist():
        acc = acc + t32[:, j]
    return acc


def _each_row_differs(a: torch.Tensor, b: torch.Tensor, rows=None) -> bool:
    d = (a.float() != b.float()).flatten(1).any(1)
    return bool(d.all() if rows is None else d[rows].all())


@pytest.mark.parametrize("D", ROW_DS)
def test_unit_rows_statistics_are_exact_in_fp32_in_any_order(D):
    g = torch.Generator().manual_seed(D)
    M = 5
    x, v = X.unit_rows(M, D, g)
    xf = x.float()
    s = _scrambled_sum(xf, g)
    mean = s / float(D)
    mu64 = x.double().mean(1)
    assert torch.equal(mean.double(), mu64)
    d = xf - mean[:, None]
    var = _scrambled_sum(d * d, g) / float(D)
    assert torch.equal(var.double(), ((x.double() - mu64[:, None]) ** 2).sum(1) / D)
    rstd = 1.0 / torch.sqrt(var)
    assert torch.equal((d * rstd[:, None]).double(), v)  # the normalised values are 0, +-1, +-2 again
    xc, vc = X.unit_rows(M, D, g, centred=True)          # the RMS form: mean(x^2) = s^2
    ms = _scrambled_sum(xc.float() ** 2, g) / float(D)
    assert torch.equal((xc.float() * (1.0 / torch.sqrt(ms))[:, None]).double(), vc)


@pytest.mark.parametrize("D", ROW_DS)
def test_ln_affine_recipe_is_exact_rounds_and_sees_a_wrong_sample(D):
    g = torch.Generator().manual_seed(100 + D)
    M, ab_rows = 6, 2
    _, v = X.unit_rows(M, D, g)
    a, b = X.affine_vectors(3, D, g)
    want64 = X.ln_affine_exact(v, a, b, ab_rows)
    idx = X.sample_of(M, ab_rows)
    f32 = torch.addcmul(b[idx], v.float(), a[idx])  # (one fused rounding) ...
    assert torch.equal(f32.double(), want64)
    assert torch.equal((v.float() * a[idx] + b[idx]).double(), want64)  # ... or two: no difference
    want = bf16_rne(want64)
    assert (want.double() != want64).double().mean().item() >= 0.25  # the final bf16 rounding is exercised
    # (a, b) of sample 0 for all samples: every row of samples 1 and 2 changes
    wrong = bf16_rne(X.ln_affine_exact(v, a, b, sample=torch.zeros(M, dtype=torch.int64)))
    assert _each_row_differs(want, wrong, rows=torch.arange(ab_rows, M))
    # b from the neighbouring column: every row changes
    assert _each_row_differs(want, bf16_rne(X.ln_affine_exact(v, a, b.roll(1, 1), ab_rows)))


@pytest.mark.parametrize("D,hd", [(512, 128), (520, 40), (480, 96), (5120, 128), (5120, 40)])
def test_rms_rope_recipe_is_exact_and_sees_a_wrong_table_row_or_pair(D, hd):
    g = torch.Generator().manual_seed(200 + D + hd)
    R, M = 3, 9
    _, v = X.unit_rows(M, D, g, centred=True)
    w = X.rms_weights(D, g)
    cs = X.rope_table(R, hd, g)
    want = X.rms_rope_exact(v, w, cs, hd)  # (bf16_rne inside asserts that the fp64 rotation is exact in fp32)
    # the same in fp32, both association orders of the two products
    t = (v.float() * w).to(BF).float()
    rows, pair = torch.arange(M) % R, torch.arange(D // 2) % (hd // 2)
    co, si = cs[rows][:, pair, 0], cs[rows][:, pair, 1]
    r0 = torch.addcmul(-(t[:, 1::2] * si), t[:, 0::2], co)
    r1 = t[:, 1::2] * co + t[:, 0::2] * si
    assert torch.equal(r0.to(BF), want[:, 0::2]) and torch.equal(r1.to(BF), want[:, 1::2])
    plain = X.rms_rope_exact(v, w)
    assert (plain.double() != X.round_bf16_f64(v) * w.double()).double().mean().item() >= 0.25
    # the table row m in place of m % R (a table that goes on with other rows past R): every row m >= R changes
    ext = torch.cat([cs, X.rope_table(M - R, hd, g)])
    assert _each_row_differs(want, X.rms_rope_exact(v, w, ext, hd, table_row=torch.arange(M)), rows=torch.arange(R, M))
    # the neighbouring pair's cos / sin: every row changes
    assert _each_row_differs(want, X.rms_rope_exact(v, w, cs, hd, pair_shift=1))
    # the other tensor's weights (the x2 / w2 launch)
    assert _each_row_differs(plain, X.rms_rope_exact(v, X.rms_weights(D, g)))


@pytest.mark.parametrize("K", [64, 1000, 16384])
def test_gemv_recipe_is_exact_and_sees_bias_zero_for_all_rows(K):
    g = torch.Generator().manual_seed(300 + K)
    N = 17
    w = int_rows(N, K, g, lo=-2, hi=2, emin=0, emax=0)
    x = X.dyadic((K,), g, -2, 2, 0)
    bias = X.gemv_bias(N, g)
    want64 = linear_f64(w, x[None, :], None)[:, 0] + bias.double()
    prod = w.float() * x[None, :]
    assert torch.equal((_scrambled_sum(prod, g) + bias).double(), want64)
    assert bias.unique().numel() == N and want64.abs().max().item() < 2048
    wrong = want64 - bias.double() + bias.double()[0]
    assert bool((wrong[1:] != want64[1:]).all())
    assert bool((bf16_rne(want64)[1:] != bf16_rne(wrong)[1:]).all())  # still seen after the flag-4 rounding


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("cfg", [True, False])
def test_unipc_recipe_is_exact_rounds_and_sees_the_wrong_history_shift(flags, cfg):
    g = torch.Generator().manual_seed(400 + flags)
    n = 4096
    vc, vu, x, xl, m0, m1 = X.unipc_state(n, g)
    vu = vu if cfg else None
    (xn, xc, m0n, m1n, x0), rounded = X.unipc_exact(vc, vu, x, xl, m0, m1, flags=flags)  # (asserts exactness of every fp32 value inside)
    if flags & 2:
        assert rounded >= 0.25, rounded
    assert torch.equal(m1n, m0) and torch.equal(m0n, x0)
    # the same in fp32, FMA-contracted like the device compiler may: no difference
    if not flags & 2 and cfg:
        c = X.UNIPC_COEF
        u = vu.float()
        v = (u + (c[0] * (vc.float() - u).to(BF).float()).to(BF).float()).to(BF).float()
        x0f = torch.addcmul(x, torch.full_like(x, -c[1]), v)
        xcf = torch.addcmul(torch.addcmul(torch.addcmul(c[3] * xl, torch.full_like(x, c[4]), m0), torch.full_like(x, c[5]), m1), torch.full_like(x, c[6]), x0f)
        xnf = c[9] * m0 + (c[8] * x0f + c[7] * xcf)
        assert torch.equal(x0f, x0) and torch.equal(xcf, xc) and torch.equal(xnf, xn)
    # a second step on the new state stays exact, and m1 <- NEW m0 differs from the contract's m1 <- old m0 in (nearly) every element
    vc2, vu2 = X.unipc_state(n, g)[:2]
    (_, _, m0b, m1b, _), _ = X.unipc_exact(vc2, vu2 if cfg else None, xn, xc, m0n, m1n, flags=flags)
    (_, _, _, m1w, _), _ = X.unipc_exact(vc2, vu2 if cfg else None, xn, xc, m0n, m1n, flags=flags, m1_from_new=True)
    assert torch.equal(m1b, m0n) and (m1w != m1b).float().mean() > 0.9
    assert (m1n != m0n).float().mean() > 0.9  # distinct values: the shift is visible


@pytest.mark.parametrize("Lq,Lk", [(5, 5), (7, 100), (64, 65), (3, 1024)])
def test_softmax_tie_recipe_is_exact_and_sees_a_wrong_head_or_an_ignored_mask(Lq, Lk):
    g = torch.Generator().manual_seed(500 + Lk)
    batch, heads = 2, 3
    rows = batch * heads * Lq
    valid_b = torch.tensor([max(Lk // 2, 1), 1 if Lk > 5 else Lk])
    valid = valid_b.repeat_interleave(heads * Lq)
    target = X.tie_targets(rows, Lk, valid, g)
    table, lut = X.t5_bias(heads, Lq, Lk, g)
    bias = X.t5_bias_rows(table, lut, batch, heads, Lq, Lk)
    scores = (target.double() - bias).float()
    assert torch.equal(scores.double(), target.double() - bias)
    total32 = scores + bias.float()
    assert torch.equal(total32.double(), target.double())
    want = X.tie_probs(target.double(), valid)
    # fp32 softmax in a scrambled order gives exactly 2^-k on the tied keys and 0 elsewhere
    mask = torch.arange(Lk)[None, :] < valid[:, None]
    e = torch.where(mask, torch.exp(total32 - total32.masked_fill(~mask, -1e30).amax(1, keepdim=True)), torch.zeros(()))
    assert torch.equal((e / _scrambled_sum(e, g)[:, None]).double(), want)
    assert want.sum(1).eq(1).all() and (want.amax(1) < 1).any()
    # head 0's bias column for every head: every row of heads 1.. changes
    h_of = (torch.arange(rows) // Lq) % heads
    wrong = X.tie_probs(scores.double() + X.t5_bias_rows(table, lut, batch, heads, Lq, Lk, head=0), valid, check=False)
    assert _each_row_differs(want, wrong, rows=((h_of > 0) & (valid > 1)).nonzero()[:, 0])
    # the offset k - q wrong by one (with the 9 buckets of the 5 x 5 case two tied keys may move by the same amount: not asserted there)
    wrong = X.tie_probs(scores.double() + X.t5_bias_rows(table, lut.roll(1), batch, heads, Lq, Lk), valid, check=False)
    if Lk > 5:
        assert _each_row_differs(want, wrong, rows=(valid > 1).nonzero()[:, 0])
    # valid_len ignored: every row with a masked key changes (the masked keys win); one key too tight: the tie count changes
    wrong = X.tie_probs(target.double(), torch.full_like(valid, Lk), check=False)
    assert _each_row_differs(want, wrong, rows=(valid < Lk).nonzero()[:, 0])
    wrong = X.tie_probs(target.double(), valid - 1, check=False)
    assert _each_row_differs(want, wrong)


# ------------------------------------------------------------------------------------------------------------------------------------
# cross-attention: two segments, shared operands, a cut per sample and a weighted last key
# ------------------------------------------------------------------------------------------------------------------------------------
_n_flat = X.n_flat_rows


def _rows_differ(a, b, B):
    """[B, n_q] bool: the rows where two [B n_q, D] tensors differ."""
    return (a != b).any(1).view(B, -1)


def _proved(c, samples=None):
    """The recipe's expectation is the plain fp64 attention of the packed buffers, rounded where the kernels round; margins; exact flat rows."""
    lead, forb, flat = X.cross_margins(c)
    assert min(lead, forb, flat) >= MIN_MARGIN_NATS, (lead, forb, flat)
    assert c.flat_exact
    assert_exact(X.cross_attention_f64(c), c.want, "fp64 reference against the recipe's expectation")
    return c


# (len1, valid per sample, m per sample): every (valid, m) pair of the flat recipe
FLAT_SETS = [(64, (1, 33, 57), (64, 32, 8)), (72, (63, 64, 65), (2, 1, 64)), (200, (97, 127, 193), (32, 2, 64)),
             (2056, (257, 449, 2049), (256, 64, 2048))]
CUT_SETS = [(72, (1, 63, 64), (9.0, 5.5, 0.0)), (136, (65, 129, 70), (9.0, 0.0, 3.25)), (200, (200, 1, 199), (0.0, 9.0, 7.0))]


@pytest.mark.parametrize("n_q,L1,L2,H,B", [(300, 100, 65, 3, 3), (513, 257, 64, 2, 1), (290, 512, 257, 8, 2)])
def test_cross_needles_equal_the_fp64_reference(n_q, L1, L2, H, B):
    c = _proved(X.cross_case(n_q, L1, L2, H, B, seed=n_q + L1 + L2))
    assert (c.c1, c.c2) == ((L1 + 7) // 8 * 8, (L2 + 7) // 8 * 8) and c.v1t.shape[1] == (B - 1) * c.c1 + X.pad64(L1)
    for b in range(B):  # the rows edge_keys(len), len - 1 and len - 2 are winners of the first and the last query rows, in every head
        must = {r for r in [L1 - 1, L1 - 2] + X.edge_keys(L1) if 0 <= r < L1}
        assert must <= set(c.win1[b, :80, 0].tolist()) and must <= set(c.win1[b, -80:, H - 1].tolist())
    assert not torch.equal(c.k1[:L1, :10], c.k1[L1:2 * L1, :10]) or B == 1  # another row order per sample


def test_cross_needles_margins_at_the_largest_shape():
    c = X.cross_case(7200, 512, 257, 2, 2, seed=7200 + 512 + 257)
    lead, forb, _ = X.cross_margins(c)
    assert min(lead, forb) >= MIN_MARGIN_NATS


@pytest.mark.parametrize("share", [(sq, s1, s2) for sq in (False, True) for s1 in (False, True) for s2 in (False, True)])
def test_cross_shared_operands_equal_the_fp64_reference_and_a_stride_in_place_of_zero_is_seen(share):
    n_q, L1, L2, H, B = 300, 100, 65, 2, 3
    sq, s1, s2 = share
    kw = dict(share_q=sq, share1=s1, share2=s2)
    _proved(X.cross_case(n_q, L1, L2, H, B, seed=20 + 4 * sq + 2 * s1 + s2, **kw))
    if sq or s1 or s2:  # the same operands with winner-if-read rows, POISON columns and other queries behind the one sample: read at stride len
        c = X.cross_case(n_q, L1, L2, H, B, seed=20 + 4 * sq + 2 * s1 + s2, extra=2 * 104 + 64, extra_cols=2 * 104, extra_q=2 * n_q, **kw)
        assert_exact(X.cross_attention_f64(c), c.want, "fp64 reference, roomy buffers")
        d = _rows_differ(X.cross_attention_f64(c, "shared operand at stride len"), c.want, B)
        assert not d[0].any() and d[1].all() and d[2].all()


@pytest.mark.parametrize("H", [2, 5])
@pytest.mark.parametrize("len1,valid,m", FLAT_SETS)
def test_cross_flat_rows_are_exact_and_see_every_wrong_weight_or_cut(len1, valid, m, H):
    n_q, L2, B = 300, 65, 3
    nf = _n_flat(n_q)
    c = _proved(X.cross_case(n_q, len1, L2, H, B, seed=len1 + H, valid=valid, m=m, n_flat=nf))
    assert 0 < nf < n_q % 256  # the partial last query block holds needle rows and flat rows
    flat = c.want.view(B, n_q, -1)[:, n_q - nf:]
    assert torch.equal(flat.float().to(BF), flat) and bool(((flat.double() * 8) % 1 == 0).all())  # multiples of 1/8, exact in bf16
    for b in range(B):  # the flat recipe on its own: three significant bits per column
        v1, out1, key = X.flat_v1(len1, valid[b], m[b], H * 128, torch.Generator().manual_seed(b))
        assert torch.equal(out1.to(BF).double(), out1) and bool((out1.abs() * 8 / torch.where(X.flat_wcols(H * 128), float(m[b]), 1.0) <= 7).all())
        assert torch.equal(v1[:valid[b]].to(BF).double(), v1[:valid[b]]) and bool(((v1[:valid[b]] != 0).sum(0) == (key >= 0)).all())
        assert {valid[b] - 1} | ({valid[b] - 2, 0} if valid[b] > 2 else set()) <= set(key.tolist())
    is_flat = torch.arange(n_q) >= n_q - nf
    d = _rows_differ(X.cross_attention_f64(c, "weight ignored"), c.want, B)
    for b in range(B):
        assert not d[b, ~is_flat].any()  # a needle row never depends on the weight
        seen = m[b] > 1 and valid[b] > 1  # (a key that is the only one has the whole softmax, whatever its weight)
        assert d[b, is_flat].all() == seen and d[b, is_flat].any() == seen
    d = _rows_differ(X.cross_attention_f64(c, "weight on key valid-2"), c.want, B)
    for b in range(B):
        assert d[b, is_flat].all() == (m[b] > 1 and valid[b] > 1)
    d = _rows_differ(X.cross_attention_f64(c, "w[0] for all samples"), c.want, B)
    for b in range(B):
        assert d[b, is_flat].all() == (m[b] != m[0] and valid[b] > 1)
    d = _rows_differ(X.cross_attention_f64(c, "valid[0] for all samples"), c.want, B)
    for b in range(B):
        assert d[b].any() == (valid[b] != valid[0]) and (valid[b] >= valid[0] or d[b].all())  # (a cut too late: a garbage key wins every row)
    for mistake in ("tail mask at valid+1", "tail mask at len1"):
        d = _rows_differ(X.cross_attention_f64(c, mistake), c.want, B)
        for b in range(B):
            assert d[b].all() or (mistake == "tail mask at len1" and valid[b] == len1)
    d = _rows_differ(X.cross_attention_f64(c, "neighbour's K1 rows"), c.want, B)
    assert all(d[b].any() or valid[b] == 1 for b in range(B))


@pytest.mark.parametrize("len1,valid,w", CUT_SETS)
def test_cross_cut_needles_equal_the_fp64_reference_and_see_every_wrong_cut_or_stride(len1, valid, w):
    n_q, L2, H, B = 300, 257, 2, 3
    c = _proved(X.cross_case(n_q, len1, L2, H, B, seed=len1, valid=valid, w=w, extra_cols=64))
    for b in range(B):  # winners from [0, valid[b]), key valid[b] - 1 (the weighted one) among them; the rows behind the cut win if read
        assert int(c.win1[b].max()) == valid[b] - 1
        assert bool((c.v1t[:, b * c.c1 + valid[b]:b * c.c1 + len1] == X.POISON).all())
        assert bool((c.k1[b * len1 + valid[b]:(b + 1) * len1, X.INVALID_DIM] == 1).all())
    for mistake in ("weight ignored", "weight on key valid-2", "w[0] for all samples"):  # needle rows: the weight decides nothing
        assert_exact(X.cross_attention_f64(c, mistake), c.want, mistake)
    d = _rows_differ(X.cross_attention_f64(c, "valid[0] for all samples"), c.want, B)
    for b in range(B):
        assert d[b].any() == (valid[b] != valid[0])
    for mistake in ("tail mask at valid+1", "tail mask at len1"):
        d = _rows_differ(X.cross_attention_f64(c, mistake), c.want, B)
        for b in range(B):
            assert d[b].all() or (mistake == "tail mask at len1" and valid[b] == len1)
    d = _rows_differ(X.cross_attention_f64(c, "neighbour's K1 rows"), c.want, B)
    assert all(d[b].any() or valid[b] == 1 for b in range(B))  # (one key: it wins wherever it is read from)
    d = _rows_differ(X.cross_attention_f64(c, "V^T column stride 64 ceil(len/64)"), c.want, B)
    assert not d[0].any() and d[1].all() and d[2].all()


@pytest.mark.parametrize("n_q,H,B", [(300, 40, 7), (2600, 5, 10)])
def test_cross_margins_of_the_many_item_shapes(n_q, H, B):
    """The construction of tests/test_exact_cross_attention_gpu.py's largest launches (the weighted one: ten different (valid, m) pairs)."""
    MANY_PAIRS = X.MANY_PAIRS
    c = X.roomy_cross_case(n_q, 200, 65, H, B, seed=n_q + H + len("weighted"), valid=[p[0] for p in MANY_PAIRS[:B]],
                           m=[p[1] for p in MANY_PAIRS[:B]], n_flat=_n_flat(n_q))
    assert c.flat_exact and min(X.cross_margins(c)) >= MIN_MARGIN_NATS
    assert len(set(MANY_PAIRS)) == len(MANY_PAIRS) == 10 and all(v <= 200 and 2 ** round(math.log2(v - 1 + m)) == v - 1 + m for v, m in MANY_PAIRS)


def test_far_first_tile_recipe_overflows_the_first_rescale_factor():
    """`far_first_tile`: margins as for every needle, the winners past tile 0, and the first tile's best score (log2 domain, after the scale)
    below -128 for every row and head - exp2 of its negative is +inf in fp32, the factor a first-tile rescale would multiply 0 by."""
    g = torch.Generator().manual_seed(77)
    q, k, v, rows = X.far_first_tile(70, 130, 3, g)
    lead, _ = needle_margins(q, k, 3, rows)
    assert lead.min() >= MIN_MARGIN_NATS and int(rows.min()) >= 64 and len(rows.unique()) > 20
    first = X.needle_scores(q, k[:64], 3).amax(-1) * X.LOG2E
    assert first.max().item() < -128 and torch.isinf(torch.exp2(-first.float())).all()


# ---- MXFP8 attention: the cases of tests/test_exact_attention_mxfp8_gpu.py, every one of them ---------------------------------------------
MX_NAMES = list(X.MX_CASES)
LN2 = math.log(2.0)


def _mx_heads(t, B, n, H):
    """[>= B n, H 128] fp64 rows -> fp32 [B, H, n, 128], exactly."""
    return X.exact_f64(t[:B * n]).view(B, n, H, 128).permute(0, 2, 1, 3)


@pytest.mark.parametrize("name", MX_NAMES)
def test_mx_case_bytes_hold_the_intended_values_and_the_contract_keeps_them(name):
    """The bytes and scale bytes of q, k and V^T de-quantise to the recipe's values (V^T through the key order and the sv layout that
    test_mxfp8_v_transpose_matches_contract states); `mx_quant` of those values returns them unchanged; block scales take all three
    offsets from the canonical one; gap columns, spare blocks and the zero padding of V^T are in place."""
    from oracle import dit_oracle as O
    c = X.mx_named_case(name)
    B, H, D, nkv, npad = c.B, c.H, c.D, c.n_kv, c.npad
    for b8, s8, val, ld in ((c.q8, c.sq, c.q, c.ldq8), (c.k8, c.sk, c.k, c.ldk8)):
        assert b8.shape[1] == ld > D and ld % 16 == 0 and bool((b8[:, D:] == X.MX_GAP_BYTE).all())
        assert torch.equal(X.mx_unpack(b8[:, :D], s8), val)
        assert torch.equal(O.mx_quant(X.exact_f64(val), -1).double(), val)
        canon = torch.floor(torch.log2(val.view(val.shape[0], -1, 32).abs().amax(-1))) - 8 + 127
        assert set((s8.double() - canon).unique().tolist()) == {0.0, 1.0, 2.0}
    pos = torch.arange(npad)
    key = pos // 64 * 64 + 32 * ((pos % 32) >> 4) + (pos % 32 & 3) + 8 * (((pos % 32) & 15) >> 2) + 4 * (pos % 64 // 32)  # key stored at position pos
    vt = torch.zeros(B, H, 128, npad, dtype=torch.float64)
    vt[..., key] = X.E4M3_LUT[c.v8t[:B].long()]
    svk = c.sv[:B].permute(0, 1, 3, 2, 4).reshape(B, H, 128, npad // 32)
    vt = vt * torch.exp2(svk.double() - 127.0).repeat_interleave(32, dim=-1)
    vp = torch.zeros(B, H, npad, 128, dtype=torch.float64)
    vp[:, :, :nkv] = c.v.view(B, nkv, H, 128).permute(0, 2, 1, 3)
    assert torch.equal(vt, vp.permute(0, 1, 3, 2))
    assert torch.equal(O.mx_quant(X.exact_f64(vp), 2).double(), vp)
    assert not X.E4M3_LUT[c.v8t[:B].long()][..., key >= nkv].any(), "V^T padding columns are not zero"
    assert bool((c.v8t[B:] == X.MX_GAP_BYTE).all()) and c.v.abs().min() >= 4.0
    assert c.q8.shape[0] >= B * c.n_q + 256 * B and c.k8.shape[0] >= B * nkv + 64 * B + 64  # roomy: a stride of 256 nqb or npad stays inside
    assert len(torch.unique(c.v.view(B * nkv, D), dim=0)) == B * nkv                       # no two keys share a V row
    if nkv > 32:
        e = svk.double()
        assert (e[..., 0] != e[..., 1]).double().mean() > 0.5 and (e[:, 0] != e[:, 1]).double().mean() > 0.5  # beta / head neighbours differ


@pytest.mark.parametrize("name", MX_NAMES)
def test_mx_case_margins_winners_and_ties(name):
    """Every winner scores exactly 0 and leads by >= 22 nats; every row nobody may read would win by as much; every tie set scores exactly 0 with
    the rest of the sample 128 octaves behind; winners cover the edge keys and differ per head; the modes are what they say."""
    c = X.mx_named_case(name)
    lead, forb, gap = X.mx_margins(c)
    assert min(lead, forb, gap) * LN2 >= MIN_MARGIN_NATS, (lead, forb, gap)
    assert min(lead, gap) >= 64.0  # exp2(-64 + 3) rounds to 0 in e4m3 (half the smallest subnormal is 2^-10) and is far below an fp32 ulp of l
    w = c.win
    if c.mode == "perm":
        must = [k for k in edge_keys(c.n_kv) if k < c.n_kv]
        for b in range(c.B):
            for h in range(c.H):
                if len(must) <= c.n_needle:
                    assert set(must) <= set(w[b, :, h].tolist()), (b, h)
                tail = set(w[b, -min(len(must), c.n_needle):, h].tolist())
                assert tail <= set(must)
        if c.n_kv > 8:
            assert not torch.equal(w[:, :, 0], w[:, :, 1])
        assert c.n_tie > 0 and all(c.n_kv - 1 in t.tolist() for s in c.tie_sets for hs in s for t in hs)
        assert [len(t) for t in c.tie_sets[0][0]] == [min(2 ** k, 2 ** (c.n_kv.bit_length() - 1)) for k in (1, 2, 3)]
        if c.n_q % 256 > c.n_tie:  # the partial last query block holds needle rows and tie rows
            assert c.n_q // 256 * 256 < c.n_needle < c.n_q
    elif c.mode == "tile0":
        assert int(w.max()) < 64 and c.n_tie == 0 and c.n_kv > 64
    elif c.mode == "mixed":
        grp = w[:, :c.n_needle // 32 * 32].reshape(c.B, -1, 32, c.H)
        assert bool(((grp < 64).any(2) & (grp >= 64).any(2)).all())
    elif c.mode == "far":
        assert int(w.min()) >= 64
        s0 = torch.einsum("qhd,khd->hqk", c.q[:c.n_q].view(c.n_q, c.H, 128), c.k[:64].view(64, c.H, 128))
        assert s0[:, :c.n_needle].max().item() <= -2304.0


@pytest.mark.parametrize("name", MX_NAMES)
def test_mx_contract_oracle_returns_the_closed_form_under_both_offset_schedules(name):
    """oracle.dit_oracle.attention_mxfp8's loop on the de-quantised operands (`attention_mxfp8_quantised`: no constant multiplied into q) gives
    exactly the expected rows, with the lazy integer offset of the default kernel and with the running maximum of the plain loop."""
    from oracle import dit_oracle as O
    c = X.mx_named_case(name)
    B, H = c.B, c.H
    qq, kq, vq = _mx_heads(c.q, B, c.n_q, H), _mx_heads(c.k, B, c.n_kv, H), _mx_heads(c.v.view(B * c.n_kv, c.D), B, c.n_kv, H)
    for lazy in (True, False):
        o = O.attention_mxfp8_quantised(qq, kq, vq, lazy_offset=lazy).permute(0, 2, 1, 3).reshape(B * c.n_q, c.D)
        assert_exact(o.to(BF), c.want, f"{name}: contract oracle, lazy_offset={lazy}")


def test_mx_oracle_factoring_keeps_what_its_callers_get():
    """`attention_mxfp8` is its quantisation front plus `attention_mxfp8_quantised`, in the input's dtype."""
    from oracle import dit_oracle as O
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(1, 2, 70, 128, generator=g).to(BF) for _ in range(3))
    for lazy in (True, False):
        got = O.attention_mxfp8(q, k, v, lazy_offset=lazy)
        want = O.attention_mxfp8_quantised(O.mx_quant(q.float() * (128 ** -0.5 * 1.4426950408889634), -1), O.mx_quant(k, -1), O.mx_quant(v, 2), lazy)
        assert got.dtype == BF and torch.equal(got, want.to(BF)) and want.dtype == torch.float32


@pytest.mark.parametrize("name", MX_NAMES)
def test_mx_f64_reference_equals_the_closed_form_and_sees_every_mistake_that_applies(name):
    """`mxfp8_attention_f64` on the packed buffers, item by item in the kernel's work order, equals the expectation (plain and with `add`); with
    any one entry of MX_MISTAKES that the shape can show, it does not."""
    c = X.mx_named_case(name)
    n_q, n_kv, H, B, mode = X.MX_CASES[name][:5]
    cache = {}
    assert_exact(X.mxfp8_attention_f64(c, cache=cache), c.want, name)
    assert_exact(X.mxfp8_attention_f64(c, add=True, cache=cache), c.want_add, name + " add")
    for m in X.MX_MISTAKES:
        if X.mx_mistake_applies(m, n_q, n_kv, H, B, mode, c.ldq8 - c.D, c.ldk8 - c.D):
            is_add = m == "neighbour sample's add rows"
            wrong = X.mxfp8_attention_f64(c, mistake=m, add=is_add, cache=cache)
            bad = X.mismatches(wrong, c.want_add if is_add else c.want)
            assert bad.any(), f"{name}: the data cannot see '{m}'"
            if m in ("neighbour head's sq dword", "neighbour head's sk dword"):
                assert bad.any(1).double().mean() > 0.5, (m, bad.any(1).double().mean())  # most rows, not a lucky one


def test_every_mx_mistake_is_seen_by_some_case():
    seen = {m for m in X.MX_MISTAKES for (n_q, n_kv, H, B, mode, _) in X.MX_CASES.values() if X.mx_mistake_applies(m, n_q, n_kv, H, B, mode)}
    assert seen == set(X.MX_MISTAKES), set(X.MX_MISTAKES) - seen
    nq, nkv, H, B = X.MX_CASES["q257-k70-h16-b17"][:4]
    assert len(X.mx_work_items(nq, H, B)) == (nq + 255) // 256 * H * B > 512
    for (n_q, n_kv, H, B, _, _) in X.MX_CASES.values():  # the work order itself: every (sample, head, block) exactly once
        items = X.mx_work_items(n_q, H, B)
        assert sorted(items) == sorted((b, h, q) for b in range(B) for h in range(H) for q in range((n_q + 255) // 256))


@pytest.mark.parametrize("name", MX_NAMES)
def test_mx_add_and_quant_expectations(name):
    """_add: bf16(bf16(o) + add) needs a real rounding on part of the elements and never comes near zero; _quant: the contract's bytes of the
    expected bf16 rows hold the needle rows exactly (four significant bits, one block of 32 channels spans 2^-1 .. 2^2)."""
    c = X.mx_named_case(name)
    exact = c.want.double() + c.add.double()
    rounded = (c.want_add.double() != exact).double().mean().item()
    assert 0.02 < rounded < 0.9 and c.want_add.float().abs().min() >= 32.0, (rounded, c.want_add.float().abs().min())
    s, q = _contract(c.want)
    needle = torch.arange(c.B * c.n_q) % c.n_q < c.n_needle
    assert torch.equal(_deq(q, s)[needle], c.want.float()[needle])
    s2, q2 = _contract(c.want_add)
    assert (_deq(q2, s2) - c.want_add.float()).abs().max() <= 8.0 and not torch.equal(q, q2)


# ------------------------------------------------------------------------------------------------------------------------------------
# The fp8 mode's operand producers and GEMM tails (tests/test_exact_fp8_producers_gpu.py): the premise of every recipe, and every entry of
# X.FP8_MISTAKES seen by the reference on the data that is launched.
# ------------------------------------------------------------------------------------------------------------------------------------
FP8_ROW_KS = (5120, 13824, 264, 8)
FP8_ROW_MS = (1, 7, 129)


def test_row_fp8_restatement_is_exact_on_power_of_two_rows():
    """448 2^e * float32(1 / 448) == 2^e for e in -6..6; on tier A rows the restatement returns 2^e, the bytes the row was built from, and they
    dequantise to the input.  On ordinary rows the division form amax / 448 is another function: most scales differ in the last bit."""
    e = torch.arange(-6, 7).float()
    assert torch.equal(torch.mul(448.0 * torch.exp2(e), X.F32_INV_448), torch.exp2(e))
    assert X.F32_INV_448.view(torch.int32).item() == 0x3B124925
    for K in FP8_ROW_KS:
        for M in FP8_ROW_MS:
            x, b, ex = X.fp8_pow2_rows(M, K, torch.Generator().manual_seed(5000 + K + M))
            s, q = X.row_fp8_ref(x)
            assert torch.equal(s, torch.exp2(ex.float())) and torch.equal(q, b)
            assert torch.equal(X.E4M3_LUT[q.long()] * s.double()[:, None], x.double())
            assert bool((b[:, 0] == 0x80).all()) and bool((x[:, 0].float() == 0).all()) and bool(torch.signbit(x[:, 0].float()).all())
    x = X.fp8_random_rows(129, 5120, torch.Generator().manual_seed(5100 + 5120 + 129))
    s, q = X.row_fp8_ref(x)
    amax = x.float().abs().amax(1)
    assert amax[128] == 0 and s[128] == 1 and not q[128].any()                         # the all-zero row
    assert x[0, :-8].float().abs().max() < x[0, -8:].float().abs().max() == 40.0       # the maximum in the last chunk only
    s_div = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert (s_div != s).double().mean() > 0.25
    q_div = (x.float() / s_div[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert (q_div != q).any()                                                            # ... and some bytes with them


def test_mx_contract_restatement_equals_the_contracts_in_use_and_the_tiled_order_inverts():
    """`mx_contract` == the tests' `_contract` (non-saturating) and dequantises to oracle.dit_oracle.mx_quant (both rules) on launched data;
    `mx_scales_tiled` is the inverse of ops.mx_scales_to_rows in both scale orders, sentinel rows included."""
    from chronoedit_amd import ops
    from oracle import dit_oracle as O
    c = X.ln_mx_case(640)
    r = X.rms_mx_case(384, 96, 3, ops.MXFP8_Q_SCALE)
    for x in (c.y, mx_operand(40, 512, torch.Generator().manual_seed(3))):
        s, q = X.mx_contract(x)
        s0, q0 = _contract(x)
        assert torch.equal(s, s0) and torch.equal(q, q0)
        assert torch.equal(_deq(q, s), O.mx_quant(x.float(), -1, saturating=False))
    xr = torch.mul(r.t.float(), torch.tensor(ops.MXFP8_Q_SCALE, dtype=torch.float32))
    s, q = X.mx_contract(xr, saturating=True)
    assert torch.equal(_deq(q, s), O.mx_quant(xr, -1)) and torch.equal(s, r.want_rows)
    assert not torch.equal(X.mx_contract(xr, saturating=False)[0], s)                    # (this data tells the two scale rules apart)
    for w_order in (False, True):
        t = X.mx_scales_tiled(c.want_rows, w_order=w_order)
        assert t.numel() == ops.mx_scale_bytes(c.M, c.D)
        rows = ops.mx_scales_to_rows(t, 256, c.D, w_order=w_order)
        assert torch.equal(rows[:c.M], c.want_rows) and bool((rows[c.M:] == X.SCALE_SENTINEL).all())


def _real_rounding_share(y_bf16, exact64):
    return (y_bf16.double() != exact64).double().mean().item()


@pytest.mark.parametrize("D", X.LN_FP8_DS)
def test_ln_fp8_case_is_exact_rounds_and_sees_the_wrong_sample(D):
    c = X.ln_fp8_case(D)
    exact = X.ln_affine_exact(c.v, c.a, c.b, c.ab_rows)
    f32 = c.v.float() * c.a[X.sample_of(c.M, c.ab_rows)] + c.b[X.sample_of(c.M, c.ab_rows)]
    assert torch.equal(f32.double(), exact) and _real_rounding_share(c.y, exact) >= 0.25
    assert c.ab_rows % 4 != 0 and c.M % 4 != 0
    wrong = X.ln_fp8_case(D, "affine row of the wrong sample")
    moved = torch.arange(c.M) % c.ab_rows == c.ab_rows - 1
    assert _each_row_differs(wrong.want_q, c.want_q, moved) and not torch.equal(wrong.want_s[moved], c.want_s[moved])
    assert torch.equal(wrong.want_q[~moved], c.want_q[~moved])


@pytest.mark.parametrize("D", X.LN_MX_DS)
def test_ln_mx_case_is_exact_has_diverse_scales_and_sees_every_mistake(D):
    c = X.ln_mx_case(D)
    exact = X.ln_affine_exact(c.v, c.a, c.b, c.ab_rows)
    idx = X.sample_of(c.M, c.ab_rows)
    assert torch.equal((c.v.float() * c.a[idx] + c.b[idx]).double(), exact) and _real_rounding_share(c.y, exact) >= 0.25
    assert X.scale_diversity(c.want_rows) >= 0.5, X.scale_diversity(c.want_rows)
    zero = c.want_rows == 1
    assert zero.any() and not c.want_q.view(c.M, -1, 32)[zero].any()                    # zero blocks: scale byte 1, zero bytes
    assert int(c.want_rows.max()) - int(c.want_rows[~zero].min()) >= 10                 # octaves apart along a row
    assert c.M % 128 == 2 and c.ab_rows % 4 != 0 and not bool((c.want_rows == X.SCALE_SENTINEL).any())
    wrong = X.ln_mx_case(D, "affine row of the wrong sample")
    moved = torch.arange(c.M) % c.ab_rows == c.ab_rows - 1
    assert _each_row_differs(wrong.want_rows, c.want_rows, moved) and _each_row_differs(wrong.want_q, c.want_q, moved)
    wrong = X.ln_mx_case(D, "scale byte of the neighbouring block")
    assert (wrong.want_rows != c.want_rows).double().mean() >= 0.5 and _each_row_differs(wrong.want_s.view(-1, 512), c.want_s.view(-1, 512))
    wrong = X.ln_mx_case(D, "W-order scale layout")
    assert torch.equal(wrong.want_rows, c.want_rows) and (wrong.want_s != c.want_s).double().mean() >= 0.25


@pytest.mark.parametrize("R", [X.RMS_MX_M, 3, None])
@pytest.mark.parametrize("D,hd", X.RMS_MX_SHAPES)
def test_rms_mx_case_is_exact_and_sees_an_ignored_post_scale_or_a_wrong_table_row(D, hd, R):
    from chronoedit_amd import ops
    for ps in (ops.MXFP8_Q_SCALE, 1.0):
        c = X.rms_mx_case(D, hd, R, ps)
        assert torch.equal(c.x.double(), c.v * (c.x.double().abs().amax(1, keepdim=True) / c.v.abs().amax(1, keepdim=True)))  # x = s v, centred
        assert c.M % 4 != 0 and (R is None or c.M % R == 0)
        if ps != 1.0:
            wrong = X.rms_mx_case(D, hd, R, ps, "post_scale ignored")
            assert (wrong.want_rows != c.want_rows).double().mean() > 0.9 and _each_row_differs(wrong.want_q, c.want_q)
            one = X.rms_mx_case(D, hd, R, 1.0)
            assert torch.equal(wrong.want_rows, one.want_rows) and torch.equal(wrong.want_q, one.want_q)
        if R == 3:
            wrong = X.rms_mx_case(D, hd, R, ps, "RoPE table row m")
            assert torch.equal(wrong.want_q[:R], c.want_q[:R]) and _each_row_differs(wrong.want_q, c.want_q, torch.arange(c.M) >= R)


def _gelu_tanh_f32(x):
    """ce_common.h gelu_tanh in torch fp32, operation by operation (the reciprocal as a correctly rounded division)."""
    c1 = torch.tensor(-2.0 * 1.4426950408889634 * 0.7978845608028654, dtype=torch.float32)
    c2 = torch.mul(c1, torch.tensor(0.044715, dtype=torch.float32))
    e = torch.exp2(x * (c2 * (x * x) + c1))
    return x * (1.0 / (1.0 + e))


def test_saturated_gelu_margins():
    """With the kernel's constants in fp32: 5.0 already returns 5.0 and -10.5 already -0, while -10.0 still returns a denormal-sized negative - the
    set {0} u [6, inf) u (-inf, -12] keeps real margins."""
    y = _gelu_tanh_f32(torch.tensor([5.0, 6.0, 16.0, 1.0e7, -10.5, -12.0, -16.0, -1.0e7, 0.0, -10.0]))
    assert torch.equal(y[:4].to(BF), torch.tensor([5.0, 6.0, 16.0, 1.0e7]).to(BF))
    assert bool((y[4:8] == 0).all()) and bool(torch.signbit(y[4:8]).all()) and y[8] == 0 and not torch.signbit(y[8])
    assert -1e-36 < y[9].item() < 0


def _sat_bytes(x64):
    """(scale rows, bytes) of the FFN-up form for an fp64 acc + bias that a mistaken reference produced (NaN where nothing is written: 0 there;
    torch's fp32 tanh GELU stands in where a mistake left the saturated set - on the set it returns x, -0 or 0 as well)."""
    xb = torch.nan_to_num(x64).float().to(BF)
    return X.mx_contract(torch.nn.functional.gelu(xb.float(), approximate="tanh").to(BF))


@pytest.mark.parametrize("M,N,K", X.SAT_SHAPES)
def test_sat_gemm_case_premises(M, N, K):
    """fp32 holds acc + bias exactly, every GELU input lies in the saturated set, at least half the 32-column blocks are mixed, -0 bytes and the
    scale byte 1 occur, neighbouring blocks differ in scale; the kernel's fp32 GELU returns the closed form on every input.  (The largest shape:
    its first and last 300 rows - the last row of tiles, ragged, is the one the plan cuts.)"""
    c = X.sat_gemm_case(M, N, K)
    rows = torch.arange(M) if M <= 600 else torch.cat([torch.arange(300), torch.arange(M - 300, M)])
    a = c.a[rows]
    for t in (a, c.w):
        s8, q8 = X.mx_contract(t)
        assert torch.equal(X.mx_unpack(q8, s8), t.double())
    f32 = a.float() @ c.w.float().t() + c.bias
    exact = a.double() @ c.w.double().t() + c.bias.double()
    assert torch.equal(f32.double(), exact)
    units = exact / c.unit[rows]
    assert torch.equal(units, units.round()) and units.abs().max().item() < 2 ** 22      # (non-negative terms: the full sum bounds every partial sum)
    x = bf16_rne(exact)
    assert _real_rounding_share(x, exact) > 0.25
    y = X.sat_gelu(x)
    assert torch.equal(_gelu_tanh_f32(x.float()).to(BF).view(torch.int16), y.view(torch.int16))
    assert X.mixed_block_share(y) >= 0.5, X.mixed_block_share(y)
    rows8, q = X.mx_contract(y)
    assert bool((q == 0x80).any()) and bool((rows8 == 1).any()) and X.scale_diversity(rows8) >= 0.5
    assert int(rows8.max()) - int(rows8[rows8 > 1].min()) >= 4 and not bool((rows8 == X.SCALE_SENTINEL).any())
    assert torch.equal(_sat_bytes(exact)[1], q) and torch.equal(_sat_bytes(exact)[0], rows8)


def test_fp8_split_k_plan_restated_on_256_compute_units():
    ws = 256 * 384 * 256 * 4
    want = {(300, 512, 13824): (2, 2, 0, 4, 6), (129, 256, 256): (1, 1, 1, 0, 1), (4352, 4096, 5120): (17, 16, 256, 16, 5),
            (300, 520, 256): (2, 3, 6, 0, 1), (300, 520, 13824): (2, 3, 0, 6, 6), (1000, 1032, 5120): (4, 5, 0, 20, 5),
            (7200, 13824, 5120): (29, 54, 1536, 30, 5)}
    for shape, plan in want.items():
        assert X.fp8_tail_plan(*shape, 256, ws) == plan, (shape, X.fp8_tail_plan(*shape, 256, ws))
    assert X.fp8_tail_plan(300, 512, 13824, 256, 0)[4] == 1                              # no scratch: nothing is cut
    for tm, tn in ((2, 2), (17, 16), (4, 5), (29, 54)):                                  # the raster visits every tile exactly once
        seen = sorted(X.fp8_tile_origin(wg, tm, tn) for wg in range(tm * tn))
        assert seen == sorted((m * 256, n * 256) for m in range(tm) for n in range(tn))


@pytest.mark.parametrize("mistake", ["one slab fewer in the tail sum", "tail raster group 1", "bias of column n+4",
                                     "scale byte of the neighbouring block", "W-order scale layout"])
def test_ffn_up_reference_sees_every_tail_mistake(mistake):
    """300 x 512 x 13824 (four tiles, all tail, cut in six): the tile-by-tile restatement of the launch equals the plain product, and with one slab
    fewer, the reduce kernel's tiles under a raster group of 1, or the bias of column n + 4 it gives other bytes in every tile."""
    M, N, K = X.SAT_SHAPES[0]
    c = X.sat_gemm_case(M, N, K)
    plan = X.fp8_tail_plan(M, N, K, 256, 256 * 384 * 256 * 4)
    exact = c.a.double() @ c.w.double().t() + c.bias.double()
    assert torch.equal(X.fp8_tail_launch_f64(c.a, c.w, c.bias, plan), exact)
    rows8, q = _sat_bytes(exact)
    if mistake == "scale byte of the neighbouring block":
        assert (X.neighbour_block(rows8) != rows8).double().mean() >= 0.5
    elif mistake == "W-order scale layout":
        assert (X.mx_scales_tiled(rows8, w_order=True) != X.mx_scales_tiled(rows8)).double().mean() >= 0.25
    else:
        r2, q2 = _sat_bytes(X.fp8_tail_launch_f64(c.a, c.w, c.bias, plan, mistake))
        moved = [X.fp8_tile_origin(wg, 2, 2) for wg in range(4) if mistake != "tail raster group 1" or X.fp8_tile_origin(wg, 2, 2, group=1) != X.fp8_tile_origin(wg, 2, 2)]
        assert len(moved) >= 2
        for m0, n0 in moved:
            assert (q2[m0:m0 + 256, n0:n0 + 256] != q[m0:m0 + 256, n0:n0 + 256])[:M - m0].double().mean() > 0.05, (mistake, m0, n0)
    if mistake == "tail raster group 1":                                                  # the largest shape cannot see this one: its tail is one row of tiles
        assert all(X.fp8_tile_origin(wg, 17, 16) == X.fp8_tile_origin(wg, 17, 16, group=1) for wg in range(256, 272))
        assert any(X.fp8_tile_origin(wg, 4, 5) != X.fp8_tile_origin(wg, 4, 5, group=1) for wg in range(20))


def test_every_fp8_mistake_has_a_reference_that_sees_it():
    covered = {"scale byte of the neighbouring block", "W-order scale layout", "affine row of the wrong sample"}      # ln_mx_case, ln_fp8_case
    covered |= {"bias of column n+4", "one slab fewer in the tail sum", "tail raster group 1"}                      # fp8_tail_launch_f64
    covered |= {"post_scale ignored", "RoPE table row m"}                                                            # rms_mx_case
    assert covered == set(X.FP8_MISTAKES)


@pytest.mark.parametrize("M,N,K", X.BEND_SHAPES)
def test_bend_gemm_case_is_exact_and_spans_the_bend(M, N, K):
    c = X.bend_gemm_case(M, N, K)
    assert torch.equal(c.a.float(), c.ia * c.sa[:, None]) and torch.equal(c.w.float(), c.iw * c.sw[:, None])
    assert torch.equal(c.ia.to(torch.float8_e4m3fn).float(), c.ia) and torch.equal(c.iw.to(torch.float8_e4m3fn).float(), c.iw)
    for t in (c.a, c.w):
        s8, q8 = X.mx_contract(t)
        assert torch.equal(X.mx_unpack(q8, s8), t.double())
    exact = c.a.double() @ c.w.double().t() + c.bias.double()
    assert torch.equal((c.a.float() @ c.w.float().t() + c.bias).double(), exact)
    x = bf16_rne(exact).float()
    assert x.min().item() > -9.0 and (x.abs() < 4).double().mean().item() >= 0.5 and _real_rounding_share(bf16_rne(exact), exact) > 0.25
    assert x.min().item() < -3.0 and x.max().item() > 3.0                                 # both sides of the bend


# ------------------------------------------------------------------------------------------------------------------------------------
# the VAE's implicit-GEMM conv, RMS_norm (+ SiLU) and the conv with the norm in its epilogue (every launch of tests/test_exact_vae_ops_gpu.py)
# ------------------------------------------------------------------------------------------------------------------------------------
CONV_NAMES = list(X.CONV_CASES)
SEEN_SHARE = 0.01  # every mistake that applies to a launch changes at least this share of its expected output elements (after the bf16 rounding)


def _differing_share(a, b):
    return X.mismatches(a, b, 0).double().mean().item()


@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_case_is_exact_and_sees_every_mistake_that_applies(name):
    """The sums are exact in fp32 (`bf16_rne` asserts it) and need a real rounding; positions the engine's layout does not zero hold data; each
    applicable entry of CONV_MISTAKES moves >= 1 % of the expected elements."""
    c = X.conv_case(name)
    want = X.conv_want(c)
    assert tuple(want.shape) == (c.n_out, c.H_out, c.W_out, c.Cout)
    exact = X.conv_frames_f64([c.in_stack[i] for i in c.in_idx], c.w, c.b, c.n_out, KT=c.KT, KH=c.KH, KW=c.KW, st=c.st, ss=c.ss, H_out=c.H_out,
                              W_out=c.W_out, in_off=c.in_off, cout_slice=c.cout_slice)
    if c.KT * c.KH * c.KW * c.Cin >= 96:
        assert _real_rounding_share(bf16_rne(exact), exact) > 0.05
    rows = (torch.arange(c.H_out) * c.ss + c.in_off)[:, None]
    assert int(rows.max()) + c.KH - 1 < c.in_stack.shape[1] and (c.W_out - 1) * c.ss + c.in_off + c.KW - 1 < c.in_stack.shape[2]  # every read in the frame
    assert (c.n_out - 1) * c.st + c.KT <= len(c.in_idx) <= 16
    live = [i for i in set(c.in_idx) if i not in X.CONV_CASES[name]["zero_frames"]]
    pad = X.CONV_CASES[name]["pad"]
    for i in live:  # what is not padding holds data: at most the share of zeros that integers in -4..4 bring
        f = c.in_stack[i]
        edges = {"top": f[0, 1:-1], "left": f[1:-1, 0], "bottom": f[-1], "right": f[:, -1]}
        for side, e in edges.items():
            zeroed = pad == "all" or (pad == "br" and side in ("bottom", "right"))
            if X.CONV_CASES[name]["in_rows"]:
                continue
            assert bool((e == 0).all()) if zeroed else (e != 0).double().mean().item() > 0.8, (name, i, side)
    mistakes = X.conv_mistakes_for(c)
    for m in mistakes:
        share = _differing_share(X.conv_want(c, m), want)
        assert share >= SEEN_SHARE, (name, m, share)
    for m in set(X.CONV_MISTAKES) - set(mistakes) - {"symmetric pad instead of bottom/right pad", "kh and kw swapped"}:
        assert torch.equal(X.conv_want(c, m), want), (name, m)  # (what does not apply names the same computation)


def test_every_conv_mistake_is_seen_by_some_case_and_the_halves_share_their_operands():
    seen = set()
    for name in CONV_NAMES:
        seen |= set(X.conv_mistakes_for(X.conv_case(name)))
    assert seen == set(X.CONV_MISTAKES)
    lo, hi = X.conv_case("time up lo"), X.conv_case("time up hi")
    assert torch.equal(lo.in_stack, hi.in_stack) and torch.equal(lo.w, hi.w) and torch.equal(lo.b, hi.b) and lo.cout_slice == (0, 96) and hi.cout_slice == (96, 192)
    assert sorted(lo.out_idx + hi.out_idx) == list(range(6))


@pytest.mark.parametrize("name", ["3x3 s2 even KT1", "3x3 s2 odd KT3", "time down T7", "k3 384->24", "1x1 off1 M126"])
def test_conv_frames_f64_equals_the_library_convolution_in_fp64(name):
    """The restated formula against torch's conv3d on the image the network sees: the interior of the stored frames under the reference's padding -
    ZeroPad2d((0, 1, 0, 1)) before the stride-2 conv, one zero pixel all round a stride-1 3 x 3, none for a 1 x 1 or a (3, 1, 1)."""
    c = X.conv_case(name)
    x = torch.stack([c.in_stack[i] for i in c.in_idx]).double()[:, 1:-1, 1:-1]                  # [n_in, H, W, Cin]
    w5 = c.w.double().view(c.Cout_all, c.KT, c.KH, c.KW, c.Cin).permute(0, 4, 1, 2, 3)
    xi = x.permute(3, 0, 1, 2)[None]
    if c.ss == 2:
        xi = torch.nn.functional.pad(xi, (0, 1, 0, 1))
    elif c.KH == 3:
        xi = torch.nn.functional.pad(xi, (1, 1, 1, 1))
    lib = torch.nn.functional.conv3d(xi, w5, c.b.double(), stride=(c.st, c.ss, c.ss))[0].permute(1, 2, 3, 0)
    mine = X.conv_frames_f64([c.in_stack[i] for i in c.in_idx], c.w, c.b, c.n_out, KT=c.KT, KH=c.KH, KW=c.KW, st=c.st, ss=c.ss, H_out=c.H_out,
                             W_out=c.W_out, in_off=c.in_off)
    assert torch.equal(mine, lib[:c.n_out, :c.H_out, :c.W_out])


def _scrambled_ss(x, gen):
    """fp32 sum of squares over the last axis in a random order of the channels, accumulated one element at a time."""
    xf = x.float().reshape(-1, x.shape[-1])[:, torch.randperm(x.shape[-1], generator=gen)]
    acc = torch.zeros(xf.shape[0])
    for j in range(xf.shape[1]):
        acc = acc + xf[:, j] * xf[:, j]
    return acc


@pytest.mark.parametrize("diverse", [False, True])
@pytest.mark.parametrize("C", X.RMS_CS)
def test_rms_case_is_exact_in_any_order_and_full_rows_return_gamma(C, diverse):
    g = torch.Generator().manual_seed(C)
    worst = 0
    for W in X.RMS_WS:
        c = X.rms_case(C, 2, 3, W, diverse)
        assert X.ss_exact_in_any_order(c.x, c.quantum[..., None])
        assert torch.equal(_scrambled_ss(c.x, g).double(), (c.x.double() ** 2).sum(-1).reshape(-1))
        pre = X.rms_restate_f32(c.x, c.gamma)
        full, zero = c.kind == 0, c.kind == 2
        if not diverse:  # a full row of +-2^k returns +-gamma exactly: sqrtf(C) / sqrtf(C 4^k) = 2^-k
            assert torch.equal(pre[full], c.x[full].float().sign() * c.gamma)
            if W > 1:
                assert bool(full.any()) and bool((c.kind == 1).any()) and bool(zero.any())
            assert _real_rounding_share(pre.to(BF), pre.double()) > 0.1
        assert bool((pre[zero] == 0).all()) and bool(torch.isfinite(pre).all())
        live = (c.x != 0).sum(-1)[c.kind == 1]
        assert live.numel() == 0 or (int(live.min()) >= max(C // 4, 1) and (diverse or int(live.max()) < C))
        # the neighbour chunk's gamma (16-byte chunk = 8 channels) and the fp64 formula's answer: seen, and within one ulp
        assert _differing_share(X.rms_restate_f32(c.x, c.gamma, gshift=8).to(BF), pre.to(BF)) >= SEEN_SHARE
        assert X.ulp_distance(pre.to(BF), X.rms_f64(c.x, c.gamma).float().to(BF)) <= 1
        if diverse:
            assert float(pre.abs().max()) <= 8.0
            d = X.ulp_distance(X.silu_fast_f32(pre).to(BF), X.silu_f64(pre))
            print(f"MEASURED rms C={C} W={W}: fp32 silu_fast vs fp64 SiLU {d} bf16 ulp, unequal {int(X.mismatches(X.silu_fast_f32(pre).to(BF), X.silu_f64(pre)).sum())}"
                  f" of {pre.numel()} (allowed {X.silu_unequal_allowed(pre)})")
            assert int(X.mismatches(X.silu_fast_f32(pre).to(BF), X.silu_f64(pre)).sum()) <= X.silu_unequal_allowed(pre)
            worst = max(worst, d)
    assert worst <= X.SILU_F32_VS_F64_ULPS


FUSED_SHAPES = [(Cin, KT) + f for Cin in X.FUSED_CINS for KT in (1, 3) for f in X.FUSED_FRAMES]


@pytest.mark.parametrize("Cin,KT,T,H,W", FUSED_SHAPES)
def test_fused_case_y_is_one_input_element_and_every_tap_and_chunk_is_addressed(Cin, KT, T, H, W):
    c = X.fused_case(Cin, KT, T, H, W, "single")
    assert set(c.tap_of.tolist()) == set(range(KT * 9)) and set((c.ci_of // 32).tolist()) == set(range(Cin // 32))
    assert len(set(zip(c.tap_of.tolist(), c.ci_of.tolist()))) == 96
    yd = c.y.double()
    mag = yd.abs()[yd != 0]
    assert bool((torch.log2(mag) == torch.log2(mag).round()).all()) and 2.0 ** -3 <= float(mag.min()) and float(mag.max()) <= 8.0
    assert X.ss_exact_in_any_order(c.y, 2.0 ** -3)
    g = torch.Generator().manual_seed(Cin + KT)
    assert torch.equal(_scrambled_ss(c.y, g).double(), (yd ** 2).sum(-1).reshape(-1))
    if H >= 5:
        assert bool((yd[:, 1, 2] == 0).all())                               # the all-zero pixel
    assert (yd != 0).double().mean().item() > 0.15                          # (T = 1 under KT = 3: two of three taps fall on front frames)
    if H * W >= 35:
        assert len(set(mag.tolist())) == 7                                  # every k in -3..3
    pre = X.fused_pre(c)
    assert bool((pre[yd.abs().sum(-1) == 0] == 0).all()) and bool(torch.isfinite(pre).all())
    assert X.ulp_distance(pre.to(BF), X.rms_f64(c.y, c.gamma).float().to(BF)) <= 1
    assert _differing_share(X.fused_pre(c, "gamma of the neighbour chunk").to(BF), pre.to(BF)) >= SEEN_SHARE
    d = X.ulp_distance(X.silu_fast_f32(pre).to(BF), X.silu_f64(pre))
    assert d <= X.SILU_F32_VS_F64_ULPS, d
    assert int(X.mismatches(X.silu_fast_f32(pre).to(BF), X.silu_f64(pre)).sum()) <= X.silu_unequal_allowed(pre)


@pytest.mark.parametrize("Cin,KT,T,H,W", FUSED_SHAPES)
def test_fused_residual_case_tells_the_three_candidate_rows_apart(Cin, KT, T, H, W):
    """out_stack = bf16(res + y) needs a real rounding, its squares sum exactly in any order, and the norm of y, the norm of the unrounded sum and
    the neighbour chunk's gamma each give other bits than the norm of bf16(res + y)."""
    c = X.fused_case(Cin, KT, T, H, W, "residual")
    live = c.y != 0
    assert (c.v.double() != c.sum32.double())[live].double().mean().item() > 0.8  # a real rounding wherever the conv contributes
    assert X.ss_exact_in_any_order(c.v, 2.0 ** -7)
    g = torch.Generator().manual_seed(Cin + KT + 1)
    assert torch.equal(_scrambled_ss(c.v, g).double(), (c.v.double() ** 2).sum(-1).reshape(-1))
    want = X.fused_pre(c).to(BF)
    for m in X.RMS_MISTAKES:
        share = _differing_share(X.fused_pre(c, m).to(BF), want)
        assert share >= (SEEN_SHARE if m == "norm before the bf16 rounding" else 0.5), (m, share)


@pytest.mark.parametrize("Cin,KT", [(32, 3), (96, 1), (192, 3)])
def test_fused_ordinary_case_is_exact_and_rounds(Cin, KT):
    c = X.fused_case(Cin, KT, 2, 5, 7, "ordinary")
    n_in = c.T + KT - 1
    exact = X.conv_frames_f64([c.in_stack[i] for i in range(n_in)], c.wp, c.b, c.T, KT=KT, KH=3, KW=3, st=1, ss=1, H_out=c.H, W_out=c.W, in_off=0)
    assert _real_rounding_share(c.y, exact) > 0.25
    assert bool((c.in_stack[:KT - 1, 1:-1, 1:-1] != 0).any()) or KT == 1


# ---- self-attention sums: tie rows and stair rows (every launch of tests/test_exact_attention_sums_gpu.py) -------------------------------
SUM_NAMES = sorted(X.SUM_CASES)


@pytest.mark.parametrize("name", SUM_NAMES)
def test_sums_case_closed_form_is_the_fp64_softmax(name):
    """The recipe's closed form (V[winner], the set's mean, +-r / 8) equals the plain fp64 softmax on the packed buffers for every family,
    every expected element is exact in bf16 by construction (`sums_case` asserts it on the fp64 value), every row kind sits in every 32-row
    group and in the partial last query block, and the large tie set holds what it must."""
    c = X.sum_named_case(name)
    for f in c.families:
        assert_exact(X.attention_sums_f64(c, family=f), c.want, f"{name} family {f}: closed form vs fp64")
    pure = X.SUM_CASES[name].get("pure", False)
    for g0 in range(0, c.n_q - 31, 32):
        kinds = set(c.kind[g0:g0 + 32].tolist())
        assert kinds == ({1, 2, 3, 4, 5} if (pure or 64 <= g0 < 128) else {0, 1, 2, 3, 4, 5}), (g0, kinds)
    if c.n_q % 256 >= 16:
        assert len(set(c.kind[c.n_q // 256 * 256:].tolist())) >= (5 if pure else 6)
    for b in range(c.B):
        for h in range(c.H):
            large = c.sets[b][h][3].tolist()
            assert [len(s) for s in c.sets[b][h]] == list(c.sizes) and 0 in large and c.n_k - 1 in large
            assert {x // c.tile for x in large} == set(range((c.n_k + c.tile - 1) // c.tile))
            allk = torch.cat(list(c.sets[b][h]) + [c.stair[b][h][0]])
            assert len(set(allk.tolist())) == len(allk)  # the sets and the stair share no key


@pytest.mark.parametrize("name", SUM_NAMES)
def test_sums_case_margins_and_step_premise(name):
    c = X.sum_named_case(name)
    sl2 = X.sum_scale_log2e(c.C)
    for f in c.families:
        lead, forb, gap = X.sum_margins(c, f)
        assert gap >= X.TIE_GAP, gap
        if not X.SUM_CASES[name].get("pure", False):
            assert lead >= MIN_MARGIN_NATS, lead
        assert forb >= MIN_MARGIN_NATS, forb
        u1, u2 = X.SUM_STEP[(f, c.C)]
        deepest = max(float(c.stair[b][h][1].max()) for b in range(c.B) for h in range(c.H))
        if f == "r":  # one component: the rounded product is exactly 1.0
            assert u2 == 0.0 and float((torch.tensor(u1, dtype=torch.float32) * sl2).to(BF)) == 1.0
        else:         # two components: the deviation from one octave per level, at the deepest level, in nats
            assert abs((u1 + u2) * sl2 - 1.0) < 2.0 ** -16 and abs((u1 + u2) * sl2 - 1.0) * deepest * math.log(2.0) < 2.0 ** -12


@pytest.mark.parametrize("schedule", ["max", "lazy"])
@pytest.mark.parametrize("name", SUM_NAMES)
def test_sums_case_fp32_online_softmax_gives_the_expected_bits(name, schedule):
    """An fp32 online softmax over 64-key tiles with P rounded to bf16 for P.V returns the expected bits whether the offset follows the
    maximum or lags by up to 8 octaves: the recipe leaves the kernels no rounding to differ in."""
    c = X.sum_named_case(name)
    for f in c.families:
        assert_exact(X.online_softmax_f32(c, f, schedule), c.want, f"{name} family {f} schedule {schedule}")


def test_sum_mistakes_are_seen():
    """Every entry of SUM_MISTAKES changes an expected element of some case, every case is changed by some mistake; a silent key changes
    tie and stair rows only (it moves l and nothing else), and the merge mistakes are seen by every case with a key split."""
    seen_by = {m: [] for m in X.SUM_MISTAKES}
    for name in SUM_NAMES:
        c = X.sum_named_case(name)
        changed = False
        for m in X.SUM_MISTAKES:
            if m.startswith("split merge") and c.nsplit == 1:
                continue
            bad = X.mismatches(X.attention_sums_f64(c, mistake=m), c.want)
            if bad.any():
                seen_by[m].append(name)
                changed = True
            if m == "one silent key counted" and c.silent and c.B == 1:
                assert bad[c.kind != 0].all(1).any(), name  # (a needle row whose winner is key 0 ties with it too)
            if m.startswith("split merge"):
                assert bad.any(), (name, m)
        assert changed, name
    for m, names in seen_by.items():
        assert names, m
    assert len(seen_by["a tied key dropped"]) == len(SUM_NAMES) and len(seen_by["the last valid key dropped"]) == len(SUM_NAMES)


def test_sum_split_rule_on_256_compute_units():
    for name, c in ((n, X.sum_named_case(n)) for n in SUM_NAMES if n.startswith("vae")):
        assert X.sum_split_count(c.n_q, c.n_k, c.C, 256, 4 * c.n_q * (c.C + 2)) == c.nsplit, name
        assert X.sum_split_count(c.n_q, c.n_k, c.C, 256, 0) == 1
    assert {X.sum_named_case(n).nsplit for n in SUM_NAMES if n.startswith("vae")} == {2, 4}
