"""The small kernels of the conditioning encoders and the VAE mid-block, element by element: gather_rows, rmsnorm (T5LayerNorm), softmax_t5,
softmax_rows and im2col_patch2d (csrc/ce_enc.hip, csrc/ce_conv.hip), which the encoder and VAE goldens cover only at model-level tolerances.

The softmaxes use the tie recipe of tests/exact_util.py: 2^k keys of a row tie at the maximum and every other key trails by >= 200, so exp
underflows to exactly 0 in fp32 and the probabilities are exactly 2^-k and 0.  For softmax_t5 the bias table holds integers that are distinct
per (bucket, head) and scores = target - bias: a wrong bucket, head or offset breaks the tie; keys at or past the valid length carry a winning
score; the last valid key is always a tied one.  rmsnorm uses centred `unit_rows` at eps = 0 (the normalised values are 0, +-1, +-2; their
product with a bf16 weight is exact, so this recipe pins the indexing and the statistics, not the last rounding).  The copies (gather, im2col)
must equal the torch gather."""
import pytest
import torch

import exact_util as X
from exact_util import BF, assert_exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -24576.0
ROW_DS = (8, 264, 520, 5112, 5120)
ROW_MS = (1, 2, 3, 5, 9)


def _ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from chronoedit_amd import ops
    return ops


def _rejects(fn, *a, **kw):
    with pytest.raises(_ops().HipKernelError):
        fn(*a, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# gather_rows
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 520, 4096])  # 4096 = 512 chunks: eight trips of the 64-lane chunk loop
@pytest.mark.parametrize("n", [1, 5])
def test_gather_rows_copies_the_clamped_rows_and_nothing_else(D, n):
    ops = _ops()
    V = 11
    g = torch.Generator().manual_seed(7000 + D)
    table = torch.full((V, D + 8), SENTINEL, dtype=BF)
    table[:, :D] = torch.randn(V, D, generator=g).to(BF)
    ids = torch.tensor([V - 1] if n == 1 else [0, V - 1, 3, 3, 7], dtype=torch.int64)
    out = torch.full((n + 2, D + 16), SENTINEL, dtype=BF, device=DEV)
    ops.gather_rows(table.to(DEV)[:, :D], ids.to(DEV), out=out[:n, :D])
    assert_exact(out[:n, :D].contiguous(), table[ids, :D], f"gather_rows D={D} n={n}")
    assert bool((out[:n, D:] == SENTINEL).all()) and bool((out[n:] == SENTINEL).all())
    # ids outside [0, vocab) are clamped (include/chronoedit_hip.h): -1 reads row 0, vocab and beyond read row vocab - 1
    bad = torch.tensor([-1, V, V + 1000, -2 ** 40, 2 ** 40][:max(n, 2)], dtype=torch.int64)
    got = ops.gather_rows(table.to(DEV)[:, :D], bad.to(DEV))
    assert_exact(got, table[bad.clamp(0, V - 1), :D], f"gather_rows clamps D={D}")


def test_gather_rows_rejects_misaligned_rows():
    ops = _ops()
    out = torch.full((2, 24), SENTINEL, dtype=BF, device=DEV)
    t = torch.zeros(4, 24, dtype=BF, device=DEV)
    ids = torch.zeros(2, dtype=torch.int64, device=DEV)
    _rejects(ops.gather_rows, t[:, :12], ids, out=out[:, :12])                                     # D % 8
    _rejects(ops.gather_rows, torch.zeros(4, 20, dtype=BF, device=DEV)[:, :16], ids, out=out[:, :16])  # ldt % 8
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# rmsnorm (T5LayerNorm)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ROW_DS)
def test_rmsnorm_exact_over_the_row_grid(D):
    ops = _ops()
    g = torch.Generator().manual_seed(7100 + D)
    w = (X.dyadic((D,), g, 1, 128, -5) * (torch.randint(0, 2, (D,), generator=g).float() * 2 - 1)).to(BF)  # exact in bf16, never 0
    for M in ROW_MS:
        x, v = X.unit_rows(M, D, g, centred=True)
        want = X.bf16_rne(X.round_bf16_f64(v) * w.double())
        wide = torch.full((M, D + 8), SENTINEL, dtype=BF)
        wide[:, :D] = x
        out = torch.full((M + 2, D + 16), SENTINEL, dtype=BF, device=DEV)
        ops.rmsnorm(wide.to(DEV)[:, :D], w.to(DEV), 0.0, out=out[:M, :D])
        assert_exact(out[:M, :D].contiguous(), want, f"rmsnorm M={M} D={D}")
        assert bool((out[:M, D:] == SENTINEL).all()) and bool((out[M:] == SENTINEL).all())
        assert_exact(ops.rmsnorm(x.to(DEV), w.to(DEV), 0.0), want, f"rmsnorm packed M={M} D={D}")


def test_rmsnorm_rejections_write_nothing():
    ops = _ops()
    out = torch.full((2, 5136), SENTINEL, dtype=BF, device=DEV)
    x = torch.zeros(2, 5136, dtype=BF, device=DEV)
    w = torch.ones(5136, dtype=BF, device=DEV)
    _rejects(ops.rmsnorm, x[:, :12], w[:12], 0.0, out=out[:, :12])          # D % 8
    _rejects(ops.rmsnorm, x[:, :5128], w[:5128], 0.0, out=out[:, :5128])    # D > 5120
    _rejects(ops.rmsnorm, torch.zeros(2, 20, dtype=BF, device=DEV)[:, :16], w[:16], 0.0, out=out[:, :16])  # ldx % 8
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# softmax_t5
# ------------------------------------------------------------------------------------------------------------------------------------
T5_SHAPES = [(5, 5), (7, 100), (64, 65), (3, 1024)]
BATCH, HEADS = 2, 3


def _t5_run(ops, scores, Lq, Lk, ldp, table, lut, valid_b):
    """scores [rows, Lk] (CPU fp32) in a buffer with ld = Lk + 3 whose padding would win if it were read; returns probs [rows, ldp] after
    checking that the row past the last one still holds the sentinel."""
    rows = scores.shape[0]
    sbuf = torch.full((rows, Lk + 3), 1.0e4)
    sbuf[:, :Lk] = scores
    probs = torch.full((rows + 1, ldp), SENTINEL, dtype=BF, device=DEV)
    ops.softmax_t5(sbuf.to(DEV)[:, :Lk], probs[:rows], BATCH, HEADS, Lq, Lk, bucket_lut=None if lut is None else lut.to(DEV),
                   table=None if table is None else table.to(DEV), valid_len=None if valid_b is None else valid_b.to(torch.int32).to(DEV))
    assert bool((probs[rows:] == SENTINEL).all()), "softmax_t5 wrote past its rows"
    return probs[:rows]


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("Lq,Lk", T5_SHAPES)
def test_softmax_t5_exact_on_ties(Lq, Lk, with_bias):
    ops = _ops()
    g = torch.Generator().manual_seed(7200 + Lk)
    rows = BATCH * HEADS * Lq
    ldps = sorted({Lk, (Lk + 8) // 8 * 8 if Lk < 1024 else 1024, 1024})
    for valid_b in (torch.tensor([1, Lk // 2]), torch.tensor([Lk, Lk // 2]), None):
        valid = torch.full((rows,), Lk) if valid_b is None else valid_b.repeat_interleave(HEADS * Lq)
        target = X.tie_targets(rows, Lk, valid, g).double()
        table, lut = X.t5_bias(HEADS, Lq, Lk, g) if with_bias else (None, None)
        scores = X.exact_f64(target - X.t5_bias_rows(table, lut, BATCH, HEADS, Lq, Lk)) if with_bias else X.exact_f64(target)
        want = X.tie_probs(target, valid)
        for ldp in ldps:
            full = torch.zeros(rows, ldp, dtype=torch.float64)
            full[:, :Lk] = want
            got = _t5_run(ops, scores, Lq, Lk, ldp, table, lut, valid_b)
            assert_exact(got, X.bf16_rne(full), f"softmax_t5 Lq={Lq} Lk={Lk} ldp={ldp} valid={valid_b}")  # (columns [Lk, ldp) are zero)


def test_softmax_t5_writes_zeros_for_a_sample_without_valid_keys():
    """valid_len[b] == 0 (include/chronoedit_hip.h): every probability of that sample is 0, not NaN; the other sample is unaffected."""
    ops = _ops()
    Lq, Lk = 5, 70
    g = torch.Generator().manual_seed(7300)
    rows = BATCH * HEADS * Lq
    valid_b = torch.tensor([0, Lk])
    valid = valid_b.repeat_interleave(HEADS * Lq)
    target = X.tie_targets(rows, Lk, valid, g).double()
    table, lut = X.t5_bias(HEADS, Lq, Lk, g)
    scores = X.exact_f64(target - X.t5_bias_rows(table, lut, BATCH, HEADS, Lq, Lk))
    want = torch.zeros(rows, 72, dtype=torch.float64)
    want[:, :Lk] = X.tie_probs(target, valid)
    assert bool((want[:rows // 2] == 0).all()) and bool((want[rows // 2:].sum(1) == 1).all())
    assert_exact(_t5_run(ops, scores, Lq, Lk, 72, table, lut, valid_b), X.bf16_rne(want), "softmax_t5 valid_len = 0")


# Cap on the share of probabilities that differ from the fp64 answer at all (by one bf16 ulp).  Measured on an MI355X with the kernels of commit
# 13e7e89 on the seed below: 0.000024 (1 of 41184).  The cap is twice that.
T5_UNEQUAL_CAP = 0.00005


def test_softmax_t5_smooth_scores_within_one_ulp():
    ops = _ops()
    Lq, Lk = 33, 200
    g = torch.Generator().manual_seed(7400)
    rows = BATCH * HEADS * Lq
    scores = torch.randn(rows, Lk, generator=g) * 3
    table = torch.randn(32, HEADS, generator=g)
    lut = torch.randint(0, 32, (Lq + Lk - 1,), generator=g).to(torch.int32)
    valid_b = torch.tensor([Lk, 77])
    total = (scores + X.t5_bias_rows(table, lut, BATCH, HEADS, Lq, Lk).float()).double()  # (the kernel's one fp32 addition)
    want = torch.zeros(rows, 208, dtype=torch.float64)
    want[:, :Lk] = X.softmax_f64(total, valid_b.repeat_interleave(HEADS * Lq))
    want = want.float().to(BF)
    got = _t5_run(ops, scores, Lq, Lk, 208, table, lut, valid_b)
    share = X.unequal_share(got, want)
    print(f"MEASURED softmax_t5 smooth: unequal share {share:.6f}")
    assert_exact(got, want, "softmax_t5 smooth", ulps=1)
    assert share <= T5_UNEQUAL_CAP, share


def test_softmax_t5_rejections_write_nothing():
    ops = _ops()
    probs = torch.full((6, 1032), SENTINEL, dtype=BF, device=DEV)
    s = torch.zeros(6, 1032, device=DEV)
    _rejects(ops.softmax_t5, s[:, :1032], probs, 1, 2, 3, 1032)             # Lk > 1024
    narrow = torch.full((6, 8), SENTINEL, dtype=BF, device=DEV)
    _rejects(ops.softmax_t5, s[:, :16], narrow, 1, 2, 3, 16)                # ldp < Lk
    assert bool((probs == SENTINEL).all()) and bool((narrow == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# softmax_rows
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("M", [1, 5])
def test_softmax_rows_exact_on_ties(n, M):
    """scale = 2^-3 and scores = target / scale: (score - max) * scale is the integer target difference, exactly."""
    ops = _ops()
    g = torch.Generator().manual_seed(7500 + n)
    scale = 0.125
    target = X.tie_targets(M, n, [n] * M, g).double()
    want = X.tie_probs(target, [n] * M)
    npad, ldp = (n + 8) // 8 * 8, (n + 8) // 8 * 8 + 8
    sbuf = torch.full((M, n + 5), 1.0e6)  # (padding that would win if it were read)
    sbuf[:, :n] = X.exact_f64(target / scale)
    probs = torch.full((M + 1, ldp), SENTINEL, dtype=BF, device=DEV)
    ops.softmax_rows(sbuf.to(DEV)[:, :n], probs[:M, :npad], n, scale)
    full = torch.zeros(M, npad, dtype=torch.float64)
    full[:, :n] = want
    assert_exact(probs[:M, :npad].contiguous(), X.bf16_rne(full), f"softmax_rows n={n} M={M}")  # (columns [n, npad) are zero)
    assert bool((probs[:M, npad:] == SENTINEL).all()) and bool((probs[M:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# im2col_patch2d
# ------------------------------------------------------------------------------------------------------------------------------------
def _unfold(img, P, kpad):
    B, C, H, W = img.shape
    cols = torch.nn.functional.unfold(img.float(), P, stride=P).transpose(1, 2).reshape(B * (H // P) * (W // P), C * P * P).to(BF)
    out = torch.zeros(cols.shape[0], kpad, dtype=BF, device=img.device)
    out[:, :C * P * P] = cols
    return out


@pytest.mark.parametrize("B,C,H,W,P,kpad", [(1, 3, 28, 28, 14, 592), (2, 1, 4, 6, 2, 8), (2, 1, 4, 6, 2, 4),
                                            (1, 3, 170 * 14, 170 * 14, 14, 592)])  # the last: 17.1 M elements > 65535 * 256, the grid-stride loop wraps
def test_im2col_patch2d_equals_unfold(B, C, H, W, P, kpad):
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(7600)
    img = torch.randn(B, C, H, W, generator=g, device=DEV).to(BF)
    rows = B * (H // P) * (W // P)
    assert rows * kpad > 65535 * 256 or H < 100
    out = torch.full((rows + 1, kpad), SENTINEL, dtype=BF, device=DEV)
    ops.im2col_patch2d(img, P, kpad, out=out[:rows])
    assert_exact(out[:rows], _unfold(img, P, kpad), f"im2col {B}x{C}x{H}x{W} P={P}")
    assert bool((out[rows:] == SENTINEL).all())


def test_im2col_patch2d_rejections_write_nothing():
    ops = _ops()
    out = torch.full((64,), SENTINEL, dtype=BF, device=DEV)
    _rejects(ops.im2col_patch2d, torch.zeros(1, 1, 5, 4, dtype=BF, device=DEV), 2, 4, out=out[:16].view(4, 4))   # H % P
    _rejects(ops.im2col_patch2d, torch.zeros(1, 2, 4, 4, dtype=BF, device=DEV), 2, 4, out=out[:16].view(4, 4))   # kpad < C P P
    assert bool((out == SENTINEL).all())
