"""The row kernels of csrc/ce_rowops.hip element by element: ln_affine, rmsnorm_rope_, rope_scatter, gemv, modulation, the timestep sinusoid and
patchify / unpatchify, each against an answer that is known exactly (recipes and their CPU checks: tests/exact_util.py,
tests/test_exact_constructions.py).

Exact cases: `unit_rows` data at eps = 0 - the fp32 statistics are exact in any order (mean = mu, rstd = 1 / s), the normalised values are
0, +-1, +-2, and the affine / weight / rotation that follows is exact in fp32, so the kernel's bf16 result must equal the fp64 answer rounded
once, bit for bit.  a, b, w, cos / sin and the bias differ in every column, row and sample: a wrong index changes the value.

Where the formula holds a transcendental (ordinary data at eps = 1e-6, silu, sin / cos) the comparison is with the fp64 evaluation of the same
formula with the kernel's documented rounding points: bf16 results within 1 ulp element by element with a cap on the share that differs at
all, fp32 results within a bound derived from the formula."""
import math

import pytest
import torch

import exact_util as X
from exact_util import BF, assert_exact, bf16_rne

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROW_DS = (8, 264, 520, 5112, 5120)
ROW_MS = (1, 2, 3, 5, 9)
SENTINEL = -24576.0  # what every element a kernel must not write holds before the call (exact in bf16)


def _ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from chronoedit_amd import ops
    return ops


def _rejects(fn, *a, **kw):
    ops = _ops()
    with pytest.raises(ops.HipKernelError):
        fn(*a, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# ln_affine
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ROW_DS)
def test_ln_affine_exact_over_the_row_grid(D):
    """Every M in 1, 2, 3, 5, 9 (at D = 5120 an odd M leaves the two-row body's last wave one real and one phantom row); one (a, b)."""
    ops = _ops()
    g = torch.Generator().manual_seed(1000 + D)
    a, b = X.affine_vectors(1, D, g)
    rounded = []
    for M in ROW_MS:
        x, v = X.unit_rows(M, D, g)
        want64 = X.ln_affine_exact(v, a, b)
        want = bf16_rne(want64)
        rounded.append((want.double() != want64).double().mean().item())
        got = ops.ln_affine(x.to(DEV), a[0].to(DEV), b[0].to(DEV), 0.0)
        assert_exact(got, want, f"ln_affine M={M} D={D}")
    assert sum(rounded) / len(rounded) >= 0.25, rounded  # the final rounding to bf16 is exercised


@pytest.mark.parametrize("D,ab_rows,M,ab_stride", [
    (5120, 4, 12, 5120),   # two-row body, M = 3 * ab_rows
    (5120, 4, 11, 5120),   # ... an M that ends inside a sample, on a phantom row
    (5120, 2, 5, 5120),
    (5120, 3, 9, 5120),    # odd ab_rows: the one-row full body
    (5120, 3, 8, 5128),    # ... with ab_stride > D
    (5120, 4, 10, 5124),   # two-row body, ab_stride > D (a multiple of 4, not of 8)
    (520, 2, 6, 520),
    (520, 3, 7, 524),
])
def test_ln_affine_exact_with_one_affine_per_sample(D, ab_rows, M, ab_stride):
    ops = _ops()
    g = torch.Generator().manual_seed(1100 + D + 7 * ab_rows + M)
    S = -(-M // ab_rows)
    x, v = X.unit_rows(M, D, g)
    a, b = X.affine_vectors(S, D, g)
    want = bf16_rne(X.ln_affine_exact(v, a, b, ab_rows))
    ad = torch.full((S, ab_stride), float("nan"))  # (what lies between two samples' rows must not be read as a value)
    bd = torch.full((S, ab_stride), float("nan"))
    ad[:, :D], bd[:, :D] = a, b
    got = ops.ln_affine(x.to(DEV), ad.to(DEV), bd.to(DEV), 0.0, ab_rows=ab_rows, ab_stride=ab_stride)
    assert_exact(got, want, f"ln_affine ab_rows={ab_rows} M={M} D={D} ab_stride={ab_stride}")


@pytest.mark.parametrize("D,M", [(5120, 5), (5120, 4), (520, 3), (8, 5)])
def test_ln_affine_exact_on_strided_input_and_writes_only_its_rows(D, M):
    """x is a column slice of a wider buffer (ldx > D); the output is a slice of a wider, taller buffer full of a sentinel: its padding columns
    and the rows past M still hold the sentinel afterwards."""
    ops = _ops()
    g = torch.Generator().manual_seed(1200 + D + M)
    x, v = X.unit_rows(M, D, g)
    a, b = X.affine_vectors(1, D, g)
    wide = torch.full((M, D + 24), SENTINEL, dtype=BF)
    wide[:, 8:8 + D] = x
    out = torch.full((M + 3, D + 16), SENTINEL, dtype=BF, device=DEV)
    ops.ln_affine(wide.to(DEV)[:, 8:8 + D], a[0].to(DEV), b[0].to(DEV), 0.0, out=out[:M, :D])
    assert_exact(out[:M, :D].contiguous(), bf16_rne(X.ln_affine_exact(v, a, b)), f"ln_affine strided M={M} D={D}")
    assert bool((out[:M, D:] == SENTINEL).all()) and bool((out[M:] == SENTINEL).all()), "ln_affine wrote outside its rows"


# Cap on the share of elements that differ from the fp64 answer at all (every one of them by one bf16 ulp).  Measured on an MI355X with the
# kernels of commit 13e7e89 on the seeds below: 0 (D = 5120, two rows per wave), 0.000043 (D = 5120, ab_rows = 3: 2 of 46080), 0 (D = 520).
# The cap is twice the largest.
LN_UNEQUAL_CAP = 0.00009


@pytest.mark.parametrize("D,M,ab_rows", [(5120, 7, 0), (5120, 9, 3), (520, 9, 0)])
def test_ln_affine_ordinary_data_within_one_ulp(D, M, ab_rows):
    """One case per kernel body (two rows per wave, one full-width row, guarded chunks) on ordinary data, eps = 1e-6."""
    ops = _ops()
    g = torch.Generator().manual_seed(1300 + D + ab_rows)
    S = -(-M // ab_rows) if ab_rows else 1
    x = (torch.randn(M, D, generator=g) * 3 + 0.5).to(BF)
    a = 1 + 0.1 * torch.randn(S, D, generator=g)
    b = 0.1 * torch.randn(S, D, generator=g)
    want = X.ln_affine_f64(x, a, b, 1e-6, ab_rows).float().to(BF)
    got = ops.ln_affine(x.to(DEV), a.to(DEV), b.to(DEV), 1e-6, ab_rows=ab_rows, ab_stride=D)
    share = X.unequal_share(got, want)
    print(f"MEASURED ln_affine D={D} ab_rows={ab_rows}: unequal share {share:.6f}")
    assert_exact(got, want, f"ln_affine ordinary D={D}", ulps=1)
    assert share <= LN_UNEQUAL_CAP, share


def test_ln_affine_rejections_write_nothing():
    ops = _ops()
    out = torch.full((4, 5128), SENTINEL, dtype=BF, device=DEV)
    x = torch.zeros(4, 5136, dtype=BF, device=DEV)
    a = torch.ones(4, 5136, device=DEV)
    _rejects(ops.ln_affine, x[:, :12], a[0, :12], a[0, :12], 0.0, out=out[:, :12])            # D % 8
    _rejects(ops.ln_affine, x[:, :5128], a[0], a[0], 0.0, out=out)                            # D > 5120
    _rejects(ops.ln_affine, x[:, :16], a[0], a[0], 0.0, out=out[:, :16], ab_rows=2, ab_stride=18)  # ab_stride % 4
    xs = torch.zeros(4, 20, dtype=BF, device=DEV)
    _rejects(ops.ln_affine, xs[:, :16], a[0], a[0], 0.0, out=out[:, :16])                     # ldx % 8
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# rmsnorm_rope_
# ------------------------------------------------------------------------------------------------------------------------------------
def _rms_case(M, D, hd, R, seed, second=False):
    g = torch.Generator().manual_seed(seed)
    x, v = X.unit_rows(M, D, g, centred=True)
    w = X.rms_weights(D, g)
    cs = X.rope_table(R, hd, g) if R else None
    out = [x, v, w, cs]
    if second:
        x2, v2 = X.unit_rows(M, D, g, centred=True)
        out += [x2, v2, X.rms_weights(D, g)]
    return out


def _run_in_middle_third(ops, x, w, cs, hd, x2=None, w2=None):
    """In place on the middle third of a [M, 3D] buffer (x2: on the last third); returns the buffer and what it held before."""
    M, D = x.shape
    buf = torch.full((M, 3 * D), SENTINEL, dtype=BF)
    buf[:, D:2 * D] = x
    if x2 is not None:
        buf[:, 2 * D:] = x2
    buf = buf.to(DEV)
    before = buf.clone()
    ops.rmsnorm_rope_(buf[:, D:2 * D], w.to(DEV), None if cs is None else cs.to(DEV), hd, 0.0,
                      x2=None if x2 is None else buf[:, 2 * D:], w2=None if w2 is None else w2.to(DEV))
    return buf, before


@pytest.mark.parametrize("D,hd", [(8, 8), (264, 8), (520, 8), (5112, 8), (5120, 128)])
def test_rmsnorm_exact_without_rope_over_the_row_grid(D, hd):
    ops = _ops()
    rounded = []
    for M in ROW_MS:
        x, v, w, _ = _rms_case(M, D, hd, 0, 2000 + D + M)
        buf, before = _run_in_middle_third(ops, x, w, None, hd)
        want = X.rms_rope_exact(v, w)
        rounded.append((want.double() != v * w.double()).double().mean().item())
        assert_exact(buf[:, D:2 * D].contiguous(), want, f"rmsnorm M={M} D={D}")
        assert torch.equal(buf[:, :D], before[:, :D]) and torch.equal(buf[:, 2 * D:], before[:, 2 * D:])
    assert sum(rounded) / len(rounded) >= 0.25, rounded


# head_dim 128 and 64 divide 512: one cos / sin load per lane (cs_once); 96 and 40 do not: the per-chunk loads.  D = 5120 is the unguarded body.
ROPE_SHAPES = [(5120, 128), (5120, 64), (512, 128), (264 * 8, 64), (5120, 40), (480, 96), (4992, 96), (520, 40), (5112, 8), (264, 24), (8, 8)]


@pytest.mark.parametrize("D,hd", ROPE_SHAPES)
@pytest.mark.parametrize("M,R", [(1, 1), (2, 2), (5, 5), (9, 9), (9, 3), (3, 1)])
def test_rmsnorm_rope_exact(D, hd, M, R):
    """R == M: one table row per token.  R < M (M = 3R or R = 1): stacked samples share the table, row m uses entry m % R."""
    ops = _ops()
    x, v, w, cs = _rms_case(M, D, hd, R, 2100 + D + hd + 13 * M + R)
    buf, before = _run_in_middle_third(ops, x, w, cs, hd)
    assert_exact(buf[:, D:2 * D].contiguous(), X.rms_rope_exact(v, w, cs, hd), f"rmsnorm_rope M={M} R={R} D={D} head_dim={hd}")
    assert torch.equal(buf[:, :D], before[:, :D]) and torch.equal(buf[:, 2 * D:], before[:, 2 * D:])


@pytest.mark.parametrize("D,hd,M,R", [(5120, 128, 6, 2), (520, 40, 5, 5), (480, 96, 9, 3), (512, 64, 3, 0)])
def test_rmsnorm_rope_exact_on_two_tensors_with_their_own_weights(D, hd, M, R):
    ops = _ops()
    x, v, w, cs, x2, v2, w2 = _rms_case(M, D, hd, R, 2200 + D + hd, second=True)
    buf, before = _run_in_middle_third(ops, x, w, cs, hd, x2=x2, w2=w2)
    assert_exact(buf[:, D:2 * D].contiguous(), X.rms_rope_exact(v, w, cs, hd), f"first tensor D={D}")
    assert_exact(buf[:, 2 * D:].contiguous(), X.rms_rope_exact(v2, w2, cs, hd), f"second tensor D={D}")
    assert torch.equal(buf[:, :D], before[:, :D])


def test_rmsnorm_rope_rejections_write_nothing():
    ops = _ops()
    buf = torch.full((4, 5136), SENTINEL, dtype=BF, device=DEV)
    w = torch.ones(5136, device=DEV)
    _rejects(ops.rmsnorm_rope_, buf[:, :5128], w[:5128], None, 8, 0.0)     # D > 5120
    _rejects(ops.rmsnorm_rope_, buf[:, :12], w[:12], None, 4, 0.0)         # D % 8
    _rejects(ops.rmsnorm_rope_, buf[:, :48], w[:48], None, 12, 0.0)        # head_dim % 8
    _rejects(ops.rmsnorm_rope_, buf[:, :48], w[:48], None, 32, 0.0)        # D % head_dim
    odd = torch.full((4, 52), SENTINEL, dtype=BF, device=DEV)
    _rejects(ops.rmsnorm_rope_, odd[:, :48], w[:48], None, 8, 0.0)         # ld % 8
    assert bool((buf == SENTINEL).all()) and bool((odd == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# rope_scatter
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 4])
@pytest.mark.parametrize("D,hd", [(5120, 128), (480, 96)])
def test_rope_scatter_exact(W, D, hd):
    """q and k normalised with their own weights and rotated with the shared table (period R = 2 over M = 6 rows), v copied, written in the
    all-to-all send layout [rank][row][tensor][D / W]."""
    ops = _ops()
    M, R = 6, 2
    g = torch.Generator().manual_seed(2300 + D + W)
    xs, vs, ws = [], [], []
    for _ in range(3):
        x, v = X.unit_rows(M, D, g, centred=True)
        xs.append(x), vs.append(v), ws.append(X.rms_weights(D, g))
    cs = X.rope_table(R, hd, g)
    pad = torch.full((M, 8), SENTINEL, dtype=BF)
    buf = torch.cat([pad, xs[0], xs[1], pad, xs[2], pad], 1).to(DEV)  # column blocks at 8, 8 + D, 16 + 2D
    cols = [8, 8 + D, 16 + 2 * D]
    got = ops.rope_scatter(buf, cols, [ws[0].to(DEV), ws[1].to(DEV), None], D, W, cs.to(DEV), hd, 0.0)
    want = torch.stack([X.rms_rope_exact(vs[0], ws[0], cs, hd), X.rms_rope_exact(vs[1], ws[1], cs, hd), xs[2]], 1)  # [M, 3, D]
    want = want.view(M, 3, W, D // W).permute(2, 0, 1, 3).contiguous()
    assert_exact(got, want, f"rope_scatter W={W} D={D}")


# ------------------------------------------------------------------------------------------------------------------------------------
# gemv
# ------------------------------------------------------------------------------------------------------------------------------------
GEMV_KS = (64, 256, 512, 1000, 5120)  # fp32 weights take 16-byte loads at K % 256 == 0, bf16 weights at K % 512 == 0; otherwise the scalar loop
GEMV_NS = (1, 15, 16, 17, 96)


def _gemv_int(N, K, g, dtype):
    w = X.int_rows(N, K, g, lo=-2, hi=2, emin=0, emax=0).to(dtype)
    return w, X.dyadic((K,), g, -2, 2, 0), X.gemv_bias(N, g)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", GEMV_KS)
def test_gemv_exact_on_integers(K, dtype):
    """Integer W and x: every partial sum is an integer below 2^24.  With and without the bias, plain and with the bf16 rounding (flag 4)."""
    ops = _ops()
    g = torch.Generator().manual_seed(3000 + K)
    for N in GEMV_NS:
        w, x, bias = _gemv_int(N, K, g, dtype)
        dot = X.linear_f64(w, x[None, :])[:, 0]
        out = torch.full((N + 3,), SENTINEL, device=DEV)
        for b in (bias, None):
            want64 = dot if b is None else dot + b.double()
            assert want64.abs().max().item() < 2048
            for flags in (0, 4):
                want = bf16_rne(want64).float() if flags else X.exact_f64(want64)
                ops.gemv(w.to(DEV), x.to(DEV), None if b is None else b.to(DEV), flags, out=out[:N])
                assert_exact(out[:N], want, f"gemv N={N} K={K} flags={flags} bias={b is not None}")
        assert bool((out[N:] == SENTINEL).all()), "gemv wrote past row N"


def test_gemv_exact_at_the_lds_limit_and_rejects_one_chunk_more():
    ops = _ops()
    g = torch.Generator().manual_seed(3100)
    for dtype in (torch.float32, BF):
        w, x, bias = _gemv_int(17, 16384, g, dtype)
        want = X.exact_f64(X.linear_f64(w, x[None, :])[:, 0] + bias.double())
        assert_exact(ops.gemv(w.to(DEV), x.to(DEV), bias.to(DEV)), want, "gemv K=16384")
    out = torch.full((4,), SENTINEL, device=DEV)
    with pytest.raises(ops.HipKernelError, match="unsupported shape"):
        ops.gemv(torch.ones(4, 16392, device=DEV), torch.ones(16392, device=DEV), None, out=out)
    assert bool((out == SENTINEL).all())


def _silu64(t):
    return t / (1.0 + torch.exp(-t))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("flags", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("N,K", [(17, 1000), (33, 512)])
def test_gemv_ordinary_data_within_the_fp32_bound(N, K, flags, dtype):
    """y = post(W . pre(x) + bias) against fp64 with the documented rounding points (flag 1: x <- bf16(silu(x)); flag 4: the sum rounded to bf16
    before the post-silu).  Bound per output: K * 2^-24 * sum_k |w_k x_k| for the fp32 accumulation in any order (each of the K additions
    rounds a partial sum that never exceeds sum |w_k x_k|, by half an ulp = 2^-24 relative; the wave's 64-way split leaves the products' and
    the bias add's roundings ample room inside it), and - silu being 1.1-Lipschitz - that times 1.1 plus 4 fp32 ulp of the result for the
    post-silu's expf and division.  With flag 4 the
    rounding to bf16 may fall to the other side when the sum lies within the bound of a rounding boundary: one bf16 ulp is then allowed."""
    ops = _ops()
    g = torch.Generator().manual_seed(3200 + K + flags)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dtype)
    x = torch.randn(K, generator=g) * 2
    bias = torch.randn(N, generator=g)
    xs = x.double()
    if flags & 1:
        xs = _silu64(xs).float().to(BF).double()
    prod = w.double() * xs[None, :]
    acc = prod.sum(1) + bias.double()
    bound = K * 2.0 ** -24 * prod.abs().sum(1)
    got = ops.gemv(w.to(DEV), x.to(DEV), bias.to(DEV), flags).cpu().double()
    want = acc
    if flags & 4:
        want = acc.float().to(BF).double()
        bound = bound + torch.where((acc - want).abs() + bound >= X.ulp_bf16(acc.float()).double() / 2, X.ulp_bf16(acc.float()).double(), 0.0)
    if flags & 2:
        want = _silu64(want)
        bound = 1.1 * bound + 4 * 2.0 ** -24 * want.abs() + 2.0 ** -40
    err = (got - want).abs()
    # (measured on an MI355X, kernels of commit 13e7e89: the largest err / bound over all cases is 0.001 - the bound is the worst case of K
    # sequential additions, the kernel adds 64 partial sums of K / 64 terms)
    print(f"MEASURED gemv flags={flags} K={K}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (err / bound).max()


# ------------------------------------------------------------------------------------------------------------------------------------
# modulation, timestep sinusoid
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 100, 5120])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("v_rows", [1, 6])
def test_modulation_equals_the_two_fp32_additions(D, L, v_rows):
    ops = _ops()
    J = 6
    g = torch.Generator().manual_seed(4000 + D + L + v_rows)
    table = torch.randn(L, J, D, generator=g).to(DEV)
    v = torch.randn(v_rows, D, generator=g).to(DEV)
    for mask in (0, 0b010010, 0b111111):
        want = table + v.view(1, v_rows, D)
        one = torch.tensor([(mask >> j) & 1 for j in range(J)], dtype=torch.bool, device=DEV).view(1, J, 1)
        want = torch.where(one, 1.0 + want, want)
        assert_exact(ops.modulation(table, v, mask), want, f"modulation L={L} D={D} v_rows={v_rows} mask={mask:#b}")


@pytest.mark.parametrize("dim", [2, 256, 258, 1024])
@pytest.mark.parametrize("t", [0, 1, 637, 999, 500.5])
def test_timestep_sinusoid_within_the_argument_bound(t, dim):
    """out = [cos(t f_i), sin(t f_i)], f_i = exp(-ln(1e4) i / half).  The fp32 argument t * f_i carries a few ulp of relative error (the
    exponent's product and quotient, expf, the product with t: below 2^-21 relative), sin and cos are 1-Lipschitz and add an ulp of their own:
    |err| <= |t| * 2^-21 + 2^-22.  At t = 0 the answer is exactly 1 and 0."""
    ops = _ops()
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    want = torch.cat([torch.cos(t * f), torch.sin(t * f)])
    dtypes = (torch.float32,) if isinstance(t, float) else (torch.int64, torch.float32)
    for dt in dtypes:
        got = ops.timestep_sinusoid(torch.tensor([t], dtype=dt, device=DEV), dim).cpu()
        if t == 0:
            assert_exact(got, torch.cat([torch.ones(half), torch.zeros(half)]), f"sinusoid t=0 dim={dim} {dt}")
        err = (got.double() - want).abs().max().item()
        # (measured on an MI355X, kernels of commit 13e7e89: at most 5.3e-5 at t = 999 against the bound's 4.8e-4, 6.0e-8 at t = 1 against 7.2e-7)
        print(f"MEASURED sinusoid t={t} dim={dim} {dt}: max err {err:.3e} bound {abs(t) * 2.0 ** -21 + 2.0 ** -22:.3e}")
        assert err <= abs(t) * 2.0 ** -21 + 2.0 ** -22, err


def test_timestep_sinusoid_rejects_an_odd_dim():
    ops = _ops()
    out = torch.full((8,), SENTINEL, device=DEV)
    for dt in (torch.int64, torch.float32):
        _rejects(ops.timestep_sinusoid, torch.tensor([3], dtype=dt, device=DEV), 7, out=out)
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# patchify / unpatchify
# ------------------------------------------------------------------------------------------------------------------------------------
PATCH_SHAPES = [(36, 2, 12, 20), (1, 1, 2, 2), (16, 3, 6, 10)]


def _patch_rows(x):
    """The torch gather: rows (t, h/2, w/2), columns c * 4 + dh * 2 + dw."""
    C, T, H, W = x.shape
    return x.view(C, T, H // 2, 2, W // 2, 2).permute(1, 2, 4, 0, 3, 5).reshape(T * (H // 2) * (W // 2), C * 4)


@pytest.mark.parametrize("C,T,H,W", PATCH_SHAPES)
def test_patchify_equals_the_gather_whole_and_in_shards(C, T, H, W):
    ops = _ops()
    g = torch.Generator().manual_seed(5000 + C)
    x = torch.randn(C, T, H, W, generator=g).to(BF).to(DEV)
    ntok = T * (H // 2) * (W // 2)
    for kpad in (4 * C, 4 * C + 12):
        want = torch.zeros(ntok, kpad, dtype=BF, device=DEV)
        want[:, :4 * C] = _patch_rows(x)
        whole = torch.full((ntok + 2, kpad), SENTINEL, dtype=BF, device=DEV)
        ops.patchify(x, kpad, out=whole[:ntok])
        assert_exact(whole[:ntok], want, f"patchify kpad={kpad}")
        assert bool((whole[ntok:] == SENTINEL).all())
        # shards that tile the tokens, the last one reaching past them: its surplus rows are zero, the shards concatenated are the whole
        per = -(-ntok // 3) + 1
        parts = []
        for s in range(3):
            buf = torch.full((per + 1, kpad), SENTINEL, dtype=BF, device=DEV)
            ops.patchify(x, kpad, out=buf[:per], row0=s * per, nrows=per)
            assert bool((buf[per:] == SENTINEL).all())
            parts.append(buf[:per])
        cat = torch.cat(parts)
        assert 3 * per > ntok
        assert_exact(cat[:ntok], want, f"patchify shards kpad={kpad}")
        assert bool((cat[ntok:] == 0).all()), "rows past the last token must be zero"


@pytest.mark.parametrize("C,T,H,W", PATCH_SHAPES)
def test_unpatchify_equals_the_gather_with_a_padded_row(C, T, H, W):
    ops = _ops()
    g = torch.Generator().manual_seed(5100 + C)
    ntok = T * (H // 2) * (W // 2)
    for ldy in (4 * C, 4 * C + 8):
        y = torch.full((ntok, ldy), SENTINEL, dtype=BF)
        y[:, :4 * C] = torch.randn(ntok, 4 * C, generator=g).to(BF)
        # column (dh * 2 + dw) * C + c of token (t, hq, wq) -> out[c][t][2 hq + dh][2 wq + dw]
        want = y[:, :4 * C].view(T, H // 2, W // 2, 2, 2, C).permute(5, 0, 1, 3, 2, 4).reshape(C, T, H, W)
        out = torch.full((C * T * H * W + 8,), SENTINEL, dtype=BF, device=DEV)
        ops.unpatchify(y.to(DEV)[:, :4 * C] if ldy > 4 * C else y.to(DEV), C, T, H, W, out=out[:C * T * H * W].view(C, T, H, W))
        assert_exact(out[:C * T * H * W].view(C, T, H, W), want.contiguous(), f"unpatchify ldy={ldy}")
        assert bool((out[C * T * H * W:] == SENTINEL).all())


def test_patchify_rejects_odd_sizes_and_a_short_row():
    ops = _ops()
    out = torch.full((64, 16), SENTINEL, dtype=BF, device=DEV)
    for shape, kpad in (((2, 1, 3, 4), 8), ((2, 1, 4, 6 + 1), 8), ((2, 1, 4, 4), 4)):
        x = torch.zeros(shape, dtype=BF, device=DEV)
        n = shape[1] * (shape[2] // 2) * (shape[3] // 2)
        _rejects(ops.patchify, x, kpad, out=out.view(-1)[:n * kpad].view(n, kpad))
    y = torch.zeros(4, 8, dtype=BF, device=DEV)
    o = out.view(-1)
    _rejects(ops.unpatchify, y, 2, 1, 3, 4, out=o[:24].view(2, 1, 3, 4))   # odd H
    _rejects(ops.unpatchify, y, 4, 1, 4, 4, out=o[:64].view(4, 1, 4, 4))   # ldy < 4 * Cout
    assert bool((out == SENTINEL).all())
