"""Everything that writes an fp8 operand on the hot path of the fp8 mode, and the split-K tails of the fp8 GEMMs, element by element (recipes
and references: tests/exact_util.py; their CPU proofs: tests/test_exact_constructions.py).  Every link of "fused form == two launches" gets a
reference of its own:
  * quant_rows_fp8, ln_affine_fp8 (one scale per row): the documented fp32 arithmetic (`row_fp8_ref`), scale bits and every byte - on rows
    whose scale is a power of two (the bytes dequantise to the input) and on ordinary rows;
  * ln_affine_mxfp8, rmsnorm_rope_mxfp8: the MX contract applied to the exactly known bf16 row (`unit_rows` at eps = 0), through an affine whose
    32-column blocks differ by octaves / through post_scale and a RoPE table shorter than M; scale bytes past row M stay untouched;
  * gemm_mxfp8_gelu_quant and its tail kernel: operands whose GELU input is exact and saturated - the expected bytes need no transcendental -
    with the split on and off, on one launch that holds full tiles and tail tiles together, and with the split-K plan restated and asserted;
  * the GELU epilogue of gemm_mxfp8 / gemm_fp8 (both main loops) within one bf16 ulp of the fp64 activation of the exact input, and their
    bias / gated-residual epilogues exactly, each with the split on and off.
Strided inputs; every output sits in a wider, taller buffer of sentinels that must come back untouched."""
import pytest
import torch

import exact_util as X
from exact_util import BF, BYTE_SENTINEL, SCALE_SENTINEL, assert_exact, bf16_rne, gate_res_ref, int_vector, mx_operand
from test_exact_fp8_gpu import _e4m3_ints
from test_exact_gemm_gpu import _gelu_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -24576.0  # bf16 padding of a strided input (never read as a value: it would change every amax)


def _ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from chronoedit_amd import ops
    return ops


@pytest.fixture
def split():
    ops = _ops()
    old = ops.set_gemm_split(True)
    yield ops.set_gemm_split
    ops.set_gemm_split(old)


@pytest.fixture(params=[0, 1], ids=["w8", "w4"])
def fp8_variant(request):
    ops = _ops()
    old = ops.set_gemm_fp8_variant(request.param)
    yield request.param
    ops.set_gemm_fp8_variant(old)


def _strided(x: torch.Tensor) -> torch.Tensor:
    """x as a column slice of a wider device buffer (row stride K + 24)."""
    M, K = x.shape
    wide = torch.full((M, K + 24), SENTINEL, dtype=x.dtype)
    wide[:, 8:8 + K] = x
    return wide.to(DEV)[:, 8:8 + K]


def _gapped(M: int, K: int, fill: int = BYTE_SENTINEL):
    """(buffer [M + 2, K + 16] of sentinels, its [M, K] corner): an output with a gap behind every row and two rows behind the last."""
    big = torch.full((M + 2, K + 16), fill, dtype=torch.uint8, device=DEV)
    return big, big[:M, :K]


def _gap_untouched(big: torch.Tensor, M: int, K: int, what: str, fill: int = BYTE_SENTINEL) -> None:
    assert bool((big[:M, K:] == fill).all()) and bool((big[M:] == fill).all()), f"{what}: wrote outside its rows"


def _bits(s: torch.Tensor) -> torch.Tensor:
    return s.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. one scale per row: quant_rows_fp8, ln_affine_fp8
# ------------------------------------------------------------------------------------------------------------------------------------
ROW_KS = (5120, 13824, 264, 8)   # the two register-resident forms; the generic form with a partial last sweep of the wave; one chunk
ROW_MS = (1, 7, 129)             # a block of four rows is ragged


def _check_quant_rows_fp8(x: torch.Tensor, want_s: torch.Tensor, want_q: torch.Tensor, what: str) -> None:
    ops = _ops()
    M, K = x.shape
    big, out = _gapped(M, K)
    sbuf = torch.full((M + 3,), -7.0, dtype=torch.float32, device=DEV)
    ops.quant_rows_fp8(_strided(x), out=out, scale=sbuf[:M])
    assert_exact(_bits(sbuf[:M]), _bits(want_s), f"{what}: scale bits")
    assert_exact(out.contiguous(), want_q, f"{what}: e4m3 bytes")
    _gap_untouched(big, M, K, what)
    assert bool((sbuf[M:] == -7.0).all()), f"{what}: wrote a scale past row M"
    q, s = ops.quant_rows_fp8(x.to(DEV))  # (contiguous operands, buffers of the wrapper's own)
    assert_exact(_bits(s), _bits(want_s), f"{what}: scale bits, contiguous")
    assert_exact(q, want_q, f"{what}: e4m3 bytes, contiguous")


@pytest.mark.parametrize("K", ROW_KS)
def test_quant_rows_fp8_power_of_two_scales_round_trip(K):
    """Tier A: rows of e4m3 values times 2^e with amax = 448 2^e - the scale is 2^e bit for bit, the bytes are the ones the row was built from
    and dequantise to the input."""
    for M in ROW_MS:
        x, b, e = X.fp8_pow2_rows(M, K, torch.Generator().manual_seed(5000 + K + M))
        want_s, want_q = X.row_fp8_ref(x)
        assert torch.equal(want_s, torch.exp2(e.float())) and torch.equal(want_q, b)
        assert torch.equal(X.E4M3_LUT[want_q.long()] * want_s.double()[:, None], x.double())
        _check_quant_rows_fp8(x, want_s, want_q, f"quant_rows_fp8 tier A {M}x{K}")


@pytest.mark.parametrize("K", ROW_KS)
def test_quant_rows_fp8_ordinary_rows_equal_the_documented_arithmetic(K):
    """Tier B: ordinary rows, a row whose maximum sits in its last chunk only, an all-zero row: s = amax * float32(1 / 448), inv = 1 / s
    (the library is built without fast-math: a correctly rounded division), bytes RNE(x * inv) - bit for bit."""
    for M in ROW_MS:
        x = X.fp8_random_rows(M, K, torch.Generator().manual_seed(5100 + K + M))
        want_s, want_q = X.row_fp8_ref(x)
        _check_quant_rows_fp8(x, want_s, want_q, f"quant_rows_fp8 tier B {M}x{K}")


@pytest.mark.parametrize("D", X.LN_FP8_DS)
def test_ln_affine_fp8_exact(D):
    """`unit_rows` at eps = 0: the bf16 row the kernel would have written is known exactly; then the per-row restatement.  One (a, b) per
    three rows (ab_stride > D, NaN between the samples' vectors), strided input, gapped output."""
    ops = _ops()
    c = X.ln_fp8_case(D)
    ad = torch.full((c.S, D + 4), float("nan"))
    bd = torch.full((c.S, D + 4), float("nan"))
    ad[:, :D], bd[:, :D] = c.a, c.b
    big, out = _gapped(c.M, D)
    sbuf = torch.full((c.M + 3,), -7.0, dtype=torch.float32, device=DEV)
    ops.ln_affine_fp8(_strided(c.x), ad.to(DEV), bd.to(DEV), 0.0, out=out, scale=sbuf[:c.M], ab_rows=c.ab_rows, ab_stride=D + 4)
    assert_exact(_bits(sbuf[:c.M]), _bits(c.want_s), f"ln_affine_fp8 D={D}: scale bits")
    assert_exact(out.contiguous(), c.want_q, f"ln_affine_fp8 D={D}: e4m3 bytes")
    _gap_untouched(big, c.M, D, f"ln_affine_fp8 D={D}")
    assert bool((sbuf[c.M:] == -7.0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. MX producers on the row side
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", X.LN_MX_DS)
def test_ln_affine_mxfp8_exact(D):
    """130 rows, an affine per 43 rows whose 32-column blocks differ by octaves (zero blocks among them): scale bytes in the tiled order - the
    whole buffer, the sentinel bytes of rows 130 .. 255 included - and every element byte."""
    ops = _ops()
    c = X.ln_mx_case(D)
    big, out = _gapped(c.M, D)
    s = torch.full((ops.mx_scale_bytes(c.M, D),), SCALE_SENTINEL, dtype=torch.uint8, device=DEV)
    ops.ln_affine_mxfp8(_strided(c.x), c.a.to(DEV), c.b.to(DEV), 0.0, out=out, scale=s, ab_rows=c.ab_rows, ab_stride=D)
    rows = ops.mx_scales_to_rows(s, 256, D).cpu()
    assert_exact(rows[:c.M], c.want_rows, f"ln_affine_mxfp8 D={D}: E8M0 bytes")
    assert bool((rows[c.M:] == SCALE_SENTINEL).all()), f"ln_affine_mxfp8 D={D}: wrote scale bytes past row M"
    assert_exact(s.cpu(), c.want_s, f"ln_affine_mxfp8 D={D}: tiled scale buffer")
    assert_exact(out.contiguous(), c.want_q, f"ln_affine_mxfp8 D={D}: e4m3 bytes")
    _gap_untouched(big, c.M, D, f"ln_affine_mxfp8 D={D}")


@pytest.mark.parametrize("post", ["q-scale", "one"])
@pytest.mark.parametrize("R", [X.RMS_MX_M, 3, None], ids=["table-per-row", "table-of-3", "no-rope"])
@pytest.mark.parametrize("D,hd", X.RMS_MX_SHAPES)
def test_rmsnorm_rope_mxfp8_exact(D, hd, R, post):
    """Centred `unit_rows` at eps = 0: the bf16 value is known exactly (`rms_rope_exact`), then one fp32 multiply by post_scale and the
    floor-rule contract of the attention operands.  The input is the middle third of a wider buffer, which must come back unchanged."""
    ops = _ops()
    ps = ops.MXFP8_Q_SCALE if post == "q-scale" else 1.0
    c = X.rms_mx_case(D, hd, R, ps)
    src = torch.full((c.M, 3 * D), 3.0, dtype=BF)
    src[:, D:2 * D] = c.x
    buf = src.to(DEV)
    big, out = _gapped(c.M, D)
    sbig = torch.full((c.M + 2, D // 32), SCALE_SENTINEL, dtype=torch.uint8, device=DEV)
    ops.rmsnorm_rope_mxfp8(buf[:, D:2 * D], c.w.to(DEV), None if c.cs is None else c.cs.to(DEV), hd, 0.0, out=out, scale=sbig[:c.M], post_scale=ps)
    what = f"rmsnorm_rope_mxfp8 D={D} R={R} post_scale={ps}"
    assert_exact(sbig[:c.M], c.want_rows, f"{what}: E8M0 bytes")
    assert_exact(out.contiguous(), c.want_q, f"{what}: e4m3 bytes")
    _gap_untouched(big, c.M, D, what)
    assert bool((sbig[c.M:] == SCALE_SENTINEL).all()), f"{what}: wrote scale bytes past row M"
    assert torch.equal(buf.cpu(), src), f"{what}: source changed"


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the fp8 GEMMs: the split-K plan, the FFN-up form and its tail kernel, the GELU bend, bias and gated residual both ways
# ------------------------------------------------------------------------------------------------------------------------------------
def _plan(M: int, N: int, K: int):
    ops = _ops()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = X.fp8_tail_plan(M, N, K, cus, ops.GEMM_WS_BYTES)
    print(f"PLAN {M}x{N}x{K} on {cus} CUs: tiles {plan[0]}x{plan[1]}, {plan[2]} whole, {plan[3]} tail tiles cut in {plan[4]}")
    return plan


def _assert_cut(M: int, N: int, K: int, cut: bool):
    """The restated plan must send this shape through the split-K tail (or, for the shapes listed as whole, must not)."""
    plan = _plan(M, N, K)
    assert (plan[4] > 1 and plan[3] > 0) == cut, f"{M}x{N}x{K}: the split-K plan returns {plan}; this shape is listed as {'cut' if cut else 'whole'}"
    return plan


def test_the_split_k_plan_cuts_the_shapes_listed_as_cut():
    for shape, cut in list(X.SAT_CUT.items()) + list(X.BEND_CUT.items()) + [((300, 520, 13824), True), ((1000, 1032, 5120), True)]:
        _assert_cut(*shape, cut)
    tm, tn, t_full, tail, _ = _plan(4352, 4096, 5120)
    assert t_full > 0 and tail > 0, "4352 x 4096 x 5120 no longer holds full tiles and tail tiles in one launch"


def _mx_operands(a: torch.Tensor, w: torch.Tensor):
    """(aq, sa, wq, sw) through the production quantiser (pinned by test_exact_fp8_gpu.py), asserting that MXFP8 holds a and w exactly."""
    ops = _ops()
    for t in (a[:512], w[:512]):
        s8, q8 = X.mx_contract(t.cpu())
        assert torch.equal(X.mx_unpack(q8, s8), t.cpu().double()), "operand not exact in MXFP8"
    aq, sa = ops.quant_rows_mxfp8(a)
    wq, sw = ops.quant_rows_mxfp8(w, w_order=True)
    return aq, sa, wq, sw


@pytest.mark.parametrize("M,N,K", X.SAT_SHAPES)
def test_gemm_mxfp8_gelu_quant_saturated_inputs_exact_both_ways(M, N, K, split):
    """The FFN-up form on operands whose GELU input bf16(acc + bias) is exact and lies in {0} u [6, inf) u (-inf, -12]: the expected bytes are the
    contract applied to x, -0 or 0 - no transcendental.  Split on (tail tiles through gemm_fp8w4_reduce_gelu_q) and off (the in-kernel
    epilogue alone); gapped output, sentinel scale bytes past row M."""
    ops = _ops()
    _assert_cut(M, N, K, X.SAT_CUT[(M, N, K)])
    c = X.sat_gemm_case(M, N, K)
    a, w, bias = c.a.to(DEV), c.w.to(DEV), c.bias.to(DEV)
    x = bf16_rne(a.double() @ w.double().t() + bias.double()).cpu()  # (asserts that fp32 holds acc + bias exactly)
    y = X.sat_gelu(x)                                                 # (asserts that every input lies in the saturated set)
    assert X.mixed_block_share(y) >= 0.5
    want_rows, want_q = X.mx_contract(y)
    want_s = X.mx_scales_tiled(want_rows)
    assert bool((want_q == 0x80).any()) and bool((want_rows == 1).any()) and X.scale_diversity(want_rows) >= 0.5
    aq, sa, wq, sw = _mx_operands(a, w)
    for on in (True, False):
        split(on)
        what = f"gemm_mxfp8_gelu_quant {M}x{N}x{K} split {'on' if on else 'off'}"
        big, out = _gapped(M, N)
        s = torch.full((ops.mx_scale_bytes(M, N),), SCALE_SENTINEL, dtype=torch.uint8, device=DEV)
        ops.gemm_mxfp8_gelu_quant(aq, sa, wq, sw, bias, out=out, scale=s)
        assert_exact(ops.mx_scales_to_rows(s, M, N).cpu(), want_rows, f"{what}: E8M0 bytes")
        assert_exact(s.cpu(), want_s, f"{what}: tiled scale buffer (sentinels past row M)")
        assert_exact(out.contiguous().cpu(), want_q, f"{what}: e4m3 bytes")
        _gap_untouched(big, M, N, what)


@pytest.mark.parametrize("M,N,K", X.BEND_SHAPES)
def test_gemm_mxfp8_gelu_within_one_ulp_of_the_exact_input_both_ways(M, N, K, split):
    """gemm_mxfp8(EPI_BIAS_GELU): the input bf16(acc + bias) is exact and spans the activation's bend; the output lies within one bf16 ulp of the
    fp64 activation of that input (bound and x > -9 guard: test_gemm_gelu_within_one_ulp_of_the_exact_input)."""
    ops = _ops()
    _assert_cut(M, N, K, X.BEND_CUT[(M, N, K)])
    c = X.bend_gemm_case(M, N, K)
    a, w, bias = c.a.to(DEV), c.w.to(DEV), c.bias.to(DEV)
    x = bf16_rne(a.double() @ w.double().t() + bias.double())
    assert x.float().min().item() > -9.0 and (x.float().abs() < 4).double().mean().item() >= 0.5
    want = _gelu_ref(x, False)
    aq, sa, wq, sw = _mx_operands(a, w)
    for on in (True, False):
        split(on)
        got = ops.gemm_mxfp8(aq, sa, wq, sw, bias, epilogue=ops.EPI_BIAS_GELU)
        assert_exact(got, want, f"gemm_mxfp8 GELU {M}x{N}x{K} split {'on' if on else 'off'}", ulps=1)


@pytest.mark.parametrize("M,N,K", X.BEND_SHAPES)
def test_gemm_fp8_gelu_within_one_ulp_of_the_exact_input_both_ways(M, N, K, fp8_variant, split):
    """The same for gemm_fp8 (one power-of-two scale per row), on both main loops."""
    ops = _ops()
    _assert_cut(M, N, K, X.BEND_CUT[(M, N, K)])
    c = X.bend_gemm_case(M, N, K)
    bias = c.bias.to(DEV)
    x = bf16_rne(c.a.to(DEV).double() @ c.w.to(DEV).double().t() + bias.double())
    assert x.float().min().item() > -9.0 and (x.float().abs() < 4).double().mean().item() >= 0.5
    want = _gelu_ref(x, False)
    aq, wq = c.ia.to(torch.float8_e4m3fn).view(torch.uint8).to(DEV), c.iw.to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    for on in (True, False):
        split(on)
        got = ops.gemm_fp8(aq, c.sa.to(DEV), wq, c.sw.to(DEV), bias, epilogue=ops.EPI_BIAS_GELU)
        assert_exact(got, want, f"gemm_fp8 GELU {M}x{N}x{K} variant {fp8_variant} split {'on' if on else 'off'}", ulps=1)


CUT_SHAPES = ((300, 520, 13824), (1000, 1032, 5120))   # six tiles cut in six; twenty tiles cut in five


def _bias_gate_both_ways(run, lin: torch.Tensor, M: int, N: int, split, what: str) -> None:
    """Bias, gated residual with one gate row, and with one gate row per sample (two samples of M / 2 rows), each with the split on and off."""
    ops = _ops()
    gd = torch.Generator(device=DEV).manual_seed(M + N)
    res = (torch.randn(M, N, device=DEV, generator=gd) * 300).to(BF)
    gate = torch.randn(N, device=DEV, generator=gd)
    gates = torch.randn(2, N, device=DEV, generator=gd)
    gates[1] = gates[0] + 0.25 + torch.rand(N, device=DEV, generator=gd)
    gr = M // 2
    want_gate = gate_res_ref(lin, gate, res)
    want_gates = gate_res_ref(lin, gates.repeat_interleave(gr, 0)[:M], res)
    for on in (True, False):
        split(on)
        tag = f"{what} split {'on' if on else 'off'}"
        assert_exact(run(), lin, f"{tag}: bias")
        assert_exact(run(epilogue=ops.EPI_GATE_RES, gate=gate, res=res), want_gate, f"{tag}: gated residual")
        assert_exact(run(epilogue=ops.EPI_GATE_RES, gate=gates.reshape(-1).contiguous(), res=res, gate_rows=gr), want_gates,
                     f"{tag}: per-sample gates")


@pytest.mark.parametrize("M,N,K", CUT_SHAPES)
def test_gemm_mxfp8_bias_and_gated_residual_exact_both_ways(M, N, K, split):
    ops = _ops()
    _assert_cut(M, N, K, True)
    g = torch.Generator().manual_seed(M + N + K + 5)
    a, w = mx_operand(M, K, g).to(DEV), mx_operand(N, K, g).to(DEV)
    bias = int_vector(N, torch.Generator(device=DEV).manual_seed(M + K), lo=-512, hi=512, e=-2)
    aq, sa, wq, sw = _mx_operands(a, w)
    lin = bf16_rne(a.double() @ w.double().t() + bias.double())
    _bias_gate_both_ways(lambda **kw: ops.gemm_mxfp8(aq, sa, wq, sw, bias, **kw), lin, M, N, split, f"gemm_mxfp8 {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", CUT_SHAPES)
def test_gemm_fp8_bias_and_gated_residual_exact_both_ways(M, N, K, fp8_variant, split):
    ops = _ops()
    _assert_cut(M, N, K, True)
    g = torch.Generator().manual_seed(M * 3 + N + K + 5)
    aq, av = _e4m3_ints(M, K, g)
    wq, wv = _e4m3_ints(N, K, g)
    sa = torch.exp2(torch.randint(-2, 3, (M,), generator=g).float()).to(DEV)
    sw = torch.exp2(torch.randint(-2, 3, (N,), generator=g).float()).to(DEV)
    aq, wq = aq.to(DEV), wq.to(DEV)
    bias = int_vector(N, torch.Generator(device=DEV).manual_seed(M + N), lo=-512, hi=512, e=-2)
    lin = bf16_rne((av.to(DEV).double() * sa.double()[:, None]) @ (wv.to(DEV).double() * sw.double()[:, None]).t() + bias.double())
    _bias_gate_both_ways(lambda **kw: ops.gemm_fp8(aq, sa, wq, sw, bias, **kw), lin, M, N, split,
                         f"gemm_fp8 {M}x{N}x{K} variant {fp8_variant}")
