"""The bf16 GEMM family element by element, bit for bit (tests/exact_util.py): operands are small integers times a power of two per row,
so the fp32 accumulator holds the exact sum whatever the tile variant, summation order or split-K slab count, and every output element
has ONE right answer - the fp64 product rounded once to bf16 (round to nearest even) at the epilogue's documented rounding points:
  * EPI_BIAS / EPI_BIAS_ROW / EPI_BIAS_T:  bf16(acc + bias);
  * EPI_GATE_RES:  bf16(res + bf16(acc + bias) * gate), the multiply and the add each rounded in fp32 (transformer_chronoedit.py:281,293;
    ce_gemm_epi.h) - one gate row per sample with gate_rows > 0;
  * EPI_MUL:  bf16(res * bf16(acc + bias));  EPI_F32: acc itself;
  * GELU (tanh / erf):  the activation of the exact input bf16(acc + bias), within one bf16 ulp of its fp64 value."""
import math

import pytest
import torch

from exact_util import BF, assert_exact, bf16_rne, gate_res_ref, int_rows, int_vector, linear_f64

pytestmark = pytest.mark.gpu

VARIANTS = [-1, 0, 1, 2, 3, 4, 5, 6, 7]
VARIANT_IDS = ["auto", "tile128", "tile256w8", "tile256w8stag", "tile256w4_3stage", "tile256w4", "tile256w4_1barrier", "tile384x256",
               "tile288x256"]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


@pytest.fixture(params=VARIANTS, ids=VARIANT_IDS)
def variant(request):
    from chronoedit_amd import ops
    old = ops.set_gemm_variant(request.param)
    yield request.param
    ops.set_gemm_variant(old)


@pytest.fixture
def split():
    from chronoedit_amd import ops
    old = ops.set_gemm_split(True)
    yield ops.set_gemm_split
    ops.set_gemm_split(old)


# M at the 128 / 288 / 384-row tile edges and the step's row counts; N multiples of 8 off the 128 / 256 grid; K one 64-wide step, odd
# step counts, and the step's 5120 / 13824 (split-K tails)
SHAPES = [(127, 264, 64), (128, 136, 192), (129, 392, 320), (287, 520, 5120), (288, 1000, 704), (289, 264, 13824), (383, 136, 448),
          (384, 392, 64), (385, 520, 13824), (7200, 5120, 5120), (14400, 1032, 5120)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_bias_is_exact(M, N, K, variant):
    from chronoedit_amd import ops
    g = _gen(M * 7 + N + K)
    a, w = int_rows(M, K, g), int_rows(N, K, g)
    bias = int_vector(N, g)
    acc = linear_f64(a, w)
    assert_exact(ops.gemm(a, w, bias), bf16_rne(acc + bias.double()), f"EPI_BIAS {M}x{N}x{K}")
    assert_exact(ops.gemm(a, w, None), bf16_rne(acc), f"EPI_BIAS bias=None {M}x{N}x{K}")


@pytest.mark.parametrize("variant_", [-1, 4, 6, 7], ids=["auto", "tile256w4", "tile384x256", "tile288x256"])
@pytest.mark.parametrize("M,N,K", [(7200, 13824, 5120), (1000, 520, 13824), (14400, 5120, 5120), (4352, 4096, 1024)])
def test_gemm_split_k_tails_are_exact_both_ways(M, N, K, variant_, split):
    from chronoedit_amd import ops
    g = _gen(M + N + K + 1)
    a, w = int_rows(M, K, g), int_rows(N, K, g)
    bias = int_vector(N, g)
    want = bf16_rne(linear_f64(a, w, bias))
    old = ops.set_gemm_variant(variant_)
    try:
        for on in (True, False):
            split(on)
            assert_exact(ops.gemm(a, w, bias), want, f"split-K {'on' if on else 'off'} {M}x{N}x{K}")
    finally:
        ops.set_gemm_variant(old)


def test_gemm_split_k_on_two_concurrent_streams_is_exact(split):
    """Two side streams queue split-K products before any synchronisation, each with operands of its own: every stream is handed a scratch of
    its own (ops._gemm_scratch), so neither meets the other's slabs - through the product library, with a selector forced (the diagnostic
    library) and again after the reset, a stream keeping its scratch across the switches."""
    from chronoedit_amd import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    cases = []
    for M, N, K in [(7200, 13824, 5120), (7200, 5120, 13824)]:  # both cut their last round along K, on the 384- and on the 256-row tile
        g = _gen(M + N + K + 2)
        a, w = int_rows(M, K, g), int_rows(N, K, g)
        bias = int_vector(N, g)
        cases.append((a, w, bias, bf16_rne(linear_f64(a, w, bias)), f"{M}x{N}x{K}"))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    scratch = []
    for variant_ in (-1, 4, -1):  # product library, a selector away from its default (diagnostic library), reset
        old = ops.set_gemm_variant(variant_)
        try:
            ptrs = []
            for s in streams:
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    ptrs.append(ops._gemm_scratch(dev)[0])
            assert None not in ptrs and ptrs[0] != ptrs[1], ptrs
            scratch.append(ptrs)
            outs = []
            for _ in range(3):
                for s, (a, w, bias, _, _) in zip(streams, cases):
                    with torch.cuda.stream(s):
                        outs.append(ops.gemm(a, w, bias))
            torch.cuda.synchronize()
            for i, out in enumerate(outs):
                _, _, _, want, name = cases[i % 2]
                assert_exact(out, want, f"stream {i % 2}, launch {i // 2}, variant {variant_}: {name}")
        finally:
            ops.set_gemm_variant(old)
    assert scratch[0] == scratch[1] == scratch[2], scratch


@pytest.mark.parametrize("M,N,K", [(289, 520, 320), (7200, 1032, 5120), (128, 136, 64)])
def test_gemm_row_bias_and_transposed_store_are_exact_with_sentinel_padding(M, N, K, variant):
    from chronoedit_amd import ops
    g = _gen(M + 3 * N + K)
    a, w = int_rows(M, K, g), int_rows(N, K, g)
    acc = linear_f64(a, w)
    # EPI_BIAS_ROW: C[m, n] = bf16(acc + bias[m]) into a wider strided buffer whose padding must survive
    brow = int_vector(M, g)
    buf = torch.full((M, N + 72), -7.5, dtype=BF, device="cuda")
    ops.gemm(a, w, brow, out=buf[:, :N], epilogue=ops.EPI_BIAS_ROW)
    assert_exact(buf[:, :N], bf16_rne(acc + brow.double()[:, None]), f"EPI_BIAS_ROW {M}x{N}x{K}")
    assert_exact(buf[:, N:], torch.full_like(buf[:, N:], -7.5), "EPI_BIAS_ROW padding columns")
    # EPI_BIAS_T: C^T[n, m] = bf16(acc[m, n] + bias[n]) (the transposed store takes M % 8 == 0: the first M8 rows of a)
    M8 = M // 8 * 8
    bcol = int_vector(N, g)
    buf = torch.full((N, M8 + 72), -7.5, dtype=BF, device="cuda")
    ops.gemm(a[:M8], w, bcol, out=buf[:, :M8], epilogue=ops.EPI_BIAS_T)
    assert_exact(buf[:, :M8], bf16_rne(acc[:M8] + bcol.double()).t(), f"EPI_BIAS_T {M8}x{N}x{K}")
    assert_exact(buf[:, M8:], torch.full_like(buf[:, M8:], -7.5), "EPI_BIAS_T padding columns")


def _gate_res_cases(a, w, bias, gate, gate_rows, label):
    """EPI_GATE_RES in place (out is res) and out of place with ldres != ldc, against the CPU reference at the kernel's rounding points."""
    from chronoedit_amd import ops
    M, N = a.shape[0], w.shape[0]
    g = _gen(M + N + 11)
    lin = bf16_rne(linear_f64(a, w, bias))
    res = (torch.randn(M, N, device="cuda", generator=g) * 200).to(BF)
    gate_full = gate
    if gate is not None and gate_rows > 0:
        gate_full = gate.view(-1, N).repeat_interleave(gate_rows, 0)[:M]
    want = gate_res_ref(lin, gate_full, res)
    x = res.clone()
    ops.gemm(a, w, bias, out=x, epilogue=ops.EPI_GATE_RES, gate=gate, res=x, gate_rows=gate_rows)
    assert_exact(x, want, f"{label} in place")
    rbuf = torch.full((M, N + 40), 5.0, dtype=BF, device="cuda")
    rbuf[:, :N] = res
    obuf = torch.full((M, N + 16), -3.0, dtype=BF, device="cuda")
    ops.gemm(a, w, bias, out=obuf[:, :N], epilogue=ops.EPI_GATE_RES, gate=gate, res=rbuf[:, :N], gate_rows=gate_rows)
    assert_exact(obuf[:, :N], want, f"{label} out of place (ldres {N + 40}, ldc {N + 16})")
    assert (obuf[:, N:] == -3.0).all() and (rbuf[:, N:] == 5.0).all() and torch.equal(rbuf[:, :N], res)


@pytest.mark.parametrize("M,N,K", [(289, 520, 320), (7200, 1032, 5120)])
def test_gemm_gate_residual_is_exact(M, N, K, variant):
    g = _gen(M + N + 5 * K)
    a, w = int_rows(M, K, g), int_rows(N, K, g)
    bias = int_vector(N, g)
    _gate_res_cases(a, w, bias, None, 0, f"EPI_GATE_RES gate=None {M}x{N}x{K}")
    gate = torch.randn(N, device="cuda", generator=g) * 1.7
    _gate_res_cases(a, w, bias, gate, 0, f"EPI_GATE_RES gate[N] {M}x{N}x{K}")


# per-sample gates: (M, gate_rows) with the sample boundary inside a 384-row tile (14400 / 7200: tile 18) and on a 288-row tile edge
# (7200 = 25 x 288), inside both (2 x 3600), on a 384-row tile edge (2 x 2304 = 12 x 384), and gate rows shorter than a tile (the
# 8-wave kernel); the last case has a short last sample
GATE_ROWS_CASES = [(14400, 1032, 640, 7200), (7200, 1032, 640, 3600), (4608, 1032, 640, 2304), (600, 264, 192, 300), (770, 264, 128, 385),
                   (1000, 264, 192, 384)]


@pytest.mark.parametrize("M,N,K,gate_rows", GATE_ROWS_CASES)
def test_gemm_per_sample_gates_are_exact(M, N, K, gate_rows, variant):
    g = _gen(M + N + K + gate_rows)
    a, w = int_rows(M, K, g), int_rows(N, K, g)
    bias = int_vector(N, g)
    S = (M + gate_rows - 1) // gate_rows
    gate = torch.randn(S, N, device="cuda", generator=g)
    gate[1:] = gate[:1] + 0.25 + torch.rand(S - 1, N, device="cuda", generator=g)  # the samples' gates differ in every column
    _gate_res_cases(a, w, bias, gate.reshape(-1).contiguous(), gate_rows, f"EPI_GATE_RES gate_rows={gate_rows} {M}x{N}x{K}")


@pytest.mark.parametrize("variant_", [-1, 6, 7], ids=["auto", "tile384x256", "tile288x256"])
@pytest.mark.parametrize("M,gate_rows", [(14400, 7200), (7200, 3600)])
def test_gemm_per_sample_gates_are_exact_at_the_step_shape(M, gate_rows, variant_):
    """The B = 2 step's out-projection / FFN-down shape: N = K = 5120 (split-K tail tiles carry the gate switch through the reduce launch)."""
    from chronoedit_amd import ops
    g = _gen(M + gate_rows + 99)
    N = K = 5120
    a, w = int_rows(M, K, g), int_rows(N, K, g)
    bias = int_vector(N, g)
    gate = torch.randn(2, N, device="cuda", generator=g)
    gate[1] = gate[0] + 0.25 + torch.rand(N, device="cuda", generator=g)
    old = ops.set_gemm_variant(variant_)
    try:
        _gate_res_cases(a, w, bias, gate.reshape(-1).contiguous(), gate_rows, f"EPI_GATE_RES gate_rows={gate_rows} {M}x{N}x{K}")
    finally:
        ops.set_gemm_variant(old)


def _gelu_ref(x: torch.Tensor, erf: bool) -> torch.Tensor:
    """fp64 GELU in forms that do not cancel for negative x: 0.5 x erfc(-x / sqrt 2) and x / (1 + exp(-2u)) (== 0.5 x (1 + tanh u))."""
    x = x.double()
    if erf:
        y = 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    else:
        y = x / (1.0 + torch.exp(-2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return y.float().to(BF)


@pytest.mark.parametrize("M,N,K", [(289, 520, 320), (7200, 1032, 5120)])
def test_gemm_gelu_within_one_ulp_of_the_exact_input(M, N, K, variant):
    """GELU's input bf16(acc + bias) is exact: the output must be within one bf16 ulp of the fp64 activation of that input (operands
    scaled so that the inputs span the activation's bend).  The data keeps x > -9: below about -9.9 the exact tanh-form result is an
    fp32 subnormal, which the kernel's v_exp_f32 / v_rcp_f32 form returns as zero (measured: -6.6e-39 came back -0.0)."""
    from chronoedit_amd import ops
    g = _gen(M + N + K + 77)
    ew = (-6, -5) if K > 1000 else (-4, -3)
    a, w = int_rows(M, K, g, emin=-5, emax=-4), int_rows(N, K, g, emin=ew[0], emax=ew[1])
    bias = int_vector(N, g, lo=-32, hi=32, e=-4)
    x = bf16_rne(linear_f64(a, w, bias))
    for epi, erf in ((ops.EPI_BIAS_GELU, False), (ops.EPI_BIAS_GELU_ERF, True)):
        assert x.float().min().item() > -9.0
        got, want = ops.gemm(a, w, bias, epilogue=epi), _gelu_ref(x, erf)
        if erf:
            # 0.5 x (1 + erf(x / sqrt 2)) in fp32 (the kernel's formula, and torch's fp32 gelu the reference model runs) cancels below
            # x = -3: 1 + erf is < 3e-3 there and carries an absolute error of a few fp32 ulps of 1.  Those elements are bounded in
            # absolute terms (2 ulp of 1, times |x| / 2, plus one bf16 ulp of the result), not in ulps of a tiny result.
            tail = x.float() < -3.0
            err = (got.float() - want.float()).abs()
            bound = x.float().abs() * 2.0 ** -23 + want.float().abs() * 2.0 ** -7
            assert bool((err[tail] <= bound[tail]).all()), f"GELU erf tail {M}x{N}x{K}: {(err - bound)[tail].max().item()}"
            got, want = torch.where(tail, want, got), want
        assert_exact(got, want, f"GELU {'erf' if erf else 'tanh'} {M}x{N}x{K}", ulps=1)


@pytest.mark.parametrize("M,N,K", [(300, 136, 640), (1000, 1032, 5120), (129, 264, 13824)])
def test_gemm_mul_and_f32_epilogues_are_exact(M, N, K):
    from chronoedit_amd import ops
    g = _gen(M + N + K + 3)
    a, w = int_rows(M, K, g), int_rows(N, K, g)
    bias = int_vector(N, g)
    acc = linear_f64(a, w)
    # EPI_F32: the accumulator itself, exact in fp32
    assert_exact(ops.gemm_f32(a, w), acc.float(), f"EPI_F32 {M}x{N}x{K}")
    # EPI_MUL (UMT5 gated FFN): bf16(res * bf16(acc + bias))
    res = (torch.randn(M, N, device="cuda", generator=g) * 3).to(BF)
    want = torch.mul(res.float().cpu(), bf16_rne(acc + bias.double()).float().cpu()).to(BF)
    assert_exact(ops.gemm(a, w, bias, epilogue=ops.EPI_MUL, res=res), want, f"EPI_MUL {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K,S", [(7200, 1032, 5120, 4), (300, 264, 640, 2), (14400, 5120, 5120, 8)])
def test_gemm_k_segmented_operand_is_exact(M, N, K, S, variant):
    """a as [S, M, K/S] (the all-to-all's receive layout, a_seg_k of ce_gemm_bf16) == the product with the segments side by side along K."""
    from chronoedit_amd import ops
    g = _gen(M + N + K + S)
    a = int_rows(M, K, g)
    w, bias = int_rows(N, K, g), int_vector(N, g)
    aseg = a.view(M, S, K // S).transpose(0, 1).contiguous()
    assert_exact(ops.gemm(aseg, w, bias), bf16_rne(linear_f64(a, w, bias)), f"K-segmented a S={S} {M}x{N}x{K}")


@pytest.mark.parametrize("f32_out", [False, True])
def test_gemm_batched_is_exact(f32_out):
    """ce_gemm_batched_bf16: 2 x 3 products with two-level strides (the second nonzero), W shared along batch[0], a padded C row stride."""
    from chronoedit_amd import ops
    g = _gen(17 + f32_out)
    B0, B1, M, N, K = 2, 3, 77, 136, 192
    a = int_rows(B0 * B1 * M, K, g).view(B0, B1, M, K)
    w = int_rows(B1 * N, K, g).view(B1, N, K)
    ldc = N + 24
    dt = torch.float32 if f32_out else BF
    out = torch.full((B0, B1, M, ldc), 9.0, dtype=dt, device="cuda")
    bias = None if f32_out else int_vector(N, g)
    ops.gemm_batched(a, w, out, M=M, N=N, K=K, lda=K, ldw=K, ldc=ldc, batch=(B0, B1), stride_a=(B1 * M * K, M * K),
                     stride_w=(0, N * K), stride_c=(B1 * M * ldc, M * ldc), f32_out=f32_out, bias=bias)
    for z0 in range(B0):
        for z1 in range(B1):
            acc = linear_f64(a[z0, z1], w[z1], bias)
            want = acc.float() if f32_out else bf16_rne(acc)
            assert_exact(out[z0, z1, :, :N], want, f"gemm_batched z=({z0},{z1}) {'fp32' if f32_out else 'bf16'}")
    assert (out[..., N:] == 9.0).all()
