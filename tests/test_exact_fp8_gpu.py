"""The fp8 GEMMs and the MX quantiser element by element (tests/exact_util.py): operands whose values have at most 4 significant bits and
lie inside the e4m3 range of their block's scale are quantised without loss, and with small-integer mantissas every sum is exact in fp32,
so the GEMM output must equal the fp64 product of the dequantised operands rounded once to bf16 (and, gated, at the epilogue's rounding
points).

Measured on MI355X (the first run of these tests): the scaled fp8 matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4) accumulates
these integer sums exactly, from K = 256 (the launchers' smallest: two 128-wide K steps) up to K = 13824 - no narrowing of the accumulator inside the fp8 dot product on
this data (|partial sums| < 2^22 units)."""
import pytest
import torch

from exact_util import BF, assert_exact, bf16_rne, gate_res_ref, int_vector, mx_operand
from test_mxfp8_gemm_gpu import _contract, _deq

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1], ids=["w8", "w4"])
def fp8_variant(request):
    from chronoedit_amd import ops
    old = ops.set_gemm_fp8_variant(request.param)
    yield request.param
    ops.set_gemm_fp8_variant(old)


@pytest.mark.parametrize("M,K", [(7, 256), (300, 5120), (1000, 13824), (129, 128)])
def test_quant_rows_mxfp8_round_trips_exactly(M, K):
    """The production quantiser: scale and element bytes == the contract's, in both scale orders, and dequantised == input."""
    from chronoedit_amd import ops
    x = mx_operand(M, K, torch.Generator().manual_seed(M + K))
    want_s, want_q = _contract(x)
    assert torch.equal(_deq(want_q, want_s), x.float())
    for w_order in (False, True):
        q, s = ops.quant_rows_mxfp8(x.cuda(), w_order=w_order)
        got_s = ops.mx_scales_to_rows(s, M, K, w_order=w_order).cpu()
        assert_exact(got_s, want_s, f"E8M0 bytes {M}x{K} w_order={w_order}")
        assert_exact(q.cpu(), want_q, f"e4m3 bytes {M}x{K} w_order={w_order}")
        assert_exact(_deq(q.cpu(), got_s), x.float(), "dequantised")


# K from the smallest the launchers take (two 128-wide steps) up to the step's 13824; M not a multiple of 128
MX_SHAPES = [(129, 264, 256), (300, 520, 256), (1000, 1032, 5120), (7200, 1280, 13824), (14400, 5120, 5120)]


@pytest.mark.parametrize("M,N,K", MX_SHAPES)
def test_gemm_mxfp8_is_exact(M, N, K, fp8_variant):
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a, w = mx_operand(M, K, g).cuda(), mx_operand(N, K, g).cuda()
    gd = torch.Generator(device="cuda").manual_seed(M + K)
    bias = int_vector(N, gd, lo=-512, hi=512, e=-2)
    aq, sa = ops.quant_rows_mxfp8(a)
    wq, sw = ops.quant_rows_mxfp8(w, w_order=True)
    lin = bf16_rne(a.double() @ w.double().t() + bias.double())
    assert_exact(ops.gemm_mxfp8(aq, sa, wq, sw, bias), lin, f"gemm_mxfp8 bias {M}x{N}x{K}")
    res = (torch.randn(M, N, device="cuda", generator=gd) * 300).to(BF)
    gate = torch.randn(N, device="cuda", generator=gd)
    out = ops.gemm_mxfp8(aq, sa, wq, sw, bias, epilogue=ops.EPI_GATE_RES, gate=gate, res=res)
    assert_exact(out, gate_res_ref(lin, gate, res), f"gemm_mxfp8 gate-residual {M}x{N}x{K}")
    if M >= 2 * 256:
        gr = M // 2
        gates = torch.randn(2, N, device="cuda", generator=gd)
        gates[1] = gates[0] + 0.25 + torch.rand(N, device="cuda", generator=gd)
        out = ops.gemm_mxfp8(aq, sa, wq, sw, bias, epilogue=ops.EPI_GATE_RES, gate=gates.reshape(-1).contiguous(), res=res, gate_rows=gr)
        assert_exact(out, gate_res_ref(lin, gates.repeat_interleave(gr, 0)[:M], res), f"gemm_mxfp8 per-sample gates {M}x{N}x{K}")


def _e4m3_ints(rows, K, g):
    """uint8 e4m3 bytes of integers in [-15, 15] (4 significant bits), an all-zero row."""
    v = torch.randint(-15, 16, (rows, K), generator=g).float()
    v[min(2, rows - 1)] = 0
    return v.to(torch.float8_e4m3fn).view(torch.uint8), v


@pytest.mark.parametrize("M,N,K", MX_SHAPES)
def test_gemm_fp8_row_scales_is_exact(M, N, K, fp8_variant):
    """ce_gemm_fp8 (one fp32 scale per row): bytes and power-of-two scales fed directly (amax / 448 of integer rows is no power of two)."""
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(M * 3 + N + K)
    aq, av = _e4m3_ints(M, K, g)
    wq, wv = _e4m3_ints(N, K, g)
    sa = torch.exp2(torch.randint(-2, 3, (M,), generator=g).float())
    sw = torch.exp2(torch.randint(-2, 3, (N,), generator=g).float())
    aq, wq, sa, sw = aq.cuda(), wq.cuda(), sa.cuda(), sw.cuda()
    gd = torch.Generator(device="cuda").manual_seed(M + N)
    bias = int_vector(N, gd, lo=-512, hi=512, e=-2)
    ad, wd = av.cuda().double() * sa.double()[:, None], wv.cuda().double() * sw.double()[:, None]
    lin = bf16_rne(ad @ wd.t() + bias.double())
    assert_exact(ops.gemm_fp8(aq, sa, wq, sw, bias), lin, f"gemm_fp8 bias {M}x{N}x{K}")
    res = (torch.randn(M, N, device="cuda", generator=gd) * 300).to(BF)
    if M >= 2 * 256:
        gr = M // 2
        gates = torch.randn(2, N, device="cuda", generator=gd)
        gates[1] = gates[0] + 0.25 + torch.rand(N, device="cuda", generator=gd)
        out = ops.gemm_fp8(aq, sa, wq, sw, bias, epilogue=ops.EPI_GATE_RES, gate=gates.reshape(-1).contiguous(), res=res, gate_rows=gr)
        assert_exact(out, gate_res_ref(lin, gates.repeat_interleave(gr, 0)[:M], res), f"gemm_fp8 per-sample gates {M}x{N}x{K}")
    else:
        gate = torch.randn(N, device="cuda", generator=gd)
        out = ops.gemm_fp8(aq, sa, wq, sw, bias, epilogue=ops.EPI_GATE_RES, gate=gate, res=res)
        assert_exact(out, gate_res_ref(lin, gate, res), f"gemm_fp8 gate-residual {M}x{N}x{K}")
