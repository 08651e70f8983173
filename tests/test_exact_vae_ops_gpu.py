"""ce_conv_igemm_bf16, ce_rms_silu_bf16 and ce_conv3d_gemm_rms_silu_bf16 element by element, at the configurations chronoedit_amd/vae.py sends
(recipes, references and their deliberately wrong variants: tests/exact_util.py; the CPU proofs: tests/test_exact_constructions.py).

conv_igemm: integer-times-power-of-two operands, so every sum is exact in fp32 and the output must equal the header's formula (`conv_frames_f64`,
on the frames as stored, border included) rounded once to bf16 - with a residual, bf16(res + that).  Every launch writes into a buffer full of
a sentinel and the WHOLE buffer is compared: borders, channels beside the slice, frames of the other half and spare rows keep the sentinel.

rms_silu / the fused norm: rows of +-2^k whose sum of squares is exact in any order.  Without SiLU the result equals the kernel's three fp32
operations restated on the CPU (`rms_restate_f32`), bit for bit - on the MI355X the restatement holds as the source states it (sqrtf and the
division are correctly rounded, nothing is contracted, no reciprocal in place of the division).  The restatement works in fp64 and rounds every
operation once to fp32: a host's vectorised fp32 sqrt need not be correctly rounded (one was seen to return 0x1.ce63b4p+4 for 835.171875
where the device and the fp64 route return 0x1.ce63b2p+4), and one such pixel's scale moves an element that sits at a bf16 tie.  With SiLU (`silu_fast`: one v_exp_f32, one v_rcp_f32) the comparison is with bf16 of
the fp64 SiLU of that exactly known pre-activation, within `SILU_ULPS` = 2 bf16 ulps: 1 ulp is the largest distance the CPU's fp32 evaluation of
silu_fast shows from the fp64 SiLU on these launches' data (test_exact_constructions.py asserts the figure), plus 1 for the two hardware
operations; the number of results that differ at all stays within `silu_unequal_allowed` (derived there from the fp32 error of the chain).
Seen on an MI355X: at most 3 of a launch's 215 040 results differ from the fp64 answer (allowance 50), every one of them by 1 ulp."""
import pytest
import torch

import exact_util as X
from exact_util import BF, assert_exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -24576.0  # what every element a kernel must not write holds before the call (exact in bf16)


def _ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from chronoedit_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------------------------------------
# conv_igemm
# ------------------------------------------------------------------------------------------------------------------------------------
def _conv_launch(c, out, **override):
    """The launch of case c into `out` (the whole output buffer, on the device), with the operands sliced as WanVAEEngine._conv slices them."""
    ops = _ops()
    stack = c.in_stack.to(DEV)
    w, b = c.w.to(DEV), c.b.to(DEV)
    lo, hi = c.cout_slice
    res = c.res.to(DEV) if c.res is not None else None
    kw = dict(Cin=c.Cin, Cout=c.Cout, KT=c.KT, KH=c.KH, KW=c.KW, st=c.st, ss=c.ss, H_out=c.H_out, W_out=c.W_out, in_Wp=c.in_Wp, in_off=c.in_off,
              out_Wp=c.out_Wp, out_border=c.out_border, out_cstride=c.out_cstride, out_coff=c.out_coff)
    frames = [stack[i] for i in c.in_idx]
    if "in_frames" in override:
        frames = override.pop("in_frames")(stack)
    kw.update(override)
    ops.conv_igemm(frames, w[lo:hi], b[lo:hi].contiguous(), [out[i] for i in c.out_idx], [res[t] for t in range(c.n_out)] if res is not None else None,
                   **kw)
    torch.cuda.synchronize()


def _sentinel(shape):
    return torch.full(tuple(shape), SENTINEL, dtype=BF, device=DEV)


SINGLE = [n for n in X.CONV_CASES if not n.startswith("time up")]


@pytest.mark.parametrize("name", SINGLE)
def test_conv_igemm_is_exact_and_writes_only_its_elements(name):
    c = X.conv_case(name)
    out = _sentinel(c.out_shape)
    _conv_launch(c, out)
    assert_exact(out, X.conv_place(c, _sentinel(c.out_shape), X.conv_want(c)), f"conv_igemm {name}")


def test_conv_igemm_channel_halves_into_the_even_and_odd_frames_of_one_buffer():
    """time_conv of the temporal upsample: weight and bias pointers in the middle of the pack, out_frames fl[0::2] then fl[1::2]; after the first
    launch the odd frames still hold the sentinel."""
    lo, hi = X.conv_case("time up lo"), X.conv_case("time up hi")
    out = _sentinel(lo.out_shape)
    _conv_launch(lo, out)
    first = X.conv_place(lo, _sentinel(lo.out_shape), X.conv_want(lo))
    assert_exact(out, first, "conv_igemm time up, channels 0..95 -> even frames")
    _conv_launch(hi, out)
    assert_exact(out, X.conv_place(hi, first, X.conv_want(hi)), "conv_igemm time up, channels 96..191 -> odd frames")


def test_conv_igemm_rejections_write_nothing():
    ops = _ops()
    c = X.conv_case("k1 32->16 in 32")
    out = _sentinel(c.out_shape)

    def rejects(**override):
        with pytest.raises(ops.HipKernelError):
            _conv_launch(c, out, **override)

    rejects(Cin=16)                                                   # Cin % 32
    rejects(Cout=12)                                                  # Cout % 8
    rejects(out_cstride=36)                                           # out_cstride % 8
    rejects(out_coff=4)                                               # out_coff % 8
    rejects(in_frames=lambda stack: [stack[0]])                       # (n_out - 1) * st + KT > n_in: two output frames from one
    rejects(st=2)                                                     # ... through the temporal stride: 1 * 2 + 1 > 2
    rejects(in_frames=lambda stack: [stack[i % 2] for i in range(17)])  # 17 frames
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# rms_silu
# ------------------------------------------------------------------------------------------------------------------------------------
RMS_T, RMS_H = 2, 3


def _rms_out(c, border):
    if border:
        return _sentinel((c.T, c.H + 2, c.W + 2, c.C))
    return _sentinel((c.T * c.H * c.W + 3, c.C))  # plain rows and three spare ones


def _rms_launch(c, border, silu, x_stored=None, gamma=None):
    ops = _ops()
    out = _rms_out(c, border)
    ops.rms_silu((c.x_stored if x_stored is None else x_stored).to(DEV), (c.gamma if gamma is None else gamma).to(DEV), out, c.T, c.C, c.H, c.W, 1, border,
                 silu)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("border", [1, 0])
@pytest.mark.parametrize("W", X.RMS_WS)
@pytest.mark.parametrize("C", X.RMS_CS)
def test_rms_norm_equals_the_fp32_restatement_bit_for_bit(C, W, border):
    """Full rows of +-2^k return bf16(+-gamma[c]); rows with n < C live channels the restated three operations; a pixel of zeros returns zeros; the
    output border, the pixels past W and the spare rows keep the sentinel."""
    c = X.rms_case(C, RMS_T, RMS_H, W)
    out = _rms_launch(c, border, False)
    pre = X.rms_restate_f32(c.x, c.gamma)
    assert_exact(out, X.rms_place(_rms_out(c, border), pre.to(BF), border), f"rms_silu C={C} W={W} out_border={border} no SiLU")
    got = (out[:, 1:-1, 1:-1] if border else out[:-3].view(c.T, c.H, c.W, C)).cpu()
    full, zero = c.kind == 0, c.kind == 2
    assert_exact(got[full], (c.x[full].float().sign() * c.gamma).to(BF), "full rows: bf16(+-gamma)")
    assert bool((got[zero] == 0).all()), "a pixel of zeros came out non-zero"


@pytest.mark.parametrize("C", X.RMS_CS)
def test_rms_norm_with_silu_within_the_measured_distance_of_fp64(C):
    """Every W and both output layouts of one width; SILU_ULPS = 2 (1 measured for the fp32 evaluation of silu_fast on the CPU, + 1 for
    v_exp_f32 and v_rcp_f32), and the count of results that differ at all within `silu_unequal_allowed`."""
    unequal, allowed = 0, 0
    for W in X.RMS_WS:
        c = X.rms_case(C, RMS_T, RMS_H, W, diverse=True)
        pre = X.rms_restate_f32(c.x, c.gamma)
        want = X.silu_f64(pre)
        for border in (1, 0):
            out = _rms_launch(c, border, True)
            exp = X.rms_place(_rms_out(c, border), want, border)
            n = int(X.mismatches(out, exp).sum())
            print(f"MEASURED rms_silu C={C} W={W} out_border={border}: {n} of {want.numel()} differ, largest distance {X.ulp_distance(out, exp)} ulp")
            assert_exact(out, exp, f"rms_silu C={C} W={W} out_border={border} SiLU", ulps=X.SILU_ULPS)
            interior = out[:, 1:-1, 1:-1] if border else out[:-3].view(c.T, c.H, c.W, C)
            assert bool((interior[(c.kind == 2).to(DEV)] == 0).all())
            untouched = exp == SENTINEL
            assert bool((out[untouched] == SENTINEL).all()), "rms_silu wrote outside its pixels"  # (bit for bit, whatever the tolerance)
            unequal += n
        allowed += 2 * X.silu_unequal_allowed(pre)
    assert unequal <= allowed, (unequal, allowed)


@pytest.mark.parametrize("C", X.RMS_CS)
def test_rms_norm_ordinary_data_within_one_ulp(C):
    """Random rows and weights against the fp64 formula, no SiLU: within one bf16 ulp element by element (a gamma chunk on the wrong lane is not)."""
    ops = _ops()
    T, H, W = 2, 3, 70
    x, gamma = X.rms_ordinary(C, T, H, W)
    stored = torch.full((T, H + 2, W + 2, C), 96.0, dtype=BF)
    stored[:, 1:-1, 1:-1] = x
    want = X.rms_f64(x, gamma).float().to(BF)
    for border in (1, 0):
        out = _sentinel((T, H + 2, W + 2, C)) if border else _sentinel((T * H * W + 3, C))
        ops.rms_silu(stored.to(DEV), gamma.to(DEV), out, T, C, H, W, 1, border, False)
        exp = X.rms_place(torch.full_like(out, SENTINEL), want, border)
        print(f"MEASURED rms ordinary C={C} out_border={border}: unequal share {X.unequal_share(out, exp):.6f}")
        assert_exact(out, exp, f"rms_silu ordinary C={C} out_border={border}", ulps=1)
        assert bool((out[exp == SENTINEL] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# conv3d_gemm_rms_silu
# ------------------------------------------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(Cin, KT) + f for Cin in X.FUSED_CINS for KT in (1, 3) for f in X.FUSED_FRAMES]


def _bordered(interior, fill=0.0):
    T, H, W, C = interior.shape
    out = torch.full((T, H + 2, W + 2, C), fill, dtype=interior.dtype)
    out[:, 1:-1, 1:-1] = interior
    return out


def _fused_launch(c, silu, two_outputs):
    """-> (normed stack [2 + T + 1 frames], out stack or None), sentinel-filled before the launch."""
    ops = _ops()
    from chronoedit_amd.vae import _ConvPack
    pk = _ConvPack(c.w5.to(DEV), c.b.to(DEV))
    shape = (c.T, c.H + 2, c.W + 2, 96)
    nstack = _sentinel((2 + c.T + 1,) + shape[1:])
    out = _sentinel(shape) if two_outputs else None
    ops.conv3d_gemm_rms_silu(c.in_stack.to(DEV), pk.gemm_weight(), pk.b, nstack[2:2 + c.T], c.gamma.to(DEV), T_out=c.T, H=c.H, W=c.W, Cin=c.Cin, Cout=96,
                             KT=c.KT, silu=silu, out_stack=out, res_stack=c.res.to(DEV) if (two_outputs and c.res is not None) else None)
    torch.cuda.synchronize()
    return nstack, out


def _normed_stack_want(c, normed):
    """Front frames and the slack frame keep the sentinel; the T frames hold `normed` inside a zero border."""
    exp = torch.full((2 + c.T + 1, c.H + 2, c.W + 2, 96), SENTINEL, dtype=BF)
    exp[2:2 + c.T] = _bordered(normed)
    return exp


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("Cin,KT,T,H,W", FUSED_SHAPES)
def test_fused_norm_single_output_is_exact(Cin, KT, T, H, W, silu):
    """out_stack = None: the interior equals the norm of the exactly known y (bit for bit without SiLU, SILU_ULPS with it), borders are zero, the
    front frames of the normed stack keep their sentinel."""
    c = X.fused_case(Cin, KT, T, H, W, "single")
    nstack, _ = _fused_launch(c, silu, False)
    pre = X.fused_pre(c)
    label = f"conv3d_gemm_rms_silu {Cin}->96 KT={KT} {T}x{H}x{W} silu={silu}"
    if not silu:
        assert_exact(nstack, _normed_stack_want(c, pre.to(BF)), label)
        return
    exp = _normed_stack_want(c, X.silu_f64(pre))
    n = int(X.mismatches(nstack, exp).sum())
    print(f"MEASURED {label}: {n} of {pre.numel()} differ, largest distance {X.ulp_distance(nstack, exp.to(DEV))} ulp (allowed {X.silu_unequal_allowed(pre)})")
    assert_exact(nstack, exp, label, ulps=X.SILU_ULPS)
    fixed = (exp == SENTINEL) | (exp == 0)  # sentinel frames, borders and zero pixels: bit for bit
    assert bool((nstack[fixed.to(DEV)] == exp[fixed].to(DEV)).all()), label + ": a border, a zero pixel or a front frame"
    assert n <= X.silu_unequal_allowed(pre), (n, X.silu_unequal_allowed(pre))


@pytest.mark.parametrize("Cin,KT,T,H,W", FUSED_SHAPES)
def test_fused_norm_two_outputs_normalise_the_rounded_residual_sum(Cin, KT, T, H, W):
    """out_stack = bf16(res + y) exactly; normed_stack = the norm of THAT value - not of y, not of the unrounded fp32 sum (three rows that differ
    in bits: test_exact_constructions.py)."""
    c = X.fused_case(Cin, KT, T, H, W, "residual")
    nstack, out = _fused_launch(c, False, True)
    label = f"conv3d_gemm_rms_silu {Cin}->96 KT={KT} {T}x{H}x{W} two outputs"
    assert_exact(out, _bordered(c.v), label + ": out_stack")
    assert_exact(nstack, _normed_stack_want(c, X.fused_pre(c).to(BF)), label + ": normed_stack")


@pytest.mark.parametrize("Cin,KT", [(32, 3), (96, 1), (192, 3)])
def test_fused_norm_ordinary_data_within_one_ulp(Cin, KT):
    """Integer weights on every tap, data in the front frames, a dyadic bias: y = bf16(conv + bias) is known exactly and the normalised output lies
    within one bf16 ulp of the fp64 norm of that y."""
    c = X.fused_case(Cin, KT, 2, 5, 7, "ordinary")
    nstack, out = _fused_launch(c, False, True)
    assert_exact(out, _bordered(c.y), f"conv3d_gemm_rms_silu ordinary {Cin}->96 KT={KT}: out_stack")
    exp = _normed_stack_want(c, X.rms_f64(c.y, c.gamma).float().to(BF))
    print(f"MEASURED fused ordinary {Cin}->96 KT={KT}: unequal share {X.unequal_share(nstack, exp):.6f}")
    assert_exact(nstack, exp, f"conv3d_gemm_rms_silu ordinary {Cin}->96 KT={KT}: normed_stack", ulps=1)
    fixed = (exp == SENTINEL) | (exp == 0)
    assert bool((nstack[fixed.to(DEV)] == exp[fixed].to(DEV)).all())
