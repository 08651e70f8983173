"""The VAE convolution and data-movement kernels element by element (tests/exact_util.py): integer-times-power-of-two activations and
weights make every convolution sum exact in fp32, so each interior element must equal the fp64 convolution (causal front frames, zero
spatial padding) plus bias, rounded once to bf16 - and, with a residual, bf16(res + that).  Borders must come back zero.
upsample2x and zero_border must equal their torch counterparts bit for bit."""
import pytest
import torch

from exact_util import BF, assert_exact, bf16_rne, conv_frames_f64, int_rows, int_vector

pytestmark = pytest.mark.gpu


def _conv_f64(x, w):
    """x [n_in, H, W, Cin] (bf16, the first KT - 1 frames are the causal front frames), w [Cout, Cin, KT, 3, 3] -> fp64 [T, H, W, Cout]: the
    general reference of exact_util.py on the zero-bordered frames (9 KT shifted fp64 GEMMs per output frame, on the device; exact for this
    data; no library convolution algorithm in the way)."""
    n_in, H, W, Cin = x.shape
    Cout, _, KT = w.shape[:3]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))  # zero spatial padding: the stored frame's border
    wp = w.permute(0, 2, 3, 4, 1).reshape(Cout, KT * 9, Cin)
    return conv_frames_f64([xp[i] for i in range(n_in)], wp, None, n_in - KT + 1, KT=KT, KH=3, KW=3, st=1, ss=1, H_out=H, W_out=W, in_off=0)


def _operands(KT, Cin, Cout, T, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n_in = T + KT - 1
    x = int_rows(n_in * H * W, Cin, g, emin=-1, emax=-1).view(n_in, H, W, Cin)   # one scale: the sum of a position mixes taps
    w = int_rows(Cout, Cin * KT * 9, g, emin=-2, emax=2).view(Cout, KT, 3, 3, Cin).permute(0, 4, 1, 2, 3).contiguous()
    b = int_vector(Cout, g)
    return x, w, b, g


def _borders_zero(t, what):
    for i, border in enumerate((t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1])):
        assert_exact(border, torch.zeros_like(border), f"{what} border {i}")


# the shapes of test_vae_gpu.py's conv3d_gemm test: both macro tiles and the slab kernel (n_tile 1), n_tile 0 / 2 / 96 / 128 / 256,
# KT 1 and 3, with and without residual, frames smaller than one 512-position tile, ragged last tiles
CONV_CASES = [(3, 192, 192, 2, 24, 40, False, 0), (3, 384, 384, 1, 22, 30, True, 256), (1, 384, 192, 3, 16, 24, False, 256),
              (3, 192, 384, 4, 45, 80, True, 128), (3, 96, 96, 2, 40, 64, True, 0), (1, 192, 96, 3, 30, 44, False, 0),
              (3, 96, 192, 1, 20, 28, False, 128), (3, 384, 384, 2, 30, 50, True, 0), (3, 96, 96, 2, 40, 64, True, 96),
              (3, 96, 96, 1, 3, 5, True, 1), (1, 96, 96, 2, 9, 7, False, 1), (3, 192, 96, 3, 33, 47, True, 1), (3, 96, 96, 4, 90, 160, False, 1),
              (3, 96, 96, 2, 40, 64, True, 2), (1, 192, 96, 3, 30, 44, False, 2), (3, 32, 96, 4, 24, 40, False, 0), (3, 32, 96, 1, 20, 36, False, 2)]


@pytest.mark.parametrize("KT,Cin,Cout,T,H,W,with_res,n_tile", CONV_CASES)
def test_conv3d_gemm_and_conv_igemm_are_exact(KT, Cin, Cout, T, H, W, with_res, n_tile):
    from chronoedit_amd import ops
    from chronoedit_amd.vae import Frames, _ConvPack
    dev = torch.device("cuda:0")
    x, w, b, g = _operands(KT, Cin, Cout, T, H, W, KT * 1000 + Cin + Cout + T + H)
    want = bf16_rne(_conv_f64(x, w) + b.double())
    f = Frames(T, H, W, Cin, dev, front=KT - 1)
    f.stack[:T + KT - 1, 1:-1, 1:-1] = x
    pk = _ConvPack(w, b)
    res = None
    if with_res:
        res = Frames(T, H, W, Cout, dev)
        res.data[:, 1:-1, 1:-1] = (torch.randn(T, H, W, Cout, device=dev, generator=g) * 64).to(BF)
        want = torch.add(res.data[:, 1:-1, 1:-1].float(), want.float()).to(BF)
    out = Frames(T, H, W, Cout, dev)
    out.data.fill_(7.0)
    ops.conv3d_gemm(f.stack, pk.gemm_weight(), pk.b, out.data, res.data if res is not None else None, T_out=T, H=H, W=W, Cin=Cin, Cout=Cout,
                    KT=KT, n_tile=n_tile)
    label = f"conv3d_gemm KT={KT} {Cin}->{Cout} {T}x{H}x{W} res={with_res} n_tile={n_tile}"
    assert_exact(out.data[:, 1:-1, 1:-1], want, label)
    _borders_zero(out.data, label)
    old = Frames(T, H, W, Cout, dev)
    old.data.fill_(7.0)
    old.data[:, 1:-1, 1:-1] = 0
    ops.conv_igemm([f.stack[i] for i in range(T + KT - 1)], pk.w, pk.b, old.frame_list(), res.frame_list() if res is not None else None,
                   Cin=Cin, Cout=Cout, KT=KT, KH=3, KW=3, st=1, ss=1, H_out=H, W_out=W, in_Wp=W + 2, in_off=0, out_Wp=W + 2, out_border=1,
                   out_cstride=Cout)
    assert_exact(old.data[:, 1:-1, 1:-1], want, "conv_igemm " + label)
    assert bool((old.data[:, 0] == 7.0).all() and (old.data[:, :, -1] == 7.0).all()), "conv_igemm wrote the border"


@pytest.mark.parametrize("KT,Cout,T,H,W", [(3, 3, 4, 40, 128), (3, 3, 1, 13, 70), (1, 3, 2, 8, 64), (3, 4, 2, 17, 129), (3, 1, 1, 3, 5)])
def test_conv3d_head_is_exact(KT, Cout, T, H, W):
    """The decoder's 96 -> <= 4 head conv: interior exact, pad channels Cout..7 zero, border untouched."""
    from chronoedit_amd import ops
    from chronoedit_amd.vae import Frames, _ConvPack
    dev = torch.device("cuda:0")
    Cin = 96
    x, w, b, _ = _operands(KT, Cin, Cout, T, H, W, KT * 100 + Cout * 10 + T + H)
    want = bf16_rne(_conv_f64(x, w) + b.double())
    f = Frames(T + KT - 1, H, W, Cin, dev)
    f.data[:, 1:-1, 1:-1] = x
    pk = _ConvPack(w, b)
    out = Frames(T, H, W, 8, dev, zero=False)
    out.data.fill_(7.0)
    ops.conv3d_head(f.frame_list(), pk.w, pk.b, out.frame_list(), Cin=Cin, Cout=Cout, KT=KT, H_out=H, W_out=W, in_Wp=W + 2, out_Wp=W + 2,
                    out_border=1, out_cstride=8)
    label = f"conv3d_head KT={KT} 96->{Cout} {T}x{H}x{W}"
    assert_exact(out.data[:, 1:-1, 1:-1, :Cout], want, label)
    pad = out.data[:, 1:-1, 1:-1, Cout:]
    assert_exact(pad, torch.zeros_like(pad), label + " pad channels")
    assert bool((out.data[:, 0] == 7.0).all() and (out.data[:, :, -1] == 7.0).all()), label + ": border written"


@pytest.mark.parametrize("T,C,H,W", [(2, 96, 9, 70), (1, 384, 4, 17), (3, 192, 45, 80), (1, 8, 1, 1)])
def test_upsample2x_equals_repeat_interleave(T, C, H, W):
    from chronoedit_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T + C + H + W)
    x = torch.randn(T, H + 2, W + 2, C, device="cuda", generator=g).to(BF)
    out = torch.full((T, 2 * H + 2, 2 * W + 2, C), 7.0, dtype=BF, device="cuda")
    ops.upsample2x(x, out, T, C, H, W)
    want = x[:, 1:-1, 1:-1].repeat_interleave(2, 1).repeat_interleave(2, 2)
    assert_exact(out[:, 1:-1, 1:-1], want, f"upsample2x {T}x{C}x{H}x{W}")
    assert bool((out[:, 0] == 7.0).all() and (out[:, -1] == 7.0).all() and (out[:, :, 0] == 7.0).all() and (out[:, :, -1] == 7.0).all())


@pytest.mark.parametrize("T,H,W,C,ld", [(2, 9, 70, 96, 96), (1, 4, 17, 384, 392), (3, 45, 80, 8, 16), (1, 1, 1, 8, 8)])
def test_zero_border_equals_slicing(T, H, W, C, ld):
    from chronoedit_amd import ops
    g = torch.Generator(device="cuda").manual_seed(T + H + W + C)
    fr = torch.randn(T, H + 2, W + 2, ld, device="cuda", generator=g).to(BF)
    want = fr.clone()
    want[:, 0, :, :C] = 0
    want[:, -1, :, :C] = 0
    want[:, :, 0, :C] = 0
    want[:, :, -1, :C] = 0
    ops.zero_border(fr, T, H, W, C)
    assert_exact(fr, want, f"zero_border {T}x{H}x{W} C={C} ld={ld}")  # interiors and the channels beyond C untouched
