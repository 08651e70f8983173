"""The three passes of csrc/ce_region.hip against their torch expressions evaluated op by op: bit-equal, no tolerance.

The multiplies, adds and subtractions of the references run on the device, one eager torch kernel (one fp32 rounding) per operation.  The
two DIVISIONS by a constant (sum / 16320, byte / 255) are taken on the CPU: torch's device kernel for `tensor / python_scalar` multiplies by
the reciprocal, which is not the correctly rounded quotient the passes (and the CPU) compute."""
import numpy as np
import pytest
import torch

from chronoedit_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def random_mask(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8))


# ----------------------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------------------
def weights_ref(mask_cpu):
    H, W = mask_cpu.shape
    return mask_cpu.view(H // 8, 8, W // 8, 8).sum((1, 3)) / 16320


def tiles_mask(h, w, seed):
    """Whole tiles of 0 and of 255 next to random ones."""
    m = random_mask(h, w, seed)
    m[:8, :8], m[:8, 8:16] = 0, 255
    m[-8:, -8:], m[-8:, :8] = 0, 255
    return m


@pytest.mark.parametrize("name, mask", [("16x24", random_mask(16, 24, 1)), ("40x8", random_mask(40, 8, 2)), ("tiles 32x48", tiles_mask(32, 48, 3)),
                                        ("tiles 24x40", tiles_mask(24, 40, 4)), ("all 255", torch.full((16, 32), 255, dtype=torch.uint8))])
def test_weights_equal_the_box_mean(name, mask):
    want = weights_ref(mask)
    got = ops.region_weights_u8(mask.to(DEV))
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(bits(got), bits(want)), name
    if name.startswith("tiles"):
        assert got[0, 0] == 0.0 and got[0, 1] == 1.0 and got[-1, -1] == 0.0 and got[-1, 0] == 1.0
    if name == "all 255":
        assert bool((got == 1.0).all())
    # a mask that starts one byte into its allocation: the byte-wise body, the same bits
    buf = torch.zeros(mask.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:].copy_(mask.reshape(-1))
    assert torch.equal(bits(ops.region_weights_u8(buf[1:].view(mask.shape))), bits(want)), name


def test_weights_refuse_sizes_that_are_no_multiple_of_8():
    for shape in ((12, 24), (16, 20)):
        with pytest.raises(ops.HipKernelError):
            ops.region_weights_u8(torch.zeros(shape, dtype=torch.uint8, device=DEV))


# ----------------------------------------------------------------------------------------------------------------------------------
# blend
# ----------------------------------------------------------------------------------------------------------------------------------
def blend_ref(x, z, e, w, sigma, bf16_state):
    """The expression of include/chronoedit_hip.h, one torch kernel per operation, sigma a device float."""
    s = sigma.reshape(())
    k = torch.mul(1.0 - s, z)
    k = torch.add(k, torch.mul(s, e))
    a = torch.mul(w, x)
    b = torch.mul(1.0 - w, k)
    out = torch.add(a, b)
    return (out.to(BF).float() if bf16_state else out), k


def blend_case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x, z, e = (torch.randn(shape, generator=g).to(DEV) for _ in range(3))
    w = torch.rand(shape[-2:], generator=g)
    flat = w.view(-1)
    flat[0], flat[-1], flat[flat.numel() // 2] = 0.0, 1.0, 1.0  # lanes with w exactly 0 and exactly 1 in every case
    flat[1] = 0.0
    # the weights a real mask gives: multiples of 1 / 16320
    w = (torch.round(w * 16320) / 16320).to(DEV)
    return x, z, e, w


SHAPES = [(1, 16, 2, 5, 7),        # an odd plane: element by element
          (2, 16, 3, 4, 6),        # batch and frame broadcast, four elements per lane
          (1, 16, 2, 136, 136),    # 591 872 elements: more than 2048 blocks of 256 single elements - the element-wise grid-stride loop runs
          (1, 16, 4, 184, 184)]    # 2 166 784 elements: more than 2048 x 256 groups of four - the vector grid-stride loop runs


@pytest.mark.parametrize("flags", [0, 2], ids=["fp32", "bf16-state"])
@pytest.mark.parametrize("sigma", [0.0, 0.37, 0.9998])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_equals_the_torch_expression(shape, sigma, flags):
    x, z, e, w = blend_case(shape, seed=sum(shape))
    if flags:
        x = x.to(BF).float()  # a bf16 trajectory's sample carries bf16 values
    s = torch.tensor([sigma], dtype=torch.float32, device=DEV)
    want, k = blend_ref(x, z, e, w, s, bool(flags))
    n = x.numel()
    for offset in (0, 1):  # 1: x starts one ELEMENT into its allocation - 4-byte aligned only, the element-wise body
        buf = torch.empty(n + offset, dtype=torch.float32, device=DEV)
        got = buf[offset:].view(shape)
        got.copy_(x)
        assert ops.region_blend_(got, z, e, w, s, bf16_state=bool(flags)) is got
        assert torch.equal(bits(got), bits(want)), (shape, sigma, flags, offset, float((got - want).abs().max()))
        keep, edit = (w == 0).expand(shape), (w == 1).expand(shape)
        assert bool(keep.any()) and bool(edit.any())
        ke = k.to(BF).float() if flags else k
        assert torch.equal(bits(got[edit]), bits(x[edit]))   # w == 1: the sample, bit-unchanged
        assert torch.equal(bits(got[keep]), bits(ke[keep]))  # w == 0: exactly k (as a bf16 value in a bf16 trajectory)
        if sigma == 0.0:
            assert torch.equal(got[keep], (z.to(BF).float() if flags else z)[keep])  # the last step: k == z_src
    assert torch.equal(bits(z), bits(blend_case(shape, seed=sum(shape))[1]))  # the inputs are only read


def test_blend_refusals():
    x, z, e, w = blend_case((1, 16, 2, 4, 6), 0)
    s = torch.zeros(1, device=DEV)
    with pytest.raises(ValueError):
        ops.region_blend_(x, z, e, w[:, :4].contiguous(), s)
    with pytest.raises(ValueError):
        ops.region_blend_(x, z[:, :8].contiguous(), e, w, s)
    with pytest.raises(ValueError):
        ops.region_blend_(x, z, e, w, torch.zeros(2, device=DEV))
    with pytest.raises(TypeError):
        ops.region_blend_(x, z.to(BF), e, w, s)
    with pytest.raises(ops.HipKernelError):
        ops.region_blend_(x.cpu(), z, e, w, s)


# ----------------------------------------------------------------------------------------------------------------------------------
# composite
# ----------------------------------------------------------------------------------------------------------------------------------
def composite_mask(h, w, seed):
    m = random_mask(h, w, seed)
    m[: h // 2, : w // 3] = 0
    m[h // 2:, w // 3: 2 * w // 3] = 255
    return m


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 16, 24), (1, 3, 2, 8, 40), (1, 3, 2, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_composite_equals_the_torch_expression(shape, dtype):
    B, _, F, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    v = (torch.randn(shape, generator=g) * 0.8).to(dtype).to(DEV)
    src = (torch.rand((B, 3, H, W), generator=g) * 2 - 1).to(BF).to(DEV)
    mask = composite_mask(H, W, seed=H * W)
    assert bool((mask == 0).any()) and bool((mask == 255).any()) and bool(((mask > 0) & (mask < 255)).any())
    m = (mask.float() / 255).to(DEV)  # (the division on the CPU: see the module's docstring)
    a = torch.mul(m, v.float())
    b = torch.mul(1.0 - m, src.float().unsqueeze(2))
    want = torch.add(a, b)
    got = ops.region_composite(v, src, mask.to(DEV))
    assert got.dtype == torch.float32 and got.shape == v.shape and got.data_ptr() != v.data_ptr()
    assert torch.equal(bits(got), bits(want)), float((got - want).abs().max())
    keep = (mask == 0).to(DEV).expand(shape)
    assert torch.equal(got[keep], src.float().unsqueeze(2).expand(shape)[keep])      # mask 0: the source, exactly
    edit = (mask == 255).to(DEV).expand(shape)
    assert torch.equal(got[edit], v.float()[edit])                                   # mask 255: the decoded video, exactly
    # a video that starts one element into its allocation: the element-wise body, the same bits
    buf = torch.empty(v.numel() + 1, dtype=dtype, device=DEV)
    v1 = buf[1:].view(shape)
    v1.copy_(v)
    assert torch.equal(bits(ops.region_composite(v1, src, mask.to(DEV))), bits(want))


def test_every_mask_byte_divides_as_the_cpu_does():
    """m = float(byte) / 255.0f for all 256 bytes, read back through a video of ones over a source of zeros."""
    mask = torch.arange(256, dtype=torch.uint8).reshape(8, 32)
    v = torch.ones((1, 3, 1, 8, 32), dtype=torch.float32, device=DEV)
    got = ops.region_composite(v, torch.zeros((1, 3, 8, 32), dtype=BF, device=DEV), mask.to(DEV))
    want = (mask.float() / 255).expand(1, 3, 1, 8, 32)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(want[0, 0, 0], (mask.double() / 255).float())  # ... which is the correctly rounded quotient


def test_composite_refusals():
    v = torch.zeros((1, 3, 2, 8, 16), dtype=BF, device=DEV)
    src, mask = torch.zeros((1, 3, 8, 16), dtype=BF, device=DEV), torch.zeros((8, 16), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.region_composite(v, src[:, :, :4].contiguous(), mask)
    with pytest.raises(ValueError):
        ops.region_composite(v, src, mask[:4].contiguous())
    with pytest.raises(TypeError):
        ops.region_composite(v.to(torch.float16), src, mask)
    with pytest.raises(TypeError):
        ops.region_composite(v, src.float(), mask)
