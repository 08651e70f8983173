"""Region-limited edits, host side (chronoedit_amd/region.py): the mask rules, the box-mean weights on the CPU, the sigma_next table, and the
C ABI's declarations.  No GPU."""
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import hiplib, region

H, W = 16, 24
ENTRY_POINTS = ("ce_region_weights_u8", "ce_region_blend_f32", "ce_region_composite")


def random_mask(h=H, w=W, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8))


def test_normalize_mask_uint8_and_bool():
    m = random_mask()
    for given in (m, m.numpy()):
        out = region.normalize_mask(given, H, W)
        assert out.dtype == torch.uint8 and out.device.type == "cpu" and out.is_contiguous() and torch.equal(out, m)
    assert region.normalize_mask(m, H, W).data_ptr() != m.data_ptr()  # a copy: the caller may go on painting its mask
    b = m > 100
    for given in (b, b.numpy()):
        out = region.normalize_mask(given, H, W)
        assert out.dtype == torch.uint8 and torch.equal(out, b.to(torch.uint8) * 255)
    assert set(region.normalize_mask(b, H, W).unique().tolist()) == {0, 255}


def test_normalize_mask_float_rounds_255_m():
    """round(255 * m), half to even, in float64: k / 255 comes back as k for every byte, from fp32 and from fp64."""
    k = torch.arange(H * W) % 256
    for dt in (torch.float32, torch.float64):
        f = (k.to(torch.float64) / 255).to(dt).reshape(H, W)
        for given in (f, f.numpy()):
            out = region.normalize_mask(given, H, W)
            assert out.dtype == torch.uint8 and torch.equal(out.reshape(-1), k.to(torch.uint8))
    bf = torch.rand(H, W, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    assert torch.equal(region.normalize_mask(bf, H, W), torch.round(bf.double() * 255).to(torch.uint8))
    f = torch.full((H, W), 0.5, dtype=torch.float64)  # 127.5 is a tie: to even
    f[0, 0], f[0, 1], f[0, 2] = 0.0, 1.0, 0.75  # 191.25
    out = region.normalize_mask(f, H, W)
    assert (out[1, 1], out[0, 0], out[0, 1], out[0, 2]) == (128, 0, 255, 191)


def test_normalize_mask_pil_and_resize_rule():
    m = random_mask()
    pil = Image.fromarray(m.numpy())  # mode "L", already at the edit's size: the bytes
    assert torch.equal(region.normalize_mask(pil, H, W), m)
    rgb = Image.fromarray(np.random.default_rng(1).integers(0, 256, size=(H, W, 3), dtype=np.uint8))
    assert torch.equal(region.normalize_mask(rgb, H, W), torch.from_numpy(np.array(rgb.convert("L"))))
    one_bit = Image.fromarray(m.numpy() > 100)  # mode "1"
    assert torch.equal(region.normalize_mask(one_bit, H, W), (m > 100).to(torch.uint8) * 255)
    big = Image.fromarray(random_mask(50, 70, seed=2).numpy())  # another size: resized on the host, bilinear
    out = region.normalize_mask(big, H, W)
    assert tuple(out.shape) == (H, W)
    assert torch.equal(out, torch.from_numpy(np.array(big.convert("L").resize((W, H), Image.BILINEAR))))
    assert not torch.equal(out, torch.from_numpy(np.array(big.convert("L").resize((W, H), Image.NEAREST))))


def test_normalize_mask_refusals():
    m = random_mask()
    for bad in (m[:8], m.T.contiguous(), m[None], m.numpy()[:, :8], torch.zeros(H, W + 8), np.zeros((W, H), dtype=bool)):
        with pytest.raises(ValueError):
            region.normalize_mask(bad, H, W)
    for bad in (torch.full((H, W), 1.5), torch.full((H, W), -0.1), torch.full((H, W), float("nan")), np.full((H, W), 255.0)):
        with pytest.raises(ValueError):
            region.normalize_mask(bad, H, W)
    for bad in (m.to(torch.int32), m.numpy().astype(np.int64), [[0] * W] * H, None):
        with pytest.raises(TypeError):
            region.normalize_mask(bad, H, W)


@pytest.mark.parametrize("shape", [(16, 24), (40, 8), (64, 96)])
def test_latent_weights_on_the_cpu(shape):
    h, w = shape[0] // 8, shape[1] // 8
    m = random_mask(*shape, seed=sum(shape))
    m[:8, :8] = 0
    m[-8:, -8:] = 255
    got = region.latent_weights(m)
    want = m.view(h, 8, w, 8).sum((1, 3)) / 16320
    assert got.dtype == torch.float32 and tuple(got.shape) == (h, w)
    assert torch.equal(got, want)
    assert got[0, 0] == 0.0 and got[-1, -1] == 1.0
    # the sum is an integer: float64 arithmetic rounded once gives the same fp32
    assert torch.equal(got, (m.double().view(h, 8, w, 8).sum((1, 3)) / 16320).float())


def test_latent_weights_all_edit_and_all_keep():
    ones = region.latent_weights(torch.full((H, W), 255, dtype=torch.uint8))
    zeros = region.latent_weights(torch.zeros((H, W), dtype=torch.uint8))
    assert torch.equal(ones, torch.ones(H // 8, W // 8)) and torch.equal(zeros, torch.zeros(H // 8, W // 8))
    with pytest.raises(ValueError):
        region.latent_weights(torch.zeros((12, 24), dtype=torch.uint8))
    with pytest.raises(ValueError):
        region.latent_weights(torch.zeros((16, 24), dtype=torch.float32))


@pytest.mark.parametrize("steps, grid", [(6, "sibling"), (8, "diffusers"), (50, "sibling")])
def test_sigma_next_table(steps, grid):
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid=grid)
    sch.set_timesteps(steps)
    t = region.sigma_next_table(sch)
    assert t.dtype == torch.float32 and tuple(t.shape) == (steps,)
    assert torch.equal(t, sch.sigmas[1:])
    assert t[-1] == 0.0 and bool((t[:-1] > 0).all()) and bool((t[1:] < t[:-1]).all())


def test_the_c_abi_declares_the_three_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_region_")] == list(ENTRY_POINTS)
    assert "ce_region.hip" in hiplib.SOURCES
