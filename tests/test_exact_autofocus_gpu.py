"""The two passes of csrc/ce_autofocus.hip against the CPU expressions of chronoedit_amd/autofocus.py: bit-equal, no tolerance."""
import numpy as np
import pytest
import torch

from chronoedit_amd import autofocus, focus, ops
from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GARBAGE = [-7, 1 << 30, 123456, -(1 << 31), 99]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------------------
# bbox
# ----------------------------------------------------------------------------------------------------------------------------------
def check_bbox(mask_cpu, view=None):
    """mask_cpu uint8 [H, W]; view: a function that takes the device copy to the view under test (and the CPU copy to the same view)."""
    dev = mask_cpu.to(DEV)
    if view is not None:
        dev, mask_cpu = view(dev), view(mask_cpu)
    out = torch.tensor(GARBAGE, dtype=torch.int32, device=DEV)  # the call initialises it
    got = ops.autofocus_bbox_u8(dev, out=out)
    want = autofocus.bbox_counts(mask_cpu)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu(), want), (got.tolist(), want.tolist())
    box, n = autofocus.mask_box(dev)
    assert box == focus.mask_bbox(mask_cpu) and n == int((mask_cpu > 0).sum())
    return box, n


def sparse_mask(H, W, seed, points=6):
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint8)
    m[rng.integers(0, H, points), rng.integers(0, W, points)] = rng.integers(1, 256, points)
    return torch.from_numpy(m)


def dense_mask(H, W, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, 2, (H, W), dtype=np.uint8) * rng.integers(0, 256, (H, W), dtype=np.uint8))


@pytest.mark.parametrize("H,W", [(37, 52), (150, 203), (5, 1), (7, 3), (9, 16), (9, 17), (3000, 40), (3, 4200), (2, 70001)])
def test_bbox_equals_the_cpu_expression(H, W):
    assert check_bbox(torch.zeros(H, W, dtype=torch.uint8)) == (None, 0)
    assert check_bbox(torch.full((H, W), 255, dtype=torch.uint8)) == ((0, 0, W, H), H * W)
    for y, x in {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}:
        for value in (1, 255):
            m = torch.zeros(H, W, dtype=torch.uint8)
            m[y, x] = value
            assert check_bbox(m) == ((x, y, x + 1, y + 1), 1)
    for seed in range(3):
        check_bbox(sparse_mask(H, W, seed))
        check_bbox(dense_mask(H, W, 10 + seed))


@pytest.mark.parametrize("rows,cols", [((40, 90), (77, 130)), ((0, 150), (1, 203)), ((149, 150), (0, 16)), ((3, 120), (16, 33)), ((10, 20), (200, 203))])
def test_bbox_of_a_view_with_a_pitch(rows, cols):
    """A box's view of a 203-wide mask: pitch 203 > W, every row starts at another alignment; what lies outside the view does not count."""
    view = lambda m: m[rows[0]:rows[1], cols[0]:cols[1]]
    for seed in range(2):
        m = dense_mask(150, 203, 20 + seed)
        check_bbox(m, view)
        inside = torch.zeros(150, 203, dtype=torch.uint8)
        view(inside)[...] = view(sparse_mask(150, 203, 30 + seed, points=40))
        outside = torch.full((150, 203), 255, dtype=torch.uint8)
        view(outside)[...] = view(inside)
        assert check_bbox(outside, view) == check_bbox(inside, view)
    empty_inside = torch.full((150, 203), 255, dtype=torch.uint8)
    view(empty_inside)[...] = 0
    assert check_bbox(empty_inside, view) == (None, 0)


def test_bbox_of_a_mask_one_byte_into_its_allocation():
    m = dense_mask(37, 52, 40)
    buf = torch.zeros(m.numel() + 1, dtype=torch.uint8, device=DEV)
    buf[1:].copy_(m.reshape(-1))
    assert torch.equal(ops.autofocus_bbox_u8(buf[1:].view(37, 52)).cpu(), autofocus.bbox_counts(m))


def test_bbox_refuses_what_it_cannot_read():
    with pytest.raises(ValueError):
        ops.autofocus_bbox_u8(torch.zeros(8, 8, dtype=torch.uint8, device=DEV).t())
    with pytest.raises(TypeError):
        ops.autofocus_bbox_u8(torch.zeros(8, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(ops.HipKernelError):
        ops.autofocus_bbox_u8(torch.zeros(8, 8, dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------------------------------------------
# restart
# ----------------------------------------------------------------------------------------------------------------------------------
SRC = (203, 150)
BOXES = {"interior": (60, 40, 156, 104), "left top": (0, 0, 126, 84), "right": (77, 20, 203, 104), "bottom": (30, 66, 156, 150),
         "narrow": (198, 146, 203, 150), "whole": (0, 0, 203, 150)}


def schedule_sigma():
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers")
    sch.set_timesteps(8)
    return float(sch.sigmas[2])


@pytest.fixture(scope="module")
def tensors():
    g = torch.Generator().manual_seed(6)
    return {hw: (torch.randn(32, *hw, generator=g), torch.randn(32, *hw, generator=g)) for hw in ((8, 12), (9, 13))}


@pytest.mark.parametrize("bf16_state", [False, True])
@pytest.mark.parametrize("hw", [(8, 12), (9, 13)])
@pytest.mark.parametrize("box", list(BOXES))
def test_restart_equals_the_cpu_expression(tensors, box, hw, bf16_state):
    x0, eps = tensors[hw]
    tabs = autofocus.restart_tables(BOXES[box], SRC, hw)
    dev_tabs = tuple(t.to(DEV) for t in tabs)
    for s in (0.0, 1.0, schedule_sigma()):
        want = autofocus.restart(x0, eps, tabs, s, bf16_state)
        got = ops.autofocus_restart(x0.to(DEV), eps.to(DEV), dev_tabs, s, bf16_state)
        assert got.dtype == torch.float32 and got.shape == x0.shape
        assert torch.equal(bits(got), bits(want)), (box, hw, s)
        via_module = autofocus.restart(x0.to(DEV), eps.to(DEV), tabs, s, bf16_state)  # (the module routes a device tensor to the kernel)
        assert torch.equal(bits(via_module), bits(want))
    if box == "whole":  # the identity box with s = 0 returns x0 exactly
        assert torch.equal(bits(ops.autofocus_restart(x0.to(DEV), eps.to(DEV), dev_tabs, 0.0, False)), bits(x0))
    elif box != "narrow":  # (a box inside the last cell: every sample is clamped to it)
        assert any(bool(t.any()) for t in (tabs[2], tabs[5]))  # the case does interpolate


def test_restart_of_a_5d_latent_and_its_refusals(tensors):
    x0, eps = tensors[(8, 12)]
    x5, e5 = x0.view(1, 16, 2, 8, 12), eps.view(1, 16, 2, 8, 12)
    tabs = autofocus.restart_tables(BOXES["interior"], SRC, (8, 12))
    dev_tabs = tuple(t.to(DEV) for t in tabs)
    got = ops.autofocus_restart(x5.to(DEV), e5.to(DEV), dev_tabs, 0.5)
    assert got.shape == x5.shape and torch.equal(bits(got), bits(autofocus.restart(x5, e5, tabs, 0.5)))
    with pytest.raises(ValueError):
        ops.autofocus_restart(x5.to(DEV), e5.to(DEV)[:, :8], dev_tabs, 0.5)
    with pytest.raises(ValueError):
        ops.autofocus_restart(x5.to(DEV), e5.to(DEV), dev_tabs[:2] + (dev_tabs[2][:-1],) + dev_tabs[3:], 0.5)
    with pytest.raises(TypeError):
        ops.autofocus_restart(x5.to(DEV), e5.to(DEV), (dev_tabs[0].long(),) + dev_tabs[1:], 0.5)
