"""Auto-focused edits, the part that needs no GPU: the warm start's tables, the CPU expressions of the two device passes, the tail schedule
and the wiring."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from chronoedit_amd import autofocus, focus, hiplib
from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler, unipc_coefficients

ENTRY_POINTS = ("ce_autofocus_bbox_u8", "ce_autofocus_restart_f32")
SOURCES = [(4032, 3024), (3024, 4032), (1280, 720), (1281, 721), (203, 150), (150, 203), (97, 64), (96, 65), (64, 48), (50, 70), (17, 5), (1, 1),
           (2000, 100), (100, 2000)]  # the source sizes of tests/test_focus_cpu.py
EDITS = [(1280, 720), (96, 64), (64, 96), (16, 16)]


def bboxes(SW, SH):
    w, h = max(1, SW // 5), max(1, SH // 7)
    return [(0, 0, w, h), (SW - w, 0, SW, h), (0, SH - h, w, SH), (SW - w, SH - h, SW, SH), (SW // 3, SH // 3, SW // 3 + 1, SH // 3 + 1), (0, 0, SW, SH)]


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def brute_axis(lo, extent, n, src):
    """The rule of the tables, cell by cell in exact rationals."""
    rows = []
    for x in range(n):
        centre = lo + (Fraction(x) + Fraction(1, 2)) * Fraction(extent, n)  # in photo pixels
        u = centre * Fraction(n, src) - Fraction(1, 2)  # in cells of the scout's grid
        u = max(Fraction(0), min(u, Fraction(n - 1)))
        i0 = u.numerator // u.denominator
        rows.append((i0, min(i0 + 1, n - 1), np.float32(float(u - i0))))
    return rows


def test_tables_equal_the_brute_force_rule():
    seen_crop = 0
    for src in SOURCES:
        for W, H in EDITS:
            h, w = H // 8, W // 8
            for bbox in bboxes(*src):
                box, reason = focus.focus_box(bbox, src, (W, H), 0.25)
                l, t, r, b = box
                ix0, ix1, fx, iy0, iy1, fy = autofocus.restart_tables(box, src, (h, w))
                assert (ix0.dtype, ix1.dtype, fx.dtype) == (torch.int32, torch.int32, torch.float32) and len(ix0) == len(ix1) == len(fx) == w
                assert len(iy0) == len(iy1) == len(fy) == h
                for tabs, want in (((ix0, ix1, fx), brute_axis(l, r - l, w, src[0])), ((iy0, iy1, fy), brute_axis(t, b - t, h, src[1]))):
                    got = list(zip(tabs[0].tolist(), tabs[1].tolist(), tabs[2].numpy()))
                    assert all(g[0] == x[0] and g[1] == x[1] and g[2] == x[2] for g, x in zip(got, want)), (src, (W, H), box)
                    n = len(want)
                    assert all(0 <= a <= b_ <= n - 1 and b_ - a <= 1 for a, b_, _ in got)  # the indices stay in range
                    assert all(0.0 <= f < 1.0 for _, _, f in got)
                seen_crop += box != (0, 0) + src
    assert seen_crop > 50


@pytest.mark.parametrize("src", SOURCES)
def test_the_whole_photo_gives_the_identity(src):
    for h, w in ((8, 12), (9, 13), (90, 160)):
        ix0, ix1, fx, iy0, iy1, fy = autofocus.restart_tables((0, 0) + src, src, (h, w))
        assert ix0.tolist() == list(range(w)) and iy0.tolist() == list(range(h))
        assert not fx.any() and not fy.any()
        assert ix1.tolist() == [min(x + 1, w - 1) for x in range(w)] and iy1.tolist() == [min(y + 1, h - 1) for y in range(h)]


def test_a_box_at_each_photo_edge_clamps():
    SW, SH, h, w = 203, 150, 8, 12
    # a box narrower than a cell of the scout's grid: its first centre lies left of / above the first cell centre, its last one right of / below the last
    left = autofocus.restart_tables((0, 40, 6, 44), (SW, SH), (h, w))
    assert left[0][0] == 0 and left[2][0] == 0.0
    top = autofocus.restart_tables((40, 0, 46, 4), (SW, SH), (h, w))
    assert top[3][0] == 0 and top[5][0] == 0.0
    right = autofocus.restart_tables((SW - 6, 40, SW, 44), (SW, SH), (h, w))
    assert right[0][-1] == right[1][-1] == w - 1 and right[2][-1] == 0.0
    bottom = autofocus.restart_tables((40, SH - 4, 46, SH), (SW, SH), (h, w))
    assert bottom[3][-1] == bottom[4][-1] == h - 1 and bottom[5][-1] == 0.0
    with pytest.raises(ValueError):
        autofocus.restart_tables((0, 0, SW + 1, SH), (SW, SH), (h, w))


# ---- the CPU expressions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16_state", [False, True])
def test_restart_equals_a_per_element_loop(bf16_state):
    g = torch.Generator().manual_seed(4)
    x0, eps = torch.randn(16, 2, 8, 12, generator=g), torch.randn(16, 2, 8, 12, generator=g)
    tabs = autofocus.restart_tables((77, 0, 203, 84), (203, 150), (8, 12))
    ix0, ix1, fx, iy0, iy1, fy = (t.numpy() for t in tabs)
    s = np.float32(0.9375 / 1.7)
    got = autofocus.restart(x0, eps, tabs, float(s), bf16_state)
    a, e = x0.numpy(), eps.numpy()
    want = np.empty_like(a)
    one = np.float32(1.0)
    for c in range(16):
        for f in range(2):
            for y in range(8):
                for x in range(12):
                    a00, a01 = a[c, f, iy0[y], ix0[x]], a[c, f, iy0[y], ix1[x]]
                    a10, a11 = a[c, f, iy1[y], ix0[x]], a[c, f, iy1[y], ix1[x]]
                    top = np.float32(a00 + np.float32(fx[x] * np.float32(a01 - a00)))
                    bot = np.float32(a10 + np.float32(fx[x] * np.float32(a11 - a10)))
                    v = np.float32(top + np.float32(fy[y] * np.float32(bot - top)))
                    want[c, f, y, x] = np.float32(np.float32(np.float32(one - s) * v) + np.float32(s * e[c, f, y, x]))
    want = torch.from_numpy(want)
    if bf16_state:
        want = want.to(torch.bfloat16).float()
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert any(f not in (0.0,) for f in fx) and any(f != 0.0 for f in fy)  # the case does interpolate


def test_restart_identity_and_pure_noise():
    g = torch.Generator().manual_seed(5)
    x0, eps = torch.randn(32, 9, 13, generator=g), torch.randn(32, 9, 13, generator=g)
    ident = autofocus.restart_tables((0, 0, 203, 150), (203, 150), (9, 13))
    assert torch.equal(autofocus.restart(x0, eps, ident, 0.0), x0)
    assert torch.equal(autofocus.restart(x0, eps, ident, 1.0), eps)


def check_bbox(mask):
    t = torch.from_numpy(mask) if isinstance(mask, np.ndarray) else mask
    got = autofocus.bbox_counts(t)
    assert got.dtype == torch.int32 and tuple(got.shape) == (5,)
    box, n = autofocus.mask_box(t)
    assert box == focus.mask_bbox(t) and n == int((t > 0).sum())
    H, W = t.shape
    assert got.tolist() == (list(box) + [n] if box is not None else [W, H, 0, 0, 0])
    return box, n


def test_bbox_equals_mask_bbox():
    H, W = 37, 52
    assert check_bbox(np.zeros((H, W), np.uint8)) == (None, 0)
    assert check_bbox(np.full((H, W), 255, np.uint8)) == ((0, 0, W, H), H * W)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        for value in (1, 255):  # both count
            m = np.zeros((H, W), np.uint8)
            m[y, x] = value
            assert check_bbox(m) == ((x, y, x + 1, y + 1), 1)
    rng = np.random.default_rng(8)
    for _ in range(20):
        m = np.zeros((H, W), np.uint8)
        m[rng.integers(0, H, 5), rng.integers(0, W, 5)] = rng.integers(1, 256, 5)
        check_bbox(m)
    big = torch.from_numpy(rng.integers(0, 2, (150, 203), dtype=np.uint8) * rng.integers(0, 256, (150, 203), dtype=np.uint8))
    view = big[40:90, 77:130]  # a pitched view: reduced where it lies
    assert not view.is_contiguous()
    check_bbox(view)
    assert autofocus.bbox_counts(view).tolist() == autofocus.bbox_counts(view.contiguous()).tolist()


def test_plan_equals_the_host_plan():
    mask = np.zeros((150, 203), np.uint8)
    mask[20:60, 110:170] = np.random.default_rng(1).integers(0, 256, (40, 60), dtype=np.uint8)
    assert autofocus.plan(torch.from_numpy(mask), (96, 64), 0.25) == focus.plan((203, 150), mask, 64, 96, 0.25)
    rep = autofocus.plan(torch.from_numpy(mask), (96, 64), 0.25)
    assert rep["reason"] == "ok" and autofocus.worth_focusing(rep)
    whole = autofocus.plan(torch.full((150, 203), 255, dtype=torch.uint8), (96, 64), 0.25)
    assert whole["box"] == (0, 0, 203, 150) and not autofocus.worth_focusing(whole)
    assert not autofocus.worth_focusing(autofocus.plan(torch.zeros((150, 203), dtype=torch.uint8), (96, 64), 0.25))  # "empty"
    from PIL import Image
    small = torch.from_numpy(mask[:64, 100:196].copy())
    lifted = autofocus.lift_mask(small, (203, 150))
    assert np.array_equal(lifted.numpy(), np.array(Image.fromarray(small.numpy()).resize((203, 150), Image.BILINEAR)))
    assert autofocus.lift_mask(small, (96, 64)) is not small and torch.equal(autofocus.lift_mask(small, (96, 64)), small)


# ---- the tail schedule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,begins", [(2, (1,)), (8, (1, 2, 5, 7)), (50, (1, 3, 25, 49))])
def test_the_tail_schedule(n, begins):
    full = FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers")
    full.set_timesteps(n)
    same = FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers")
    same.set_timesteps(n, begin=0)
    assert torch.equal(same.timesteps, full.timesteps) and torch.equal(same.sigmas, full.sigmas) and np.array_equal(same.coef, full.coef)
    assert same.num_inference_steps == n
    for b in begins:
        tail = FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers")
        tail.set_timesteps(n, begin=b)
        assert tail.num_inference_steps == n - b
        assert torch.equal(tail.timesteps, full.timesteps[b:]) and torch.equal(tail.sigmas, full.sigmas[b:])
        assert tail.model_outputs == [None, None] and tail.last_sample is None and tail.step_index is None
        assert tail.coef.shape == (n - b, 10)
        assert np.array_equal(tail.coef, unipc_coefficients(full.sigmas[b:].numpy().astype(np.float64), 2, True, ()))
        assert np.array_equal(tail.coef[:, 1], full.coef[b:, 1])  # the sigmas
        assert tail.coef[0, 2] == 0.0 and not tail.coef[0, 3:7].any()  # row 0: no corrector ...
        assert tail.coef[0, 9] == 0.0  # ... and an order-1 predictor (no weight on a history that is not there)
        for j in range(2, n - b):
            assert np.array_equal(tail.coef[j], full.coef[b + j]), (n, b, j)
    for bad in (-1, n):
        with pytest.raises(ValueError):
            full.set_timesteps(n, begin=bad)


# ---- the wiring --------------------------------------------------------------------------------------------------------------------
def test_the_c_abi_declares_the_two_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_autofocus_")] == list(ENTRY_POINTS)
    assert "ce_autofocus.hip" in hiplib.SOURCES


def test_the_pipeline_switches():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline()
    assert pipe._auto_focus is None and not hasattr(pipe, "_focus_pass")  # a focused pass is handed over explicitly, not through a slot
    assert pipe.enable_auto_focus() is pipe and pipe._auto_focus == autofocus.AutoFocusConfig(0.25, False)
    assert pipe.enable_auto_focus(context=1, warm_start=True) is pipe and pipe._auto_focus == autofocus.AutoFocusConfig(1.0, True)
    assert pipe._region_focus is None  # `enable_region_focus` keeps its own switch
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pipe.enable_auto_focus(bad)
    with pytest.raises(ValueError):
        pipe.enable_auto_focus(0.25, warm_start=1)
    assert pipe._auto_focus == autofocus.AutoFocusConfig(1.0, True)  # a refused call changes nothing
    assert pipe.disable_auto_focus() is pipe and pipe._auto_focus is None


def test_denoise_takes_the_tail_arguments():
    import inspect

    from chronoedit_amd.pipeline import denoise
    sig = inspect.signature(denoise).parameters
    assert sig["start_step"].default == 0 and sig["start_eps"].default is None
