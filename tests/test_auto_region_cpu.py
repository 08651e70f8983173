"""Automatic edit regions, host side (chronoedit_amd/auto_region.py): the config's validation, every pass as a CPU torch expression against
a brute-force evaluation, the decision rule, and the four entry points in the header and the signature table.  No GPU."""
import numpy as np
import pytest
import torch

from chronoedit_amd import auto_region as ar
from chronoedit_amd import hiplib

ENTRY_POINTS = ("ce_auto_region_change_f32", "ce_auto_region_otsu_f32", "ce_auto_region_ramp_f32", "ce_auto_region_mask_u8")
F32 = np.float32


# -- the config -----------------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    c = ar.AutoRegionConfig(2)
    assert (c.detect_step, c.threshold, c.floor, c.dilate, c.feather, c.max_area, c.composite) == (2, "otsu", 0.0, 1, 1, 0.5, True)
    assert ar.AutoRegionConfig(0, threshold=0.25, dilate=3, feather=5, max_area=1.0).threshold == 0.25
    assert ar.AutoRegionConfig(0, dilate=0, feather=8).feather == 8
    bad = [dict(detect_step=-1), dict(detect_step=1.0), dict(detect_step=True), dict(detect_step=1, threshold="mean"),
           dict(detect_step=1, threshold=-0.5), dict(detect_step=1, threshold=float("nan")), dict(detect_step=1, threshold=float("inf")),
           dict(detect_step=1, floor=-1.0), dict(detect_step=1, floor=float("nan")), dict(detect_step=1, dilate=-1),
           dict(detect_step=1, feather=1.5), dict(detect_step=1, dilate=4, feather=5), dict(detect_step=1, dilate=9, feather=0),
           dict(detect_step=1, max_area=0.0), dict(detect_step=1, max_area=1.5), dict(detect_step=1, max_area=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            ar.AutoRegionConfig(**kw)


def test_detect_index():
    c = ar.AutoRegionConfig(1)
    assert ar.detect_index(c, 6) == 1
    assert ar.detect_index(ar.AutoRegionConfig(5), 6) == 5 and ar.detect_index(ar.AutoRegionConfig(6), 6) is None
    # temporal reasoning: the first step at or behind detect_step that runs at the truncated shape
    assert ar.detect_index(c, 6, True, 3) == 3 and ar.detect_index(ar.AutoRegionConfig(4), 6, True, 3) == 4
    assert ar.detect_index(c, 6, True, 0) == 1
    assert ar.detect_index(c, 6, True, 6) == 1  # no truncation inside the schedule
    assert ar.detect_index(c, 6, False, 3) == 1


# -- the change map -------------------------------------------------------------------------------------------------------------------
def change_bruteforce(x0, z, frame):
    B, C, T, h, w = x0.shape
    x0, z = x0.numpy(), z.numpy()
    out = np.zeros((h, w), dtype=F32)
    for y in range(h):
        for x in range(w):
            best = None
            for b in range(B):
                s = F32(0.0)
                for c in range(C):
                    df = F32(x0[b, c, frame, y, x] - z[b, c, frame, y, x])
                    s = F32(s + F32(df * df))
                v = F32(s / F32(C))
                best = v if best is None or v > best or np.isnan(v) else best
            out[y, x] = best
    return torch.from_numpy(out)


@pytest.mark.parametrize("shape, frame", [((1, 16, 2, 8, 12), -1), ((2, 16, 3, 6, 10), 1), ((3, 5, 1, 3, 5), 0)])
def test_change_map_against_a_brute_force_loop(shape, frame):
    g = torch.Generator().manual_seed(3)
    x0, z = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    x0[0, 2, frame, 1, 1] = float("nan")
    d = ar.change_map(x0, z, frame)
    want = change_bruteforce(x0, z, frame % shape[2])
    assert d.dtype == torch.float32 and torch.equal(torch.nan_to_num(d, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert bool(torch.isnan(d[1, 1])) and int(torch.isnan(d).sum()) == 1


# -- the ramp -------------------------------------------------------------------------------------------------------------------------
def ramp_bruteforce(seed, dilate, feather):
    h, w = seed.shape
    R = dilate + feather
    out = np.zeros((h, w), dtype=F32)
    for y in range(h):
        for x in range(w):
            best = F32(0.0)
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and seed[yy, xx]:
                        r = max(abs(dy), abs(dx))
                        v = F32(1.0) if r <= dilate else F32(F32(feather + 1 - (r - dilate)) / F32(feather + 1))
                        best = max(best, v)
            out[y, x] = best
    return torch.from_numpy(out)


def seed_grids():
    rng = np.random.default_rng(0)
    grids = {"empty": np.zeros((8, 12), bool), "all": np.ones((8, 12), bool), "random": rng.random((8, 12)) < 0.08,
             "tiny": np.array([[True, False], [False, False]]), "one-row": rng.random((1, 9)) < 0.3}
    corners = np.zeros((8, 12), bool)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    edges = np.zeros((8, 12), bool)
    edges[0, 5] = edges[4, 0] = edges[-1, 7] = edges[3, -1] = True
    rect = np.zeros((8, 12), bool)
    rect[2:5, 3:7] = True
    return dict(grids, corners=corners, edges=edges, rect=rect)


@pytest.mark.parametrize("dilate, feather", [(0, 0), (1, 1), (0, 8), (3, 5), (2, 0), (8, 0)])
def test_ramp_against_a_brute_force_double_loop(dilate, feather):
    for name, seed in seed_grids().items():  # (grids smaller than the window among them)
        d = torch.from_numpy(np.where(seed, 2.0, 0.5).astype(F32))
        d[0, -1] = float("nan") if not seed[0, -1] else d[0, -1]  # a NaN is never a seed
        w = ar.ramp_weights(d, torch.tensor([1.0]), dilate, feather)
        want = ramp_bruteforce(seed, dilate, feather)
        assert w.dtype == torch.float32 and torch.equal(w, want), (name, dilate, feather)
        if name == "all":
            assert bool((w == 1).all())
        if name == "empty":
            assert bool((w == 0).all())
    with pytest.raises(ValueError):
        ar.ramp_weights(torch.zeros(4, 4), torch.tensor([1.0]), 5, 4)


def test_ramp_is_1_on_the_core_and_0_beyond_the_radius():
    seed = seed_grids()["rect"]
    d = torch.from_numpy(np.where(seed, 2.0, 0.0).astype(F32))
    w = ar.ramp_weights(d, torch.tensor([1.0]), 1, 2)
    assert bool((w[1:6, 2:8] == 1).all()) and float(w[0, 2]) == float(F32(2) / F32(3)) and float(w[7, 2]) == float(F32(1) / F32(3))
    assert bool((w[:, 10:] == 0).all())
    assert bool((w[:, 9] == torch.tensor(float(F32(1) / F32(3)))).all())  # rows 0..7 lie within 3 of rows 2..4


# -- Otsu -----------------------------------------------------------------------------------------------------------------------------
def otsu_bruteforce(d, floor=0.0):
    d = d.numpy().astype(F32).reshape(-1)
    ok = d[~np.isnan(d)]
    dmax = F32(max(ok.max(), 0.0)) if ok.size else F32(0.0)
    if not dmax > 0:
        return float("inf"), float(dmax)
    scale = F32(256.0) / dmax
    hist = [0] * 256
    for v in d:
        p = F32(v * scale)
        hist[min(255, int(p)) if p >= 0 else 0] += 1
    N, S = len(d), sum(i * n for i, n in enumerate(hist))
    best, t_best, w0, s0 = None, 0, 0, 0
    for t in range(256):
        w0, s0 = w0 + hist[t], s0 + t * hist[t]
        if 0 < w0 < N:
            num = np.float64(s0 * N - S * w0)
            sc = num * num / np.float64(w0 * (N - w0))
            if best is None or sc > best:
                best, t_best = sc, t
    thr = F32(F32(t_best + 1) * F32(dmax / F32(256.0)))
    return float(max(thr, F32(F32(floor) * F32(floor)))), float(dmax)


def otsu_maps():
    g = torch.Generator().manual_seed(1)
    two = torch.rand(8, 12, generator=g) * 0.05
    two[2:5, 3:7] += 3.0 + torch.rand(3, 4, generator=g)
    big = torch.rand(90, 160, generator=g) ** 3
    big[20:50, 40:100] += 2.0
    nan = two.clone()
    nan[0, 0] = float("nan")
    return {"two-clusters": two, "720p": big, "nan": nan, "constant": torch.full((8, 12), 0.75), "zero": torch.zeros(8, 12)}


@pytest.mark.parametrize("name", list(otsu_maps()))
def test_otsu_against_a_brute_force_evaluation(name):
    d = otsu_maps()[name]
    thr, dmax = ar.otsu_threshold(d)
    want = otsu_bruteforce(d)
    assert thr.dtype == torch.float32 and tuple(thr.shape) == (1,) and (float(thr), float(dmax)) == want, (float(thr), float(dmax), want)
    seed = d > thr
    if name in ("two-clusters", "nan"):
        rect = torch.zeros(8, 12, dtype=torch.bool)
        rect[2:5, 3:7] = True
        assert torch.equal(seed, rect)
    if name == "720p":
        assert 0.05 < float(seed.float().mean()) < 0.5


def test_otsu_on_a_constant_map_an_all_zero_map_and_the_floor():
    cfg = ar.AutoRegionConfig(1)
    # a constant map: every cell in the last bin, t = 0, thr = dmax / 256: everything is active, which max_area declines
    d = otsu_maps()["constant"]
    thr, dmax = ar.otsu_threshold(d)
    assert float(dmax) == 0.75 and float(thr) == 0.75 / 256 and bool((d > thr).all())
    w = ar.ramp_weights(d, thr, cfg.dilate, cfg.feather)
    assert bool((w == 1).all()) and ar.decide(w, cfg) == (False, "max_area", 1.0)
    # all zero: +inf, nothing is active, declined as empty
    d = otsu_maps()["zero"]
    thr, dmax = ar.otsu_threshold(d)
    assert float(thr) == float("inf") and float(dmax) == 0.0
    w = ar.ramp_weights(d, thr, cfg.dilate, cfg.feather)
    assert bool((w == 0).all()) and ar.decide(w, cfg) == (False, "empty", 0.0)
    # the floor: fp32(floor)^2 when Otsu's own threshold lies below it
    d = otsu_maps()["two-clusters"]
    low = float(ar.otsu_threshold(d)[0])
    assert float(ar.otsu_threshold(d, floor=0.01)[0]) == low  # (0.0001 < low)
    fl = 1.9
    assert float(ar.otsu_threshold(d, floor=fl)[0]) == float(F32(fl) * F32(fl)) > low
    assert (float(ar.otsu_threshold(d, floor=fl)[0]), float(d.max())) == otsu_bruteforce(d, fl)
    assert float(ar.otsu_threshold(d, floor=3.0)[0]) == 9.0 and not bool((d > 9.0).any())
    # a number for a threshold: fp32(t) * fp32(t)
    assert float(ar.number_threshold(0.3)) == float(F32(0.3) * F32(0.3)) and tuple(ar.number_threshold(2).shape) == (1,)


# -- the pixel mask, the decision, the report -----------------------------------------------------------------------------------------
def test_pixel_mask_rounds_half_to_even_and_round_trips_through_the_box_mean():
    from chronoedit_amd import region
    w = torch.tensor([[0.0, 1.0, 0.5, 1.0 / 3.0], [2.0 / 3.0, 0.25, 0.75, 0.1]], dtype=torch.float32)
    m = ar.pixel_mask(w)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (16, 32)
    want = np.rint(F32(255.0) * w.numpy()).astype(np.uint8)  # 127.5 -> 128 (half to even)
    assert want[0, 2] == 128 and np.array_equal(m.numpy(), np.repeat(np.repeat(want, 8, 0), 8, 1))
    hard = (torch.rand(4, 6, generator=torch.Generator().manual_seed(0)) < 0.5).float()
    assert torch.equal(region.latent_weights(ar.pixel_mask(hard)), hard)  # what set_edit_region makes of the reported mask


def test_decision_rule():
    cfg = ar.AutoRegionConfig(1, max_area=0.25)
    w = torch.zeros(8, 12)
    assert ar.decide(w, cfg) == (False, "empty", 0.0)
    w[2, 4] = 0.5  # one cell: one patch of 24
    assert ar.decide(w, cfg) == (True, "accepted", 1 / 24)
    assert ar.decide(w, cfg, margin=1) == (False, "max_area", 9 / 24)  # the sparse margin counts: 3 x 3 patches
    w[0:4, 0:6] = 1.0  # 2 x 3 patches = 6 of 24: exactly max_area is still accepted
    assert ar.decide(w, cfg) == (True, "accepted", 0.25)
    w[4, 0] = 0.01
    assert ar.decide(w, cfg) == (False, "max_area", 7 / 24)
    rep = ar.report(1, 0.5, 2.0, 1 / 24, True, "accepted", w)
    assert set(rep) == {"step", "threshold", "dmax", "active_fraction", "accepted", "reason", "w", "mask"}
    assert rep["mask"].mode == "L" and rep["mask"].size == (96, 64)
    assert np.array_equal(np.asarray(rep["mask"]), ar.pixel_mask(w).numpy())


def test_measurement_rows():
    table = torch.zeros(3, 8, 12)
    table[0] = torch.rand(8, 12, generator=torch.Generator().manual_seed(0))
    table[1, 2:5, 3:7] = 1.0
    table[1, 6, 6] = 1.0
    table[2, 2:5, 3:7] = 1.0
    rows = ar.measurement(table, ar.AutoRegionConfig(0, threshold=0.9))
    assert [r["step"] for r in rows] == [0, 1, 2] and rows[2]["iou"] == 1.0 and rows[1]["iou"] == 12 / 13
    assert rows[2]["active_fraction"] == 12 / 96 and rows[1]["threshold"] == float(F32(0.9) * F32(0.9))
    assert 0.0 <= rows[0]["iou"] < 1.0


# -- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_c_abi_declares_the_four_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_auto_region_")] == list(ENTRY_POINTS)
    assert "ce_region_auto.hip" in hiplib.SOURCES
