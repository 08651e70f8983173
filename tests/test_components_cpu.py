"""Connected components, host side (chronoedit_amd/components.py): `components.reference` against scipy's labelling on the shapes a
labelling goes wrong on, `sums` / `keep` / the counters against numpy, the two switches' validation, the sketch chain with `min_stroke`,
the automatic region's definition on a hand-built change map, and the entry points in the header and the signature table.  No GPU."""
import re

import components_shapes as S
import numpy as np
import pytest
import torch

from chronoedit_amd import auto_region as ar
from chronoedit_amd import components, hiplib, sketch

ENTRY_POINTS = ("ce_components_roots_i32", "ce_components_sums_i32", "ce_components_keep_u8", "ce_components_seeds_f32", "ce_components_masked_f32")


def test_the_c_abi_declares_the_components_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_components_")] == list(ENTRY_POINTS) == list(components.ENTRY_POINTS)
    assert "ce_components.hip" in hiplib.SOURCES
    core = open(hiplib.CSRC + "/ce_components_core.h").read()
    assert (int(re.search(r"#define CC_TH (\d+)", core).group(1)), int(re.search(r"#define CC_TW (\d+)", core).group(1))) == components.TILE


# ---- roots against scipy ------------------------------------------------------------------------------------------------------------------
def planes():
    for H, W in ((1, 1), (1, 23), (19, 1), (7, 9), (33, 65), (53, 131)):
        for name, p in S.adversarial(H, W).items():
            yield f"{name}-{H}x{W}", p
    yield "noise-211x307", S.noise(211, 307, 0.4, 5)


PLANES = dict(planes())


@pytest.mark.parametrize("name", list(PLANES))
def test_roots_and_sizes_equal_scipys_labelling(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    plane = PLANES[name]
    H, W = plane.shape
    r = components.roots(torch.from_numpy(plane))
    assert r.dtype == torch.int32 and tuple(r.shape) == (H, W)
    r = r.numpy()
    lab, n = ndimage.label(plane, structure=np.ones((3, 3)))
    assert np.array_equal(r < 0, plane == 0)
    found = np.unique(r[r >= 0])
    assert len(found) == n
    # scipy numbers the components in the order of their first pixel: its label k is the component with the k-th smallest root
    for k, root in enumerate(found):
        assert np.flatnonzero(lab.reshape(-1) == k + 1)[0] == root
    assert np.array_equal(r, np.where(lab > 0, np.append(found, -1)[lab - 1], -1))
    s = components.sums(torch.from_numpy(r)).numpy()
    sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
    assert np.array_equal(s.reshape(-1)[found], sizes) and int(s.sum()) == int((plane != 0).sum()) and int((s != 0).sum()) == n


def test_the_named_shapes_are_what_they_claim():
    one = lambda p: len(np.unique(components.roots(torch.from_numpy(p)).numpy())) - (1 if (p == 0).any() else 0)
    for H, W in ((33, 65), (53, 131)):
        for name in ("full", "checkerboard", "diagonal", "comb", "u", "serpentine", "spiral"):
            assert one(S.adversarial(H, W)[name]) == 1, (name, H, W)
        assert one(S.empty(H, W)) == 0
        assert int((S.serpentine(H, W) != 0).sum()) == (H + 1) // 2 * W + H // 2 and int((S.spiral(H, W) != 0).sum()) > H * W // 3


def test_any_non_zero_byte_is_foreground_and_the_limits():
    p = torch.tensor([[1, 0, 200], [0, 0, 0], [7, 0, 255]], dtype=torch.uint8)
    assert components.roots(p).tolist() == [[0, -1, 2], [-1, -1, -1], [6, -1, 8]]
    for bad in (p.to(torch.int32), p[0], torch.zeros(0, 3, dtype=torch.uint8), p.numpy()):
        with pytest.raises(ValueError):
            components.roots(bad)
    with pytest.raises(ValueError, match="2\\^31"):
        components.roots(torch.zeros(1, dtype=torch.uint8).expand(1 << 16, 1 << 15))


# ---- sums, keep, stats ----------------------------------------------------------------------------------------------------------------
def test_sums_with_a_weight_plane_that_differs_from_the_plane():
    plane, weight = S.noise(61, 97, 0.45, 1), S.noise(61, 97, 0.3, 2)
    r = components.roots(torch.from_numpy(plane))
    s = components.sums(r, torch.from_numpy(weight)).numpy()
    rn = r.numpy()
    for root in np.unique(rn[rn >= 0]):
        assert s.reshape(-1)[root] == int(((rn == root) & (weight != 0)).sum())
    assert int(s.sum()) == int(((plane != 0) & (weight != 0)).sum())
    assert not np.array_equal(s, components.sums(r).numpy())


def three_blobs():
    """Components of 3, 10 and 40 pixels."""
    p = np.zeros((20, 30), np.uint8)
    p[1, 1:4] = 9
    p[5:7, 10:15] = 255
    p[12:16, 2:12] = 1
    return p


@pytest.mark.parametrize("mw, kept", [(9, (10, 40)), (10, (10, 40)), (11, (40,)), (3, (3, 10, 40)), (41, ()),
                                       (0.25, (10, 40)),      # 1 / 4 of 40 = 10 exactly: kept
                                       (0.26, (40,)),         # 13 / 50 of 40 = 10.4 -> 11
                                       (0.075, (3, 10, 40)),  # 3 / 40 of 40 = 3 exactly
                                       (0.076, (10, 40))])    # 19 / 250 of 40 = 3.04 -> 4
def test_keep_at_the_threshold_and_the_counters(mw, kept):
    p = three_blobs()
    plane = torch.from_numpy(p)
    r = components.roots(plane)
    s = components.sums(r)
    out, stats = components.keep(plane, r, s, mw)
    sizes = {3: p == 9, 10: p == 255, 40: p == 1}
    want = np.zeros_like(p)
    for n in kept:
        want[sizes[n]] = p[sizes[n]]
    assert out.dtype == torch.uint8 and np.array_equal(out.numpy(), want)
    dropped = [n for n in sizes if n not in kept]
    assert stats.dtype == torch.int32 and stats.tolist() == [len(kept), len(dropped), sum(dropped), 40]
    o2, s2 = components.filter(plane, mw)
    assert torch.equal(o2, out) and torch.equal(s2, stats)
    o3, s3 = components.reference(plane, mw)
    assert torch.equal(o3, out) and torch.equal(s3, stats)


def test_filter_weighs_by_the_weight_plane():
    p = three_blobs()
    weight = np.zeros_like(p)
    weight[1, 1:4] = 1      # the small blob: weight 3
    weight[12, 2:4] = 1     # the large one: weight 2; the middle one: 0
    out, stats = components.filter(torch.from_numpy(p), 3, torch.from_numpy(weight))
    assert np.array_equal(out.numpy(), np.where(p == 9, p, 0)) and stats.tolist() == [1, 2, 2, 3]
    out, stats = components.filter(torch.from_numpy(np.zeros((4, 5), np.uint8)), 0.5)
    assert not out.any() and stats.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("bad", [True, 0, -1, 1.0, 0.0, 1.5, float("nan"), "3", None, 1 << 31, 1e-9])
def test_min_weight_refusals(bad):
    p = torch.from_numpy(three_blobs())
    with pytest.raises(ValueError):
        components.filter(p, bad)


def test_fraction_rule():
    assert components.fraction(0.02) == (1, 50) and components.least_weight(0.02, 4032) == 81
    assert components.least_weight(0.5, 0) == 0 and components.least_weight(7, 3) == 7


# ---- the two switches -------------------------------------------------------------------------------------------------------------------
def test_config_validation():
    assert sketch.SketchConfig().min_stroke == 0 and sketch.SketchConfig(min_stroke=4).min_stroke == 4 and sketch.SketchConfig(min_stroke=0.25).min_stroke == 0.25
    assert sketch.SketchConfig(2, 1, 5, 0.5, False, 7) == sketch.SketchConfig(grow=2, feather=1, threshold=5, context=0.5, composite=False, min_stroke=7)
    assert ar.AutoRegionConfig(1).min_area == 0 and ar.AutoRegionConfig(1, min_area=3).min_area == 3 and ar.AutoRegionConfig(1, min_area=0.5).min_area == 0.5
    assert ar.AutoRegionConfig(1, "otsu", 0.0, 1, 1, 0.5, True, 2).min_area == 2
    for bad in (True, False, -1, 1.0, 0.0, -0.5, float("nan"), "2", None):
        with pytest.raises(ValueError):
            sketch.SketchConfig(min_stroke=bad)
        with pytest.raises(ValueError):
            ar.AutoRegionConfig(1, min_area=bad)
    with pytest.raises(ValueError):
        ar.AutoRegionConfig(1, threshold=-0.5)  # (no threshold is below 0: d' = -1 is never a seed)


def test_pipeline_switches_take_the_new_keywords():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline.__new__(ChronoEditPipeline)
    pipe._sketch_region = None
    assert pipe.enable_sketch_region(min_stroke=5)._sketch_region == sketch.SketchConfig(min_stroke=5)
    assert pipe.enable_sketch_region()._sketch_region.min_stroke == 0
    with pytest.raises(ValueError):
        pipe.enable_sketch_region(min_stroke=True)

    class Transformer:
        def enable_auto_region(self, *a):
            self.args = a

    pipe.transformer = Transformer()
    pipe.enable_auto_region(2, min_area=0.1)
    assert ar.AutoRegionConfig(*pipe.transformer.args) == ar.AutoRegionConfig(2, min_area=0.1)


# ---- the sketch chain -------------------------------------------------------------------------------------------------------------------
GROW, FEATHER = 3, 2
R = GROW + FEATHER


def sketch_pair(extra=()):
    """A 120 x 90 photo with a stroke, dotted strokes (single pixels 4 apart: one cluster, since 4 <= 2 R) and `extra` pixels."""
    rng = np.random.default_rng(3)
    bg = rng.integers(0, 256, (90, 120, 3), dtype=np.uint8)
    cp = bg.copy()
    cp[10:14, 70:100] ^= 128                      # a stroke: 120 pixels
    for k in range(8):
        cp[40 + 4 * k, 20 + 4 * k] ^= 128         # a dotted diagonal: 8 pixels, each a component of `changed` of its own
    for y, x in extra:
        cp[y, x] ^= 128
    return torch.from_numpy(bg), torch.from_numpy(cp)


def chebyshev_reach(points: np.ndarray, radius: int) -> np.ndarray:
    """True within `radius` (Chebyshev) of a True pixel."""
    out = np.zeros_like(points)
    for y, x in zip(*np.nonzero(points)):
        out[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1] = True
    return out


def test_a_far_speck_goes_a_near_one_stays_and_dots_are_one_cluster():
    far, near = [(85, 5), (85, 6)], [(16, 104)]  # near: within 2 R of the stroke's end, so inside its cluster
    bg, cp = sketch_pair(far + near)
    ch, grown, kept, m, stats = sketch.filtered_stages(bg, cp, GROW, FEATHER, 0, 4)
    ch0, grown0, m0 = sketch.stages(bg, cp, GROW, FEATHER, 0)
    assert torch.equal(ch, ch0) and torch.equal(grown, grown0)
    assert stats.tolist() == [2, 1, 2, 121]  # the stroke with the near speck, the dots | the far speck, its two pixels
    clean = sketch.stages(*sketch_pair(near), GROW, FEATHER, 0)
    assert torch.equal(kept, clean[1]) and torch.equal(m, clean[2]) and not torch.equal(m, m0)
    assert torch.equal(m, sketch.reference(bg, cp, GROW, FEATHER, 0, 4)) and torch.equal(m, sketch.mask(bg, cp, GROW, FEATHER, 0, 4))
    assert torch.equal(m0, sketch.reference(bg, cp, GROW, FEATHER, 0)) and torch.equal(m0, sketch.reference(bg, cp, GROW, FEATHER, 0, 0))
    # the guarantees, now about the changed pixels of KEPT clusters
    kept_changed = ch.numpy().astype(bool) & kept.numpy().astype(bool)
    assert kept_changed.sum() == 129 and not kept_changed[85, 5] and kept_changed[16, 104] and kept_changed[40, 20]
    mask = m.numpy()
    assert (mask[chebyshev_reach(kept_changed, GROW)] == 255).all()
    assert (mask[~chebyshev_reach(kept_changed, GROW + 2 * FEATHER)] == 0).all() and mask[80:, :15].max() == 0
    # as a fraction of the heaviest cluster: 8 / 121 keeps the dots, 9 / 121 drops them
    assert sketch.filtered_stages(bg, cp, GROW, FEATHER, 0, 8 / 121)[4].tolist() == [2, 1, 2, 121]
    assert sketch.filtered_stages(bg, cp, GROW, FEATHER, 0, 9 / 121)[4].tolist() == [1, 2, 10, 121]


def test_masks_entries_and_all_clusters_dropped():
    from PIL import Image
    bg, cp = sketch_pair([(85, 5), (85, 6)])
    images = [Image.fromarray(bg.numpy())], [Image.fromarray(cp.numpy())]
    e = sketch.masks(sketch.SketchConfig(GROW, FEATHER, min_stroke=4), *images)[0]
    assert (e["clusters"], e["dropped_clusters"], e["dropped_pixels"], e["changed_pixels"]) == (2, 1, 2, 130)
    off = sketch.masks(sketch.SketchConfig(GROW, FEATHER), *images)[0]
    assert "clusters" not in off and off["changed_pixels"] == 130
    assert off["bbox"][0] == 0 and off["bbox"][3] == 90 and e["bbox"][3] < 85 and e["bbox"][0] > 5
    gone = sketch.masks(sketch.SketchConfig(GROW, FEATHER, min_stroke=1000), *images)[0]
    assert gone["bbox"] is None and gone["mask_pixels"] == 0 and (gone["clusters"], gone["dropped_clusters"], gone["dropped_pixels"]) == (0, 3, 130)
    assert not gone["mask_u8"].any()
    plan = sketch.focus_plan(gone, 96, 64, 0.25)
    assert plan.report["reason"] == "empty"


# ---- the automatic region ------------------------------------------------------------------------------------------------------------
def test_auto_region_definition_on_a_hand_built_change_map():
    d = torch.zeros(9, 14)
    d[2:5, 3:7] = 4.0          # the region: 12 cells
    d[8, 13] = 5.0             # an isolated cell, far away
    d[0, 0] = d[1, 1] = 3.0    # two cells touching diagonally: ONE component of 2
    thr = torch.tensor([1.0])
    dk, stats = ar.kept_map(d, thr, 3)
    want = torch.full_like(d, -1.0)
    want[2:5, 3:7] = 4.0
    assert torch.equal(dk, want) and stats.tolist() == [1, 2, 3, 12]
    dk2, stats2 = ar.kept_map(d, thr, 2)
    assert dk2[0, 0] == 3.0 and dk2[1, 1] == 3.0 and dk2[8, 13] == -1.0 and stats2.tolist() == [2, 1, 1, 12]
    assert ar.kept_map(d, thr, 1 / 6)[1].tolist() == [2, 1, 1, 12]  # ceil(12 / 6) = 2
    region = torch.zeros_like(d)
    region[2:5, 3:7] = 4.0
    assert torch.equal(ar.ramp_weights(dk, thr, 1, 1), ar.ramp_weights(region, thr, 1, 1))
    assert not torch.equal(ar.ramp_weights(dk, thr, 1, 1), ar.ramp_weights(d, thr, 1, 1))
    assert torch.equal(ar.seed_plane(d, thr), (d > 1.0).to(torch.uint8) * 255)


def test_weights_with_min_area_and_the_measurement_columns():
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(1, 16, 2, 8, 12, generator=g) * 0.01
    z = x0.clone()
    z[:, :, -1, 2:5, 3:7] += 2.0
    z[:, :, -1, 7, 11] += 2.0
    cfg = ar.AutoRegionConfig(1, threshold=1.0, min_area=2)
    d, thr, dmax, w = ar.weights(x0, z, cfg)
    clean = z.clone()
    clean[:, :, -1, 7, 11] = x0[:, :, -1, 7, 11]
    off = ar.AutoRegionConfig(1, threshold=1.0)
    assert torch.equal(w, ar.weights(x0, clean, off)[3]) and not torch.equal(w, ar.weights(x0, z, off)[3])
    table = torch.zeros(2, 8, 12)
    table[0, 2:5, 3:7] = 1.0
    table[0, 7, 11] = table[0, 0, 0] = 1.0
    rows = ar.measurement(table, ar.AutoRegionConfig(0, threshold=0.9))
    assert (rows[0]["components"], rows[0]["largest_fraction"]) == (3, 12 / 14) and (rows[1]["components"], rows[1]["largest_fraction"]) == (0, 0.0)
