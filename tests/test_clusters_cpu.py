"""One crop per group of stroke clusters, host side (chronoedit_amd/clusters.py): the cluster table against a brute-force evaluation per
label, the grouping on hand-built rows, what follows from the arithmetic (the selected planes partition `kept`; a pixel within `grow` of a
kept changed pixel is 255 in exactly one group's mask; the output carries the background where every mask is 0), `host_paste` against a
hand-written PIL chain, `max_crops` validation, and the entry points in the header and the signature table.  No GPU."""
import re

import components_shapes as S
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import clusters, components, focus, hiplib, sketch

ENTRY_POINTS = ("ce_clusters_table_i32", "ce_clusters_select_u8", "ce_clusters_paste_u8")


def test_the_c_abi_declares_the_clusters_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_clusters_")] == list(ENTRY_POINTS) == list(clusters.ENTRY_POINTS)
    assert [n for n in hiplib.SIGNATURES if n.startswith("ce_clusters_")] == list(ENTRY_POINTS)
    assert "ce_clusters.hip" in hiplib.SOURCES
    src = open(hiplib.CSRC + "/ce_clusters.hip").read()
    assert int(re.search(r"#define CL_ROWS (\d+)", src).group(1)) == clusters.ROWS == 256


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def brute_force(roots: np.ndarray, sums: np.ndarray, kept: np.ndarray):
    """(count, rows) label by label: what the table is, written the slow way."""
    H, W = roots.shape
    rows = []
    for p in range(H * W):
        y, x = divmod(p, W)
        if roots[y, x] == p and kept[y, x] != 0:
            ys, xs = np.nonzero((roots == p) & (kept != 0))
            rows.append([p, xs.min(), ys.min(), xs.max() + 1, ys.max() + 1, len(ys), sums[y, x], 0])
    return len(rows), rows


def planes():
    for H, W in ((1, 1), (1, 23), (19, 1), (7, 9), (33, 65), (53, 131)):
        for name, p in S.adversarial(H, W).items():
            yield f"{name}-{H}x{W}", p


PLANES = dict(planes())


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("name", list(PLANES))
def test_table_equals_the_brute_force_evaluation(name, filtered):
    plane = torch.from_numpy(PLANES[name])
    weight = torch.from_numpy(S.noise(*plane.shape, 0.5, 3))
    roots = components.roots(plane)
    sums = components.sums(roots, weight)
    kept = components.keep(plane, roots, sums, 2)[0] if filtered else plane
    count, rows = clusters.table(roots, sums, kept)
    assert count.dtype == torch.int32 and tuple(count.shape) == (1,) and rows.dtype == torch.int32 and tuple(rows.shape) == (clusters.ROWS, 8)
    n, want = brute_force(roots.numpy(), sums.numpy(), kept.numpy())
    assert int(count) == n
    if n <= clusters.ROWS:
        assert rows[:n].tolist() == want and not rows[n:].any()
        labels = [r[0] for r in want]
        assert labels == sorted(labels) and sum(r[5] for r in want) == int((kept != 0).sum())


def test_an_empty_plane_and_more_clusters_than_rows():
    z = torch.zeros(9, 14, dtype=torch.uint8)
    r = components.roots(z)
    count, rows = clusters.table(r, components.sums(r), z)
    assert int(count) == 0 and not rows.any()
    p = torch.zeros(40, 40, dtype=torch.uint8)
    p[::2, ::2] = 255  # isolated pixels on a stride-2 grid: 400 clusters
    r = components.roots(p)
    count, rows = clusters.table(r, components.sums(r), p)
    assert int(count) == 400 > clusters.ROWS
    for bad in (r.to(torch.int64), r[0]):
        with pytest.raises(ValueError):
            clusters.table(bad, components.sums(r), p)
    with pytest.raises(ValueError):
        clusters.table(r, components.sums(r), p[:, :39])


# ---- the grouping ---------------------------------------------------------------------------------------------------------------------
SRC, EDIT, CONTEXT, FEATHER_PX = (400, 300), (96, 64), 0.25, 4


def row(l, t, r, b):
    return [t * SRC[0] + l, l, t, r, b, (r - l) * (b - t), 1, 0]


A, B = row(20, 20, 50, 40), row(350, 250, 380, 280)  # near opposite corners
C = row(200, 22, 220, 42)  # right of A: its trial box is disjoint from A's, and its union with A is far smaller than either's with B


def boxes(rows, groups):
    return [clusters.trial_box(rows, g, SRC, EDIT, CONTEXT, FEATHER_PX) for g in groups]


def check_groups(rows, groups, max_crops):
    assert sorted(i for g in groups for i in g) == list(range(len(rows)))  # every row in exactly one group
    assert 1 <= len(groups) <= max_crops or not rows
    firsts = [min(rows[i][0] for i in g) for g in groups]
    assert firsts == sorted(firsts)  # the paste order: by smallest label
    assert groups == clusters.group(rows, SRC, EDIT, CONTEXT, FEATHER_PX, max_crops)  # a pure function: the same twice


def test_two_far_clusters_are_two_groups_with_the_boxes_worked_by_hand():
    rows = [A, B]
    groups = clusters.group(rows, SRC, EDIT, CONTEXT, FEATHER_PX, 2)
    check_groups(rows, groups, 2)
    assert groups == [[0], [1]]
    # A: extent (16, 16, 54, 44), 38 x 28, padded by ceil(38 / 4) = 10 -> 58 x 48, raised to 96 x 64, centred on (35, 30) and shifted in
    assert clusters.extent(rows, [0], SRC, FEATHER_PX) == (16, 16, 54, 44)
    assert boxes(rows, groups) == [((0, 0, 96, 64), "ok"), ((304, 233, 400, 297), "ok")]
    assert clusters.group([A], SRC, EDIT, CONTEXT, FEATHER_PX, 5) == [[0]] and clusters.group([], SRC, EDIT, CONTEXT, FEATHER_PX, 2) == []
    assert clusters.group(torch.tensor(rows), SRC, EDIT, CONTEXT, FEATHER_PX, 2) == groups and clusters.group(np.array(rows), SRC, EDIT, CONTEXT, FEATHER_PX, 2) == groups


def test_trial_boxes_that_share_a_pixel_merge_and_boxes_that_only_abut_do_not():
    near = row(133, 22, 153, 42)  # extent (129, 18, 157, 46) -> 96 x 64 around (143, 32): (95, 0, 191, 64) - one column in common with A's box
    assert boxes([A, near], [[1]])[0] == ((95, 0, 191, 64), "ok") and clusters.intersect((0, 0, 96, 64), (95, 0, 191, 64))
    assert clusters.group([A, near], SRC, EDIT, CONTEXT, FEATHER_PX, 4) == [[0, 1]]
    apart = row(134, 22, 154, 42)  # one pixel further: (96, 0, 192, 64) abuts A's box and shares no pixel
    assert boxes([A, apart], [[1]])[0] == ((96, 0, 192, 64), "ok") and not clusters.intersect((0, 0, 96, 64), (96, 0, 192, 64))
    groups = clusters.group([A, apart], SRC, EDIT, CONTEXT, FEATHER_PX, 4)
    assert groups == [[0], [1]]
    check_groups([A, apart], groups, 4)
    # the trial boxes are pairwise disjoint whenever the cap forced no merge
    for rows in ([A, near, C, B], [A, apart, C, B], [A, C, B]):
        groups = clusters.group(rows, SRC, EDIT, CONTEXT, FEATHER_PX, 16)
        check_groups(rows, groups, 16)
        bs = [b for b, _ in boxes(rows, groups)]
        assert all(not clusters.intersect(bs[i], bs[j]) for i in range(len(bs)) for j in range(i + 1, len(bs)))


def test_three_clusters_under_a_cap_of_two_merge_the_pair_with_the_smaller_union():
    rows = [A, C, B]  # (ascending labels)
    assert [r[0] for r in rows] == sorted(r[0] for r in rows)
    assert clusters.group(rows, SRC, EDIT, CONTEXT, FEATHER_PX, 3) == [[0], [1], [2]]
    groups = clusters.group(rows, SRC, EDIT, CONTEXT, FEATHER_PX, 2)
    check_groups(rows, groups, 2)
    assert groups == [[0, 1], [2]]
    area = lambda g: (lambda b: (b[2] - b[0]) * (b[3] - b[1]))(boxes(rows, [g])[0][0])
    assert area([0, 1]) < area([1, 2]) and area([0, 1]) < area([0, 2])
    assert clusters.group(rows, SRC, EDIT, CONTEXT, FEATHER_PX, 1) == [[0, 1, 2]]
    # the order is by smallest label, whatever merged: the first and the last row share a box, the middle one is far from both
    far = row(350, 21, 380, 41)
    below = row(22, 44, 40, 60)
    rows = [A, far, below]
    groups = clusters.group(rows, SRC, EDIT, CONTEXT, FEATHER_PX, 3)
    check_groups(rows, groups, 3)
    assert groups == [[0, 2], [1]]


def test_a_box_that_is_not_ok_meets_every_other_box():
    tall = (70, 300)  # the largest 96 : 64 box in it is 70 x 46: a cluster 60 rows high does not fit
    rows = [[5 * 70 + 5, 5, 5, 30, 65, 1500, 1, 0], [200 * 70 + 5, 5, 200, 30, 260, 1500, 1, 0]]
    assert clusters.trial_box(rows, [0], tall, EDIT, CONTEXT, FEATHER_PX) == ((0, 0, 70, 300), "fit")
    assert clusters.group(rows, tall, EDIT, CONTEXT, FEATHER_PX, 2) == [[0, 1]]


# ---- what follows from the arithmetic --------------------------------------------------------------------------------------------------
GROW, FEATHER = 3, 2


def sketch_pair():
    """A 120 x 90 photo with a stroke, dotted strokes (one cluster), a third stroke and a far speck of two pixels."""
    rng = np.random.default_rng(3)
    bg = rng.integers(0, 256, (90, 120, 3), dtype=np.uint8)
    cp = bg.copy()
    cp[10:14, 70:100] ^= 128
    for k in range(8):
        cp[40 + 4 * k, 20 + 4 * k] ^= 128
    cp[70:80, 100:104] ^= 128
    cp[85, 5:7] ^= 128
    return torch.from_numpy(bg), torch.from_numpy(cp)


def chebyshev_reach(points: np.ndarray, radius: int) -> np.ndarray:
    out = np.zeros_like(points)
    for y, x in zip(*np.nonzero(points)):
        out[max(y - radius, 0):y + radius + 1, max(x - radius, 0):x + radius + 1] = True
    return out


@pytest.mark.parametrize("min_stroke", [0, 4])
def test_the_groups_masks_partition_the_region(min_stroke):
    bg, cp = sketch_pair()
    ch, _, roots, sums, kept, m, stats = sketch.labelled_stages(bg, cp, GROW, FEATHER, 0, min_stroke)
    assert torch.equal(m, sketch.reference(bg, cp, GROW, FEATHER, 0, min_stroke))  # the union mask is the single-box call's
    count, rows = clusters.table(roots, sums, kept)
    n = int(count)
    assert n == (3 if min_stroke else 4) and (stats is None) == (min_stroke == 0)
    rows = rows[:n].tolist()
    assert [r[6] for r in rows] == ([120, 8, 40] if min_stroke else [120, 8, 40, 2])  # the weights: changed pixels per cluster
    groups = [[0, 2], [1]] if min_stroke else [[0, 3], [1], [2]]
    planes = [clusters.select(roots, kept, [rows[i][0] for i in g]) for g in groups]
    total = sum(p.to(torch.int32) for p in planes)
    assert torch.equal(total.to(torch.uint8), kept) and all(set(p.unique().tolist()) <= {0, 255} for p in planes)  # a partition of `kept`
    masks = clusters.group_masks(roots, kept, None, rows, groups, FEATHER)
    for p, mk in zip(planes, masks):
        assert torch.equal(mk, sketch.box(sketch.box(p, FEATHER, 0), FEATHER, 1))
    kept_changed = ch.numpy().astype(bool) & kept.numpy().astype(bool)
    core = chebyshev_reach(kept_changed, GROW)
    stack = np.stack([mk.numpy() for mk in masks])
    assert ((stack[:, core] == 255).sum(0) == 1).all() and ((stack[:, core] == 0).sum(0) == len(groups) - 1).all()
    # the output: the background's bytes wherever every group's mask is 0
    size, frames = (32, 24), 2
    rng = np.random.default_rng(5)
    videos = [[Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)) for _ in range(frames)] for _ in groups]
    bxs = []
    for mk in masks:
        box, reason = focus.focus_box(focus.mask_bbox(mk), (120, 90), size, 0.25)
        assert reason == "ok"
        bxs.append(box)
    background = Image.fromarray(bg.numpy())
    out = clusters.host_paste(background, videos, masks, bxs)
    outside = stack.max(0) == 0
    assert outside.any() and len(out) == frames
    for f in out:
        assert f.size == (120, 90) and np.array_equal(np.asarray(f)[outside], bg.numpy()[outside])
        assert not np.array_equal(np.asarray(f)[core], bg.numpy()[core])


def test_host_paste_is_pils_paste_chained():
    rng = np.random.default_rng(7)
    background = Image.fromarray(rng.integers(0, 256, (60, 80, 3), dtype=np.uint8))
    boxes_ = [(3, 5, 51, 37), (29, 21, 77, 53)]  # overlapping, at odd offsets
    masks = []
    for k in range(2):
        m = rng.integers(0, 256, (60, 80), dtype=np.uint8)
        m[:, 10 * k:10 * k + 20] = 0
        m[20:30] = 255
        masks.append(torch.from_numpy(m))
    videos = [[Image.fromarray(rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)) for _ in range(3)] for _ in range(2)]
    for composite in (True, False):
        got = clusters.host_paste(background, videos, masks if composite else None, boxes_)
        for f in range(3):
            want = background.copy()
            for g, (l, t, r, b) in enumerate(boxes_):
                frame = videos[g][f].resize((r - l, b - t), Image.LANCZOS)
                if composite:
                    want.paste(frame, (l, t), Image.fromarray(masks[g].numpy()).crop((l, t, r, b)))
                else:
                    want.paste(frame, (l, t))
            assert np.array_equal(np.asarray(got[f]), np.asarray(want)), (composite, f)
    assert np.array_equal(np.asarray(background), np.asarray(Image.fromarray(np.asarray(background))))  # (the background itself is untouched)


# ---- the switch -------------------------------------------------------------------------------------------------------------------------
def test_max_crops_validation():
    assert sketch.SketchConfig().max_crops == 1 and sketch.SketchConfig(max_crops=16).max_crops == 16
    assert sketch.SketchConfig(2, 1, 5, 0.5, False, 7, 3) == sketch.SketchConfig(grow=2, feather=1, threshold=5, context=0.5, composite=False, min_stroke=7, max_crops=3)
    for bad in (True, False, 0, -1, 17, 2.0, "2", None, float("nan")):
        with pytest.raises(ValueError, match="max_crops"):
            sketch.SketchConfig(max_crops=bad)
        with pytest.raises(ValueError):
            clusters.group([A], SRC, EDIT, CONTEXT, FEATHER_PX, bad)
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline.__new__(ChronoEditPipeline)
    pipe._sketch_region = None
    assert pipe.enable_sketch_region(max_crops=4)._sketch_region == sketch.SketchConfig(max_crops=4)
    assert pipe.enable_sketch_region()._sketch_region.max_crops == 1
    with pytest.raises(ValueError):
        pipe.enable_sketch_region(max_crops=True)
    pipe.disable_sketch_region()
    with pytest.raises(ValueError, match="enable_sketch_region"):
        pipe.sketch_crops(None, None, 64, 96)


def test_masks_and_plan_on_the_host():
    """`sketch.masks` with max_crops >= 2 holds what the single-box entry holds, plus the table; `clusters.plan` turns it into crops."""
    bg, cp = sketch_pair()
    images = [Image.fromarray(bg.numpy())], [Image.fromarray(cp.numpy())]
    for min_stroke in (0, 4):
        one = sketch.masks(sketch.SketchConfig(GROW, FEATHER, min_stroke=min_stroke), *images)[0]
        e = sketch.masks(sketch.SketchConfig(GROW, FEATHER, min_stroke=min_stroke, max_crops=3), *images)[0]
        assert torch.equal(e["mask_u8"], one["mask_u8"]) and all(e[k] == one[k] for k in one if k not in ("mask_u8", "background", "composite"))
        assert e["count"] == (3 if min_stroke else 4) and len(e["rows"]) == clusters.ROWS and not any(any(r) for r in e["rows"][e["count"]:])
        crops = clusters.plan(e, 3, 16, 12, 0.0)  # (crops of 16 x 12 without context: the four clusters' trial boxes are disjoint)
        assert crops.groups == clusters.group(e["rows"][:e["count"]], (120, 90), (16, 12), 0.0, FEATHER, 3)
        if not min_stroke:
            assert len(clusters.group(e["rows"][:4], (120, 90), (16, 12), 0.0, FEATHER, 4)) == 4  # the cap forces one merge
        assert crops.reason == "crops" and len(crops.plans) == len(crops.groups) == 3 and sorted(i for g in crops.groups for i in g) == list(range(e["count"]))
        assert crops.labels == [[e["rows"][i][0] for i in g] for g in crops.groups]
        for p, g in zip(crops.plans, crops.groups):
            want = clusters.group_masks(e["roots"], e["kept"], None, e["rows"], [g], FEATHER)[0]
            assert torch.equal(p.mask_u8, want) and p.report["reason"] == "ok" and p.paste_image is images[0][0] and p.image is images[1][0]
            assert p.report["box"] == focus.focus_box(focus.mask_bbox(want), (120, 90), (16, 12), 0.0)[0]
            assert p.report["scale"] < sketch.focus_plan(one, 16, 12, 0.0).report["scale"]
        two = clusters.plan(e, 2, 16, 12, 0.0)  # (a merge under the cap may make the next one under the first rule: never more than the cap)
        assert len(two.groups) <= 2 and two.reason == ("crops" if len(two.groups) == 2 else "single") and len(two.plans) in (0, 2)
        assert clusters.plan(dict(e, count=400), 3, 16, 12, 0.0).reason == "many"
        assert clusters.plan(e, 3, 96, 64, 0.25).reason in ("single", "unfit")  # crops of 96 x 64 in a 120 x 90 photo all meet
