"""Tiled edits on the host (chronoedit_amd/tiles.py): the planner's properties on a sweep, the three CPU definitions the kernels of
csrc/ce_tiles.hip are held to, the family pin, the options and every refusal of `enable_tiled_edit` that needs no device."""
import re
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import hiplib, tiles
from chronoedit_amd.pipeline import ChronoEditPipeline

ENTRY_POINTS = ("ce_tiles_fuse_f32", "ce_tiles_scatter_f32", "ce_tiles_blend_u8")


def test_family_pin():
    text = open(hiplib.HEADER).read()
    declared = re.findall(r"^int (ce_\w+)\(", text, flags=re.M)
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1
    assert [n for n in declared if n.startswith("ce_tiles_")] == list(ENTRY_POINTS) == list(tiles.ENTRY_POINTS)
    assert [n for n in hiplib.SIGNATURES if n.startswith("ce_tiles_")] == list(ENTRY_POINTS)
    assert "ce_tiles.hip" in hiplib.SOURCES
    assert len(declared) == 107  # the README's count


# ---- the planner ------------------------------------------------------------------------------------------------------------------
def _fewer_tiles_fail(C, T, v, n):
    """n - 1 tiles cannot cover C with v in common between neighbours: (n - 1) T - (n - 2) v < C."""
    return n <= 2 or (n - 1) * T - (n - 2) * v < C


@pytest.mark.parametrize("T", [64, 96, 720, 1280])
def test_axis_origins_properties(T):
    overlaps = sorted({16, 32, tiles.overlap_px(0.25, T), tiles.overlap_px(0.5, T), tiles.overlap_px(0.1, T)})
    for v in overlaps:
        if v >= T:
            continue
        for C in range(T, 5 * T + 1, 16):
            o = tiles.axis_origins(C, T, v)
            n = len(o)
            assert all(x % 16 == 0 for x in o) and o[0] == 0 and o[-1] == C - T
            assert all(b > a for a, b in zip(o, o[1:]))
            assert all(a + T - b >= v - 15 for a, b in zip(o, o[1:]))
            assert (n == 1) == (C == T)
            assert _fewer_tiles_fail(C, T, v, n), (C, T, v, n)
            covered = np.zeros(C, dtype=bool)
            for x in o:
                covered[x:x + T] = True
            assert covered.all()


def test_the_issue_s_example_is_triple_covered():
    o = tiles.axis_origins(176, 96, 32)
    assert o == (0, 32, 80)
    cover = sum(np.pad(np.ones(96, int), (x, 176 - 96 - x)) for x in o)
    assert cover.max() == 3 and cover.min() == 1 and list(np.flatnonzero(cover == 3)) == list(range(80, 96))


def test_overlap_and_size_options():
    assert tiles.overlap_px(0.25, 96) == 32 and tiles.overlap_px(0.25, 64) == 16 and tiles.overlap_px(0.5, 96) == 48
    assert tiles.overlap_px(0.25, 1280) == 320 and tiles.overlap_px(0.25, 720) == 192 and tiles.overlap_px(48, 96) == 48
    for bad in (0.0, 0.6, -0.1, float("nan"), 24, 0, -16, True, "0.25", None):
        with pytest.raises(ValueError, match="overlap"):
            tiles.overlap_px(bad, 96)
    with pytest.raises(ValueError, match="not smaller"):
        tiles.overlap_px(96, 96)
    assert tiles.target_size(None, (150, 90)) == (150, 90) and tiles.target_size((300, 200), (150, 90)) == (300, 200)
    assert tiles.target_size(2.0, (150, 90)) == (300, 180) and tiles.target_size(0.5, (151, 91)) == (round(Fraction(151, 2)), round(Fraction(91, 2)))
    for bad in (0, -1.0, (0, 5), (3,), "big", float("inf"), True, (2.5, 3)):
        with pytest.raises(ValueError, match="size"):
            tiles.target_size(bad, (150, 90))
    for kw in (dict(clip="crop"), dict(max_tiles=0), dict(max_tiles=17), dict(max_tiles=2.0), dict(overlap=0.7), dict(size=-1)):
        with pytest.raises(ValueError):
            tiles.TileConfig(**kw)


def test_plan_and_report():
    p = tiles.plan((150, 90), 64, 96)
    assert p.canvas == (160, 96) and p.target == (150, 90) and p.tile == (96, 64) and p.xs == (0, 64) and p.ys == (0, 32)
    assert p.origins == [(0, 0), (64, 0), (0, 32), (64, 32)] and p.count == 4 and not p.single  # row-major: the batch order
    assert p.cells == ((0, 8), (0, 4), 8, 12, 12, 20)
    r = p.report
    assert r["count"] == 4 and r["grid"] == (2, 2) and r["overlaps"] == ((32,), (32,)) and r["min_overlap"] == (32, 16) and r["frames"] == (150, 90)
    small = tiles.plan((90, 60), 64, 96).report  # one tile with a smaller target: the plain call, frames of the tile's size
    assert small["count"] == 1 and small["target"] == (90, 60) and small["canvas"] == (96, 64) and small["frames"] == (96, 64)
    assert tiles.plan((150, 90), 64, 96, size=(96, 64)).single and tiles.plan((90, 60), 64, 96, size=(96, 64)).single
    with pytest.raises(ValueError, match=r"24 tiles.*max_tiles = 16.*4032x3024"):  # (a 12-megapixel photo at 1280x720 tiles: 4 x 6 at the default overlap, 4 x 5 at the very least)
        tiles.plan((4032, 3024), 720, 1280, max_tiles=16)
    assert tiles.plan((4032, 3024), 720, 1280, size=0.75).count == 12
    with pytest.raises(ValueError, match="smaller than the tile"):
        tiles.plan((80, 90), 64, 96)
    with pytest.raises(ValueError, match="divisible by 16"):
        tiles.plan((150, 90), 60, 96)


def test_padded_canvas_replicates_the_edge():
    im = Image.fromarray(np.random.default_rng(0).integers(0, 256, (90, 150, 3), dtype=np.uint8))
    c = np.array(tiles.padded_canvas(im, (160, 96)))
    a = np.array(im)
    assert c.shape == (96, 160, 3) and np.array_equal(c[:90, :150], a)
    assert all(np.array_equal(c[:90, x], a[:, 149]) for x in range(150, 160)) and all(np.array_equal(c[y, :150], a[89]) for y in range(90, 96))
    assert (c[90:, 150:] == a[89, 149]).all()
    crops = tiles.tile_images(im, tiles.plan((150, 90), 64, 96))
    assert [t.size for t in crops] == [(96, 64)] * 4 and np.array_equal(np.array(crops[3]), c[32:, 64:])


# ---- reference_fuse ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _cover(xs, T, C):
    return sum(np.pad(np.ones(T, int), (x, C - T - x)) for x in xs)


def test_reference_fuse_single_cover_and_identical_tiles():
    xs, ys, th, tw, ch, cw = tiles.plan((150, 90), 64, 96).cells
    g = torch.Generator().manual_seed(1)
    t = torch.randn(4, 16, 2, th, tw, generator=g)
    t[0, 0, 0, 0, 0], t[0, 1, 0, 0, 1], t[3, 2, 1, -1, -1], t[1, 0, 0, 0, -1] = -0.0, float("inf"), float("nan"), 1e-45  # a corner is under one tile
    c = tiles.reference_fuse(t, xs, ys, ch, cw)
    one = torch.from_numpy(np.outer(_cover(ys, th, ch), _cover(xs, tw, cw)) == 1)
    assert one.any() and not one.all()
    own = tiles.reference_fuse(torch.stack([torch.full_like(t[0], float(k)) for k in range(4)]), xs, ys, ch, cw)  # which tile owns a cell
    for k, (y, x) in enumerate([(y, x) for y in ys for x in xs]):
        full = torch.zeros(16, 2, ch, cw)
        full[..., y:y + th, x:x + tw] = t[k]
        m = one & (own[0, 0] == k)
        assert m.any()
        a, b = _bits(c)[..., m], _bits(full)[..., m]
        nan = torch.isnan(full[..., m])
        assert torch.equal(a[~nan], b[~nan]) and torch.isnan(c[..., m][nan]).all()
    assert _bits(c)[0, 0, 0, 0] == _bits(torch.tensor([-0.0]))[0] and torch.isinf(c[1, 0, 0, 1]) and torch.isnan(c[2, 1, -1, -1])
    canvas = torch.randn(16, 1, ch, cw, generator=g)
    same = tiles.reference_scatter(canvas, xs, ys, th, tw)
    assert torch.equal(_bits(tiles.reference_fuse(same, xs, ys, ch, cw)), _bits(canvas))  # identical tiles return themselves
    assert torch.equal(tiles.reference_scatter(tiles.reference_fuse(t, xs, ys, ch, cw), xs, ys, th, tw)[0, ..., :4, :8], t[0, ..., :4, :8])


def test_reference_fuse_order_of_additions_matters_where_three_tiles_meet():
    """The 176-wide plan of 96-wide tiles, in cells: origins 0, 4, 10 of 12-wide tiles on 22 columns; columns 10 and 11 lie under all three.
    Column 10 is tile 0's column 10 (w = 2), tile 1's column 6 (w = 6) and tile 2's column 0 (w = 1).  With 3 * 2^60, -2^60 and 1 there the
    ascending order cancels the big products first and keeps the 1; any order that adds the 1 to a big product first loses it."""
    xs, th, tw, cw = tuple(x // 8 for x in tiles.axis_origins(176, 96, 32)), 8, 12, 22
    assert xs == (0, 4, 10) and [int(tiles.tent(tw)[k]) for k in (10, 6, 0)] == [2, 6, 1]
    big = 2.0 ** 60
    t = torch.randn(3, 2, th, tw, generator=torch.Generator().manual_seed(2))
    t[0, :, :, 10], t[1, :, :, 6], t[2, :, :, 0] = 3.0 * big, -big, 1.0
    a, b, c = 2 * 3.0 * big, 6 * -big, 1 * 1.0  # the three products of a row of weight 1: exact in double
    assert (a + b) + c == 1.0 and a + (b + c) == 0.0 and (a + c) + b == 0.0  # the order changes the sum
    out = tiles.reference_fuse(t, xs, (0,), th, cw)
    want = torch.tensor(1.0 / 9.0, dtype=torch.float64).float()  # (the row's weight cancels in the one division)
    assert torch.equal(_bits(out[:, :, 10]), _bits(want.expand(2, th)))
    # the mirror image - the same tiles flipped, in reverse order - adds the same three products the other way round ...
    mirrored = tiles.reference_fuse(t.flip(0).flip(-1), tuple(cw - tw - x for x in reversed(xs)), (0,), th, cw).flip(-1)
    assert not torch.equal(mirrored[:, :, 10], out[:, :, 10]) and (mirrored[:, :, 10] == 0).all()  # ... and loses the 1


# ---- reference_blend --------------------------------------------------------------------------------------------------------------
def _brute_blend(frames, xs, ys, target):
    n, F, TH, TW, _ = frames.shape
    W, H = target
    out = np.zeros((F, H, W, 3), np.uint8)
    wt = lambda x, T: min(x + 1, T - x)
    a = frames.numpy()
    for Y in range(H):
        for X in range(W):
            num, den = np.zeros((F, 3), object), 0
            for k, (y0, x0) in enumerate([(y, x) for y in ys for x in xs]):
                y, x = Y - y0, X - x0
                if 0 <= y < TH and 0 <= x < TW:
                    w = wt(x, TW) * wt(y, TH)
                    num = num + w * a[k, :, y, x].astype(object)
                    den += w
            for f in range(F):
                for c in range(3):
                    out[f, Y, X, c] = int((Fraction(int(num[f, c]), den) + Fraction(1, 2)).__floor__())  # round half up = (num + den // 2) // den
    return out


@pytest.mark.parametrize("xs,ys,TW,TH,target", [((0, 8), (0, 8), 16, 16, (21, 23)), ((0, 6, 14), (0,), 16, 8, (30, 8)), ((0,), (0, 5), 9, 7, (9, 12))])
def test_reference_blend_equals_fractions(xs, ys, TW, TH, target):
    fr = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (len(xs) * len(ys), 2, TH, TW, 3), dtype=np.uint8))
    fr[0, 0, :2], fr[-1, 1, -2:] = 255, 0
    assert np.array_equal(tiles.reference_blend(fr, xs, ys, target).numpy(), _brute_blend(fr, xs, ys, target))


def test_reference_blend_constant_tiles_monotone_and_bounded():
    """T = 96, v = 32: tiles of 0 and 255.  A row across the overlap rises monotonically, and neighbours differ by no more than
    `blend_step_bound` derives (8: the weight sum is 33 across the overlap, 255 // 33 + 1) - the reference reaches it."""
    p = tiles.plan((160, 96), 64, 96)
    assert p.xs == (0, 64) and p.ys == (0, 32)
    bound = tiles.blend_step_bound(96, 32)
    assert bound == 255 // 33 + 1 == 8
    fr = torch.zeros(4, 1, 64, 96, 3, dtype=torch.uint8)
    fr[1], fr[3] = 255, 255  # the right column of tiles
    out = tiles.reference_blend(fr, p.xs, p.ys, p.target).numpy().astype(int)
    rows = out[0, :, :, 0]
    assert (rows[:, :64] == 0).all() and (rows[:, 96:] == 255).all()
    d = np.diff(rows, axis=1)
    assert (d >= 0).all() and d.max() <= bound and d.max() == 8  # monotone; the derived bound holds and is met
    assert (rows == rows[0]).all()  # the other axis' weights cancel
    fr = torch.zeros(4, 1, 64, 96, 3, dtype=torch.uint8)
    fr[2], fr[3] = 255, 255  # the bottom row of tiles: T = 64, v = 32
    cols = tiles.reference_blend(fr, p.xs, p.ys, p.target).numpy().astype(int)[0, :, :, 1]
    d = np.diff(cols, axis=0)
    assert (d >= 0).all() and d.max() <= tiles.blend_step_bound(64, 32) == 255 // 33 + 1


# ---- the switch: options and the refusals that need no device ----------------------------------------------------------------------
IMAGE = Image.fromarray(np.random.default_rng(5).integers(0, 256, (90, 150, 3), dtype=np.uint8))
CALL = dict(prompt_embeds=torch.zeros(1, 4, 8), negative_prompt_embeds=torch.zeros(1, 4, 8), height=64, width=96, num_frames=5, num_inference_steps=2)


def _pipe(**transformer):
    pipe = ChronoEditPipeline()
    pipe.transformer = SimpleNamespace(**transformer)
    return pipe.enable_tiled_edit()


def test_switch_and_plan_without_a_device():
    pipe = ChronoEditPipeline()
    assert pipe._tiled is None and pipe.tile_report is None
    with pytest.raises(ValueError, match="enable_tiled_edit"):
        pipe.tile_plan((150, 90), 64, 96)
    assert pipe.enable_tiled_edit(size=[300, 180], overlap=16, clip="photo", max_tiles=16) is pipe
    assert pipe.tile_plan((150, 90), 64, 96) == tiles.plan((150, 90), 64, 96, (300, 180), 16, 16).report
    for kw in (dict(size=0), dict(overlap=0.75), dict(overlap=24), dict(clip="both"), dict(max_tiles=17), dict(max_tiles=0)):
        with pytest.raises(ValueError):
            pipe.enable_tiled_edit(**kw)
    assert pipe._tiled.clip == "photo"  # a refused option leaves the switch as it was
    assert pipe.disable_tiled_edit() is pipe and pipe._tiled is None


def test_refusals_name_the_switch():
    not_impl = [dict(image=[IMAGE, IMAGE]), dict(prompt_embeds=torch.zeros(2, 4, 8)), dict(prompt=["a", "b"], prompt_embeds=None),
                dict(num_videos_per_prompt=2), dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=1), dict(offload_model=True)]
    for kw in not_impl:
        with pytest.raises(NotImplementedError, match="enable_tiled_edit"):
            _pipe()(**dict(dict(CALL, image=IMAGE), **kw))
    for attr in ("_teacache", "_guidance_reuse", "_cfgp"):
        with pytest.raises(NotImplementedError, match="enable_tiled_edit"):
            _pipe(**{attr: object()})(image=IMAGE, **CALL)
    with pytest.raises(NotImplementedError, match="enable_tiled_edit"):
        _pipe(_sp=SimpleNamespace(sharded=True))(image=IMAGE, **CALL)
    for attr in ("_guidance_measure", "_auto_region_measure"):  # a measuring edit is refused up front, not inside the loop
        pipe = _pipe()
        setattr(pipe, attr, (3, False))
        with pytest.raises(NotImplementedError, match="enable_tiled_edit.*measur"):
            pipe(image=IMAGE, **CALL)
    with pytest.raises(NotImplementedError, match="enable_tiled_edit.*calibrate_teacache"):
        _pipe(_tea_measure=True)(image=IMAGE, **CALL)
    pipe = _pipe()
    pipe._preview = {"on_preview": print}
    with pytest.raises(NotImplementedError, match="enable_tiled_edit.*preview"):
        pipe(image=IMAGE, **CALL)
    for image in (np.zeros((90, 150, 3), np.float32), torch.zeros(1, 3, 90, 150)):
        with pytest.raises(ValueError, match="enable_tiled_edit.*PIL"):
            _pipe()(image=image, **CALL)
    # an edit region in force: two ways to decide what is edited
    with pytest.raises(ValueError, match="enable_tiled_edit"):
        _pipe().set_edit_region(np.ones((90, 150), np.uint8))(image=IMAGE, **CALL)
    with pytest.raises(ValueError, match="enable_tiled_edit"):
        _pipe(_auto_region=object())(image=IMAGE, **CALL)
    with pytest.raises(ValueError, match="enable_tiled_edit"):
        _pipe().enable_auto_focus()(image=IMAGE, **CALL)
    with pytest.raises(ValueError, match="enable_tiled_edit"):
        _pipe().enable_sketch_region()(image={"background": IMAGE, "composite": IMAGE}, **CALL)
    with pytest.raises(ValueError, match="enable_tiled_edit"):
        _pipe()(image={"background": IMAGE, "composite": IMAGE}, **CALL)
    # two ways to reach the photo's size
    with pytest.raises(ValueError, match="enable_tiled_edit"):
        _pipe().enable_detail_lift()
    with pytest.raises(ValueError, match="enable_detail_lift"):
        ChronoEditPipeline().enable_detail_lift().enable_tiled_edit()
    pipe = _pipe()
    pipe._detail_lift = object()
    with pytest.raises(ValueError, match="enable_detail_lift"):
        pipe(image=IMAGE, **CALL)
    # what the plan refuses, still before anything runs
    with pytest.raises(ValueError, match="5 tiles.*max_tiles = 4"):
        _pipe().enable_tiled_edit(size=(400, 64), overlap=16, max_tiles=4)(image=IMAGE, **CALL)
    with pytest.raises(ValueError, match="smaller than the tile"):
        _pipe().enable_tiled_edit(size=(80, 90))(image=IMAGE, **CALL)
