"""Sketch edits, host side (chronoedit_amd/sketch.py): the entry points in the header and the signature table, `sketch.reference` against
the installed PIL's own filters byte for byte, the three guarantees of the arithmetic, the fraction rule, and every refusal.  No GPU."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageChops, ImageFilter

from chronoedit_amd import hiplib
from chronoedit_amd import sketch

ENTRY_POINTS = ("ce_sketch_changed_u8", "ce_sketch_dilate_u8", "ce_sketch_box_u8")


def test_the_c_abi_declares_the_sketch_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_sketch_")] == list(ENTRY_POINTS) == list(sketch.ENTRY_POINTS)
    assert "ce_sketch.hip" in hiplib.SOURCES


def pil_recipe(background, composite, grow, feather, threshold):
    """ImageChops.difference -> the bands' maximum -> point(v > threshold) -> MaxFilter(2 R + 1) -> BoxBlur(feather)."""
    d = ImageChops.difference(composite.convert("RGB"), background.convert("RGB"))
    r, g, b = d.split()
    m = ImageChops.lighter(ImageChops.lighter(r, g), b).point(lambda v: 255 if v > threshold else 0)
    R = grow + feather
    if R:
        m = m.filter(ImageFilter.MaxFilter(2 * R + 1))
    if feather:
        m = m.filter(ImageFilter.BoxBlur(feather))
    return torch.from_numpy(np.array(m, dtype=np.uint8))


def editor_pair(size, seed, strokes, faint=0):
    """(background, composite): a random photo and a copy with `strokes` = (left, top, right, bottom) rectangles overwritten - every byte of a
    stroke differs from the photo's by at least 128 -; faint: every other byte of the composite is moved by 1..faint."""
    SW, SH = size
    rng = np.random.default_rng(seed)
    bg = rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    cp = bg.copy()
    if faint:
        step = rng.integers(1, faint + 1, bg.shape)
        cp = np.where(bg >= 128, bg - step, bg + step).astype(np.uint8)
    for l, t, r, b in strokes:
        cp[t:b, l:r] = bg[t:b, l:r] ^ 128
    return Image.fromarray(bg), Image.fromarray(cp)


# (SW, SH), threshold, (grow, feather), strokes: two opposite corners among them, and windows larger than the image
PIL_CASES = [
    ((9, 7), 0, (0, 0), [(0, 0, 2, 1), (8, 6, 9, 7)]),
    ((16, 12), 5, (3, 0), [(5, 4, 7, 6)]),
    ((31, 17), 0, (2, 3), [(0, 16, 1, 17), (30, 0, 31, 1)]),
    ((40, 33), 5, (0, 5), [(10, 8, 20, 12), (30, 30, 31, 31)]),
    ((9, 7), 0, (7, 7), [(4, 3, 5, 4)]),
    ((64, 41), 5, (1, 12), [(0, 0, 3, 3), (60, 38, 64, 41)]),
    ((90, 23), 0, (2, 6), [(40, 10, 52, 13), (0, 22, 1, 23)]),
]


@pytest.mark.parametrize("size,threshold,radii,strokes", PIL_CASES)
def test_reference_is_pils_recipe_byte_for_byte(size, threshold, radii, strokes):
    bg, cp = editor_pair(size, sum(size) + threshold, strokes, faint=5 if threshold else 0)
    want = pil_recipe(bg, cp, radii[0], radii[1], threshold)
    got = sketch.reference(bg, cp, radii[0], radii[1], threshold)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (size[1], size[0])
    assert torch.equal(got, want)
    assert int(want.max()) == 255  # (the strokes are there: the comparison is not one of two empty planes)
    if threshold:  # the faint differences (<= threshold) mark nothing: the same mask as without them
        assert torch.equal(got, sketch.reference(bg, editor_pair(size, sum(size) + threshold, strokes)[1], radii[0], radii[1], 0))


@pytest.mark.parametrize("feather", [1, 2, 5, 9])
def test_the_box_mean_is_pils_box_blur_on_random_grey(feather):
    g = np.random.default_rng(feather).integers(0, 256, (37, 53), dtype=np.uint8)
    want = torch.from_numpy(np.array(Image.fromarray(g).filter(ImageFilter.BoxBlur(feather)), dtype=np.uint8))
    x = torch.from_numpy(g)
    assert torch.equal(sketch.box(sketch.box(x, feather, 0), feather, 1), want)


def test_the_stages_against_brute_force():
    rng = np.random.default_rng(3)
    H, W, r = 6, 11, 2
    x = torch.from_numpy(rng.integers(0, 256, (H, W), dtype=np.uint8))
    b = torch.from_numpy((rng.random((H, W)) < 0.1).astype(np.uint8) * 255)
    ww = (1 << 24) // (2 * r + 1)
    for axis, n in ((0, W), (1, H)):
        bx, dl = sketch.box(x, r, axis), sketch.dilate(b, r, axis)
        assert bx.is_contiguous() and dl.is_contiguous()
        for y in range(H):
            for xx in range(W):
                i = xx if axis == 0 else y
                at = lambda t, j: int(t[y, j]) if axis == 0 else int(t[j, xx])
                acc = sum(at(x, min(max(j, 0), n - 1)) for j in range(i - r, i + r + 1))
                assert int(bx[y, xx]) == (acc * ww + (1 << 23)) >> 24
                assert int(dl[y, xx]) == max(at(b, j) for j in range(max(i - r, 0), min(i + r, n - 1) + 1))


def test_the_three_guarantees():
    grow, feather = 3, 4
    bg, cp = editor_pair((83, 61), 11, [(20, 15, 31, 22), (70, 50, 72, 58), (0, 40, 2, 41)])
    ch, grown, mask = sketch.stages(bg, cp, grow, feather, 0)
    assert torch.equal(mask, sketch.reference(bg, cp, grow, feather, 0))
    ys, xs = torch.nonzero(ch, as_tuple=True)
    Y, X = torch.arange(61).reshape(-1, 1, 1), torch.arange(83).reshape(1, -1, 1)
    dist = torch.maximum((Y - ys.reshape(1, 1, -1)).abs(), (X - xs.reshape(1, 1, -1)).abs()).amin(2)  # Chebyshev, to the nearest changed pixel
    assert bool((mask[dist <= grow] == 255).all()) and bool((dist <= grow).any())
    assert bool((mask[dist > grow + 2 * feather] == 0).all()) and bool((dist > grow + 2 * feather).any())
    assert 0 < int(((mask > 0) & (mask < 255)).sum())
    a, b = np.asarray(bg), np.asarray(cp)
    assert np.array_equal(a[mask.numpy() < 255], b[mask.numpy() < 255])  # threshold 0: the strokes lie where the mask is 255
    assert not np.array_equal(a, b)


def test_the_fraction_rule():
    assert sketch.pixels(0.02, (4032, 3024)) == 81 and sketch.pixels(0.01, (4032, 3024)) == 41
    assert sketch.pixels(0.02, (3024, 4032)) == 81  # the longer side, whichever it is
    assert sketch.pixels(0.0, (4032, 3024)) == 0 and sketch.pixels(0.5, (7, 3)) == 4
    assert sketch.pixels(12, (4032, 3024)) == 12 and sketch.pixels(0, (1, 1)) == 0
    c = sketch.SketchConfig()
    assert (c.grow, c.feather, c.threshold, c.context, c.composite) == (0.02, 0.01, 0, 0.25, True)
    assert c.pixels((4032, 3024)) == (81, 41) and c.pixels((203, 150)) == (5, 3)
    assert sketch.SketchConfig(grow=4000, feather=96).pixels((10, 10)) == (4000, 96)
    assert sketch.SketchConfig(grow=0.9, feather=0.01).pixels((100, 100)) == (90, 1)
    with pytest.raises(ValueError):
        sketch.SketchConfig(grow=0.9, feather=0.01).pixels((8000, 100))  # 7200 + 80 > 4096


def test_config_validation():
    bad = [dict(grow=-1), dict(feather=-1), dict(grow=1.0), dict(feather=1.5), dict(grow=-0.1), dict(grow=float("nan")), dict(grow="3"),
           dict(grow=True), dict(grow=4000, feather=97), dict(grow=0, feather=1025), dict(grow=4097, feather=0), dict(threshold=-1),
           dict(threshold=255), dict(threshold=1.0), dict(threshold=True), dict(context=-0.1), dict(context=float("nan")), dict(composite=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            sketch.SketchConfig(**kw)
    with pytest.raises(ValueError):
        sketch.reference(*editor_pair((8, 8), 0, []), 4000, 97)
    with pytest.raises(ValueError):
        sketch.reference(*editor_pair((8, 8), 0, []), 1, 1, 255)


def test_the_editor_value():
    bg, cp = editor_pair((12, 9), 0, [(1, 1, 3, 3)])
    assert sketch.is_editor_value({"background": bg, "composite": cp}) and sketch.is_editor_value([{}, {}])
    assert not sketch.is_editor_value(bg) and not sketch.is_editor_value([bg]) and not sketch.is_editor_value([]) and not sketch.is_editor_value([{}, bg])
    assert sketch.editor_images({"background": bg, "composite": cp, "layers": [object()]}) == ([bg], [cp])  # other keys are ignored
    assert sketch.editor_images([{"background": bg, "composite": cp}, {"background": cp, "composite": bg}]) == ([bg, cp], [cp, bg])
    other = Image.new("RGB", (12, 10))
    for value in ({"background": bg}, {"composite": cp}, {"background": bg, "composite": None}, {"background": None, "composite": cp},
                  {"background": bg, "composite": other}, {"background": bg, "composite": np.asarray(cp)}, [{"background": bg, "composite": cp}, {}]):
        with pytest.raises(ValueError):
            sketch.editor_images(value)
    with pytest.raises(ValueError):
        sketch.reference(bg, other, 1, 1)
    # an "RGBA" layer stack flattened by the editor, or a palette image: the RGB bytes count
    assert torch.equal(sketch.reference(bg.convert("RGBA"), cp, 1, 1), sketch.reference(bg, cp, 1, 1))


def test_the_pipeline_switch_and_its_refusals():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline()
    bg, cp = editor_pair((40, 30), 1, [(10, 8, 14, 12)])
    assert pipe._sketch_region is None and pipe.sketch_report is None
    with pytest.raises(ValueError, match="enable_sketch_region"):
        pipe(image={"background": bg, "composite": cp}, prompt="x", height=32, width=48)
    with pytest.raises(ValueError, match="enable_sketch_region"):
        pipe(image=[{"background": bg, "composite": cp}], prompt=["x"], height=32, width=48)
    with pytest.raises(ValueError, match="enable_sketch_region"):
        pipe.sketch_mask(bg, cp)
    assert pipe.enable_sketch_region() is pipe and pipe._sketch_region == sketch.SketchConfig()
    assert pipe.enable_sketch_region(grow=2, feather=1, threshold=5, context=0.5, composite=False)._sketch_region == sketch.SketchConfig(2, 1, 5, 0.5, False)
    for kw in (dict(grow=-1), dict(feather=2000), dict(threshold=255), dict(context=-1.0)):
        with pytest.raises(ValueError):
            pipe.enable_sketch_region(**kw)
    m = pipe.sketch_mask(bg, cp)
    assert m.mode == "L" and m.size == (40, 30)
    assert torch.equal(torch.from_numpy(np.array(m)), sketch.reference(bg, cp, 2, 1, 5))
    other = Image.new("RGB", (40, 31))
    for value in ({"background": bg, "composite": other}, {"background": bg}, {"background": bg, "composite": None}, {"composite": cp},
                  {"background": None, "composite": cp}):
        with pytest.raises(ValueError):
            pipe(image=value, prompt="x", height=32, width=48)
    with pytest.raises(ValueError):
        pipe.sketch_mask(bg, other)
    assert pipe.disable_sketch_region() is pipe and pipe._sketch_region is None
    with pytest.raises(ValueError, match="enable_sketch_region"):
        pipe(image={"background": bg, "composite": cp}, prompt="x", height=32, width=48)
