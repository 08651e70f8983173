"""Sketch edits from the editor's layers, host side (chronoedit_amd/layers.py): the `over` form against the installed PIL's
`Image.alpha_composite` on every (source byte, alpha, destination byte) triple, the chained composite and the strokes plane against PIL's own
recipes, the layer boxes against `getbbox()`, the entry points in the header and the signature table, the validation of the three new
arguments and of the "layers" value, and - on the call-trace rig of tests/test_call_trace_cpu.py - the black stroke on a black patch that
the difference misses and the layers find.  No GPU."""
import layers_values as V
import numpy as np
import pytest
import torch
from PIL import Image
from test_call_trace_cpu import H, W, Rig

from chronoedit_amd import focus, hiplib, layers, sketch

ENTRY_POINTS = ("ce_layers_strokes_u8", "ce_layers_over_u8")


def test_the_c_abi_declares_the_layers_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_layers_")] == list(ENTRY_POINTS) == list(layers.ENTRY_POINTS)
    assert [n for n in hiplib.SIGNATURES if n.startswith("ce_layers_")] == list(ENTRY_POINTS)
    assert "ce_layers.hip" in hiplib.SOURCES
    # the blend is ce_focus_paste_u8's, shared and not restated: one definition, in the common header
    sources = {n: open(f"{hiplib.CSRC}/{n}").read() for n in ("ce_common.h", "ce_focus.hip", "ce_layers.hip")}
    assert sources["ce_common.h"].count("uint32_t focus_blend8(") == 1
    for n in ("ce_focus.hip", "ce_layers.hip"):
        assert "focus_blend8(" in sources[n] and "uint32_t focus_blend8(" not in sources[n], n
    readme = open(hiplib.ROOT + "/README.md").read()
    assert f"{len(declared)} entry points" in readme


# ---- over ---------------------------------------------------------------------------------------------------------------------------------
def test_over_equals_alpha_composite_on_all_triples():
    """2^24 triples: per alpha one 256 x 256 picture, the source byte along a row, the destination byte along a column - in all three
    channels, each with another pairing."""
    s = np.arange(256, dtype=np.uint8)
    src = np.zeros((256, 256, 4), np.uint8)
    src[..., 0], src[..., 1], src[..., 2] = s[None, :], s[None, ::-1], (s[None, :] * 7 + 3).astype(np.uint8)
    dst = np.stack([np.broadcast_to(s[:, None], (256, 256)), np.broadcast_to((s[:, None] * 5 + 1).astype(np.uint8), (256, 256)),
                    np.broadcast_to(s[::-1, None], (256, 256))], axis=-1).copy()
    assert len({(int(a), int(b)) for a, b in zip(src[0, :, 2], dst[:, 0, 1])}) == 256  # (7 and 5 are odd: every byte once)
    background = Image.fromarray(dst, mode="RGB")
    for a in range(256):
        src[..., 3] = a
        ly = Image.fromarray(src, mode="RGBA")
        want = Image.alpha_composite(background.convert("RGBA"), ly)
        assert np.asarray(want)[..., 3].min() == 255  # the output alpha
        want_rgb = np.asarray(want.convert("RGB"))
        assert np.array_equal(want_rgb, np.asarray(want)[..., :3])  # convert("RGB") keeps the bytes
        got = layers.over(torch.from_numpy(dst.copy()), layers.LayerBox(0, (0, 0, 256, 256), torch.from_numpy(src.copy())))
        assert np.array_equal(got.numpy(), want_rgb), a
        # the closed form, spelled out
        u = src[..., :3].astype(np.int64) * a + dst.astype(np.int64) * (255 - a) + 128
        assert np.array_equal(((u >> 8) + u) >> 8, want_rgb), a


@pytest.mark.parametrize("size", [(53, 131), (33, 65), (1, 1), (400, 300)])
def test_the_chained_composite_equals_pils_chain(size):
    rng = np.random.default_rng(size[0])
    background = Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8))
    ls = V.random_layers(size, 3, seed=size[1]) if min(size) > 16 else [Image.fromarray(rng.integers(0, 256, (size[1], size[0], 4), dtype=np.uint8), mode="RGBA")] * 3
    alphas = np.concatenate([np.asarray(ly)[..., 3].ravel() for ly in ls])
    if min(size) > 16:
        assert (alphas == 0).any() and (alphas == 255).any() and ((alphas > 0) & (alphas < 255)).any()
    got = layers.composite(background, layers.boxes(ls))
    assert got.mode == "RGB" and got.size == background.size and np.array_equal(np.asarray(got), np.asarray(V.pil_composite(background, ls)))
    if min(size) > 16:  # the order matters
        assert not np.array_equal(np.asarray(got), np.asarray(V.pil_composite(background, ls[::-1])))
    # an RGBA background: convert("RGB") first, as the definition says
    rgba = background.convert("RGBA")
    assert np.array_equal(np.asarray(layers.composite(rgba, layers.boxes(ls))), np.asarray(got))


# ---- strokes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0, 1, 127, 254])
def test_the_strokes_plane_equals_pils_point_and_lighter(threshold):
    size = (53, 131)
    ls = V.random_layers(size, 3, seed=2)
    ls[0] = ls[0].copy()
    for k, a in enumerate((0, 1, 2, 127, 128, 254, 255)):  # the bytes around every threshold, in the first layer
        ls[0].putpixel((10 + k, 40), (1, 2, 3, a))
    got = layers.strokes(layers.boxes(ls), size, threshold)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (131, 53) and set(got.unique().tolist()) <= {0, 255}
    assert np.array_equal(got.numpy(), np.asarray(V.pil_strokes(size, ls, threshold)))
    assert np.array_equal(got.numpy(), layers.strokes(layers.boxes(ls[::-1]), size, threshold).numpy())  # the order does not matter
    assert not layers.strokes([], size, threshold).any()


def test_the_boxes_are_getbbox_and_an_empty_layer_is_skipped():
    size = (53, 131)
    ls = V.random_layers(size, 3, seed=4)
    ls.insert(1, Image.new("RGBA", size))
    # colour without alpha is no stroke: getbbox looks at the alpha alone for RGBA
    tinted = np.zeros((131, 53, 4), np.uint8)
    tinted[..., :3] = 200
    tinted[50:60, 7:9, 3] = 9
    ls.append(Image.fromarray(tinted, mode="RGBA"))
    lbs = layers.boxes(ls)
    assert [lb.index for lb in lbs] == [0, 2, 3, 4]
    for lb in lbs:
        assert lb.box == ls[lb.index].getbbox() and lb.rgba.dtype == torch.uint8
        l, t, r, b = lb.box
        assert tuple(lb.rgba.shape) == (b - t, r - l, 4) and np.array_equal(lb.rgba.numpy(), np.asarray(ls[lb.index])[t:b, l:r])
        outside = np.asarray(ls[lb.index])[..., 3].copy()
        outside[t:b, l:r] = 0
        assert not outside.any()  # outside the box the alpha is 0 by construction
    assert lbs[-1].box == (7, 50, 9, 60)
    assert layers.uploaded(lbs, None) == lbs


# ---- the switch ---------------------------------------------------------------------------------------------------------------------------
def test_the_new_arguments_are_validated():
    c = sketch.SketchConfig()
    assert (c.strokes, c.alpha_threshold, c.layer_prompts) == ("difference", 0, False)
    c = sketch.SketchConfig(strokes="layers", alpha_threshold=254, layer_prompts=True)
    assert (c.strokes, c.alpha_threshold, c.layer_prompts) == ("layers", 254, True)
    assert sketch.SketchConfig(2, 1, 5, 0.5, False, 7, 3, "layers", 9, True) == sketch.SketchConfig(
        grow=2, feather=1, threshold=5, context=0.5, composite=False, min_stroke=7, max_crops=3, strokes="layers", alpha_threshold=9, layer_prompts=True)
    for bad in ("alpha", "Layers", "", None, 1, True):
        with pytest.raises(ValueError, match="strokes"):
            sketch.SketchConfig(strokes=bad)
    for bad in (True, False, -1, 255, 1.0, "0", None, float("nan")):
        with pytest.raises(ValueError, match="alpha_threshold"):
            sketch.SketchConfig(strokes="layers", alpha_threshold=bad)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError, match="layer_prompts"):
            sketch.SketchConfig(strokes="layers", layer_prompts=bad)
    with pytest.raises(ValueError, match='strokes="layers"'):
        sketch.SketchConfig(layer_prompts=True)  # "difference" refuses a prompt per layer
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline.__new__(ChronoEditPipeline)
    pipe._sketch_region = None
    assert pipe.enable_sketch_region(strokes="layers", alpha_threshold=3)._sketch_region == sketch.SketchConfig(strokes="layers", alpha_threshold=3)
    assert pipe.enable_sketch_region()._sketch_region == sketch.SketchConfig()
    with pytest.raises(ValueError):
        pipe.enable_sketch_region(layer_prompts=True)


PHOTO = Image.fromarray(np.random.default_rng(1).integers(0, 256, (30, 40, 3), dtype=np.uint8))
LAYER = V.layer(PHOTO.size, [(5, 6, 15, 12)], (255, 0, 0))


def test_the_layers_value_is_validated():
    good = {"background": PHOTO, "layers": [LAYER, LAYER.convert("LA"), Image.new("RGBA", PHOTO.size)]}
    got = layers.editor_layers(good)
    assert [g.mode for g in got] == ["RGBA"] * 3 and got[0] is LAYER and np.array_equal(np.asarray(got[1])[..., 3], np.asarray(LAYER)[..., 3])
    assert layers.editor_layers({"background": PHOTO, "layers": []}) == []
    assert layers.editor_layers({"background": PHOTO}, 0, [LAYER]) == [LAYER]  # (handed in: sketch_mask's and sketch_crops's `layers=`)
    for bad, what in (({"background": PHOTO}, '"layers"'), ({"background": PHOTO, "layers": None}, '"layers"'), ({"background": PHOTO, "layers": LAYER}, '"layers"'),
                      ({"background": PHOTO, "layers": ["junk"]}, "PIL image"), ({"background": PHOTO, "layers": [np.zeros((30, 40, 4), np.uint8)]}, "PIL image"),
                      ({"background": PHOTO, "layers": [LAYER.convert("RGB")]}, "alpha"), ({"background": PHOTO, "layers": [LAYER.convert("L")]}, "alpha"),
                      ({"background": PHOTO, "layers": [LAYER, LAYER.crop((0, 0, 39, 30))]}, "size")):
        with pytest.raises(ValueError, match=what):
            layers.editor_layers(bad, 3)
    # the composite may be missing under strokes="layers", and only there
    assert sketch.editor_images(good, need_composite=False) == ([PHOTO], [None])
    with pytest.raises(ValueError, match='"composite"'):
        sketch.editor_images(good)
    with pytest.raises(ValueError, match="size"):
        sketch.editor_images(dict(good, composite=PHOTO.crop((0, 0, 39, 30))), need_composite=False)


def test_masks_from_layers_and_from_the_difference_agree_on_opaque_strokes():
    """Opaque strokes in a colour that differs from the photo at every pixel: `changed` is the same plane either way, and so is everything
    behind it - with the speck filter and with the cluster table too.  A built composite is PIL's."""
    photo = Image.fromarray(np.random.default_rng(3).integers(0, 256, (90, 120, 3), dtype=np.uint8))
    ls = [V.layer(photo.size, [(70, 10, 100, 14), (100, 70, 104, 80)], photo=photo), Image.new("RGBA", photo.size), V.layer(photo.size, [(5, 85, 7, 86)], photo=photo)]
    v = V.value(photo, ls)
    by_difference = sketch.changed(sketch.rgb_bytes(photo), sketch.rgb_bytes(v["composite"]))
    assert torch.equal(by_difference, layers.strokes(layers.boxes(ls), photo.size))
    for kw in ({}, {"min_stroke": 4}, {"max_crops": 3}, {"min_stroke": 4, "max_crops": 3}):
        d = sketch.masks(sketch.SketchConfig(3, 2, **kw), [photo], [v["composite"]])[0]
        for cp in (v["composite"], None):
            e = sketch.masks(sketch.SketchConfig(3, 2, strokes="layers", **kw), [photo], [cp], None, [ls])[0]
            assert torch.equal(e["mask_u8"], d["mask_u8"]) and np.array_equal(np.asarray(e["composite"]), np.asarray(v["composite"]))
            skip = ("mask_u8", "background", "composite", "roots", "kept", "table")
            assert {k: x for k, x in e.items() if k not in skip + ("built",)} == {k: x for k, x in d.items() if k not in skip}
            assert e.get("built", False) == (cp is None)
    with pytest.raises(ValueError, match="layers"):
        sketch.masks(sketch.SketchConfig(3, 2, strokes="layers"), [photo], [None])
    # the changed plane handed to the chains: the signatures existing callers use still work, and the plane is checked
    ch = layers.strokes(layers.boxes(ls), photo.size)
    assert torch.equal(sketch.stages(photo, None, 3, 2, 0, ch)[2], sketch.reference(photo, v["composite"], 3, 2))
    assert torch.equal(sketch.stages(photo, v["composite"], 3, 2)[2], sketch.reference(photo, v["composite"], 3, 2))
    with pytest.raises(ValueError, match="changed plane"):
        sketch.stages(photo, None, 3, 2, 0, ch.to(torch.int32))
    # one layer per entry under layer_prompts: the layer alone over the background, its own alpha
    entries = sketch.layer_entries(sketch.SketchConfig(3, 2, strokes="layers", layer_prompts=True), photo, ls)
    assert entries[1] is None and [e["layer"] for e in entries if e is not None] == [0, 2]
    for k in (0, 2):
        alone = V.pil_composite(photo, [ls[k]])
        assert np.array_equal(np.asarray(entries[k]["composite"]), np.asarray(alone))
        assert torch.equal(entries[k]["mask_u8"], sketch.reference(photo, alone, 3, 2))
    # a layer whose alpha stays at or below the threshold has a box and no stroke
    faint = V.layer(photo.size, [(10, 10, 20, 20)], (0, 0, 0), alpha=9)
    assert sketch.layer_entries(sketch.SketchConfig(3, 2, strokes="layers", alpha_threshold=9, layer_prompts=True), photo, [faint]) == [None]
    assert sketch.layer_entries(sketch.SketchConfig(3, 2, strokes="layers", alpha_threshold=8, layer_prompts=True), photo, [faint])[0]["changed_pixels"] == 100


# ---- the call, on the CPU rig ------------------------------------------------------------------------------------------------------------
def black_on_black():
    """A photo with a black patch, and a black opaque stroke on it: the composite is the photo, byte for byte."""
    a = np.random.default_rng(8).integers(1, 256, (150, 203, 3), dtype=np.uint8)
    a[20:70, 100:180] = 0
    photo = Image.fromarray(a)
    stroke = (120, 30, 160, 50)
    ls = [V.layer(photo.size, [stroke], (0, 0, 0))]
    v = V.value(photo, ls)
    assert np.array_equal(np.asarray(v["composite"]), a)
    return v, stroke


def test_a_black_stroke_on_a_black_patch_is_found_by_the_layers_only(monkeypatch):
    rig = Rig(monkeypatch)
    v, (l, t, r, b) = black_on_black()
    rig.pipe.enable_sketch_region(grow=4, feather=2)
    trace = rig.call(v, ("sketch_report", "focus_report"))
    rep = rig.pipe.sketch_report[0]
    assert rep["reason"] == "empty" and rep["changed_pixels"] == 0 and rig.pipe.focus_report is None
    assert not any(s.startswith("-> ") and "Error" in s for s in trace) and f"clip {203}x{150}" in trace  # the plain call, on the whole photo
    rig.pipe.enable_sketch_region(grow=4, feather=2, strokes="layers")
    trace = rig.call(v, ("sketch_report", "focus_report"))
    rep, frep = rig.pipe.sketch_report[0], rig.pipe.focus_report[0]
    assert rep["reason"] == "ok" and rep["changed_pixels"] == (r - l) * (b - t) and rep["strokes"] == "layers" and rep["alpha_threshold"] == 0
    assert "composite" not in rep  # the value came with one
    mask = np.array(rep["mask"])
    assert focus.mask_bbox(torch.from_numpy(mask)) == (l - 8, t - 8, r + 8, b + 8)  # the stroke's box, grown by 4 + 2 and feathered by 2 more
    assert (mask[t - 4:b + 4, l - 4:r + 4] == 255).all()
    want_box = focus.focus_box((l - 8, t - 8, r + 8, b + 8), (203, 150), (W, H), 0.25)[0]
    assert rep["box"] == frep["box"] == want_box and f"clip {want_box[2] - want_box[0]}x{want_box[3] - want_box[1]}" in trace
    # the same value without its composite: built, reported, the same call
    del v["composite"]
    assert rig.call(v, ("focus_report",)) == [s for s in trace if not s.startswith("sketch_report")]
    built = rig.pipe.sketch_report[0]["composite"]
    assert np.array_equal(np.asarray(built), np.asarray(v["background"]))
    # an empty list of layers: no strokes
    rig.call({"background": v["background"], "layers": []}, ())
    assert rig.pipe.sketch_report[0]["reason"] == "empty"
    rig.pipe.disable_sketch_region()


def test_the_default_still_ignores_junk_under_layers(monkeypatch):
    rig = Rig(monkeypatch)
    v, _ = black_on_black()
    rig.pipe.enable_sketch_region(grow=4, feather=2)
    clean = rig.call({k: x for k, x in v.items() if k != "layers"}, ("sketch_report", "focus_report"))
    assert rig.call(dict(v, layers=["junk", 3]), ("sketch_report", "focus_report")) == clean
    assert rig.call(dict(v, layers=None), ("sketch_report", "focus_report")) == clean
    assert "strokes" not in rig.pipe.sketch_report[0]
    rig.pipe.enable_sketch_region(grow=4, feather=2, strokes="layers")
    for junk in (["junk", 3], None):
        out = rig.call(dict(v, layers=junk), ("sketch_report",))
        assert out[0].startswith("-> ValueError: sketch region:") and out[-1] == "sketch_report = None" and len(out) == 2  # before anything runs
    rig.pipe.disable_sketch_region()


def test_a_prompt_per_layer_on_the_rig(monkeypatch):
    """Two layers, two prompts: two crops, the text encoder once with both prompts, CLIP on both crops, one video of the photo's size; and
    the refusals, each before the VAE or an encoder is called."""
    rig = Rig(monkeypatch)
    photo = black_on_black()[0]["background"]
    ls = [V.layer(photo.size, [(10, 10, 30, 25)], (0, 0, 0)), Image.new("RGBA", photo.size), V.layer(photo.size, [(120, 30, 160, 50)], (0, 0, 0))]
    v = {"background": photo, "layers": ls}
    rig.pipe.enable_sketch_region(grow=4, feather=2, strokes="layers", layer_prompts=True)
    trace = rig.call(v, ("sketch_report", "focus_report"), prompt=["a mug", "nothing", "a hat"], negative_prompt=["", "", ""])
    assert trace.count("t5 ['a mug', 'nothing', 'a hat']") == 1 and sum(s.startswith("clip ") for s in trace) == 1
    assert sum(s.startswith("denoise ") for s in trace) == 2 and trace[-3].startswith("-> pil 5x203x150:")  # ONE video, the photo's size
    rep = rig.pipe.sketch_report[0]
    assert [c["layer"] for c in rep["crops"]] == [0, 2] and [x["reason"] for x in rep["layers"]] == ["ok", "empty", "ok"]
    assert [x["stroke_pixels"] for x in rep["layers"]] == [20 * 15, 0, 40 * 20] and rep["layers"][1]["bbox"] is None
    assert [c["box"] for c in rep["crops"]] == [f["box"] for f in rig.pipe.focus_report] and len(rig.pipe.focus_report) == 2
    for bad, kind in ((dict(prompt=["a", "b"]), "ValueError"), (dict(prompt="a"), "ValueError"), (rig.embeds(2), "ValueError"),
                      (dict(prompt=["a", "b", "c"], num_videos_per_prompt=2), "NotImplementedError")):
        out = rig.call(v, ("sketch_report",), **bad)
        assert out[0].startswith(f"-> {kind}: a sketch edit with a prompt per layer") and out[1] == "sketch_report = None" and len(out) == 2, out
    out = rig.call([v], ("sketch_report",), prompt=["a", "b", "c"])
    assert out[0].startswith("-> NotImplementedError: a sketch edit with a prompt per layer takes ONE") and len(out) == 2
    out = rig.call({"background": photo, "layers": [ls[1], ls[1]]}, ("sketch_report",), prompt=["a", "b"])
    assert out[0].startswith("-> ValueError: a sketch edit with a prompt per layer found no stroke") and len(out) == 2
    rig.pipe.disable_sketch_region()
