"""Sketch edits from the editor's layers through `ChronoEditPipeline.__call__` (`enable_sketch_region(strokes="layers", alpha_threshold=,
layer_prompts=)`), on the tiny synthetic pipeline of tests/test_sketch_gpu.py (whose helpers, and those of tests/test_clusters_gpu.py, are
used here): a 400 x 300 photo, a 96 x 64 edit, 5 frames, grow 3, feather 4.  Every comparison is byte equality.

Where the strokes are opaque and differ from the photo the layers give the call the difference gives; a black stroke on a black patch is an
edit only with the layers; a value without a composite is the call with PIL's chained `alpha_composite` as its composite; and two layers
with two prompts are ONE video, equal to a second implementation from public pieces: `set_edit_region([m0, m1], composite=False)` +
`enable_region_focus` + `__call__([composite_0, composite_1])` with the two prompt rows and the noise row repeated, then PIL's chained paste
into the background through the masks."""
import contextlib

import layers_values as V
import numpy as np
import pytest
import test_clusters_gpu as C
import test_sketch_gpu as T
import torch
from PIL import Image
from test_sketch_gpu import pipe  # noqa: F401  (fixture)

from chronoedit_amd import clusters, layers, sketch, sparse_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, GROW, FEATHER, CONTEXT = C.W, C.H, C.GROW, C.FEATHER, C.CONTEXT
PHOTO, NW, SE = C.PHOTO, C.NW, C.SE
assert (NW, SE, PHOTO.size, W, H, GROW, FEATHER) == ((20, 20, 50, 40), (350, 250, 380, 280), (400, 300), 96, 64, 3, 4)
NEW_KEYS = ("strokes", "alpha_threshold", "composite")


def opaque(photo, strokes):
    """Opaque strokes in a colour that differs from the photo at every stroke pixel (every byte moved by 128), all in one layer."""
    v = V.value(photo, [V.layer(photo.size, strokes, photo=photo)])
    assert np.array_equal(np.asarray(v["composite"]), np.asarray(T.draw(photo, strokes)))
    by_difference = sketch.changed(sketch.rgb_bytes(photo), sketch.rgb_bytes(v["composite"]))
    assert torch.equal(by_difference, layers.strokes(layers.boxes(v["layers"]), photo.size)) and by_difference.any()  # the precondition
    return v


ONE = opaque(T.IMAGE, T.STROKES)
TWO = opaque(PHOTO, [NW, SE])


@contextlib.contextmanager
def graph(pipe, use_graph):  # noqa: F811
    """The calls inside run replayed (the default) or eager."""
    pipe.use_graph = use_graph
    try:
        yield
    finally:
        pipe.use_graph = True


def strip(report):
    """A report without its images and without the keys the layers add: what must equal the difference mode's."""
    out = []
    for rep in report:
        r = {k: v for k, v in rep.items() if k not in NEW_KEYS + ("mask",)}
        if "crops" in r:
            r["crops"] = [{k: v for k, v in c.items() if k != "mask"} for c in r["crops"]]
        out.append(r)
    return out


def images(report):
    return [np.array(rep["mask"]) for rep in report] + [np.array(c["mask"]) for rep in report for c in rep.get("crops", [])]


def assert_layers_equal_difference(pipe, value, kw, **switch):  # noqa: F811
    want, wreport, wfocus = T.sketched(pipe, value, kw, **switch)
    got, report, focus_report = T.sketched(pipe, value, kw, strokes="layers", **switch)
    want, got = T.arrays(want), T.arrays(got)
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert strip(report) == strip(wreport) and focus_report == wfocus and wfocus is not None
    assert all(np.array_equal(a, b) for a, b in zip(images(report), images(wreport))) and len(images(report)) == len(images(wreport))
    for rep in report:
        assert rep["strokes"] == "layers" and rep["alpha_threshold"] == 0 and "composite" not in rep
    assert not any(k in rep for rep in wreport for k in NEW_KEYS)
    return got, report


# ---- 1. layers mode against difference mode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_opaque_strokes_give_the_difference_modes_call(pipe, use_graph, guidance_scale):  # noqa: F811
    kw = T.inputs(guidance_scale=guidance_scale)
    pipe.use_graph = use_graph
    try:
        got, report = assert_layers_equal_difference(pipe, ONE, kw)
        two, treport = assert_layers_equal_difference(pipe, TWO, kw, max_crops=2)
    finally:
        pipe.use_graph = True
    assert report[0]["reason"] == "ok" and report[0]["changed_pixels"] == 40 * 8 + 8 * 30 + 9 * 14 and got[0].shape == (5, 150, 203, 3)
    assert treport[0]["crops_reason"] == "crops" and len(treport[0]["crops"]) == 2 and two[0].shape == (5, 300, 400, 3)


@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_opaque_strokes_with_the_speck_filter_sparse_steps_and_on_the_host(pipe, use_graph, guidance_scale):  # noqa: F811
    kw = T.inputs(guidance_scale=guidance_scale)
    specked = opaque(PHOTO, [NW, (200, 150, 202, 151)])
    with graph(pipe, use_graph):
        _, report = assert_layers_equal_difference(pipe, specked, kw, min_stroke=4)
        assert report[0]["dropped_clusters"] == 1 and report[0]["dropped_pixels"] == 2
        pipe.enable_sparse_region(refresh_every=2)
        try:
            small = opaque(T.IMAGE, [(30, 106, 40, 112)])
            assert_layers_equal_difference(pipe, small, kw, context=1.0)
            rep = pipe.transformer.sparse_report
            assert rep["plan"] == ["refresh", "sparse"] and sparse_region.PAD <= rep["active"] < rep["tokens"] == 48, rep
        finally:
            pipe.disable_sparse_region()
        on_device = [T.sketched(pipe, v, kw, strokes="layers", max_crops=m) for v, m in ((ONE, 1), (TWO, 2))]
        pipe.enable_device_image_io(False)
        try:
            on_host = [assert_layers_equal_difference(pipe, v, kw, max_crops=m) for v, m in ((ONE, 1), (TWO, 2))]
        finally:
            pipe.enable_device_image_io(True)
    for (dev_frames, dev_report, _), (host_frames, host_report) in zip(on_device, on_host):
        assert np.array_equal(T.arrays(dev_frames)[0], host_frames[0]) and strip(dev_report) == strip(host_report)
        assert all(np.array_equal(a, b) for a, b in zip(images(dev_report), images(host_report)))


# ---- 2. the black-on-black value ------------------------------------------------------------------------------------------------------------
def black_on_black():
    a = np.array(T.IMAGE)
    a[20:70, 100:180] = 0
    photo = Image.fromarray(a)
    stroke = (120, 30, 160, 50)
    v = V.value(photo, [V.layer(photo.size, [stroke], (0, 0, 0))])
    assert np.array_equal(np.asarray(v["composite"]), a)  # the stroke changes no byte
    return v, stroke


@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_a_black_stroke_on_a_black_patch(pipe, use_graph, guidance_scale):  # noqa: F811
    kw = T.inputs(guidance_scale=guidance_scale)
    v, stroke = black_on_black()
    pipe.use_graph = use_graph
    try:
        plain = T.arrays(T.call(pipe, v["composite"], kw))[0]
        missed, mreport, mfocus = T.sketched(pipe, v, kw)
        assert mreport[0]["reason"] == "empty" and mfocus is None and np.array_equal(T.arrays(missed)[0], plain)  # the difference sees nothing
        got, report, focus_report = T.sketched(pipe, v, kw, strokes="layers")
        mask = Image.fromarray(sketch.reference(v["background"], T.draw(v["background"], [stroke]), GROW, FEATHER).numpy(), mode="L")
        want, wreport = T.explicit(pipe, v, [mask], kw)
    finally:
        pipe.use_graph = True
    got = T.arrays(got)
    assert got[0].shape == want[0].shape == (5, 150, 203, 3) and np.array_equal(got[0], want[0]) and not np.array_equal(got[0][-1], np.asarray(v["background"]))
    assert focus_report == wreport and report[0]["reason"] == "ok" and report[0]["changed_pixels"] == 40 * 20
    assert np.array_equal(np.array(report[0]["mask"]), np.array(mask))
    T.assert_mask_is_not_trivial(report[0])


# ---- 3. composite missing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_a_value_without_a_composite_gets_pils_chain(pipe, use_graph, guidance_scale):  # noqa: F811
    kw = T.inputs(guidance_scale=guidance_scale)
    ls = [V.layer(T.IMAGE.size, T.STROKES[:1], (255, 0, 0), alpha=200), Image.new("RGBA", T.IMAGE.size), V.layer(T.IMAGE.size, T.STROKES[1:], (0, 0, 255), alpha=90),
          V.layer(T.IMAGE.size, [(155, 14, 165, 30)], (0, 255, 0), alpha=255)]  # half-transparent strokes, and one over the two others
    chain = V.pil_composite(T.IMAGE, ls)
    assert not np.array_equal(np.asarray(chain), np.asarray(V.pil_composite(T.IMAGE, ls[::-1])))
    pipe.use_graph = use_graph
    try:
        want, wreport, wfocus = T.sketched(pipe, {"background": T.IMAGE, "layers": ls, "composite": chain}, kw, strokes="layers")
        for missing in ({"background": T.IMAGE, "layers": ls}, {"background": T.IMAGE, "layers": ls, "composite": None}):
            got, report, focus_report = T.sketched(pipe, missing, kw, strokes="layers")
            assert np.array_equal(T.arrays(got)[0], T.arrays(want)[0]) and focus_report == wfocus and strip(report) == strip(wreport)
            built = report[0]["composite"]
            assert built.mode == "RGB" and built.size == T.IMAGE.size and np.array_equal(np.asarray(built), np.asarray(chain))
    finally:
        pipe.use_graph = True
    assert "composite" not in wreport[0] and wreport[0]["reason"] == "ok"
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER, strokes="layers", alpha_threshold=90)
    try:
        shown = pipe.sketch_mask(T.IMAGE, None, layers=ls)
        crops = pipe.sketch_crops(T.IMAGE, None, H, W, layers=ls)
        with pytest.raises(ValueError, match='"layers"'):
            pipe.sketch_mask(T.IMAGE, chain)
    finally:
        pipe.disable_sketch_region()
    stronger = [ls[0], ls[3]]  # (alpha 90 is not above the threshold)
    assert np.array_equal(np.array(shown), sketch.reference(T.IMAGE, V.pil_composite(T.IMAGE, stronger), GROW, FEATHER).numpy())
    assert len(crops) == 1 and np.array_equal(np.array(crops[0]["mask"]), np.array(shown))


# ---- 4. - 6. a prompt per layer -------------------------------------------------------------------------------------------------------------
def layered_inputs(n, guidance_scale=5.0):
    """n prompt rows, ONE noise row."""
    kw = T.inputs(n=n, guidance_scale=guidance_scale)
    return dict(kw, latents=kw["latents"][:1].clone())


def with_rows(kw, rows):
    idx = torch.tensor(rows)
    return dict(kw, **{k: kw[k].index_select(0, idx.to(kw[k].device)) for k in ("prompt_embeds", "negative_prompt_embeds")})


def layer_plan(photo, layer, max_crops=1):
    """(the composite of the layer alone, its host entry, its masks as PIL in paste order, its boxes): the definition, on the host."""
    alone = V.pil_composite(photo, [layer])
    cfg = sketch.SketchConfig(GROW, FEATHER, context=CONTEXT, max_crops=max_crops)
    e = sketch.masks(cfg, [photo], [alone])[0]
    plans = [sketch.focus_plan(e, W, H, CONTEXT)]
    if max_crops >= 2:
        crops = clusters.plan(e, max_crops, W, H, CONTEXT)
        plans = crops.plans if crops.reason == "crops" else plans
    return alone, e, [Image.fromarray(p.host_mask().numpy(), mode="L") for p in plans], [p.report["box"] for p in plans]


def second_implementation(pipe, photo, composites, masks, kw, rows):  # noqa: F811
    """-> (frames uint8 [F, SH, SW, 3], the focused call's focus_report): sample j edits composites[j] under masks[j] from prompt row rows[j]
    and the one noise row; the boxes' contents go into the background through the masks, in order."""
    n = len(masks)
    kw = dict(with_rows(kw, rows), latents=kw["latents"].repeat(n, 1, 1, 1, 1))
    pipe.enable_region_focus(CONTEXT).set_edit_region(masks, composite=False)
    try:
        content = T.arrays(T.call(pipe, composites, kw))
        freport = pipe.focus_report
    finally:
        pipe.disable_region_focus().clear_edit_region()
    frames = []
    for f in range(content[0].shape[0]):
        canvas = photo.copy()
        for g, m in enumerate(masks):
            box = freport[g]["box"]
            canvas.paste(Image.fromarray(content[g][f]).crop(box), box[:2], m.crop(box))
        frames.append(np.asarray(canvas))
    return np.stack(frames), freport


def prompted(pipe, value, kw, **switch):  # noqa: F811
    got, report, freport = T.sketched(pipe, value, kw, strokes="layers", layer_prompts=True, **switch)
    got = T.arrays(got)
    assert len(got) == 1 and len(report) == 1
    return got[0], report[0], freport


@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_two_layers_two_prompts_equal_the_second_implementation(pipe, use_graph, guidance_scale):  # noqa: F811
    ls = [V.layer(PHOTO.size, [NW], photo=PHOTO), V.layer(PHOTO.size, [SE], photo=PHOTO)]
    value = {"background": PHOTO, "layers": ls, "composite": V.pil_composite(PHOTO, ls)}
    kw = layered_inputs(2, guidance_scale)
    assert not torch.equal(kw["prompt_embeds"][0], kw["prompt_embeds"][1])
    plans = [layer_plan(PHOTO, ly) for ly in ls]
    pipe.use_graph = use_graph
    try:
        frames, rep, freport = prompted(pipe, value, kw)
        want, wreport = second_implementation(pipe, PHOTO, [p[0] for p in plans], [p[2][0] for p in plans], kw, [0, 1])
        swapped, _, _ = prompted(pipe, value, with_rows(kw, [1, 0]))
    finally:
        pipe.use_graph = True
    assert frames.shape == want.shape == (5, 300, 400, 3) and np.array_equal(frames, want)  # ONE video of 400 x 300
    assert not np.array_equal(swapped, frames)  # the rows are not ignored
    boxes = [p[3][0] for p in plans]
    assert [f["box"] for f in freport] == [f["box"] for f in wreport] == boxes == [(0, 0, 102, 68), (283, 222, 400, 300)] and freport == wreport
    assert [c["layer"] for c in rep["crops"]] == [0, 1] and [c["box"] for c in rep["crops"]] == boxes
    assert rep["layers"] == [{"bbox": p[1]["bbox"], "stroke_pixels": p[1]["changed_pixels"], "reason": "ok"} for p in plans]
    assert rep["reason"] == "layers" and rep["changed_pixels"] == 30 * 20 + 30 * 30 and rep["source_size"] == (400, 300) and rep["edit_size"] == (W, H)
    m0, m1 = (np.array(c["mask"]) for c in rep["crops"])
    assert np.array_equal(m0, np.array(plans[0][2][0])) and np.array_equal(m1, np.array(plans[1][2][0]))
    nowhere, bg = (m0 == 0) & (m1 == 0), np.array(PHOTO)
    for f in range(5):
        assert np.array_equal(frames[f][nowhere], bg[nowhere]), f  # the background's bytes wherever both masks are 0
    for c in rep["crops"]:
        T.assert_mask_is_not_trivial(c)
    # without a composite in the value: the same call (the per-layer composites are built either way)
    assert np.array_equal(prompted(pipe, {"background": PHOTO, "layers": ls}, kw)[0], frames)


@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_overlapping_layers_the_later_one_wins_and_an_empty_one_consumes_its_prompt(pipe, use_graph, guidance_scale):  # noqa: F811
    first, second = (20, 20, 50, 40), (40, 30, 70, 50)
    ls = [V.layer(PHOTO.size, [first], (255, 0, 0), alpha=255), Image.new("RGBA", PHOTO.size), V.layer(PHOTO.size, [second], (0, 0, 255), alpha=140)]
    value = {"background": PHOTO, "layers": ls}
    kw = layered_inputs(3, guidance_scale)
    plans = [layer_plan(PHOTO, ls[k]) for k in (0, 2)]
    with graph(pipe, use_graph):
        frames, rep, freport = prompted(pipe, value, kw)
        want, wreport = second_implementation(pipe, PHOTO, [p[0] for p in plans], [p[2][0] for p in plans], kw, [0, 2])
        other, _ = second_implementation(pipe, PHOTO, [p[0] for p in plans[::-1]], [p[2][0] for p in plans[::-1]], kw, [2, 0])
        # the middle prompt is consumed: with the last two rows swapped the last layer gets the empty layer's prompt
        moved = prompted(pipe, value, with_rows(kw, [0, 2, 1]))[0]
        kept = prompted(pipe, value, with_rows(kw, [0, 0, 2]))[0]
    assert np.array_equal(frames, want) and freport == wreport
    m0, m1 = (np.array(p[2][0]) for p in plans)
    assert ((m0 == 255) & (m1 == 255)).any()  # the masks overlap ...
    assert not np.array_equal(other, want)  # ... and the order of the paste shows
    assert [x["reason"] for x in rep["layers"]] == ["ok", "empty", "ok"] and rep["layers"][1] == {"bbox": None, "stroke_pixels": 0, "reason": "empty"}
    assert [c["layer"] for c in rep["crops"]] == [0, 2] and rep["alpha_threshold"] == 0
    assert not np.array_equal(moved, frames) and np.array_equal(kept, frames)


@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_one_layer_with_both_corners_is_the_two_crop_call(pipe, use_graph, guidance_scale):  # noqa: F811
    kw = T.inputs(guidance_scale=guidance_scale)
    kw2 = layered_inputs(2, guidance_scale)
    extra = dict(TWO, layers=TWO["layers"] + [V.layer(PHOTO.size, [(190, 140, 210, 160)], photo=PHOTO)])
    alone = layer_plan(PHOTO, extra["layers"][1])
    with graph(pipe, use_graph):
        want, wreport, wfocus = T.sketched(pipe, TWO, kw, strokes="layers", max_crops=2)
        frames, rep, freport = prompted(pipe, TWO, kw, max_crops=2)
        three, rep3, freport3 = prompted(pipe, extra, kw2, max_crops=2)
        # the repeated row: crops 0 and 1 run from prompt row 0, crop 2 from row 1 - the explicit-mask call with the rows [0, 0, 1]
        masks = [c["mask"] for c in rep["crops"]] + [alone[2][0]]
        want3, wreport3 = second_implementation(pipe, PHOTO, [TWO["composite"]] * 2 + [alone[0]], masks, kw2, [0, 0, 1])
    assert np.array_equal(frames, T.arrays(want)[0]) and freport == wfocus and len(freport) == 2
    assert [c["layer"] for c in rep["crops"]] == [0, 0] and rep["layers"][0]["reason"] == "crops"
    assert [{k: v for k, v in c.items() if k not in ("mask", "layer")} for c in rep["crops"]] == strip(wreport)[0]["crops"]
    assert [c["layer"] for c in rep3["crops"]] == [0, 0, 1] and [x["reason"] for x in rep3["layers"]] == ["crops", "ok"] and len(freport3) == 3
    assert np.array_equal(three, want3) and freport3 == wreport3


# ---- 7. the refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_refusals_come_before_the_vae_and_the_encoders(pipe, monkeypatch):  # noqa: F811
    ls = [V.layer(PHOTO.size, [NW], photo=PHOTO), V.layer(PHOTO.size, [SE], photo=PHOTO)]
    value = {"background": PHOTO, "layers": ls}
    calls = []
    encode, clip = pipe.vae.encode, pipe.encode_image
    monkeypatch.setattr(pipe.vae, "encode", lambda *a, **k: calls.append("vae") or encode(*a, **k))
    monkeypatch.setattr(pipe, "encode_image", lambda *a, **k: calls.append("clip") or clip(*a, **k))

    chain = sketch.layer_entries
    monkeypatch.setattr(sketch, "layer_entries", lambda *a, **k: calls.append("chain") or chain(*a, **k))

    def refused(kind, match, v, kw, launched=[], **switch):
        """launched []: decided on the host, before an upload or a launch; ["chain"]: behind the layers' mask chains, before any encoder."""
        pipe.enable_sketch_region(**dict(dict(grow=GROW, feather=FEATHER, strokes="layers", layer_prompts=True), **switch))
        try:
            with pytest.raises(kind, match=match):
                T.call(pipe, v, kw)
        finally:
            pipe.disable_sketch_region()
        assert pipe.sketch_report is None and calls == launched
        del calls[:]

    refused(ValueError, "one prompt per layer", value, layered_inputs(1))
    refused(ValueError, "one prompt per layer", value, layered_inputs(3))
    refused(ValueError, "no stroke", {"background": PHOTO, "layers": [Image.new("RGBA", PHOTO.size)] * 2}, layered_inputs(2))
    refused(ValueError, "no stroke", dict(value, layers=[V.layer(PHOTO.size, [NW], (0, 0, 0), alpha=7)] * 2), layered_inputs(2), alpha_threshold=7)
    many = [V.layer(PHOTO.size, [(20 + 120 * (k % 3), 20 + 100 * (k // 3), 30 + 120 * (k % 3), 30 + 100 * (k // 3))], photo=PHOTO) for k in range(9)]
    refused(ValueError, "at most 16 crops", {"background": PHOTO, "layers": many + many[:8]}, layered_inputs(17))
    refused(NotImplementedError, "ONE editor value", [value], layered_inputs(2))
    # what only the chain knows: the speck filter drops every stroke (600 and 900 pixels); two crops per layer make 18 of nine layers
    refused(ValueError, "no stroke", value, layered_inputs(2), launched=["chain"], min_stroke=1000)
    pairs = [V.layer(PHOTO.size, [(10 + 40 * k, 10, 20 + 40 * k, 20), (10 + 40 * k, 270, 20 + 40 * k, 280)], photo=PHOTO) for k in range(9)]
    refused(ValueError, "at most 16 crops", {"background": PHOTO, "layers": pairs}, layered_inputs(9), launched=["chain"], max_crops=2)
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER, strokes="layers", layer_prompts=True)
    try:
        with pytest.raises(NotImplementedError, match="num_videos_per_prompt"):
            T.call(pipe, value, layered_inputs(2), num_videos_per_prompt=2)
        assert pipe.sketch_report is None and calls == []
        with pytest.raises(ValueError, match="latents"):
            T.call(pipe, value, T.inputs(n=2))  # two noise rows for one value
        assert calls == ["chain"]
        del calls[:]
    finally:
        pipe.disable_sketch_region()
    with pytest.raises(ValueError, match="layer_prompts"):
        pipe.enable_sketch_region(layer_prompts=True)  # "difference" refuses it
    for junk in (None, ["junk"], [PHOTO]):
        with pytest.raises(ValueError, match="sketch region"):
            T.sketched(pipe, {"background": PHOTO, "composite": PHOTO, "layers": junk}, T.inputs(), strokes="layers")
        assert pipe.sketch_report is None and calls == []
    # an explicit mask still wins: the value stands for its composite (built here), one prompt
    m = np.zeros((300, 400), np.uint8)
    m[90:130, 20:70] = 255
    kw = T.inputs()
    built = V.pil_composite(PHOTO, ls)
    want, wreport = T.explicit(pipe, {"composite": built}, [Image.fromarray(m)], kw)
    del calls[:]
    pipe.enable_region_focus().set_edit_region(Image.fromarray(m))
    try:
        got, report, freport = T.sketched(pipe, value, kw, strokes="layers", layer_prompts=True)
    finally:
        pipe.disable_region_focus().clear_edit_region()
    assert report is None and freport == wreport and np.array_equal(T.arrays(got)[0], want[0]) and "vae" in calls and "chain" not in calls


# ---- 8. the reads ---------------------------------------------------------------------------------------------------------------------------
def test_the_reads_in_front_of_the_edit(pipe, monkeypatch):  # noqa: F811
    ls = [TWO["layers"][0], Image.new("RGBA", PHOTO.size), V.layer(PHOTO.size, [(190, 140, 210, 160)], photo=PHOTO)]
    value = {"background": PHOTO, "layers": ls}
    kw = layered_inputs(3)
    plans = [layer_plan(PHOTO, ls[0], 2), layer_plan(PHOTO, ls[2], 2)]
    assert [len(p[2]) for p in plans] == [2, 1]
    masks = plans[0][2] + plans[1][2]
    composites = [plans[0][0]] * 2 + [plans[1][0]]
    reads = T.HostReads(monkeypatch)
    before = {}

    def first_step(name):
        def cb(p, i, t, kwargs):
            before.setdefault(name, list(reads.log))
            return {}
        return cb

    first = 10 + 1 + 8 * clusters.ROWS  # the ten integers, the count, the table
    dev = torch.device(DEV)
    del reads.log[:]
    e = sketch.masks(sketch.SketchConfig(GROW, FEATHER, strokes="layers"), [PHOTO], [None], dev, [ls])[0]
    assert reads.log == [10] and e["mask_u8"] is None and e["cp_u8"].is_cuda and e["built"]  # one read per value, the composite built without one
    del reads.log[:]
    sketch.masks(sketch.SketchConfig(GROW, FEATHER, min_stroke=4, strokes="layers"), [PHOTO], [TWO["composite"]], dev, [ls])
    assert reads.log == [14]
    del reads.log[:]
    entries = sketch.layer_entries(sketch.SketchConfig(GROW, FEATHER, max_crops=2, strokes="layers", layer_prompts=True), PHOTO, ls, dev)
    assert reads.log == [first, first] and entries[1] is None  # one per layer with strokes
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=2, strokes="layers", layer_prompts=True)
    try:
        del reads.log[:]
        got = T.arrays(T.call(pipe, value, kw, callback_on_step_end=first_step("layers")))[0]
    finally:
        pipe.disable_sketch_region()
    del reads.log[:]
    pipe.enable_region_focus(CONTEXT).set_edit_region(masks, composite=False)
    try:
        T.call(pipe, composites, dict(with_rows(kw, [0, 0, 2]), latents=kw["latents"].repeat(3, 1, 1, 1, 1)), callback_on_step_end=first_step("explicit"))
    finally:
        pipe.disable_region_focus().clear_edit_region()
    extra = list(before["layers"])
    for n in before["explicit"]:
        extra.remove(n)  # (whatever the focused call itself reads in front of the first step, this call reads too)
    # every stroked layer's counts, then the boxes of the one layer that has two groups: two reads for that layer, one for the other
    assert extra == [first, first, 10], (before["layers"], before["explicit"])
    assert 400 * 300 not in before["layers"] and 400 * 300 * 3 not in before["layers"] and got.shape == (5, 300, 400, 3)
