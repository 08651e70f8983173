"""Sketch edits with one crop per group of stroke clusters through `ChronoEditPipeline.__call__` (`enable_sketch_region(max_crops=)`), on the
tiny synthetic pipeline of tests/test_sketch_gpu.py (whose helpers are used here): a 400 x 300 photo with strokes near two opposite corners
is edited as two crops of 102 x 68 and 117 x 78 instead of as the whole photo (the one box around both does not fit), and returns ONE video at the photo's size.

Bit for bit what a second implementation from public pieces gives: `set_edit_region([m0, m1], composite=False)` with the masks of
`clusters`' host forms as PIL images + `enable_region_focus(context)` + `__call__(image=[composite, composite])` with the embeds and the
`latents` rows repeated, and then PIL's own paste of the boxes' contents into the BACKGROUND through the masks, in order."""
import numpy as np
import pytest
import test_sketch_gpu as T
import torch
from PIL import Image
from test_sketch_gpu import pipe  # noqa: F401  (fixture)

from chronoedit_amd import clusters, focus, sketch, sparse_region

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, GROW, FEATHER = T.W, T.H, T.GROW, T.FEATHER
assert (W, H, GROW, FEATHER) == (96, 64, 3, 4)
CONTEXT = 0.25
PHOTO = T.photo((400, 300))
NW, SE = (20, 20, 50, 40), (350, 250, 380, 280)  # (left, top, right, bottom) strokes near opposite corners
TWO = {"background": PHOTO, "composite": T.draw(PHOTO, [NW, SE])}
MEET = {"background": PHOTO, "composite": T.draw(PHOTO, [NW, (120, 30, 150, 50)])}  # two clusters whose trial boxes intersect
THREE = {"background": PHOTO, "composite": T.draw(PHOTO, [NW, (140, 20, 160, 40), SE])}  # the middle one: a box of its own that abuts the first one's
TALL = T.photo((70, 300), seed=4)  # the largest 96 : 64 box in it is 70 x 46: a stroke 60 rows high does not fit
UNFIT = {"background": TALL, "composite": T.draw(TALL, [(10, 10, 30, 70), (10, 200, 30, 260)])}
PLAN_KEYS = ("box", "reason", "source_size", "edit_size", "scale", "mask_fraction_of_box")


def host_plan(value, max_crops=2, min_stroke=0, width=W, height=H, context=CONTEXT):
    """(entry, Crops) of the host forms: the definition."""
    cfg = sketch.SketchConfig(GROW, FEATHER, context=context, min_stroke=min_stroke, max_crops=max_crops)
    e = sketch.masks(cfg, [value["background"]], [value["composite"]])[0]
    return e, clusters.plan(e, max_crops, width, height, context)


def pil_masks(crops):
    return [Image.fromarray(p.mask_u8.numpy(), mode="L") for p in crops.plans]


def repeated(kw, rows):
    idx = torch.tensor(rows)
    return dict(kw, **{k: kw[k].index_select(0, idx.to(kw[k].device)) for k in ("prompt_embeds", "negative_prompt_embeds", "latents")})


def second_implementation(pipe, value, kw, masks, context=CONTEXT):  # noqa: F811
    """-> (frames uint8 [F, SH, SW, 3], the focused call's focus_report)."""
    n = len(masks)
    pipe.enable_region_focus(context).set_edit_region(masks, composite=False)
    try:
        content = T.arrays(T.call(pipe, [value["composite"]] * n, repeated(kw, [0] * n)))
        freport = pipe.focus_report
    finally:
        pipe.disable_region_focus().clear_edit_region()
    frames = []
    for f in range(content[0].shape[0]):
        canvas = value["background"].copy()
        for g, m in enumerate(masks):
            box = freport[g]["box"]
            canvas.paste(Image.fromarray(content[g][f]).crop(box), box[:2], m.crop(box))
        frames.append(np.asarray(canvas))
    return np.stack(frames), freport


def assert_crops_equal_second_implementation(pipe, value, kw, max_crops=2, **switch):  # noqa: F811
    _, crops = host_plan(value, max_crops)
    assert crops.reason == "crops"
    masks = pil_masks(crops)
    got, report, freport = T.sketched(pipe, value, kw, max_crops=max_crops, **switch)
    want, wreport = second_implementation(pipe, value, kw, masks)
    got = T.arrays(got)
    assert len(got) == 1 and got[0].shape == want.shape == (5, value["background"].size[1], value["background"].size[0], 3)
    assert np.array_equal(got[0], want)
    rep = report[0]
    assert rep["crops_reason"] == "crops" and rep["max_crops"] == max_crops and len(rep["crops"]) == len(masks) == len(freport)
    assert freport == wreport == [p.report for p in crops.plans]  # the flat list of the plans that ran: what explicit masks get
    for c, m, p, labels in zip(rep["crops"], masks, crops.plans, crops.labels):
        assert c["mask"].mode == "L" and np.array_equal(np.array(c["mask"]), np.array(m)) and c["clusters"] == labels
        assert {k: c[k] for k in ("box", "reason", "scale", "mask_fraction_of_box")} == {k: p.report[k] for k in ("box", "reason", "scale", "mask_fraction_of_box")}
        T.assert_mask_is_not_trivial(c)
    return got[0], rep, crops


def test_the_geometry_two_groups_two_small_boxes():
    e, crops = host_plan(TWO)
    assert e["count"] == 2 and [r[1:5] for r in e["rows"][:2]] == [[13, 13, 57, 47], [343, 243, 387, 287]]  # the strokes grown by 3 + 4
    assert crops.reason == "crops" and crops.groups == [[0], [1]]
    b0, b1 = (p.report["box"] for p in crops.plans)
    # the first: extent 52 x 42, padded by 13 to 78 x 68, raised to 96 wide, widened to 96 : 64 -> 102 x 68; the second: 52 x 52 -> 78 x 78 -> 117 x 78
    assert b0 == (0, 0, 102, 68) and b1 == (283, 222, 400, 300)
    assert all(p.report["reason"] == "ok" for p in crops.plans) and not clusters.intersect(b0, b1)
    single = sketch.focus_plan(e, W, H, CONTEXT).report
    # the single box: the union's bounding box is 382 x 282, the largest 96 : 64 box in the photo 400 x 266 - too low: "fit", the whole photo
    assert single["reason"] == "fit" and single["box"] == (0, 0, 400, 300)
    assert [p.report["scale"] for p in crops.plans] == [102 / 96, 117 / 96] and single["scale"] == 400 / 96  # about 1.1 and 1.2 against 4.2
    for value, reason in ((MEET, "single"), (UNFIT, "unfit")):
        assert host_plan(value)[1].reason == reason
    e3, c3 = host_plan(THREE)
    assert e3["count"] == 3 and c3.reason == "crops" and c3.groups == [[0, 1], [2]] and host_plan(THREE, 3)[1].groups == [[0], [1], [2]]


@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_two_crops_equal_the_second_implementation(pipe, use_graph, guidance_scale):  # noqa: F811
    kw = T.inputs(guidance_scale=guidance_scale)
    pipe.use_graph = use_graph
    try:
        frames, rep, crops = assert_crops_equal_second_implementation(pipe, TWO, kw)
    finally:
        pipe.use_graph = True
    # today's keys, from the union mask: the box the single-box call would have used
    assert rep["box"] == (0, 0, 400, 300) and rep["reason"] == "fit" and rep["scale"] == 400 / 96 and rep["changed_pixels"] == 30 * 20 + 30 * 30
    assert np.array_equal(np.array(rep["mask"]), sketch.reference(PHOTO, TWO["composite"], GROW, FEATHER).numpy())
    bg, cp = np.array(PHOTO), np.array(TWO["composite"])
    m0, m1 = (np.array(c["mask"]) for c in rep["crops"])
    assert np.array_equal(np.maximum(m0, m1), np.array(rep["mask"])) and not (m0 & m1).any()
    nowhere = (m0 == 0) & (m1 == 0)
    for f in range(5):
        assert np.array_equal(frames[f][nowhere], bg[nowhere]), f  # the background's bytes wherever both masks are 0
    for m in (m0, m1):
        assert not np.array_equal(frames[-1][m == 255], cp[m == 255])  # the strokes are gone in both corners: the model's pixels


def test_two_crops_sparse(pipe):  # noqa: F811
    kw = T.inputs()
    pipe.enable_sparse_region(refresh_every=2)
    try:
        assert_crops_equal_second_implementation(pipe, TWO, kw)
        rep = pipe.transformer.sparse_report  # (of the second implementation's last sample)
        assert rep["plan"] == ["refresh", "sparse"] and sparse_region.PAD <= rep["active"] <= rep["tokens"] == 48, rep
    finally:
        pipe.disable_sparse_region()


def test_the_host_path_gives_the_same_bytes(pipe):  # noqa: F811
    kw = T.inputs()
    on_device, report, freport = T.sketched(pipe, TWO, kw, max_crops=2)
    pipe.enable_device_image_io(False)
    try:
        frames, host_report, crops = assert_crops_equal_second_implementation(pipe, TWO, kw)
        pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=2)
        shown_host = pipe.sketch_crops(PHOTO, TWO["composite"], H, W)
    finally:
        pipe.enable_device_image_io(True)
        pipe.disable_sketch_region()
    assert np.array_equal(frames, T.arrays(on_device)[0])
    strip = lambda rep: {k: ([{a: b for a, b in c.items() if a != "mask"} for c in v] if k == "crops" else v) for k, v in rep.items() if k != "mask"}
    assert strip(host_report) == strip(report[0])
    for a, b in zip(host_report["crops"], report[0]["crops"]):
        assert np.array_equal(np.array(a["mask"]), np.array(b["mask"]))
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=2)
    try:
        shown = pipe.sketch_crops(PHOTO, TWO["composite"], H, W)
        union = pipe.sketch_mask(PHOTO, TWO["composite"])
    finally:
        pipe.disable_sketch_region()
    for s in (shown, shown_host):
        assert [{k: v for k, v in c.items() if k != "mask"} for c in s] == strip(report[0])["crops"]
        assert all(np.array_equal(np.array(c["mask"]), np.array(b["mask"])) for c, b in zip(s, report[0]["crops"]))
    assert np.array_equal(np.array(union), np.array(report[0]["mask"]))  # sketch_mask stays the union mask


def test_max_crops_1_is_todays_call_and_has_no_new_keys(pipe):  # noqa: F811
    kw = T.inputs()
    today, treport, tfocus = T.sketched(pipe, TWO, kw)
    got, report, freport = T.sketched(pipe, TWO, kw, max_crops=1)
    assert np.array_equal(T.arrays(got)[0], T.arrays(today)[0]) and freport == tfocus
    assert set(report[0]) == set(treport[0]) and not {"max_crops", "crops", "crops_reason"} & set(report[0])
    two = T.arrays(T.sketched(pipe, TWO, kw, max_crops=2)[0])[0]
    assert not np.array_equal(two, T.arrays(today)[0])
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER)
    try:
        shown = pipe.sketch_crops(PHOTO, TWO["composite"], H, W)
    finally:
        pipe.disable_sketch_region()
    assert len(shown) == 1 and shown[0]["box"] == treport[0]["box"] and shown[0]["clusters"] is None


@pytest.mark.parametrize("value, reason", [(MEET, "single"), (UNFIT, "unfit")], ids=["single", "unfit"])
def test_the_fallbacks_are_the_single_box_call(pipe, value, reason):  # noqa: F811
    kw = T.inputs()
    today, treport, tfocus = T.sketched(pipe, value, kw)
    got, report, freport = T.sketched(pipe, value, kw, max_crops=2)
    rep = report[0]
    assert rep["crops_reason"] == reason and rep["max_crops"] == 2 and freport == tfocus and len(freport) == 1
    assert np.array_equal(T.arrays(got)[0], T.arrays(today)[0])
    assert {k: rep[k] for k in treport[0] if k != "mask"} == {k: treport[0][k] for k in treport[0] if k != "mask"}
    assert len(rep["crops"]) == 1 and rep["crops"][0]["box"] == rep["box"] and np.array_equal(np.array(rep["crops"][0]["mask"]), np.array(rep["mask"]))
    assert rep["crops"][0]["clusters"] == [r[0] for r in host_plan(value)[0]["rows"][:2]]
    if reason == "unfit":
        assert rep["reason"] == "fit" and rep["box"] == (0, 0, 70, 300)


def test_three_clusters_under_a_cap_of_two_are_two_crops(pipe):  # noqa: F811
    kw = T.inputs()
    frames, rep, crops = assert_crops_equal_second_implementation(pipe, THREE, kw)
    e, _ = host_plan(THREE)
    assert crops.groups == clusters.group(e["rows"][:3], PHOTO.size, (W, H), CONTEXT, FEATHER, 2) == [[0, 1], [2]]
    assert [c["clusters"] for c in rep["crops"]] == [[e["rows"][0][0], e["rows"][1][0]], [e["rows"][2][0]]]
    # with the speck filter on: a far speck is no cluster, and no crop
    specked = {"background": PHOTO, "composite": T.draw(PHOTO, [NW, SE, (200, 150, 202, 151)])}
    assert host_plan(specked, 3)[1].groups == [[0], [1], [2]]
    got, report, _ = T.sketched(pipe, specked, kw, max_crops=3, min_stroke=4)
    clean, creport, _ = T.sketched(pipe, TWO, kw, max_crops=3)
    assert report[0]["crops_reason"] == "crops" and len(report[0]["crops"]) == 2 and report[0]["dropped_clusters"] == 1
    assert np.array_equal(T.arrays(got)[0], T.arrays(clean)[0])


def test_a_list_of_values_returns_one_video_per_value(pipe):  # noqa: F811
    one = {"background": T.IMAGE, "composite": T.draw(T.IMAGE, T.STROKES)}  # one cluster: its single-box plan
    values = [TWO, one]
    kw = T.inputs(n=2)
    got, report, freport = T.sketched(pipe, values, kw, max_crops=2)
    got = T.arrays(got)
    assert len(got) == 2 and got[0].shape[1:3] == (300, 400) and got[1].shape[1:3] == (150, 203)
    assert [r["crops_reason"] for r in report] == ["crops", "single"] and len(freport) == 3
    for i, v in enumerate(values):
        alone, arep, afocus = T.sketched(pipe, v, repeated(kw, [i]), max_crops=2)
        assert np.array_equal(T.arrays(alone)[0], got[i]), i
        assert arep[0]["crops_reason"] == report[i]["crops_reason"] and afocus == (freport[:2] if i == 0 else freport[2:])
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=2)
    try:
        with pytest.raises(NotImplementedError, match="num_videos_per_prompt"):
            T.call(pipe, TWO, T.inputs(), num_videos_per_prompt=2)
        with pytest.raises(ValueError, match="one size"):
            T.call(pipe, values, kw, "np")
        lat = T.call(pipe, TWO, T.inputs(), "latent")
        assert tuple(lat.shape) == (2, 16, 2, H // 8, W // 8)  # the crops' latents, flat
        as_np, as_pil = T.call(pipe, TWO, T.inputs(), "np"), T.arrays(T.call(pipe, TWO, T.inputs()))[0]
        assert as_np.shape == (1, 5, 300, 400, 3) and np.array_equal((as_np[0] * 255).round().astype(np.uint8), as_pil)
    finally:
        pipe.disable_sketch_region()


def test_a_generator_draws_what_the_single_box_call_draws(pipe):  # noqa: F811
    kw = {k: v for k, v in T.inputs().items() if k != "latents"}
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=2)
    try:
        got = T.arrays(pipe(image=TWO, output_type="pil", generator=torch.Generator().manual_seed(3), **kw).frames)[0]
    finally:
        pipe.disable_sketch_region()
    noise = torch.randn((1, 16, 2, H // 8, W // 8), generator=torch.Generator().manual_seed(3), dtype=torch.bfloat16)
    want = T.arrays(T.sketched(pipe, TWO, dict(kw, latents=noise.float()), max_crops=2)[0])[0]
    assert np.array_equal(got, want)


def test_previews_name_their_crop(pipe):  # noqa: F811
    kw = T.inputs()
    plain = T.arrays(T.sketched(pipe, TWO, kw, max_crops=2)[0])[0]
    seen = []
    pipe.enable_preview(seen.append, factors=torch.randn(17, 3, generator=torch.Generator().manual_seed(11)) * 0.2)
    try:
        got = T.arrays(T.sketched(pipe, TWO, kw, max_crops=2)[0])[0]
        assert [(d["sample"], d["crop"], d["step"]) for d in seen] == [(0, (0, 0), 0), (0, (0, 0), 1), (1, (0, 1), 0), (1, (0, 1), 1)]
        del seen[:]
        T.sketched(pipe, TWO, kw)
        assert seen and all("crop" not in d for d in seen)
    finally:
        pipe.disable_preview()
    assert np.array_equal(got, plain)


def test_at_most_two_reads_per_value_before_the_edit(pipe, monkeypatch):  # noqa: F811
    kw = T.inputs()
    _, crops = host_plan(TWO)
    masks = pil_masks(crops)
    reads = T.HostReads(monkeypatch)
    before = {}

    def first_step(name):
        def cb(p, i, t, kwargs):
            before.setdefault(name, list(reads.log))
            return {}
        return cb

    first = 10 + 1 + 8 * clusters.ROWS  # today's ten integers, the count, the table
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=2)
    try:
        del reads.log[:]
        e = sketch.masks(pipe._sketch_region, [PHOTO], [TWO["composite"]], torch.device(DEV))[0]
        assert reads.log == [first] and e["mask_u8"] is None and e["roots"].is_cuda and e["count"] == 2
        del reads.log[:]
        assert clusters.plan(e, 2, W, H, CONTEXT).reason == "crops" and reads.log == [5 * 2]  # the second read: 5 G integers
        del reads.log[:]
        T.call(pipe, TWO, kw, callback_on_step_end=first_step("crops"))
        del reads.log[:]
        T.call(pipe, MEET, kw, callback_on_step_end=first_step("single"))
        assert pipe.sketch_report[0]["crops_reason"] == "single"
    finally:
        pipe.disable_sketch_region()
    pipe.enable_region_focus(CONTEXT).set_edit_region(masks, composite=False)
    try:
        del reads.log[:]
        T.call(pipe, [TWO["composite"]] * 2, repeated(kw, [0, 0]), callback_on_step_end=first_step("explicit2"))
        pipe.set_edit_region(masks[0], composite=False)
        del reads.log[:]
        T.call(pipe, TWO["composite"], kw, callback_on_step_end=first_step("explicit1"))
    finally:
        pipe.disable_region_focus().clear_edit_region()
    for name, other, want in (("crops", "explicit2", [first, 10]), ("single", "explicit1", [first])):
        extra = list(before[name])
        for n in before[other]:
            extra.remove(n)  # (whatever the focused call itself reads in front of the first step, the sketch call reads too)
        assert extra == want, (name, before[name], before[other])
    assert 400 * 300 not in before["crops"]  # the masks' copies for the report are made behind the edit
