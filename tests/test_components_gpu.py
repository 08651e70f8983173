"""Speckle removal through the public switches: `enable_sketch_region(min_stroke=)` and `enable_auto_region(min_area=)` on the tiny
synthetic pipeline of tests/test_sketch_gpu.py (whose photo, strokes and helpers are used here) and the tiny loop of
tests/test_auto_region_gpu.py.

Sketch: the photo and strokes of that file plus a 2-pixel speck in the opposite corner.  Without the filter the speck stretches the box
to the whole photo ("fit"); with min_stroke=4 the call is, byte for byte, the sketch call on the composite WITHOUT the speck.
Automatic regions: a region planted in the source latents plus isolated far cells; the filtered loop equals a second implementation (the
plain loop with a hook that builds w from the CPU expressions - `components.reference` among them - and blends in torch).  Through
`__call__` the change map itself is planted (the pass that computes it is replaced by one that returns a hand-built map): the filtered call
on the speckled map is the unfiltered call on the clean one, and under `enable_auto_focus` it is accepted with the region's box where the
unfiltered call reports "whole"."""
import numpy as np
import pytest
import test_auto_region_gpu as A
import test_sketch_gpu as T
import torch
from test_auto_region_gpu import base  # noqa: F401  (fixtures)
from test_sketch_gpu import pipe  # noqa: F401

from chronoedit_amd import auto_region as ar
from chronoedit_amd import components, ops, sketch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPECK = (2, 147, 4, 148)  # (left, top, right, bottom): two pixels in the bottom left corner, the strokes are near the top right one
SPECKED = {"background": T.IMAGE, "composite": T.draw(T.IMAGE, T.STROKES + [SPECK])}
PLAN_KEYS = ("box", "reason", "source_size", "edit_size", "scale", "mask_fraction_of_box")


def test_the_speck_lies_farther_than_two_radii_from_the_strokes():
    R = T.GROW + T.FEATHER
    assert all(l - SPECK[2] > 2 * R and SPECK[1] - b > 2 * R for l, t, r, b in T.STROKES)


@pytest.mark.parametrize("use_graph", [True, False])
def test_a_far_speck_is_dropped_and_the_call_is_the_one_without_it(pipe, use_graph):  # noqa: F811
    kw = T.inputs()
    pipe.use_graph = use_graph
    try:
        want, want_report, want_focus = T.sketched(pipe, T.VALUE, kw)
        got, report, freport = T.sketched(pipe, SPECKED, kw, min_stroke=4)
        unfiltered, report0, freport0 = T.sketched(pipe, SPECKED, kw, min_stroke=0)
    finally:
        pipe.use_graph = True
    got, want = T.arrays(got)[0], T.arrays(want)[0]
    assert got.shape == (5, 150, 203, 3) and np.array_equal(got, want)
    rep, wrep = report[0], want_report[0]
    assert freport == want_focus and rep["reason"] == "ok" and rep["box"] == wrep["box"] and {k: rep[k] for k in PLAN_KEYS} == {k: wrep[k] for k in PLAN_KEYS}
    assert np.array_equal(np.array(rep["mask"]), np.array(wrep["mask"]))
    assert np.array_equal(np.array(rep["mask"]), sketch.reference(T.IMAGE, SPECKED["composite"], T.GROW, T.FEATHER, 0, 4).numpy())
    assert (rep["min_stroke"], rep["clusters"], rep["dropped_clusters"], rep["dropped_pixels"]) == (4, 1, 1, 2)
    assert rep["changed_pixels"] == wrep["changed_pixels"] + 2 and "clusters" not in wrep and "min_stroke" not in wrep
    bg, cp = np.array(T.IMAGE), np.array(SPECKED["composite"])
    l, t, r, b = SPECK
    assert not np.array_equal(cp[t:b, l:r], bg[t:b, l:r])
    for f in range(5):
        assert np.array_equal(got[f][t:b, l:r], bg[t:b, l:r]), f  # the dropped speck does not come back: the background's bytes
    # the switch at 0: the speck stretches the box to the whole photo
    assert report0[0]["reason"] == "fit" and freport0[0]["reason"] == "fit" and "clusters" not in report0[0]
    assert not np.array_equal(T.arrays(unfiltered)[0], got)


def test_the_host_path_gives_the_same_bytes(pipe):  # noqa: F811
    kw = T.inputs()
    on_device, report, _ = T.sketched(pipe, SPECKED, kw, min_stroke=4)
    pipe.enable_device_image_io(False)
    try:
        on_host, host_report, _ = T.sketched(pipe, SPECKED, kw, min_stroke=4)
    finally:
        pipe.enable_device_image_io(True)
    assert np.array_equal(T.arrays(on_host)[0], T.arrays(on_device)[0])
    assert np.array_equal(np.array(host_report[0]["mask"]), np.array(report[0]["mask"]))
    assert {k: v for k, v in host_report[0].items() if k != "mask"} == {k: v for k, v in report[0].items() if k != "mask"}
    pipe.enable_sketch_region(grow=T.GROW, feather=T.FEATHER, min_stroke=4)
    try:
        shown = pipe.sketch_mask(T.IMAGE, SPECKED["composite"])
    finally:
        pipe.disable_sketch_region()
    assert np.array_equal(np.array(shown), np.array(report[0]["mask"]))


def test_a_fraction_of_the_heaviest_cluster(pipe):  # noqa: F811
    kw = T.inputs()
    _, report, _ = T.sketched(pipe, SPECKED, kw, min_stroke=0.01)  # ceil(686 / 100) = 7 changed pixels
    assert (report[0]["min_stroke"], report[0]["clusters"], report[0]["dropped_clusters"], report[0]["dropped_pixels"]) == (0.01, 1, 1, 2)
    assert report[0]["reason"] == "ok"


def test_all_clusters_dropped_is_the_plain_call_on_the_composite(pipe):  # noqa: F811
    kw = T.inputs()
    plain, plain_lat = T.arrays(T.call(pipe, SPECKED["composite"], kw))[0], T.call(pipe, SPECKED["composite"], kw, "latent")
    got, report, freport = T.sketched(pipe, SPECKED, kw, min_stroke=5000)
    rep = report[0]
    assert freport is None and rep["reason"] == "empty" and rep["box"] == (0, 0, 203, 150) and not np.array(rep["mask"]).any()
    assert (rep["clusters"], rep["dropped_clusters"], rep["dropped_pixels"], rep["changed_pixels"]) == (0, 2, 688, 688)
    frames = T.arrays(got)[0]
    assert frames.shape == (5, T.H, T.W, 3) and np.array_equal(frames, plain)
    assert torch.equal(T.sketched(pipe, SPECKED, kw, "latent", min_stroke=5000)[0], plain_lat)


class HostReads:
    """Counts what comes back from the device: every `.cpu()`, `.tolist()`, `.item()`, `.numpy()` and `.to(<cpu>)` of a CUDA tensor, as the
    number of elements it moves, in the order of the calls."""

    def __init__(self, monkeypatch):
        self.log, self.depth = [], 0
        for name in ("cpu", "tolist", "item", "numpy", "to"):
            monkeypatch.setattr(torch.Tensor, name, self.wrap(name, getattr(torch.Tensor, name)))

    def wrap(self, name, inner):
        def counted(t, *a, **k):
            to_host = name != "to" or any(str(v) == "cpu" or (isinstance(v, torch.device) and v.type == "cpu") for v in list(a) + list(k.values()))
            record = t.is_cuda and to_host and self.depth == 0
            if record:
                self.log.append(t.numel())
            self.depth += 1
            try:
                return inner(t, *a, **k)
            finally:
                self.depth -= 1
        return counted


def test_one_read_of_fourteen_integers_per_image_before_the_edit(pipe, monkeypatch):  # noqa: F811
    other = T.photo((150, 180), seed=11)
    values = [SPECKED, {"background": other, "composite": T.draw(other, [(12, 130, 50, 140), (20, 140, 28, 168), (140, 3, 141, 4)])}]
    kw = T.inputs(n=2)
    bgs, cps = [v["background"] for v in values], [v["composite"] for v in values]
    masks = [T.Image.fromarray(sketch.reference(v["background"], v["composite"], T.GROW, T.FEATHER, 0, 4).numpy(), mode="L") for v in values]
    reads = HostReads(monkeypatch)
    before = {}

    def first_step(name):
        def cb(p, i, t, kwargs):
            before.setdefault(name, list(reads.log))
            return {}
        return cb

    pipe.enable_sketch_region(grow=T.GROW, feather=T.FEATHER, min_stroke=4)
    try:
        del reads.log[:]
        entries = sketch.masks(pipe._sketch_region, bgs, cps, torch.device(DEV))
        assert reads.log == [14, 14] and all(e["mask_u8"] is None and e["mask_dev"].is_cuda and e["dropped_clusters"] == 1 for e in entries)
        del reads.log[:]
        T.call(pipe, values, kw, callback_on_step_end=first_step("sketch"))
        report = pipe.sketch_report
        pipe.enable_sketch_region(grow=T.GROW, feather=T.FEATHER, min_stroke=0)
        del reads.log[:]
        sketch.masks(pipe._sketch_region, bgs, cps, torch.device(DEV))
        assert reads.log == [10, 10]  # the switch at 0: the ten integers of the call without it
    finally:
        pipe.disable_sketch_region()
    pipe.enable_region_focus().set_edit_region(masks)
    try:
        del reads.log[:]
        T.call(pipe, cps, kw, callback_on_step_end=first_step("explicit"))
    finally:
        pipe.disable_region_focus().clear_edit_region()
    extra = list(before["sketch"])
    for n in before["explicit"]:
        extra.remove(n)  # (whatever the focused call itself reads in front of the first step, the sketch call reads too)
    assert extra == [14, 14], (before["sketch"], before["explicit"])
    for rep, m in zip(report, masks):
        assert np.array_equal(np.array(rep["mask"]), np.array(m)) and rep["dropped_clusters"] == 1


# ---- automatic regions: the loop ----------------------------------------------------------------------------------------------------------
FAR = ((0, 0), (7, 11), (7, 0))  # isolated cells, at least two cells away from A.RECT (rows 2..3, columns 4..5) and from each other


def speckled_source(x0):
    z = A._source(x0)
    for y, x in FAR:
        z[:, :, -1, y, x] += 2.0
    return z.contiguous()


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("kind", ["otsu", "number"])
def test_filtered_loop_equals_the_second_implementation(base, kind, use_graph):  # noqa: F811
    cfg = {"otsu": ar.AutoRegionConfig(A.K, min_area=2), "number": ar.AutoRegionConfig(A.K, threshold=1.0, dilate=0, feather=2, min_area=0.5)}[kind]
    off = ar.AutoRegionConfig(cfg.detect_step, cfg.threshold, cfg.floor, cfg.dilate, cfg.feather)
    inp, z = A._inputs(), speckled_source(base.x0)
    d, thr, _, w_cpu = ar.weights(base.x0.cpu(), z.cpu(), cfg)
    seeds = A._rect_mask().clone()
    for y, x in FAR:
        seeds[y, x] = True
    assert torch.equal(d > thr, seeds)  # the planted region and the three far cells, nothing else
    assert torch.equal(w_cpu, ar.ramp_weights(torch.where(A._rect_mask(), d, torch.tensor(-1.0)), thr, cfg.dilate, cfg.feather))
    assert torch.equal(components.reference(seeds.to(torch.uint8), cfg.min_area)[0] != 0, A._rect_mask())
    m = A._model()
    got, a = A._auto(m, inp, z, cfg, use_graph=use_graph)
    want = A._callback_loop(A._model(), inp, z, cfg)
    assert torch.equal(got, want) and not torch.equal(got, base.plain)
    rep = a.report
    assert rep is m.auto_region_report and rep["accepted"] and torch.equal(rep["w"], w_cpu)
    assert (rep["min_area"], rep["components"], rep["dropped_components"], rep["dropped_cells"]) == (cfg.min_area, 1, 3, 3)
    assert torch.equal(a.mask_u8.cpu(), ar.pixel_mask(w_cpu)) and np.array_equal(np.asarray(rep["mask"]), ar.pixel_mask(w_cpu).numpy())
    # the switch at 0 on the same inputs: the far cells are part of the region, and the report has no counters
    got0, a0 = A._auto(A._model(), inp, z, off, use_graph=use_graph)
    assert "components" not in a0.report and not torch.equal(a0.report["w"], w_cpu) and not torch.equal(got0, got)
    assert torch.equal(got0, A._callback_loop(A._model(), inp, z, off))


def test_the_detection_reads_the_device_once(base, monkeypatch):  # noqa: F811
    x0, z = base.x0, speckled_source(base.x0)
    reads = HostReads(monkeypatch)
    for cfg, n in ((ar.AutoRegionConfig(A.K, min_area=2), 8 * 12 + 2 + 4), (ar.AutoRegionConfig(A.K), 8 * 12 + 2)):
        del reads.log[:]
        out = ar.detect(x0, z, cfg)
        assert reads.log == [n], reads.log
    assert len(out) == 5 and len(ar.detect(x0, z, ar.AutoRegionConfig(A.K, min_area=2))) == 6


# ---- automatic regions and auto focus through __call__, on a planted change map -------------------------------------------------------
def planted(corners: bool) -> torch.Tensor:
    d = torch.zeros(8, 12)
    d[2:5, 4:8] = 4.0
    if corners:
        d[0, 0] = d[0, 11] = d[7, 0] = d[7, 11] = 4.0
    return d


@pytest.fixture()
def plant(monkeypatch):
    """Replaces the pass that computes the change map by one that returns a hand-built map."""
    def use(d):
        def change(x0, z, frame=-1, out=None):
            v = d.to(x0.device)
            return v.clone() if out is None else out.copy_(v)
        monkeypatch.setattr(ops, "auto_region_change", change)
    return use


DET = dict(detect_step=0, threshold=1.0, dilate=1, feather=1, max_area=1.0)


def auto_call(pipe, kw, focus=False, **det):  # noqa: F811
    pipe.enable_auto_region(**dict(DET, **det))
    if focus:
        pipe.enable_auto_focus(0.0)
    try:
        out = T.arrays(T.call(pipe, T.IMAGE, kw))[0]
        return out, pipe.auto_region_report, pipe.focus_report
    finally:
        pipe.disable_auto_region().disable_auto_focus()


@pytest.mark.parametrize("use_graph", [True, False])
def test_filtered_call_on_a_speckled_map_is_the_call_on_the_clean_map(pipe, plant, use_graph):  # noqa: F811
    kw = T.inputs(steps=3)
    pipe.use_graph = use_graph
    try:
        plant(planted(False))
        want, wrep, _ = auto_call(pipe, kw)
        plant(planted(True))
        got, rep, _ = auto_call(pipe, kw, min_area=2)
        loose, rep0, _ = auto_call(pipe, kw)
    finally:
        pipe.use_graph = True
    thr = torch.tensor([1.0])
    w = ar.ramp_weights(planted(False), thr, 1, 1)
    assert rep["accepted"] and torch.equal(rep["w"], w) and torch.equal(wrep["w"], w) and np.array_equal(np.asarray(rep["mask"]), ar.pixel_mask(w).numpy())
    assert torch.equal(rep["w"], ar.ramp_weights(ar.kept_map(planted(True), thr, 2)[0], thr, 1, 1))
    assert (rep["min_area"], rep["components"], rep["dropped_components"], rep["dropped_cells"]) == (2, 1, 4, 4)
    assert np.array_equal(got, want)
    assert "components" not in rep0 and "components" not in wrep and torch.equal(rep0["w"], ar.ramp_weights(planted(True), thr, 1, 1))
    assert not np.array_equal(loose, got)


def test_auto_focus_accepts_the_filtered_region_where_the_unfiltered_one_is_the_whole_photo(pipe, plant):  # noqa: F811
    kw = T.inputs(steps=3)
    plant(planted(False))
    want, _, wfocus = auto_call(pipe, kw, focus=True)
    plant(planted(True))
    got, rep, gfocus = auto_call(pipe, kw, focus=True, min_area=2)
    whole, rep0, focus0 = auto_call(pipe, kw, focus=True)
    assert focus0[0]["reason"] == "whole" and focus0[0]["box"] == (0, 0) + T.IMAGE.size and whole.shape == (5, T.H, T.W, 3)
    assert gfocus[0]["reason"] == "ok" and gfocus[0]["box"] == wfocus[0]["box"] != (0, 0) + T.IMAGE.size
    assert gfocus[0]["detect"]["dropped_components"] == 4 and got.shape == (5, 150, 203, 3)  # the photo's size
    assert np.array_equal(got, want)
