"""Focused region edits, the part that needs no GPU: the box, the bilinear tables, the paste expression, the C ABI and the host form."""
import random
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import focus, hiplib, image_io

ENTRY_POINTS = ("ce_focus_resample_l8", "ce_focus_paste_u8")


def test_the_worked_example():
    box, reason = focus.focus_box((1000, 1200, 1400, 1500), (4032, 3024), (1280, 720), 0.25)
    assert (box, reason) == ((560, 990, 1840, 1710), "ok")
    # at scale 1 the crop has the edit's size: resize_u8 has nothing to resample
    assert (box[2] - box[0], box[3] - box[1]) == (1280, 720)


def check_box(bbox, src, edit, context):
    (SW, SH), (W, H) = src, edit
    box, reason = focus.focus_box(bbox, src, edit, context)
    l, t, r, b = box
    assert all(isinstance(v, int) for v in box)
    assert 0 <= l < r <= SW and 0 <= t < b <= SH, (box, src)
    if bbox is None:
        assert reason == "empty" and box == (0, 0, SW, SH)
        return reason
    assert l <= bbox[0] and t <= bbox[1] and r >= bbox[2] and b >= bbox[3], (box, bbox)
    bw, bh = r - l, b - t
    if reason == "ok":
        assert abs(bw * H - bh * W) < max(W, H), (box, edit)
        if SW >= W and SH >= H:
            assert bw >= W and bh >= H, (box, edit)
    else:
        assert reason == "fit" and box == (0, 0, SW, SH)
        # "fit" only when the largest box of the edit's aspect ratio cannot hold the bare bbox
        assert min(SW * H, SH * W) // H < bbox[2] - bbox[0] or min(SW * H, SH * W) // W < bbox[3] - bbox[1]
    return reason


SOURCES = [(4032, 3024), (3024, 4032), (1280, 720), (1281, 721), (203, 150), (150, 203), (97, 64), (96, 65), (64, 48), (50, 70), (17, 5), (1, 1),
           (2000, 100), (100, 2000)]
EDITS = [(1280, 720), (96, 64), (64, 96), (16, 16)]


def bboxes(SW, SH):
    w, h = max(1, SW // 5), max(1, SH // 7)
    yield (0, 0, w, h)
    yield (SW - w, 0, SW, h)
    yield (0, SH - h, w, SH)
    yield (SW - w, SH - h, SW, SH)
    yield (0, SH // 2, SW, SH // 2 + 1)  # full width
    yield (SW // 2, 0, SW // 2 + 1, SH)  # full height
    yield (SW // 3, SH // 3, SW // 3 + 1, SH // 3 + 1)  # one pixel
    yield (0, 0, SW, SH)


def test_box_properties_over_a_grid():
    reasons = set()
    for src in SOURCES:
        for edit in EDITS:
            for context in (0, 0.25, 2):
                reasons.add(check_box(None, src, edit, context))
                for bbox in bboxes(*src):
                    reasons.add(check_box(bbox, src, edit, context))
    assert reasons == {"ok", "fit", "empty"}


def test_box_properties_on_random_cases():
    rng = random.Random(20240607)
    reasons = []
    for _ in range(600):
        SW, SH = rng.randint(1, 5000), rng.randint(1, 5000)
        W, H = 16 * rng.randint(1, 90), 16 * rng.randint(1, 90)
        l, t = rng.randrange(SW), rng.randrange(SH)
        r, b = rng.randint(l + 1, SW), rng.randint(t + 1, SH)
        reasons.append(check_box((l, t, r, b), (SW, SH), (W, H), rng.choice([0, 0.1, 0.25, 0.5, 2, rng.random() * 3])))
    assert reasons.count("ok") > 100 and reasons.count("fit") > 10


def test_box_rejects_bad_arguments():
    with pytest.raises(ValueError):
        focus.focus_box((0, 0, 11, 5), (10, 10), (16, 16), 0.25)
    with pytest.raises(ValueError):
        focus.focus_box((0, 0, 5, 5), (10, 10), (16, 16), -0.1)
    with pytest.raises(ValueError):
        focus.focus_box((0, 0, 5, 5), (10, 10), (16, 16), float("nan"))


def random_l(size, seed):
    w, h = size
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def resample_np(a, axis, coeff, bounds):
    """One pass of the 8-bit resampler in numpy: what ce_focus_resample_l8 computes."""
    a = a.astype(np.int64)
    rows = []
    for o, (first, count) in enumerate(bounds):
        taps = a[:, first:first + count] if axis == 0 else a[first:first + count, :].T
        ss = (1 << 21) + taps @ np.array(coeff[o][:count], dtype=np.int64)
        rows.append(np.clip(ss >> 22, 0, 255))
    out = np.stack(rows, axis=1) if axis == 0 else np.stack(rows, axis=0)
    return out.astype(np.uint8)


def resize_np(a, size):
    (W2, H2), (H, W) = size, a.shape
    if W2 != W:
        a = resample_np(a, 0, *image_io.resize_tables(W, W2, image_io.BILINEAR)[:2])
    if H2 != H:
        a = resample_np(a, 1, *image_io.resize_tables(H, H2, image_io.BILINEAR)[:2])
    return a


@pytest.mark.parametrize("src,dst", [((37, 53), (16, 24)), ((37, 53), (80, 96)), ((37, 53), (37, 20)), ((37, 53), (50, 53)), ((20, 31), (45, 31))])
def test_bilinear_tables_equal_pil(src, dst):
    a = random_l(src, 3)
    want = np.array(Image.fromarray(a).resize(dst, Image.BILINEAR))
    assert np.array_equal(resize_np(a, dst), want)


def test_bilinear_is_the_triangle_with_support_one():
    coeff, bounds, ksize = image_io.resize_tables(10, 20, image_io.BILINEAR)
    assert ksize == 3 and all(sum(row) in range((1 << 22) - 2, (1 << 22) + 3) for row in coeff)


def test_the_paste_expression_equals_pil_on_every_triple():
    s = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)  # s varies down, e across, one image per m
    e = np.ascontiguousarray(s.T)
    src, edit = Image.fromarray(s), Image.fromarray(e)
    s32, e32 = s.astype(np.uint32), e.astype(np.uint32)
    for m in range(256):
        out = src.copy()
        out.paste(edit, (0, 0), Image.new("L", (256, 256), m))
        t = s32 * (255 - m) + e32 * m + 128
        got = (((t >> 8) + t) >> 8).astype(np.uint8)
        assert np.array_equal(got, np.array(out)), m
        if m == 0:
            assert np.array_equal(got, s)
        if m == 255:
            assert np.array_equal(got, e)


def test_the_c_abi_declares_the_two_entry_points():
    declared = hiplib.header_symbols()
    for name in ENTRY_POINTS:
        assert declared.count(name) == 1, name
        assert name in hiplib.SIGNATURES, name
    assert [n for n in declared if n.startswith("ce_focus_")] == list(ENTRY_POINTS)
    assert "ce_focus.hip" in hiplib.SOURCES


def photo_and_mask(size=(203, 150), seed=1):
    w, h = size
    rng = np.random.default_rng(seed)
    image = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    mask = np.zeros((h, w), np.uint8)
    mask[20:60, 110:170] = rng.integers(0, 256, (40, 60), dtype=np.uint8)
    mask[30:50, 120:150] = 255
    return image, mask


def test_plan_reports_the_box():
    image, mask = photo_and_mask()
    rep = focus.plan(image.size, mask, 64, 96, 0.25)
    bbox = focus.mask_bbox(torch.from_numpy(mask))
    assert bbox[0] >= 110 and bbox[1] >= 20 and bbox[2] <= 170 and bbox[3] <= 60
    box, reason = focus.focus_box(bbox, image.size, (96, 64), 0.25)
    assert rep["box"] == box and rep["reason"] == reason == "ok"
    assert rep["source_size"] == (203, 150) and rep["edit_size"] == (96, 64) and rep["scale"] == (box[2] - box[0]) / 96
    l, t, r, b = box
    assert rep["mask_fraction_of_box"] == float((mask[t:b, l:r] > 0).sum()) / ((r - l) * (b - t))
    # a PIL mask of another size is resized to the source's, an empty one plans the whole image
    small = Image.fromarray(mask).resize((100, 75), Image.BILINEAR)
    assert focus.plan(image.size, small, 64, 96)["reason"] == "ok"
    assert focus.plan(image.size, np.zeros_like(mask), 64, 96) == {"box": (0, 0, 203, 150), "reason": "empty", "source_size": (203, 150),
                                                                  "edit_size": (96, 64), "scale": 203 / 96, "mask_fraction_of_box": 0.0}
    with pytest.raises(ValueError):
        focus.plan(image.size, mask[:-1], 64, 96)


@pytest.mark.parametrize("with_mask", [True, False])
def test_the_host_form_equals_the_pil_calls_it_restates(with_mask):
    image, mask = photo_and_mask()
    mask_u8 = torch.from_numpy(mask)
    box = focus.plan(image.size, mask, 64, 96, 0.25)["box"]
    l, t, r, b = box
    assert (r - l, b - t) != (96, 64)
    crop, edit_mask = focus.host_inputs(image, mask_u8, box, 96, 64)
    assert np.array_equal(np.array(crop), np.array(image)[t:b, l:r])
    assert np.array_equal(edit_mask.numpy(), np.array(Image.fromarray(mask).crop(box).resize((96, 64), Image.BILINEAR)))
    frames = [Image.fromarray(np.random.default_rng(10 + i).integers(0, 256, (64, 96, 3), dtype=np.uint8)) for i in range(2)]
    got = focus.host_paste(image, frames, mask_u8 if with_mask else None, box)
    for f, g in zip(frames, got):
        want = image.copy()
        want.paste(f.resize((r - l, b - t), Image.LANCZOS), (l, t), Image.fromarray(mask).crop(box) if with_mask else None)
        assert g.size == image.size and np.array_equal(np.array(g), np.array(want))
        if with_mask:  # the photo's bytes wherever the source-size mask is 0
            assert np.array_equal(np.array(g)[mask == 0], np.array(image)[mask == 0])
        else:
            assert np.array_equal(np.array(g)[t:b, l:r], np.array(f.resize((r - l, b - t), Image.LANCZOS)))
    assert np.array_equal(np.array(image), np.array(photo_and_mask()[0]))  # the caller's image is untouched


def test_the_pipeline_switches():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    pipe = ChronoEditPipeline()
    assert pipe._region_focus is None and pipe.focus_report is None
    assert pipe.enable_region_focus() is pipe and pipe._region_focus == 0.25
    assert pipe.enable_region_focus(context=1) is pipe and pipe._region_focus == 1.0
    with pytest.raises(ValueError):
        pipe.enable_region_focus(-1)
    assert pipe.disable_region_focus() is pipe and pipe._region_focus is None
