"""csrc/ce_focus.hip against PIL on the host, bit for bit: the single-channel resampler through a row pitch and the source-size paste."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import focus, hiplib, image_io, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def random_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def on_device(a: np.ndarray, offset: int = 0) -> torch.Tensor:
    """The array on the device, its first byte `offset` bytes into the allocation."""
    buf = torch.empty(a.size + offset, dtype=torch.uint8, device=DEV)
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    return view


# (W, H) -> (W2, H2): both axes shrinking and enlarging; rows that keep the dword body aligned (multiples of 4) and rows that do not;
# one axis unchanged (a single pass)
L_SHAPES = [((53, 37), (24, 16)), ((53, 37), (96, 80)), ((53, 37), (23, 17)), ((52, 36), (24, 80)), ((36, 53), (36, 20)), ((37, 53), (37, 70)),
            ((31, 20), (45, 20)), ((31, 20), (44, 20)), ((300, 7), (40, 7)), ((5, 300), (5, 64))]


@pytest.mark.parametrize("src_size,dst_size", L_SHAPES)
def test_resize_l8_equals_pil(src_size, dst_size):
    a = random_u8((src_size[1], src_size[0]), 1)
    want = np.array(Image.fromarray(a).resize(dst_size, Image.BILINEAR))
    got = focus.resize_l8(on_device(a), dst_size).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


# a crop of a [37, 53] / [40, 56] mask addressed through the pitch: odd offsets, and a crop whose rows stay dword aligned inside a 56-byte pitch
@pytest.mark.parametrize("shape,box", [((37, 53), (3, 5, 40, 30)), ((40, 56), (4, 5, 40, 30)), ((40, 56), (3, 5, 39, 30)), ((40, 56), (0, 0, 56, 40))])
@pytest.mark.parametrize("dst_size", [(96, 64), (16, 8), (36, 50), (37, 25)])
def test_resize_l8_of_a_crop_through_the_pitch(shape, box, dst_size):
    a = random_u8(shape, 2)
    l, t, r, b = box
    want = np.array(Image.fromarray(a).crop(box).resize(dst_size, Image.BILINEAR))
    view = on_device(a)[t:b, l:r]
    assert view.stride(0) == shape[1] and (view.stride(0) != view.shape[1] or box == (0, 0, 56, 40))
    got = focus.resize_l8(view, dst_size).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("axis", [0, 1])
def test_resample_l8_with_bases_one_byte_into_their_allocations(axis):
    a = random_u8((36, 52), 3)  # (rows of a multiple of 4: only the bases break the alignment)
    out_len = 24
    tables = image_io._device_tables(a.shape[1 - axis], out_len, image_io.BILINEAR, torch.device(DEV))
    shape = (36, out_len) if axis == 0 else (out_len, 52)
    want = np.array(Image.fromarray(a).resize((out_len, 36) if axis == 0 else (52, out_len), Image.BILINEAR))
    for src_off, dst_off in ((1, 0), (0, 1), (1, 1), (0, 0)):
        out = on_device(np.zeros(shape, np.uint8), dst_off)
        ops.focus_resample_l8(on_device(a, src_off), axis, *tables, out=out)
        assert np.array_equal(out.cpu().numpy(), want), (src_off, dst_off)


@pytest.mark.parametrize("filter", [image_io.LANCZOS, image_io.BICUBIC])
def test_rgb_enlargement_through_resize_u8(filter):
    a = random_u8((16, 24, 3), 4)
    want = np.array(Image.fromarray(a).resize((37, 25), {image_io.LANCZOS: Image.LANCZOS, image_io.BICUBIC: Image.BICUBIC}[filter]))
    got = image_io.resize_u8(on_device(a), (37, 25), filter).cpu().numpy()
    assert np.array_equal(got, want)


SH = 41


def boxes(SW):
    return {"odd left": (7, 9, 30, 28), "top left": (0, 0, 20, 13), "top right": (SW - 21, 0, SW, 16), "bottom left": (0, SH - 11, 24, SH),
            "bottom right": (SW - 19, SH - 17, SW, SH), "whole image": (0, 0, SW, SH), "one pixel": (SW - 1, SH - 1, SW, SH)}


def masks(SW):
    rng = np.random.default_rng(5)
    tiles = rng.integers(0, 256, (SH, SW), dtype=np.uint8)
    tiles[:16] = 0
    tiles[16:32, :24] = 255
    return {"none": None, "random": rng.integers(0, 256, (SH, SW), dtype=np.uint8), "tiles": tiles}


# 52 columns: the frame's bytes are a multiple of 4 (the dword body, unless a base is misaligned); 53: they are not
@pytest.mark.parametrize("SW,offset", [(52, 0), (53, 0), (52, 1), (53, 3)])
def test_paste_equals_pil(SW, offset):
    src = random_u8((SH, SW, 3), 6)
    src_pil, src_dev = Image.fromarray(src), on_device(src, offset)
    for name, box in boxes(SW).items():
        l, t, r, b = box
        for F in (1, 3):
            edit = random_u8((F, b - t, r - l, 3), 7 + F)
            for kind, mask in masks(SW).items():
                mask_dev = None if mask is None else on_device(mask, offset)
                out = on_device(np.zeros((F, SH, SW, 3), np.uint8), offset)
                ops.focus_paste_u8(on_device(edit, offset), src_dev, mask_dev, l, t, out=out)
                got = out.cpu().numpy()
                for f in range(F):
                    want = src_pil.copy()
                    want.paste(Image.fromarray(edit[f]), (l, t), None if mask is None else Image.fromarray(mask).crop(box))
                    want = np.array(want)
                    assert np.array_equal(got[f], want), (name, F, kind, f)
                    outside = np.ones((SH, SW), bool)
                    outside[t:b, l:r] = False
                    assert np.array_equal(got[f][outside], src[outside])  # outside the box: the source
                    inside = got[f][t:b, l:r]
                    m = np.full((b - t, r - l), 255, np.uint8) if mask is None else mask[t:b, l:r]
                    assert np.array_equal(inside[m == 0], src[t:b, l:r][m == 0])  # m == 0: the source byte
                    assert np.array_equal(inside[m == 255], edit[f][m == 255])  # m == 255: the edit byte
    assert np.array_equal(src_dev.cpu().numpy(), src)  # the source is only read


def test_paste_of_resized_frames_equals_host_paste():
    """focus.device_paste (Lanczos to the box, then the paste) against focus.host_paste (PIL itself), enlarging and shrinking."""
    src = random_u8((150, 203, 3), 8)
    mask = np.zeros((150, 203), np.uint8)
    mask[20:60, 110:170] = random_u8((40, 60), 9)
    frames = random_u8((2, 64, 96, 3), 10)
    for box in ((80, 10, 200, 90), (100, 20, 172, 68), (90, 15, 186, 79)):  # scale 1.25, 0.75 and 1
        for m in (mask, None):
            want = focus.host_paste(Image.fromarray(src), [Image.fromarray(f) for f in frames], None if m is None else torch.from_numpy(m), box)
            got = focus.device_paste(on_device(frames), on_device(src), None if m is None else on_device(m), box).cpu().numpy()
            assert np.array_equal(got, np.stack([np.array(w) for w in want])), (box, m is None)


def test_bad_arguments_are_refused():
    lib = hiplib.load()
    src, edit = on_device(random_u8((SH, 52, 3), 1)), on_device(random_u8((1, 10, 10, 3), 2))
    out = torch.zeros((1, SH, 52, 3), dtype=torch.uint8, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    paste = lambda left, top, bw=10, bh=10, sh=SH, sw=52, o=out: lib.ce_focus_paste_u8(P(edit), P(src), None, P(o), 1, sh, sw, left, top, bw, bh, None)
    for left, top in ((43, 0), (0, SH - 9), (-1, 0), (0, -1)):  # a box that leaves the image
        assert paste(left, top) == -1
        with pytest.raises(ValueError):
            ops.focus_paste_u8(edit, src, None, left, top, out=out)
    assert paste(0, 0, bw=0) == -1 and paste(0, 0, o=src) == -1
    assert paste(0, 0, sh=30000, sw=30000) == -2  # 2^31 bytes or more (refused before anything is launched)
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched
    coeff, bounds = image_io._device_tables(52, 24, image_io.BILINEAR, torch.device(DEV))
    mask, dst = on_device(random_u8((SH, 52), 3)), torch.zeros((SH, 24), dtype=torch.uint8, device=DEV)
    resample = lambda pitch=52, axis=0, h=SH, w=52: lib.ce_focus_resample_l8(P(mask), pitch, P(dst), axis, h, w, 24, P(coeff), P(bounds), 3, None)
    assert resample(pitch=51) == -1 and resample(axis=2) == -1
    assert resample(pitch=1 << 20, h=1 << 11) == -2
    torch.cuda.synchronize()
    assert not dst.any()
    with pytest.raises(ValueError):
        ops.focus_resample_l8(mask.t(), 0, coeff, bounds)
