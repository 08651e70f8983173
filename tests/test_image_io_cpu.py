"""Host side of the device image pre- / post-processing (chronoedit_amd/image_io.py): the resize tables replayed in numpy equal PIL's
resize bit for bit, the lookup tables equal the host path on every byte, the CLIP front end declines what it does not reproduce."""
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import image_io

# (W, H) -> (W2, H2)
SHAPES = [((37, 23), (16, 16)), ((64, 48), (80, 96)), ((301, 200), (128, 80)), ((129, 77), (129, 40)), ((77, 129), (40, 129)),
          ((50, 50), (224, 224)), ((640, 360), (398, 224)), ((1, 9), (5, 3)), ((1000, 40), (150, 40)), ((1280, 720), (1280, 720))]
FILTERS = {image_io.LANCZOS: Image.LANCZOS, image_io.BICUBIC: Image.BICUBIC}


def random_rgb(size, seed=0):
    w, h = size
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def replay_pass(src, axis, coeff, bounds):
    """The integer pass of PIL's 8-bit resampler along `axis` of uint8 [H, W, 3] (axis 0: horizontal)."""
    src = src.astype(np.int32)
    rows = []
    for k, (first, count) in zip(coeff, bounds):
        window = src[:, first:first + count] if axis == 0 else src[first:first + count]
        kk = np.asarray(k[:count], dtype=np.int32)
        ss = (1 << 21) + np.tensordot(window, kk, axes=([1 if axis == 0 else 0], [0]))
        rows.append(np.clip(ss >> 22, 0, 255).astype(np.uint8))
    return np.stack(rows, axis=1 if axis == 0 else 0)


def replay_resize(src, size, filter):
    (W2, H2), (H, W) = size, src.shape[:2]
    launches = 0
    if W2 != W:
        coeff, bounds, _ = image_io.resize_tables(W, W2, filter)
        src, launches = replay_pass(src, 0, coeff, bounds), launches + 1
    if H2 != H:
        coeff, bounds, _ = image_io.resize_tables(H, H2, filter)
        src, launches = replay_pass(src, 1, coeff, bounds), launches + 1
    return src, launches


@pytest.mark.parametrize("filter", list(FILTERS))
@pytest.mark.parametrize("src_size,dst_size", SHAPES)
def test_resize_tables_replayed_in_numpy_equal_pil(src_size, dst_size, filter):
    src = random_rgb(src_size, seed=sum(src_size) + sum(dst_size))
    want = np.asarray(Image.fromarray(src).resize(dst_size, FILTERS[filter]))
    got, launches = replay_resize(src, dst_size, filter)
    assert launches == (src_size[0] != dst_size[0]) + (src_size[1] != dst_size[1])
    assert got.shape == want.shape and np.array_equal(got, want)


def test_tables_have_the_shape_the_kernel_reads():
    coeff, bounds, ksize = image_io.resize_tables(1000, 150, image_io.LANCZOS)
    assert ksize == 41 and len(coeff) == len(bounds) == 150 and all(len(r) == ksize for r in coeff)
    assert max(c for _, c in bounds) == 40  # a 6.7x reduction: windows of 2 * 3 * 6.67 = 40 source pixels in rows of ksize = 41
    assert all(f >= 0 and c >= 1 and f + c <= 1000 for f, c in bounds)
    assert all(abs(sum(r) - (1 << 22)) <= ksize for r in coeff)  # normalised weights, each rounded to 22 bits


def test_vae_table_equals_preprocess_image_on_every_byte():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    img = Image.fromarray(np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2))
    want = ChronoEditPipeline.preprocess_image(img, 16, 16).to(torch.bfloat16)  # [1, 3, 16, 16]
    lut = image_io.vae_table()
    assert lut.dtype == torch.bfloat16 and lut.shape == (3, 256)
    assert torch.equal(lut.view(torch.int16), want[0].reshape(3, 256).view(torch.int16))


def clip_processors():
    from transformers import CLIPImageProcessor
    return [CLIPImageProcessor(), CLIPImageProcessor(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})]


@pytest.mark.parametrize("which", [0, 1])
def test_clip_table_equals_the_processor_on_every_channel_and_byte(which):
    proc = clip_processors()[which]
    assert image_io.clip_recipe(proc) == ((224, 224, 224, True), (56, 56, 56, True))[which]
    lut = image_io.clip_table(proc)
    assert lut.dtype == torch.float32 and lut.shape == (3, 256)
    s = (224, 56)[which]
    # every (channel, byte) pair through the WHOLE processor: a constant image stays constant under the resize and the crop
    for c in range(3):
        for lo in range(0, 256, 64):
            imgs = []
            for v in range(lo, lo + 64):
                a = np.zeros((s, s, 3), dtype=np.uint8)
                a[..., c] = v
                imgs.append(Image.fromarray(a))
            px = proc(images=imgs, return_tensors="pt")["pixel_values"]
            assert px.shape == (64, 3, s, s)
            assert torch.equal(px[:, c, 0, 0].view(torch.int32), lut[c, lo:lo + 64].view(torch.int32))
            assert torch.equal(px[:, c].view(torch.int32), px[:, c, :1, :1].expand(-1, s, s).contiguous().view(torch.int32))
            other = [k for k in range(3) if k != c]
            assert torch.equal(px[:, other, 0, 0].view(torch.int32), lut[other, 0].expand(64, 2).contiguous().view(torch.int32))


def test_clip_front_end_declines_what_it_does_not_reproduce():
    from transformers import CLIPImageProcessor
    img = Image.fromarray(random_rgb((90, 70)))
    assert image_io.clip_pixel_values(CLIPImageProcessor(do_center_crop=False), img, "cpu") is None
    assert image_io.clip_pixel_values(CLIPImageProcessor(resample=Image.BILINEAR), img, "cpu") is None
    assert image_io.clip_pixel_values(CLIPImageProcessor(), np.asarray(img), "cpu") is None
    assert image_io.clip_pixel_values(CLIPImageProcessor(), [img, np.asarray(img)], "cpu") is None
    assert image_io.clip_pixel_values(CLIPImageProcessor(do_normalize=False), img, "cpu") is None
    assert image_io.clip_pixel_values(CLIPImageProcessor(size={"height": 224, "width": 224}), img, "cpu") is None
    # a crop larger than the resized image makes the processor pad
    assert image_io.clip_pixel_values(CLIPImageProcessor(size={"shortest_edge": 56}), img, "cpu") is None

    class NotClip:
        size = 56

        def __call__(self, images=None, return_tensors="pt"):
            raise AssertionError("not called")
    assert image_io.clip_pixel_values(NotClip(), img, "cpu") is None


def test_entry_points_are_declared_with_the_headers_arity():
    from chronoedit_amd import hiplib
    assert "ce_image.hip" in hiplib.SOURCES
    for name in ("ce_image_resample_u8", "ce_image_u8_lut_planar", "ce_video_to_u8"):
        assert name in hiplib.header_symbols() and name in hiplib.SIGNATURES, name
