"""The two device passes of csrc/ce_layers.hip bit for bit against the host forms of chronoedit_amd/layers.py: boxes of 1 x 1, one pixel
wide, one pixel high and the whole photo; boxes at odd left / top in photos whose width is no multiple of 4; layer, plane and canvas at every
base address modulo 4 (and the layer at 4 and 8 modulo 16: dwords, but no 16-byte loads); garbage in the plane and the canvas, and guard
bytes around them, all compared; every alpha against every threshold; two overlapping layers in both orders; a second run."""
import ctypes

import layers_values as V
import numpy as np
import pytest
import torch

from chronoedit_amd import layers, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
PHOTOS = [(53, 131), (65, 33), (64, 40)]  # (SW, SH): 131 x 53 and 33 x 65 planes as the cluster tests use, and a width that is a multiple of 4
THRESHOLDS = (0, 1, 127, 254)


def boxes_of(SW, SH):
    """(left, top, right, bottom): 1 x 1, one pixel wide, one pixel high, the whole photo, and boxes at odd corners with every width modulo 4."""
    out = [(SW - 1, SH - 1, SW, SH), (0, 0, 1, 1), (5, 0, 6, SH), (0, 7, SW, 8), (0, 0, SW, SH)]
    out += [(3, 5, 3 + w, 5 + 9) for w in (4, 5, 6, 7, 17)] + [(1, 1, SW - 2, SH - 3), (2, 3, SW, SH), (7, 2, 7 + 32, SH - 1)]
    return out


def guarded(t: torch.Tensor, offset: int):
    """(the whole allocation, its view of t's shape whose first byte lies `offset` past a 256-byte aligned address) - guard bytes around the view."""
    base = torch.full((GUARD + offset + t.numel() + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    assert base.data_ptr() % 256 == 0
    v = base[GUARD + offset:GUARD + offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == offset % 16 and v.is_contiguous()
    return base, v


def rgba(rng, bh, bw):
    a = rng.integers(0, 256, (bh, bw, 4), dtype=np.uint8)
    u = rng.random((bh, bw))
    a[..., 3][u < 0.3] = 0
    a[..., 3][u > 0.7] = 255
    return torch.from_numpy(a)


def want_strokes(plane: torch.Tensor, lb, threshold):
    l, t, r, b = lb.box
    out = plane.clone()
    out[t:b, l:r][lb.rgba[:, :, 3] > threshold] = 255
    return out


@pytest.mark.parametrize("photo", PHOTOS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_passes_equal_the_host_forms_for_every_box_and_base(photo):
    SW, SH = photo
    rng = np.random.default_rng(SW)
    garbage_plane = torch.from_numpy(rng.integers(0, 256, (SH, SW), dtype=np.uint8))
    garbage_canvas = torch.from_numpy(rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8))
    wide = 0
    for k, box in enumerate(boxes_of(SW, SH)):
        l, t, r, b = box
        host = layers.LayerBox(0, box, rgba(rng, b - t, r - l))
        for layer_off, image_off in ((0, 0), (4, 1), (1, 2), (8, 3), (3, 0), (2, 1), (0, 3), (0, 2)):
            _, dev_rgba = guarded(host.rgba, layer_off)
            lb = layers.LayerBox(0, box, dev_rgba)
            threshold = THRESHOLDS[(k + layer_off) % 4]
            pbase, plane = guarded(garbage_plane, image_off)
            before = pbase.clone()
            assert ops.layers_strokes_u8(dev_rgba, l, t, plane, threshold) is plane
            assert torch.equal(plane.cpu(), want_strokes(garbage_plane, host, threshold)), (box, layer_off, image_off)
            before[GUARD + image_off:GUARD + image_off + SH * SW] = plane.reshape(-1)
            assert torch.equal(pbase, before)  # the guard bytes
            cbase, canvas = guarded(garbage_canvas, image_off)
            before = cbase.clone()
            assert layers.over(canvas, lb) is canvas
            want = layers.over(garbage_canvas.clone(), host)
            assert torch.equal(canvas.cpu(), want), (box, layer_off, image_off)
            before[GUARD + image_off:GUARD + image_off + SH * SW * 3] = canvas.reshape(-1)
            assert torch.equal(cbase, before)
            outside = torch.ones(SH, SW, dtype=torch.bool)
            outside[t:b, l:r] = False
            assert torch.equal(canvas.cpu()[outside], garbage_canvas[outside]) and torch.equal(plane.cpu()[outside], garbage_plane[outside])
            # run twice, the same bits: fresh copies of the same garbage, at the same addresses modulo 16
            _, plane2 = guarded(garbage_plane, image_off)
            _, canvas2 = guarded(garbage_canvas, image_off)
            ops.layers_strokes_u8(dev_rgba, l, t, plane2, threshold), ops.layers_over_u8(dev_rgba, l, t, canvas2)
            assert torch.equal(plane2, plane) and torch.equal(canvas2, canvas), (box, layer_off, image_off)
            # and a second run on the first run's output: the strokes stay (idempotent), the blend goes on from there - the same bits as the host's
            ops.layers_strokes_u8(dev_rgba, l, t, plane, threshold)
            assert torch.equal(plane.cpu(), want_strokes(garbage_plane, host, threshold))
            assert torch.equal(layers.over(canvas, lb).cpu(), layers.over(want.clone(), host))
            wide += (r - l) >= 8 and layer_off % 4 == 0
    assert wide >= 8  # (boxes with runs of four at aligned addresses were among them)
    # the public forms where the bytes lie: a zeroed plane, a copy of the background
    lbs = [layers.LayerBox(i, bx, rgba(rng, bx[3] - bx[1], bx[2] - bx[0])) for i, bx in enumerate(boxes_of(SW, SH)[4:8])]
    dev = layers.uploaded(lbs, DEV)
    assert all(d.rgba.is_cuda and d.box == h.box and d.index == h.index for d, h in zip(dev, lbs))
    for threshold in THRESHOLDS:
        got = layers.strokes(dev, photo, threshold, DEV)
        assert got.is_cuda and torch.equal(got.cpu(), layers.strokes(lbs, photo, threshold))
    bg = garbage_canvas.to(DEV)
    got = layers.composite_u8(bg, dev)
    assert got.data_ptr() != bg.data_ptr() and torch.equal(bg.cpu(), garbage_canvas) and torch.equal(got.cpu(), layers.composite_u8(garbage_canvas, lbs))


def test_every_alpha_against_every_threshold_and_every_byte_pair():
    """A row of 256 pixels whose alpha counts 0..255: the strokes at each threshold; and the blend of every (source, alpha, destination)
    triple, 2^24 of them, as 256 boxes of 256 x 256 in one canvas."""
    a = np.zeros((1, 256, 4), np.uint8)
    a[0, :, 3] = np.arange(256)
    row = layers.LayerBox(0, (2, 3, 258, 4), torch.from_numpy(a))
    dev = layers.uploaded([row], DEV)
    for threshold in THRESHOLDS:
        got = layers.strokes(dev, (261, 5), threshold, DEV).cpu()
        assert torch.equal(got, layers.strokes([row], (261, 5), threshold)) and int((got != 0).sum()) == 255 - threshold
        assert got[3, 2 + threshold] == 0 and got[3, 3 + threshold] == 255
    s = np.arange(256, dtype=np.uint8)
    src = np.zeros((256, 256, 4), np.uint8)
    src[..., 0], src[..., 1], src[..., 2] = s[None, :], s[None, ::-1], (s[None, :] * 7 + 3).astype(np.uint8)
    dst = np.stack([np.broadcast_to(s[:, None], (256, 256)), np.broadcast_to((s[:, None] * 5 + 1).astype(np.uint8), (256, 256)),
                    np.broadcast_to(s[::-1, None], (256, 256))], axis=-1)
    canvas = torch.from_numpy(np.tile(dst, (1, 16, 1)).copy())  # 256 x 4096: sixteen boxes side by side, sixteen rounds
    for rnd in range(16):
        lbs = []
        for i in range(16):
            src[..., 3] = 16 * rnd + i
            lbs.append(layers.LayerBox(i, (256 * i, 0, 256 * i + 256, 256), torch.from_numpy(src.copy())))
        got = layers.composite_u8(canvas.to(DEV), layers.uploaded(lbs, DEV))
        assert torch.equal(got.cpu(), layers.composite_u8(canvas, lbs)), rnd


def test_two_overlapping_layers_in_both_orders():
    SW, SH = 53, 131
    rng = np.random.default_rng(5)
    photo = torch.from_numpy(rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8))
    a = layers.LayerBox(0, (3, 5, 40, 90), rgba(rng, 85, 37))
    b = layers.LayerBox(1, (21, 60, 53, 131), rgba(rng, 71, 32))
    ab, ba = layers.composite_u8(photo, [a, b]), layers.composite_u8(photo, [b, a])
    assert not torch.equal(ab, ba)  # the order matters for `over`
    da, db = layers.uploaded([a, b], DEV)
    assert torch.equal(layers.composite_u8(photo.to(DEV), [da, db]).cpu(), ab) and torch.equal(layers.composite_u8(photo.to(DEV), [db, da]).cpu(), ba)
    for threshold in THRESHOLDS:
        want = layers.strokes([a, b], (SW, SH), threshold)
        one, two = layers.strokes([da, db], (SW, SH), threshold, DEV), layers.strokes([db, da], (SW, SH), threshold, DEV)
        assert torch.equal(one, two) and torch.equal(one.cpu(), want)  # ... and not for the strokes
    # against PIL itself, from PIL layers
    from PIL import Image
    ls = V.random_layers((SW, SH), 3, seed=6)
    background = Image.fromarray(photo.numpy())
    host = layers.boxes(ls)
    dev = layers.uploaded(host, DEV)
    assert np.array_equal(layers.composite_u8(photo.to(DEV), dev).cpu().numpy(), np.asarray(V.pil_composite(background, ls)))
    assert np.array_equal(layers.strokes(dev, (SW, SH), 127, DEV).cpu().numpy(), np.asarray(V.pil_strokes((SW, SH), ls, 127)))


def test_the_launchers_refusals():
    from chronoedit_amd.hiplib import load
    lib = load()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    layer = torch.zeros(4, 4, 4, dtype=torch.uint8, device=DEV)
    plane, canvas = torch.zeros(8, 8, dtype=torch.uint8, device=DEV), torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV)
    assert lib.ce_layers_strokes_u8(P(layer), 4, 4, 5, 5, P(plane), 8, 8, 0, stream) == -1  # the box leaves the photo
    assert lib.ce_layers_strokes_u8(P(layer), 4, 4, -1, 0, P(plane), 8, 8, 0, stream) == -1
    assert lib.ce_layers_strokes_u8(P(layer), 4, 4, 0, 0, P(plane), 8, 8, 255, stream) == -1  # the threshold
    assert lib.ce_layers_strokes_u8(P(layer), 0, 4, 0, 0, P(plane), 8, 8, 0, stream) == -1
    assert lib.ce_layers_strokes_u8(None, 4, 4, 0, 0, P(plane), 8, 8, 0, stream) == -1
    assert lib.ce_layers_strokes_u8(P(layer), 4, 4, 0, 0, P(layer), 8, 8, 0, stream) == -1  # in place on the layer itself
    # a layer that shares some bytes with the image, at another base address, is refused too; one that ends where the image begins is not
    assert lib.ce_layers_over_u8(P(canvas, 100), 4, 4, 0, 0, P(canvas), 8, 8, stream) == -1
    assert lib.ce_layers_strokes_u8(P(plane, 63), 4, 4, 0, 0, P(plane), 8, 8, 0, stream) == -1
    both = torch.zeros(64 + 64, dtype=torch.uint8, device=DEV)
    assert lib.ce_layers_strokes_u8(P(both), 4, 4, 0, 0, P(both, 64), 8, 8, 0, stream) == 0
    assert lib.ce_layers_over_u8(P(layer), 4, 4, 4, 5, P(canvas), 8, 8, stream) == -1
    assert lib.ce_layers_over_u8(P(layer), 4, 4, 0, 0, None, 8, 8, stream) == -1
    assert lib.ce_layers_over_u8(P(layer), 4, 4, 4, 4, P(canvas), 8, 8, stream) == 0  # (the last box that fits)
    with pytest.raises(ValueError, match="does not lie inside"):
        ops.layers_over_u8(layer, 5, 5, canvas)
    with pytest.raises(ValueError, match="threshold"):
        ops.layers_strokes_u8(layer, 0, 0, plane, 255)
    torch.cuda.synchronize()
    assert not plane.any() and not canvas.any()
