"""Editor values with layers for the layers tests (no test in here): rectangles drawn into RGBA layers, PIL's own recipes for the strokes
plane and the composite."""
import numpy as np
from PIL import Image, ImageChops


def layer(size, strokes, color=None, alpha=255, photo=None):
    """An RGBA layer of `size` = (W, H), transparent black except for the rectangles `strokes` = (left, top, right, bottom): `color`
    (r, g, b), or - color None - the photo's bytes ^ 128 (what tests/test_sketch_gpu.py's `draw` writes into a composite)."""
    a = np.zeros((size[1], size[0], 4), np.uint8)
    for l, t, r, b in strokes:
        a[t:b, l:r, :3] = color if color is not None else np.array(photo.convert("RGB"))[t:b, l:r] ^ 128
        a[t:b, l:r, 3] = alpha
    return Image.fromarray(a, mode="RGBA")


def pil_composite(background, layers):
    """The definition of the issue: PIL's alpha_composite, chained."""
    canvas = background.convert("RGB")
    for ly in layers:
        canvas = Image.alpha_composite(canvas.convert("RGBA"), ly.convert("RGBA")).convert("RGB")
    return canvas


def pil_strokes(size, layers, threshold):
    """The definition of the issue: point() on the alpha channel, combined by ImageChops.lighter."""
    out = Image.new("L", size, 0)
    for ly in layers:
        out = ImageChops.lighter(out, ly.convert("RGBA").getchannel("A").point(lambda v: 255 if v > threshold else 0))
    return out


def value(background, layers, composite=True):
    v = {"background": background, "layers": list(layers)}
    if composite:
        v["composite"] = pil_composite(background, layers)
    return v


def random_layers(size, n=3, seed=0):
    """Random RGBA layers: alpha 0, 255 and in between, each with an empty margin so that the boxes differ and sit at odd offsets."""
    rng = np.random.default_rng(seed)
    W, H = size
    out = []
    for k in range(n):
        a = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        u = rng.random((H, W))
        a[..., 3][u < 0.3] = 0
        a[..., 3][u > 0.7] = 255
        a[:3 + 2 * k], a[H - 1 - k:], a[:, :1 + 3 * k], a[:, W - 2 - k:] = 0, 0, 0, 0
        out.append(Image.fromarray(a, mode="RGBA"))
    return out
