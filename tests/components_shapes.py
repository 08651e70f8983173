"""Planes for the connected-components tests (tests/test_components_cpu.py, tests/test_exact_components_gpu.py) and for
tools/components_host_check.py: the shapes on which a labelling goes wrong - labels that must be merged late, the longest parent chains,
contacts that exist only diagonally - as uint8 [H, W] numpy arrays with 255 for foreground."""
import numpy as np


def empty(H, W):
    return np.zeros((H, W), np.uint8)


def full(H, W):
    return np.full((H, W), 255, np.uint8)


def checkerboard(H, W):
    """One component under 8-connectivity, and no two foreground pixels share an edge."""
    y, x = np.mgrid[:H, :W]
    return (((y + x) % 2 == 0) * 255).astype(np.uint8)


def diagonal_touch(H, W):
    """Two blobs that touch at ONE diagonal, near the middle (on a tile corner when the middle is one)."""
    p = empty(H, W)
    cy, cx = H // 2, W // 2
    p[max(cy - 3, 0):cy, max(cx - 3, 0):cx] = 255
    p[cy:cy + 3, cx:cx + 3] = 255
    return p


def comb(H, W):
    """Teeth in every other column that meet only in the LAST row: every tooth starts as a label of its own."""
    p = empty(H, W)
    p[:, ::2] = 255
    p[H - 1, :] = 255
    return p


def u_shape(H, W):
    """Two arms in the first and the last column that meet only in the last row."""
    p = empty(H, W)
    p[:, 0] = p[:, W - 1] = p[H - 1, :] = 255
    return p


def serpentine(H, W):
    """A one-pixel path through the whole plane: every other row, joined at alternating ends - the longest parent chains."""
    p = empty(H, W)
    p[::2, :] = 255
    for k, y in enumerate(range(1, H, 2)):
        p[y, W - 1 if k % 2 == 0 else 0] = 255
    return p


def spiral(H, W):
    """A one-pixel path that winds from the rim to the middle, one background pixel between its laps: one component, whose labels meet
    lap by lap."""
    p = empty(H, W)
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    p[0, 0] = 255
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ok = 0 <= ny < H and 0 <= nx < W and not p[ny, nx] and not (0 <= ay < H and 0 <= ax < W and p[ay, ax])
        if ok:
            y, x, turns = ny, nx, 0
            p[y, x] = 255
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return p


def noise(H, W, density, seed=0):
    return ((np.random.default_rng(seed).random((H, W)) < density) * 255).astype(np.uint8)


def root_in_last_tile(H, W, th, tw):
    """One blob wholly inside the last tile of a th x tw tiling (background everywhere else)."""
    p = empty(H, W)
    y0, x0 = (H - 1) // th * th, (W - 1) // tw * tw
    p[y0 + (H - y0) // 2:, x0 + (W - x0) // 2:] = 255
    return p


def adversarial(H, W, seed=0):
    """name -> plane: the whole list at one size."""
    out = {"empty": empty(H, W), "full": full(H, W), "checkerboard": checkerboard(H, W), "diagonal": diagonal_touch(H, W), "comb": comb(H, W),
           "u": u_shape(H, W), "serpentine": serpentine(H, W), "spiral": spiral(H, W)}
    for d in (0.2, 0.4, 0.6):
        out[f"noise{d}"] = noise(H, W, d, seed)
    return out
