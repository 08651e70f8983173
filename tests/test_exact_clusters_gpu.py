"""The device passes of csrc/ce_clusters.hip bit for bit against the host forms of chronoedit_amd/clusters.py: the cluster table on planes
around the 32 x 64 tile of the labelling (1 x 1, 1 x 70, 33 x 65, 70 x 130; clusters across the tile borders; with and without the weight
filter; garbage in the table and the counters; byte planes at odd addresses; a second run; 400 clusters for 256 rows), the select pass on
its 16-byte and its element path, and the in-place paste against PIL's own paste, chained over two overlapping boxes."""
import ctypes

import components_shapes as S
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import clusters, components, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (1, 70), (33, 65), (70, 130)]


def unaligned(t: torch.Tensor, offset: int) -> torch.Tensor:
    """A copy of the byte plane t on the device whose first byte lies `offset` past an allocation's start."""
    base = torch.full((t.numel() + 8,), 0xA5, dtype=torch.uint8, device=DEV)
    v = base[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == offset % 4 and v.is_contiguous()
    return v


def garbage_i32(*shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int64, device=DEV).to(torch.int32)


def blobs(H, W, seed):
    """Rectangles, some of them across the borders of the 32 x 64 tiles, and single pixels: a few dozen clusters at most."""
    rng = np.random.default_rng(seed)
    p = np.zeros((H, W), np.uint8)
    for _ in range(12):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        p[y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 9))] = 255
    for y0, x0 in ((30, 60), (28, 100), (60, 62)):  # across a tile corner, a horizontal and a vertical border
        if y0 < H and x0 < W:
            p[y0:y0 + 5, x0:x0 + 7] = 200
    p[0, 0] = 1  # (label 0 is a label like any other)
    return p


def cases(H, W):
    out = {"blobs": blobs(H, W, H + W), "blobs2": blobs(H, W, 3 * H + W), "empty": S.empty(H, W), "full": S.full(H, W)}
    for name in ("comb", "serpentine", "spiral", "diagonal", "noise0.2"):
        out[name] = S.adversarial(H, W, seed=H)[name]
    return out


def host_chain(plane: np.ndarray, filtered: bool):
    p = torch.from_numpy(plane)
    weight = torch.from_numpy(S.noise(*plane.shape, 0.5, 3))
    r = components.roots(p)
    s = components.sums(r, weight)
    kept = components.keep(p, r, s, 2)[0] if filtered else p
    return r, s, kept


def device_table(r, s, kept, offset):
    table, counters = garbage_i32(clusters.ROWS, 8), garbage_i32(1 + clusters.ROWS)
    t, c = ops.clusters_table_i32(r.to(DEV), s.to(DEV), unaligned(kept, offset), table, counters)
    assert t is table and c is counters
    return t, c


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_table_equals_the_host_form(size, filtered):
    H, W = size
    compared = 0
    for k, (name, plane) in enumerate(cases(H, W).items()):
        r, s, kept = host_chain(plane, filtered)
        count, want = clusters.table(r, s, kept)
        t, c = device_table(r, s, kept, 1 + k % 3)
        assert int(c[0]) == int(count), name
        if int(count) <= clusters.ROWS:
            assert t.dtype == torch.int32 and torch.equal(t.cpu(), want), name
            compared += int(count) > 0
        t2, c2 = device_table(r, s, kept, (k + 2) % 4)  # a second run, other garbage, another address
        assert int(c2[0]) == int(count) and (int(count) > clusters.ROWS or torch.equal(t2, t)), name
        got = clusters.table(r.to(DEV), s.to(DEV), kept.to(DEV))  # the public form, where the planes lie
        assert got[0].is_cuda and int(got[0]) == int(count) and (int(count) > clusters.ROWS or torch.equal(got[1].cpu(), want)), name
    assert compared >= (3 if H * W > 1 else int(not filtered))  # (a single pixel of weight 1 does not pass the filter: nothing to compare there)


def test_more_clusters_than_rows_gives_the_exact_count():
    p = torch.zeros(40, 40, dtype=torch.uint8)
    p[::2, ::2] = 255
    r = components.roots(p)
    s = components.sums(r)
    t, c = device_table(r, s, p, 3)
    assert int(c[0]) == 400 == int(clusters.table(r, s, p)[0])


def test_the_launchers_refusals():
    from chronoedit_amd.hiplib import load
    lib = load()
    r, s, kept = (t.to(DEV) for t in host_chain(blobs(33, 65, 1), False))
    table, counters = garbage_i32(clusters.ROWS, 8), garbage_i32(2 + clusters.ROWS)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ce_clusters_table_i32(P(r), P(s), P(kept), P(table), P(counters), 100, 33, 65, stream) == -1  # another table in mind
    assert lib.ce_clusters_table_i32(P(r), P(s), P(kept), P(table), P(counters, 2), 256, 33, 65, stream) == -3
    assert lib.ce_clusters_table_i32(P(r), P(s), P(kept), P(table), P(counters), 256, 0, 65, stream) == -1
    assert lib.ce_clusters_select_u8(P(r), P(kept), P(table), P(counters), 0, P(kept), 33, 65, stream) == -1  # out aliases kept
    canvas, edit = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV)
    assert lib.ce_clusters_paste_u8(P(edit), None, P(canvas), 1, 8, 8, 5, 5, 4, 4, stream) == -1  # the box leaves the image
    with pytest.raises(ValueError, match="does not lie inside"):
        ops.clusters_paste_u8(edit, None, canvas, 5, 5)
    torch.cuda.synchronize()


# ---- select ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_equals_the_host_expression_for_every_group(size, aligned):
    H, W = size
    n = H * W
    for name in ("blobs", "blobs2"):
        r, s, kept = host_chain(cases(H, W)[name], True)
        count, rows = clusters.table(r, s, kept)
        c = int(count)
        assert c <= clusters.ROWS
        groups = [g for g in ([i for i in range(c) if i % 3 == k] for k in range(3)) if g]
        gor = clusters.group_of_row(groups).to(DEV)
        if aligned:
            labels, kp = r.to(DEV), kept.to(DEV)
            assert labels.data_ptr() % 16 == 0 and kp.data_ptr() % 4 == 0
        else:  # labels 4 bytes past a 16-byte boundary, the byte planes at odd addresses
            base = garbage_i32(n + 8)
            labels = base[1:1 + n].view(H, W)
            labels.copy_(r)
            kp = unaligned(kept, 1)
            assert labels.data_ptr() % 16 == 4
        table = rows.to(DEV)
        total = torch.zeros(H, W, dtype=torch.int32)
        for g in range(len(groups) + 1):  # (one group past the last: nothing selected)
            out = unaligned(torch.full((H, W), 0x5A, dtype=torch.uint8), 0 if aligned else 3)
            got = ops.clusters_select_u8(labels, kp, table, gor, g, out)
            want = clusters.select(r, kept, [int(rows[i, 0]) for i in groups[g]] if g < len(groups) else [])
            assert got is out and torch.equal(got.cpu(), want), (name, g)
            total += want.to(torch.int32)
        assert torch.equal(total.to(torch.uint8), kept.clamp(max=1) * 255)
        if c and min(H, W) > 1:  # the masks of the pipeline's path: select, then the two box passes (pinned on their own elsewhere)
            masks = clusters.group_masks(labels, kp, table, rows.tolist(), groups, 2)
            want = clusters.group_masks(r, kept, None, rows.tolist(), groups, 2)
            assert all(torch.equal(a.cpu(), b) for a, b in zip(masks, want))


# ---- paste -----------------------------------------------------------------------------------------------------------------------------
SH, SW = 37, 53
BOXES = [(3, 5, 30, 26), (17, 13, 52, 36)]  # (left, top, right, bottom): overlapping, at odd offsets


def paste_mask(seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 255, (SH, SW), dtype=np.uint8)
    m[:, seed % 7::5] = 0
    m[seed % 3::4] = 255
    assert (m == 0).any() and (m == 255).any() and ((m > 0) & (m < 255)).any()
    return m


@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("F", [1, 5])
def test_paste_equals_pils_paste_chained(F, with_mask):
    rng = np.random.default_rng(F)
    pattern = rng.integers(0, 256, (F, SH, SW, 3), dtype=np.uint8)
    edits = [rng.integers(0, 256, (F, b - t, r - l, 3), dtype=np.uint8) for l, t, r, b in BOXES]
    masks = [paste_mask(11), paste_mask(12)] if with_mask else [None, None]
    canvas = torch.from_numpy(pattern.copy()).to(DEV)
    for (l, t, r, b), e, m in zip(BOXES, edits, masks):
        out = ops.clusters_paste_u8(torch.from_numpy(e).to(DEV), None if m is None else unaligned(torch.from_numpy(m), 1), canvas, l, t)
        assert out is canvas
    got = canvas.cpu().numpy()
    outside = np.ones((SH, SW), bool)
    for f in range(F):
        want = Image.fromarray(pattern[f])
        for (l, t, r, b), e, m in zip(BOXES, edits, masks):
            want.paste(Image.fromarray(e[f]), (l, t), None if m is None else Image.fromarray(m).crop((l, t, r, b)))
            outside[t:b, l:r] = False
        assert np.array_equal(got[f], np.asarray(want)), f
    assert outside.any() and np.array_equal(got[:, outside], pattern[:, outside])  # the pattern outside the boxes comes back unchanged
    # the first crop through ce_focus_paste_u8 (which builds the canvas), the second in place: the pipeline's chain for one photo
    src = torch.from_numpy(pattern[0]).to(DEV)
    dm = [None if m is None else torch.from_numpy(m).to(DEV) for m in masks]
    chained = ops.focus_paste_u8(torch.from_numpy(edits[0]).to(DEV), src, dm[0], BOXES[0][0], BOXES[0][1])
    ops.clusters_paste_u8(torch.from_numpy(edits[1]).to(DEV), dm[1], chained, BOXES[1][0], BOXES[1][1])
    for f in range(F):
        want = Image.fromarray(pattern[0])
        for (l, t, r, b), e, m in zip(BOXES, edits, masks):
            want.paste(Image.fromarray(e[f]), (l, t), None if m is None else Image.fromarray(m).crop((l, t, r, b)))
        assert np.array_equal(chained[f].cpu().numpy(), np.asarray(want)), f
