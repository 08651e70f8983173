"""The four gather / scatter passes of csrc/ce_sparse.hip, element by element: each is bit-equal (torch.equal) to its torch indexing
expression, and a destination pre-filled with a pattern is untouched outside the listed rows / columns / cells.

Na 1, 8, 63, 64, 200; N = 160 (latents 2 x 16 x 20: 2.5 key tiles) - and 7 200 for the row scatter; D 256 and 5 120; B 1 and 2 (for V^T sample 1
then starts at column 160, mid-tile, with ldvt = vt_columns(B * N)); ids as one long run, as singletons, and as a set that holds token 0 and
token N - 1; int32 and int64.  200 ids do not fit 160 tokens (the launchers refuse Na > N, checked below): that row count runs on 4 frames of the
same plane, N = 320, where sample 1 starts at column 320."""
import pytest
import torch

from chronoedit_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAS = (1, 8, 63, 64, 200)
KINDS = ("run", "singletons", "ends")
Hh, Ww = 16, 20  # latent plane: 8 x 10 patches


def frames_for(na):
    return 2 if na <= 160 else 4


def make_ids(na, N, kind, seed=0):
    g = torch.Generator().manual_seed(1000 * na + seed)
    if kind == "run":  # one long run, off the start
        s = min(37, N - na)
        ids = torch.arange(s, s + na)
    elif kind == "singletons" and 2 * na <= N:  # no two neighbours
        ids = torch.arange(na) * 2 + 1
    elif kind == "singletons":  # (more than half the tokens: as scattered as they can be)
        ids = torch.randperm(N, generator=g)[:na].sort().values
    else:  # token 0 and token N - 1 (one id: the last token), the rest anywhere
        mid = (torch.randperm(N - 2, generator=g)[: max(na - 2, 0)] + 1).sort().values
        ids = torch.cat([torch.tensor([0]), mid, torch.tensor([N - 1])]) if na >= 2 else torch.tensor([N - 1])
    assert ids.numel() == na and bool((ids[1:] > ids[:-1]).all()) and 0 <= int(ids[0]) and int(ids[-1]) < N
    return ids


def dev_ids(ids, i64):
    return ids.to(device="cuda:0", dtype=torch.int64 if i64 else torch.int32)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator(device="cuda:0").manual_seed(seed), device="cuda:0")


def pattern(shape, seed):
    """The pre-fill of a destination: finite bf16 values around 100, far from anything a source holds."""
    return (_randn(shape, seed) * 3.0 + 100.0).to(BF)


def rnd(shape, seed):
    return _randn(shape, seed).to(BF)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na", NAS)
def test_patchify_rows_of_the_listed_tokens(na, kind):
    C, T, kpad = 36, frames_for(na), 192
    Hp, Wp = Hh // 2, Ww // 2
    N = T * Hp * Wp
    x = rnd((C, T, Hh, Ww), 1)
    full = torch.zeros((N, kpad), dtype=BF, device="cuda:0")
    full[:, : C * 4] = x.view(C, T, Hp, 2, Wp, 2).permute(1, 2, 4, 0, 3, 5).reshape(N, C * 4)  # k = c*4 + dh*2 + dw
    ids = make_ids(na, N, kind)
    for i64 in (False, True):
        out = pattern((na + 2, kpad), 2)  # two guard rows behind the result
        guard = out[na:].clone()
        got = ops.sparse_patchify(x, dev_ids(ids, i64), kpad, out=out[:na])
        assert torch.equal(got, full[ids.cuda()]), (na, kind, i64)
        assert torch.equal(out[na:], guard)
    assert torch.equal(ops.patchify(x, kpad), full)  # (the expression is the dense pass's)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na", NAS)
def test_scatter_rows(na, kind):
    for N in ((160, 7200) if na <= 160 else (320, 7200)):
        ids = make_ids(na, N, kind)
        for B in (1, 2):
            for D in (256, 5120):
                wide = rnd((B * na, 2 * D), 3)
                src = wide[:, D:]  # the K half of a q | k buffer: row stride 2 D
                dst = pattern((B * N, D), 4)
                want = dst.clone()
                for b in range(B):
                    want[b * N + ids.cuda()] = src[b * na:(b + 1) * na]
                ops.sparse_scatter_rows_(dst, src, dev_ids(ids, (B + D) % 3 == 0), batch=B)
                assert torch.equal(dst, want), (na, kind, N, B, D)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na", NAS)
def test_scatter_vt_both_source_forms(na, kind):
    N = 160 if na <= 160 else 320
    ids = make_ids(na, N, kind)
    for B in (1, 2):
        for D in (256, 5120):
            v = rnd((B * na, D), 5)  # row-major V of the active rows
            ldvt = ops.vt_columns(B * N)
            for src_rows in (False, True):
                if src_rows:
                    src = v
                else:  # V^T [D][B*Na] with a row stride of its own, as a view of a wider buffer
                    src = torch.zeros((D, B * na + 8), dtype=BF, device="cuda:0")[:, : B * na]
                    src.copy_(v.t())
                vt = pattern((D, ldvt), 6)
                want = vt.clone()
                for b in range(B):
                    want[:, b * N + ids.cuda()] = v[b * na:(b + 1) * na].t()
                ops.sparse_scatter_vt_(vt, src, dev_ids(ids, src_rows), N, batch=B, src_rows=src_rows)
                assert torch.equal(vt, want), (na, kind, B, D, src_rows)
                assert torch.equal(vt[:, B * N:], want[:, B * N:])  # the padding columns in particular


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na", NAS)
def test_unpatchify_cells_of_the_listed_tokens(na, kind):
    Cout, T = 16, frames_for(na)
    Hp, Wp = Hh // 2, Ww // 2
    N = T * Hp * Wp
    ids = make_ids(na, N, kind)
    head = rnd((na, 4 * Cout + 8), 7)[:, : 4 * Cout]  # row stride 72
    full = torch.zeros((N, 4 * Cout), dtype=BF, device="cuda:0")
    full[ids.cuda()] = head
    dense = full.view(T, Hp, Wp, 2, 2, Cout).permute(5, 0, 1, 3, 2, 4).reshape(Cout, T, Hh, Ww)  # col = (dh*2 + dw)*Cout + c
    cells = torch.zeros(N, dtype=torch.bool, device="cuda:0")
    cells[ids.cuda()] = True
    cells = cells.view(T, Hp, 1, Wp, 1).expand(T, Hp, 2, Wp, 2).reshape(1, T, Hh, Ww)
    for i64 in (False, True):
        out = pattern((Cout, T, Hh, Ww), 8)
        want = torch.where(cells, dense, out)
        ops.sparse_unpatchify_(out, head, dev_ids(ids, i64))
        assert torch.equal(out, want), (na, kind, i64)
    # all tokens listed: the dense pass
    every = torch.arange(N, dtype=torch.int32, device="cuda:0")
    y = rnd((N, 4 * Cout), 9)
    assert torch.equal(ops.sparse_unpatchify_(pattern((Cout, T, Hh, Ww), 8), y, every), ops.unpatchify(y, Cout, T, Hh, Ww))


def test_bad_arguments_are_refused():
    ids = torch.arange(8, dtype=torch.int32, device="cuda:0")
    x = rnd((36, 2, Hh, Ww), 1)
    with pytest.raises(TypeError):
        ops.sparse_patchify(x, ids.float(), 192)
    with pytest.raises(ValueError):
        ops.sparse_patchify(x, ids[::2], 192)
    with pytest.raises(ops.HipKernelError):
        ops.sparse_patchify(x, ids.cpu(), 192)
    with pytest.raises(ValueError):  # more ids than tokens
        ops.sparse_scatter_rows_(pattern((4, 256), 1), rnd((8, 256), 2), ids)
    with pytest.raises(ValueError):
        ops.sparse_scatter_vt_(pattern((256, 128), 1), rnd((256, 8), 2), ids, 4)
    with pytest.raises(ops.HipKernelError):  # a row of 4 elements is no whole 16-byte chunk
        ops.sparse_scatter_rows_(pattern((16, 4), 1), rnd((8, 4), 2), ids)
    # an id outside the grid writes nothing (the host check is the contract; the passes skip it all the same)
    dst = pattern((16, 256), 3)
    keep = dst.clone()
    bad = torch.tensor([3, 16, 99, -1], dtype=torch.int64, device="cuda:0")
    src = rnd((4, 256), 4)
    ops.sparse_scatter_rows_(dst, src, bad)
    keep[3] = src[0]
    assert torch.equal(dst, keep)
