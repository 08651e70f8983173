"""ce_lora_merge_bf16 element by element, exactly (in the style of tests/exact_util.py).

The contract: W[n,k] = bf16_rne( fp32(W0[n,k]) + sum_i scales[i] * dot_i[n,k] ), dot_i the fp32-accumulated rank product of adapter i.

Data: W0 = integers in [-8, 8] times 2^e per row, e in [-2, 2]; B = integers in [-3, 3] times 2^e per row, e in [-1, 1]; A = integers in
[-3, 3] times 2^-1; scales = signed powers of two in [2^-2, 2].  Every product B*A is a multiple of 2^-2 below 2^5, every partial sum of a rank
product in ANY order a multiple of 2^-2 below 512 * 9 < 2^13 (15 bits), every scaled term a multiple of 2^-4 below 2^14 and the sum of W0 and up
to three terms a multiple of 2^-4 below 2^16 (20 bits): all of it is exact in fp32, whatever the tile shape, chunking or order, so the kernel's
result must equal the fp32 torch evaluation of the contract rounded once to bf16 - bit for bit.  The premise is asserted on the CPU first (the
fp64 and fp32 evaluations agree exactly).  A few rows are built to land exactly half way between two bf16 values (256 + 1, 258 + 1 and their
negatives, where the bf16 spacing is 2): they pin round-to-nearest-EVEN (256, 260)."""
import pytest
import torch

import exact_util as X

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TIE_ROWS = (1, 130)  # one in the first 128-row tile, one in the next (or the ragged last) tile


def _case(N, K, ranks, scales, seed):
    g = torch.Generator().manual_seed(seed)
    w0 = X.int_rows(N, K, g, lo=-8, hi=8, emin=-2, emax=2)
    adapters = []
    for r, s in zip(ranks, scales):
        b = X.int_rows(N, r, g, lo=-3, hi=3, emin=-1, emax=1)
        a = X.int_rows(r, K, g, lo=-3, hi=3, emin=-1, emax=-1)
        adapters.append([a, b, float(s)])
    if adapters:
        # the tie rows: W0 = +-256 / +-258 by column and delta = +-1 exactly, from adapter 0 alone - A0[0, k] = the column's sign, the row of
        # B0 = 1 / s0 at rank 0 and zero elsewhere, the rows of the other adapters' B zero (all of it inside the value ranges above)
        rows = [r for r in TIE_ROWS if r < N]
        pat = torch.tensor([256.0, 258.0, -256.0, -258.0]).repeat(K // 4).to(BF)
        adapters[0][0][0, :] = torch.tensor([1.0, 1.0, -1.0, -1.0]).repeat(K // 4).to(BF)
        for a, b, s in adapters:
            b[rows, :] = 0.0
        for r in rows:
            w0[r] = pat
            adapters[0][1][r, 0] = 1.0 / adapters[0][2]
    return w0, [tuple(t) for t in adapters]


def _expected(w0, adapters):
    """The contract in fp32 torch arithmetic on the CPU (and the same in fp64: the premise is that both are exact), rounded once."""
    acc32, acc64 = w0.float(), w0.double()
    for a, b, s in adapters:
        acc32 = acc32 + s * (b.float() @ a.float())
        acc64 = acc64 + s * (b.double() @ a.double())
    assert torch.equal(acc32.double(), acc64), "exactness premise broken: the fp32 and fp64 evaluations of the contract differ"
    return acc32, acc32.to(BF)


def _assert_ties(w0, acc32, want, adapters):
    if not adapters:
        return
    for r in TIE_ROWS:
        if r >= w0.shape[0]:
            continue
        assert torch.equal(acc32[r].abs() % 2, torch.ones_like(acc32[r])), "tie rows must sit on odd integers in [257, 259]"
        assert set(want[r].float().abs().tolist()) == {256.0, 260.0}  # 257 -> 256, 259 -> 260: nearest EVEN, not away from zero


CASES = [
    # (N, K, ranks, scales)
    (264, 320, [], []),                               # n_adapters == 0: a copy
    (264, 320, [32], [1.0]),                          # odd tiles: 2 full + 8 rows, 2 full + 64 columns
    (264, 320, [96, 32], [0.5, -2.0]),
    (264, 320, [512, 16, 96], [1.0, -0.5, 0.25]),     # rank 16 is zero-padded to 32 by the host wrapper
    (5120, 5120, [32, 96], [2.0, 0.25]),              # the attention projections
    (5120, 5120, [512], [-1.0]),
    (13824, 5120, [32], [0.5]),                       # FFN up
    (5120, 13824, [96, 32, 32], [1.0, 1.0, -0.25]),   # FFN down
]


@pytest.mark.parametrize("N,K,ranks,scales", CASES, ids=[f"{n}x{k}_r{'+'.join(map(str, r)) or '0'}" for n, k, r, _ in CASES])
def test_merge_is_exact(N, K, ranks, scales):
    from chronoedit_amd import ops
    w0, adapters = _case(N, K, ranks, scales, seed=N + K + sum(ranks))
    acc32, want = _expected(w0, adapters)
    _assert_ties(w0, acc32, want, adapters)
    dev = "cuda:0"
    w0d = w0.to(dev)
    ad = [(a.to(dev), b.to(dev), s) for a, b, s in adapters]
    out = torch.full((N, K), float("nan"), dtype=BF, device=dev)
    assert ops.lora_merge(w0d, ad, out=out) is out
    X.assert_exact(out, want, f"lora_merge {N}x{K} ranks {ranks}")
    assert torch.equal(w0d.cpu(), w0), "the base must not be written"
    # W aliasing W0
    alias = w0d.clone()
    ops.lora_merge(alias, ad, out=alias)
    X.assert_exact(alias, want, f"lora_merge in place {N}x{K} ranks {ranks}")
    # a destination that is a row view of a taller buffer (the fused q|k|v case): the rows around it stay as they were
    tall = torch.full((N + 24, K), 7.0, dtype=BF, device=dev)
    ops.lora_merge(w0d, ad, out=tall[8:8 + N])
    X.assert_exact(tall[8:8 + N], want, f"lora_merge into a row view {N}x{K} ranks {ranks}")
    assert bool((tall[:8] == 7.0).all()) and bool((tall[8 + N:] == 7.0).all())
    # ... and a base that is such a view
    tall0 = torch.zeros((N + 16, K), dtype=BF, device=dev)
    tall0[16:] = w0d
    X.assert_exact(ops.lora_merge(tall0[16:], ad), want, f"lora_merge from a row view {N}x{K} ranks {ranks}")


def test_merge_rejects_bad_arguments():
    """Bad shapes and arguments come back as the library's error codes (raised by the wrapper), nothing is launched."""
    from chronoedit_amd import ops
    dev = "cuda:0"
    z = lambda *s: torch.zeros(s, dtype=BF, device=dev)
    with pytest.raises(ops.HipKernelError, match="unsupported shape"):
        ops.lora_merge(z(264, 96), [(z(32, 96), z(264, 32), 1.0)])           # K % 64
    with pytest.raises(ops.HipKernelError, match="unsupported shape"):
        ops.lora_merge(z(260, 128), [(z(32, 128), z(260, 32), 1.0)])         # N % 8
    with pytest.raises(ValueError, match="rank"):
        ops.lora_merge(z(64, 128), [(z(544, 128), z(64, 544), 1.0)])         # rank > 512
    with pytest.raises(ValueError, match="adapter 0"):
        ops.lora_merge(z(64, 128), [(z(32, 64), z(64, 32), 1.0)])            # A does not match K
    with pytest.raises(TypeError):
        ops.lora_merge(z(64, 128), [(z(32, 128).float(), z(64, 32), 1.0)])
    with pytest.raises(ops.HipKernelError, match="GPU"):
        ops.lora_merge(z(64, 128).cpu(), [])
    with pytest.raises(ValueError, match="contiguous rows"):
        ops.lora_merge(z(128, 64).t(), [])
    lib = ops.lib()
    import ctypes
    w = z(64, 128)
    none = ctypes.c_void_p(0)
    assert lib.ce_lora_merge_bf16(none, 128, ctypes.c_void_p(w.data_ptr()), 128, 64, 128, 0, none, none, none, none, none) == -1
    assert lib.ce_lora_merge_bf16(ctypes.c_void_p(w.data_ptr()), 128, ctypes.c_void_p(w.data_ptr()), 128, 64, 128, 9, none, none, none, none, none) == -1
    assert lib.ce_lora_merge_bf16(ctypes.c_void_p(w.data_ptr()), 132, ctypes.c_void_p(w.data_ptr()), 128, 64, 128, 0, none, none, none, none, none) == -3
    assert lib.ce_lora_merge_bf16(ctypes.c_void_p(w.data_ptr()), 64, ctypes.c_void_p(w.data_ptr()), 128, 64, 128, 0, none, none, none, none, none) == -1
