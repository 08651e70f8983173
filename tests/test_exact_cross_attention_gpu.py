"""The cross-attention family element by element: ce_attention_2seg_vt_bf16, _strided_bf16 (shared operands), _weighted_bf16 (segment 1 cut
per sample, its last key weighted) and _quant_bf16 (MX fp8 output) against answers that are known exactly (tests/exact_util.py, "cross-attention";
the constructions are proved on the CPU in tests/test_exact_constructions.py).  Every comparison is `assert_exact(..., ulps=0)`.

  * Needle rows: one winner per row, head and segment, ahead by >= 22 nats with the weight counted in; the output is
    bf16(bf16(V1[winner 1]) + bf16(V2[winner 2])).  Every sample's keys sit in a row order of their own, V^T samples stand at the engine's
    column stride 8 ceil(len / 8) - the tail of a sample's last 64-key tile is the NEXT sample's columns (K: the next sample's rows) - and
    whatever a kernel must not read (rows past a sample's cut, the neighbours, rows and columns behind the last sample) wins if read and
    brings POISON.  They pin masking, the per-sample cut, strides and positions - never the weight.
  * Flat rows pin the weight: every readable key of segment 1 scores exactly 0, the last counts m = 2^w times and valid - 1 + m = 2^k, V1 has one
    nonzero per column: the output is +-r mult / 8 (+ an integer from segment 2), whatever the route through the online softmax.
  * More (sample, head, query block) items than the launcher's 2 x #CUs workgroups: the persistent loop derives sample, head, block, the cut,
    the weight and every stride again per item.

Routes: the diagnostic build's counter (ops.attention_exact_route_hits) is available to the tests;
test_attention_2seg_vt_weighted_route_of_each_flat_pair asserts it on rows that are all flat.  Observed on an MI355X: 0 hits past tile 0 for
every pair with m <= 1024 (the weighted tile stays speculative, P = m), and 6 hits = 3 waves with rows x 2 heads for (2049, 2048) - it does
take the exact route, once per wave, where the weight is applied a second time and the earlier tiles are rescaled by 2^-11.

What the needle rows found: with every sample's keys in a row order of its own, a row's near keys need not sit in key tile 0.  Where the whole
first tile lay more than 128 octaves below 0, `alpha = exp2(-row maximum)` of the first tile was +inf and 0 * inf made the row NaN (23 to
256 (row, head) pairs per launch in three of the four stacked shapes).  Fixed in ce_attn.hip (alpha = 1 at t == 0, both bodies);
test_attention_2seg_vt_first_tile_far_below_the_winner and two tests in tests/test_exact_attention_gpu.py pin it by design.

`valid1` together with `out8` is refused inside the common launcher, but no exported entry point takes both, so that rejection cannot be
asked for.  Operands stand in roomy buffers (exact_util.roomy_cross_case): a wrong sample stride reads rows and columns the test owns.

Run time on an MI355X: 48 tests, 5.3 s for the file including the imports, 3.4 s in the tests (the previous exact-test batch: 3.3 s); the
largest, 0.6 s, is the first to touch the GPU.

Mutants: each one-line change applied to a scratch copy of ce_attn.hip, the product library rebuilt from it, this file (48 tests) and the
kernel-level tests of tests/test_text_compaction_gpu.py and tests/test_shared_guidance_gpu.py (17) run against it:

    mutant                                              new tests failing   older tests failing
    weigh_last uses sg.len - 2                                 14                  7
    w_last = blk.w0[0]                                         12                  7
    valid0[0] in place of valid0[bz]                           21                  8
    second weigh_last() (exact route) removed                  12                  0   (not caught before)
    Q += bz * Nq * ldq, ignoring q_rows                         8                  9
    seg1.v += bz * 64 ceil(len / 64), not blk.stride           44                  4
    the cut hoisted out of the item loop                        2                  0   (not caught before; the two weighted
                                                                                        more-items-than-workgroups cases)
    first-tile alpha = exp2(-shift) again, sp body              3 first-tile tests fail (attention[auto], attention_vt[sp-2-waves-per-simd], this file's)
    the same in the one-wave-per-SIMD body (the diagnostic      2 fail: attention_vt first-tile [w4-1-wave-per-simd] and [w4-persistent]
    library rebuilt from it: the selectable bodies live there)
"""

import pytest
import torch

import exact_util as X
from exact_util import BF, MIN_MARGIN_NATS, assert_exact
from test_mxfp8_gemm_gpu import _contract

pytestmark = pytest.mark.gpu
SENTINEL = 7.0


_n_flat, _case, MANY_PAIRS = X.n_flat_rows, X.roomy_cross_case, X.MANY_PAIRS


def _checked(c, margins=True):
    """The construction's own premises (the big cases: tests/test_exact_constructions.py)."""
    if margins:
        lead, forb, flat = X.cross_margins(c)
        assert min(lead, forb, flat) >= MIN_MARGIN_NATS, (lead, forb, flat)
    assert c.flat_exact
    return c


def _launch(c, entry, valid1=None, q=None, k1=None, v1t=None, k2=None, v2t=None, out=None):
    """One launch of `entry` ("plain", "shared", "weighted") on the operands of `c` (any of them replaced by a device view of the same
    values); the output rows, taken from a taller buffer whose rows past B n_q must come back untouched."""
    from chronoedit_amd import ops
    B, H, nq, D = c.B, c.H, c.n_q, c.H * 128
    q = c.q.cuda()[:(1 if c.share_q else B) * nq] if q is None else q    # (a view: under share_q other queries stand behind it)
    k1 = c.k1.cuda()[:(1 if c.share1 else B) * c.len1] if k1 is None else k1    # (a view: the rows behind it win if read)
    k2 = c.k2.cuda()[:(1 if c.share2 else B) * c.len2] if k2 is None else k2
    v1t = c.v1t.cuda() if v1t is None else v1t
    v2t = c.v2t.cuda() if v2t is None else v2t
    tall = None
    if out is None:
        tall = torch.full((B * nq + 8, D), SENTINEL, dtype=BF, device="cuda")
        out = tall[:B * nq]
    c1, c2 = (None if c.share1 else c.c1), (None if c.share2 else c.c2)
    if entry == "plain":
        assert not (c.share_q or c.share1 or c.share2)
        ops.attention_2seg_vt(q, k1, v1t, c.len1, k2, v2t, c.len2, H, out=out, batch=B, cols1=c1, cols2=c2)
    elif entry == "shared":
        ops.attention_2seg_vt_shared(q, k1, v1t, c.len1, k2, v2t, c.len2, H, out=out, batch=B, share_q=c.share_q, share1=c.share1,
                                     share2=c.share2, cols1=c1, cols2=c2)
    else:
        valid = torch.tensor(c.valid if valid1 is None else valid1, dtype=torch.int32, device="cuda")
        w = torch.tensor(c.w, dtype=torch.float32, device="cuda")
        ops.attention_2seg_vt_weighted(q, k1, v1t, c.len1, k2, v2t, c.len2, H, out=out, batch=B, valid1=valid, w1=w, share_q=c.share_q,
                                       share2=c.share2, cols1=c1, cols2=c2)
    if tall is not None:
        assert bool((tall[B * nq:] == SENTINEL).all()), "rows behind the last sample's output were written"
    return out


# ---- ce_attention_2seg_vt_bf16 -----------------------------------------------------------------------------------------------------
PLAIN_SHAPES = [(300, 100, 65, 3, 3), (513, 257, 64, 2, 1), (290, 512, 257, 8, 2), (7200, 512, 257, 2, 2)]


@pytest.mark.parametrize("n_q,L1,L2,H,B", PLAIN_SHAPES)
def test_attention_2seg_vt_needles(n_q, L1, L2, H, B):
    c = _checked(_case(n_q, L1, L2, H, B, seed=n_q + L1 + L2), margins=n_q < 7200)
    assert c.c1 % 64 or c.c2 % 64
    assert_exact(_launch(c, "plain"), c.want, f"attention_2seg_vt needles {n_q}x({L1}+{L2}) H={H} B={B}")


def test_attention_2seg_vt_needles_on_strided_operands():
    """Q a column slice of a wider buffer (its other columns POISON), K1 and the rows V1^T is made of the two halves of one fused
    [rows, 2 D] buffer, V2^T a column slice of a wider one, out a column slice of a wider and taller buffer filled with 7.0."""
    from chronoedit_amd import ops
    n_q, L1, L2, H, B = 300, 100, 65, 3, 3
    D = H * 128
    c = _checked(_case(n_q, L1, L2, H, B, seed=11))
    qw = torch.full((B * n_q, D + 256), X.POISON, dtype=BF, device="cuda")
    qw[:, 128:128 + D] = c.q.cuda()
    fused = torch.full((c.k1.shape[0], 2 * D), X.POISON, dtype=BF, device="cuda")
    fused[:, :D] = c.k1.cuda()
    v1t = c.v1t.cuda()
    v1t_f = torch.full_like(v1t, X.POISON)
    for b in range(B):  # V1 rows into the fused buffer's other half; V1^T by the project's transpose kernel from that strided source
        fused[b * L1:(b + 1) * L1, D:] = v1t[:, b * c.c1:b * c.c1 + L1].t()
        v1t_f[:, b * c.c1:b * c.c1 + L1] = ops.v_transpose(fused[b * L1:(b + 1) * L1, D:], H)[:, :L1]
    assert torch.equal(v1t_f, v1t)
    v2w = torch.full((D, c.v2t.shape[1] + 48), X.POISON, dtype=BF, device="cuda")
    v2w[:, 16:16 + c.v2t.shape[1]] = c.v2t.cuda()
    ow = torch.full((B * n_q + 40, D + 256), SENTINEL, dtype=BF, device="cuda")
    out = _launch(c, "plain", q=qw[:, 128:128 + D], k1=fused[:B * L1, :D], v1t=v1t_f, v2t=v2w[:, 16:16 + c.v2t.shape[1]],
                  out=ow[:B * n_q, 128:128 + D])
    assert_exact(out, c.want, "attention_2seg_vt needles, strided operands")
    ow[:B * n_q, 128:128 + D] = SENTINEL
    assert bool((ow == SENTINEL).all()), "the output buffer's other columns or rows were written"


def test_attention_2seg_vt_first_tile_far_below_the_winner():
    """Segment 1's first key tile thousands of octaves below every row's winner (tests/exact_util.py `far_first_tile`): exp2(-first tile's
    maximum) is +inf, and the first tile has nothing to rescale.  Before `alpha = 1 at t == 0` in ce_attn.hip the body multiplied l = 0 and
    O = 0 by it and returned NaN rows; the per-sample row orders of the needle cases above met the same bug by chance, this case by design."""
    from chronoedit_amd import ops
    H, n_q, L1, L2 = 3, 70, 130, 64
    g = torch.Generator().manual_seed(5)
    q1, k1, v1, rows1 = X.far_first_tile(n_q, L1, H, g)
    rows2 = X.winners_for(n_q, L2, H, g, must=X.edge_keys(L2))
    q = X.two_segment_q(q1.double(), X.needle_q(rows2), H).to(BF)
    k2 = X.seg2_keys(X.needle_k(L2, H), H).to(BF)
    v1, v2 = v1.abs(), X.needle_v(L2, H * 128, g, positive=True)
    lead1, _ = X.needle_margins(q, k1, H, rows1)
    lead2, _ = X.needle_margins(q, k2, H, rows2)
    assert min(lead1.min(), lead2.min()) >= MIN_MARGIN_NATS
    vt = lambda v, n: torch.cat([v.t(), torch.full((H * 128, X.pad64(n) - n), X.POISON, dtype=BF)], 1).contiguous().cuda()
    want = (X._gather_rows(v1, rows1, H).float() + X._gather_rows(v2, rows2, H).float()).to(BF)
    out = ops.attention_2seg_vt(q.cuda(), k1.cuda(), vt(v1, L1), L1, k2.cuda(), vt(v2, L2), L2, H, cols1=X.pad64(L1), cols2=X.pad64(L2))
    assert_exact(out, want, "attention_2seg_vt, first tile far below the winner")


# ---- ce_attention_2seg_vt_strided_bf16 ---------------------------------------------------------------------------------------------
SHARE8 = [(sq, s1, s2) for sq in (False, True) for s1 in (False, True) for s2 in (False, True)]
SHARE4 = [(True, False, True), (False, False, True), (True, True, True), (False, True, False)]  # (tests/test_shared_guidance_gpu.py's)


@pytest.mark.parametrize("H,share", [(5, s) for s in SHARE8] + [(8, s) for s in SHARE4])
def test_attention_2seg_vt_shared_needles(H, share):
    n_q, L1, L2, B = 300, 100, 65, 3
    sq, s1, s2 = share
    c = _checked(_case(n_q, L1, L2, H, B, seed=100 + H + 4 * sq + 2 * s1 + s2, share_q=sq, share1=s1, share2=s2))
    rows = c.want.view(B, n_q, -1)
    for a, b in ((0, 1), (1, 2), (0, 2)):  # each sample has its own answer - unless every operand is shared
        assert torch.equal(rows[a], rows[b]) == (sq and s1 and s2)
    assert_exact(_launch(c, "shared"), c.want, f"attention_2seg_vt_shared needles H={H} share_q={sq} share1={s1} share2={s2}")


# ---- ce_attention_2seg_vt_weighted_bf16 --------------------------------------------------------------------------------------------
# (len1, valid per sample, m per sample | None, w per sample | None): needle rows only where valid - 1 + 2^w is no power of two
WEIGHTED_SETS = [
    (72, (1, 63, 64), None, (9.0, 5.5, 0.0)),
    (136, (65, 129, 70), None, (9.0, 0.0, 3.25)),
    (200, (200, 1, 199), None, (0.0, 9.0, 7.0)),
    (64, (1, 33, 57), (64, 32, 8), None),          # the weighted key is the only key / in tile 0 as the row maximum
    (72, (63, 64, 65), (2, 1, 64), None),          # ... / w = 0 on a full first tile / alone in tile 1: speculative, P = 64
    (200, (97, 127, 193), (32, 2, 64), None),      # mid tile 1, speculative / the reference's 512-key total
    (2056, (257, 449, 2049), (256, 64, 2048), None),  # 512-key totals / P = 2^11 > SP_SPEC_THR: the exact route past the first tile
]


@pytest.mark.parametrize("H", [8, 5])
@pytest.mark.parametrize("len1,valid,m,w", WEIGHTED_SETS, ids=[f"valid{'-'.join(map(str, s[1]))}" for s in WEIGHTED_SETS])
def test_attention_2seg_vt_weighted_needles_and_flat_rows(len1, valid, m, w, H):
    n_q, L2, B = 300, 65 if H == 8 else 257, 3
    c = _checked(_case(n_q, len1, L2, H, B, seed=len1 + H + sum(valid), valid=valid, w=w, m=m, n_flat=_n_flat(n_q) if m else 0))
    assert_exact(_launch(c, "weighted"), c.want, f"attention_2seg_vt_weighted len1={len1} valid={valid} m={m} w={w} H={H}")


@pytest.mark.parametrize("share_q", [False, True])
@pytest.mark.parametrize("share2", [False, True])
def test_attention_2seg_vt_weighted_shared_operands(share_q, share2):
    """One image segment for all samples cannot carry a scale per sample: under share2 the samples differ in `valid` only."""
    n_q, L1, L2, H, B = 300, 200, 65, 5, 3
    valid, m = ((65, 193, 1), (64, 64, 64)) if share2 else ((97, 127, 193), (32, 2, 64))
    c = _checked(_case(n_q, L1, L2, H, B, seed=7 + 2 * share_q + share2, share_q=share_q, share2=share2, valid=valid, m=m,
                              n_flat=_n_flat(n_q)))
    assert_exact(_launch(c, "weighted"), c.want, f"attention_2seg_vt_weighted share_q={share_q} share2={share2}")


def test_attention_2seg_vt_weighted_without_cut_or_weight_is_the_strided_entry():
    n_q, L1, L2, H, B = 300, 100, 65, 5, 3
    c = _checked(_case(n_q, L1, L2, H, B, seed=3, valid=(L1,) * B, w=(0.0,) * B))
    got = _launch(c, "weighted")
    assert_exact(got, c.want, "weighted entry, valid == len1 and w == 0")
    assert torch.equal(got, _launch(c, "shared"))


def test_attention_2seg_vt_weighted_clamps_valid_into_1_len1():
    """The contract is 1 <= valid1[b] <= len1; the kernel clamps: 0 behaves as 1, len1 + 5 as len1 (include/chronoedit_hip.h)."""
    n_q, L1, L2, H, B = 300, 100, 65, 5, 3
    c = _checked(_case(n_q, L1, L2, H, B, seed=4, valid=(1, L1, 70), w=(3.0, 2.0, 9.0)))
    assert_exact(_launch(c, "weighted", valid1=(0, L1 + 5, 70)), c.want, "weighted entry, valid = (0, len1 + 5, 70)")


def test_attention_2seg_vt_weighted_route_of_each_flat_pair():
    """Which route the weighted tile takes, counted by the diagnostic build (waves x key tiles on the exact route past tile 0): rows that are
    all flat, one key tile in segment 2.  m <= 1024 stays speculative - P = m - and (2049, 2048) goes through the exact route, once per wave
    with rows, where the weight is applied a second time and the earlier tiles are rescaled by 2^-11."""
    from chronoedit_amd import ops
    n_q, L2, H = 70, 64, 2
    waves = (n_q + 31) // 32
    forced = ops._force_diag
    ops.force_diagnostics(True)
    try:
        for len1, valid, m, hits in ((456, (65, 193, 449), (64, 64, 64), 0), (456, (97, 257, 127), (32, 256, 2), 0),
                                     (2056, (2049, 449), (2048, 64), waves * H)):
            c = _checked(_case(n_q, len1, L2, H, len(valid), seed=len1 + sum(m), valid=valid, m=m, n_flat=n_q))
            ops.attention_exact_route_hits(reset=True)
            got = _launch(c, "weighted")
            torch.cuda.synchronize()
            assert ops.attention_exact_route_hits(reset=True)[0] == hits, (valid, m)
            assert_exact(got, c.want, f"all-flat rows valid={valid} m={m}")
    finally:
        ops.force_diagnostics(forced)


# ---- more items than workgroups ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["plain", "shared", "weighted"])
@pytest.mark.parametrize("n_q,H,B", [(300, 40, 7), (2600, 5, 10)])
def test_more_items_than_workgroups(n_q, H, B, entry):
    L1, L2 = 200, 65
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (n_q + 255) // 256 * H * B > 2 * cus, "every workgroup has one item at most on this device: the case checks nothing"
    kw = {}
    if entry == "shared":
        kw = dict(share2=True)
    elif entry == "weighted":
        kw = dict(valid=[p[0] for p in MANY_PAIRS[:B]], m=[p[1] for p in MANY_PAIRS[:B]], n_flat=_n_flat(n_q))
    c = _checked(_case(n_q, L1, L2, H, B, seed=n_q + H + len(entry), **kw), margins=False)
    assert_exact(_launch(c, entry), c.want, f"{entry} entry, {(n_q + 255) // 256 * H * B} items on {cus} CUs")


# ---- ce_attention_2seg_vt_quant_bf16 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q,L1,L2,H,B", [PLAIN_SHAPES[0], PLAIN_SHAPES[2]])
def test_attention_2seg_vt_quantised_output_is_the_contract_of_the_known_answer(n_q, L1, L2, H, B):
    from chronoedit_amd import ops
    D, M = H * 128, B * n_q
    c = _checked(_case(n_q, L1, L2, H, B, seed=n_q + L1 + L2))
    Mp = (M + 127) // 128 * 128
    o8 = torch.full((M + 40, D), 0xA5, dtype=torch.uint8, device="cuda")
    s8 = torch.full((ops.mx_scale_bytes(M, D) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    ops.attention_2seg_vt(c.q.cuda(), c.k1.cuda()[:B * L1], c.v1t.cuda(), L1, c.k2.cuda()[:B * L2], c.v2t.cuda(), L2, H, batch=B,
                          cols1=c.c1, cols2=c.c2, out8=o8[:M], scale8=s8)
    want_s, want_q = _contract(c.want)
    assert_exact(o8[:M].cpu(), want_q, "e4m3 bytes")
    rows = ops.mx_scales_to_rows(s8[:ops.mx_scale_bytes(M, D)], Mp, D).cpu()
    assert_exact(rows[:M], want_s, "E8M0 bytes")
    assert bool((o8[M:] == 0xA5).all()) and bool((rows[M:] == 0xA5).all()) and bool((s8[ops.mx_scale_bytes(M, D):] == 0xA5).all())


# ---- the launcher's rejections -------------------------------------------------------------------------------------------------------
def test_launcher_rejections_leave_the_output_untouched():
    """(`valid1` together with `out8` is refused inside the common launcher, but no exported entry point takes both: it cannot be asked for.)"""
    from chronoedit_amd import ops
    L, Nq, H, B, D = 40, 64, 2, 2, 256
    z = torch.zeros(B * L, D, dtype=BF, device="cuda")
    q = torch.zeros(B * Nq, D, dtype=BF, device="cuda")
    vt = torch.zeros(D, 128, dtype=BF, device="cuda")
    o = torch.full((B * Nq, D), SENTINEL, dtype=BF, device="cuda")
    va, wa = torch.tensor([32, 1], dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    lib = ops.lib()

    def weighted(cols=40, ldv=128, v=ops._ptr(va), w=ops._ptr(wa)):
        return lib.ce_attention_2seg_vt_weighted_bf16(ops._ptr(q), ops._ptr(z), ops._ptr(vt), L, D, ldv, cols, ops._ptr(z), ops._ptr(vt), L, D, 128, 40,
                                                      ops._ptr(o), Nq, H, 128, D, D, 0.1, B, Nq, L, L, v, w, ops._stream())

    def plain(cols=40, ldv=128):
        return lib.ce_attention_2seg_vt_bf16(ops._ptr(q), ops._ptr(z), ops._ptr(vt), L, D, ldv, cols, ops._ptr(z), ops._ptr(vt), L, D, 128, 40,
                                             ops._ptr(o), Nq, H, 128, D, D, 0.1, B, ops._stream())

    assert weighted(w=None) == -1                         # valid1 without w1
    assert weighted(cols=41) == -3 and plain(cols=41) == -3  # an odd column stride
    assert (B - 1) * 40 + 64 == 104
    assert weighted(ldv=103) == -2 and plain(ldv=103) == -2  # a V^T row one short of (batch - 1) cols + 64 ceil(len / 64)
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())
    assert weighted() == 0 and plain(ldv=104) == 0        # (the same arguments, valid: launched)
    torch.cuda.synchronize()
    assert not bool((o == SENTINEL).any())
