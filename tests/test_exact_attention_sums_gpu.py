"""The sums of the bf16 self-attention kernels, element by element: tie rows and stair rows (tests/exact_util.py, `sums_case`) share every
launch and every 32-row wave group with needle rows.  A tie row's answer is the mean of its set's V rows, a stair row's is +-r / 8 per
column; both are exact in bf16 and come out exact whatever the kernel's offset schedule - so every element of every launch is compared with
`ulps=0`.  What they pin beyond the needles: the row sum l (a key dropped, doubled or a zero-padded key let in), the accumulation of P.V
over keys and tiles, rescales by factors that are neither 1 nor 0, and the key-split merge of attention_1head.  The constructions, an fp32
model of the online softmax under both offset schedules and eight deliberate mistakes are checked on the CPU (tests/test_exact_constructions.py)."""
import pytest
import torch

import exact_util as X
from exact_util import BF, assert_exact, needle_k, needle_q, seg2_keys, two_segment_q, winners_for

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 64, 8, 4], ids=["auto", "swpipe", "wg8", "wg4"])
def attn_waves(request):
    from chronoedit_amd import ops
    old = ops.set_attention_waves(request.param)
    yield request.param
    ops.set_attention_waves(old)


@pytest.fixture(params=[0, 128, 129, 16], ids=["sp-2-waves-per-simd", "w4-1-wave-per-simd", "w4-persistent", "x16"])
def vt_body(request):
    from chronoedit_amd import ops
    old = ops.set_attention_waves(request.param)
    yield request.param
    ops.set_attention_waves(old)


@pytest.fixture(params=[0, 128, 129], ids=["sp-2-waves-per-simd", "w4-1-wave-per-simd", "w4-persistent"])
def blocked_body(request):
    from chronoedit_amd import ops
    old = ops.set_attention_waves(request.param)
    yield request.param
    ops.set_attention_waves(old)


@pytest.mark.parametrize("name", ["mid-a", "mid-b", "rows-700", "one-tile", "long"])
def test_attention_sums(name, attn_waves):
    """ops.attention, B = 1 and B >= 2: the software-pipelined body (family "r") and the register-staged kernel (family "f").  The rows past
    L in the same buffers are silent keys or winner-if-read keys over POISON."""
    from chronoedit_amd import ops
    c = X.sum_named_case(name)
    L = c.B * c.n_k
    kd, vd = c.k.cuda(), c.v.cuda()
    out = ops.attention(c.q[X.SUM_FAMILY[("attention", attn_waves)]].cuda(), kd[:L], vd[:L], c.H, batch=c.B)
    assert_exact(out, c.want, f"attention sums {name} waves={attn_waves}")


@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("name", ["mid-a", "mid-b", "rows-700"])
def test_attention_two_segment_sums(name, waves):
    """The register-staged two-segment form: tie and stair rows in segment 1, a needle over integer V rows in segment 2; the output is
    bf16(bf16(o1) + V2[winner])."""
    from chronoedit_amd import ops
    c = X.sum_named_case(name)
    L2, extra = 65, 64
    g = torch.Generator().manual_seed(len(name) + c.n_k)
    q2s, k2s, o2 = [], [], []
    v2 = torch.randint(1, 16, (c.B * L2 + extra, c.H * 128), generator=g).to(BF)
    v2[c.B * L2:] = X.POISON
    for b in range(c.B):
        win = winners_for(c.n_q, L2, c.H, g, must=X.edge_keys(L2))
        q2s.append(needle_q(win, sample=b, batch=c.B))
        k2s.append(needle_k(L2, c.H, sample=b))
        o2.append(torch.cat([v2[b * L2 + win[:, h], h * 128:(h + 1) * 128] for h in range(c.H)], 1))
    k2s.append(needle_k(extra, c.H, sample=c.B - 1, invalid=torch.ones(extra, dtype=torch.bool)))
    q = two_segment_q(c.q["f"].double(), torch.cat(q2s), c.H).to(BF)
    k2 = seg2_keys(torch.cat(k2s), c.H).to(BF).cuda()
    want = (c.want.float() + torch.cat(o2).float()).to(BF)
    L = c.B * c.n_k
    kd, vd, v2d = c.k.cuda(), c.v.cuda(), v2.cuda()
    old = ops.set_attention_waves(waves)
    try:
        out = ops.attention(q.cuda(), kd[:L], vd[:L], c.H, k2=k2[:c.B * L2], v2=v2d[:c.B * L2], batch=c.B)
    finally:
        ops.set_attention_waves(old)
    assert_exact(out, want, f"attention 2-segment sums {name} waves={waves}")


@pytest.mark.parametrize("name", ["mid-a", "mid-b", "one-tile", "long"])
def test_attention_vt_sums(name, vt_body):
    """ops.attention_vt on v_transpose's V^T (its padding columns zero) under the software-pipelined body, both one-wave-per-SIMD forms and
    the diagnostic library's 16 x 16 x 32 body (key counts are multiples of 8: it takes no other column stride)."""
    from chronoedit_amd import ops
    c = X.sum_named_case(name)
    assert c.B == 1 or c.n_k % 8 == 0
    L = c.B * c.n_k
    kd = c.k.cuda()
    vt = ops.v_transpose(c.v[:L].cuda(), c.H)
    assert not vt[:, L:].any()
    out = ops.attention_vt(c.q[X.SUM_FAMILY[("attention_vt", vt_body)]].cuda(), kd[:L], vt, c.H, batch=c.B)
    assert_exact(out, c.want, f"attention_vt sums {name} body={vt_body}")


@pytest.mark.parametrize("name,n,W", [("blk-300", 128, 3), ("blk-500", 64, 8)])
def test_attention_vt_blocked_sums(name, n, W, blocked_body):
    """The all-to-all receive layout with a padded last block: the padding tokens are silent keys (blk-300) or winner-if-read keys
    (blk-500); every query row, padded ones included, has an answer."""
    from chronoedit_amd import ops
    c = X.sum_named_case(name)
    T, D, B, H, N = W * n, c.H * 128, c.B, c.H, c.n_k
    assert c.stride == T and c.n_q == T and c.extra == 0

    def blocked(t):
        return t.view(B, W, n, D).permute(1, 0, 2, 3).contiguous().view(W * B * n, D).cuda()
    vt = ops.v_transpose_blocked(blocked(c.v), H, B, n, N)
    cols = vt.shape[1] // B
    for b in range(B):
        assert not vt[:, b * cols + N:(b + 1) * cols].any()
    out = ops.attention_vt_blocked(blocked(c.q[X.SUM_FAMILY[("attention_vt_blocked", blocked_body)]]), blocked(c.k), vt, H, B, n, N)
    got = out.view(W, B, n, D).permute(1, 0, 2, 3).reshape(B * T, D)
    assert_exact(got, c.want, f"attention_vt_blocked sums {name} body={blocked_body}")


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", ["vae-1000-128", "vae-1000-384", "vae-2040-128", "vae-2040-384"])
def test_attention_1head_sums(name, split):
    """attention_1head at C = 128 and 384, one workgroup per query block and the key split (two splits at 1000 keys, four at 2040: the
    launcher's rule, restated in `sum_split_count`, on this device's compute units - another count fails here, loudly).  V^T holds its
    contract's zero padding up to 64 ceil(N / 64) columns and POISON behind; the K rows past Nk are silent or win if read."""
    from chronoedit_amd import ops
    c = X.sum_named_case(name)
    N, C = c.n_k, c.C
    if split:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        got = X.sum_split_count(c.n_q, N, C, cus, 4 * c.n_q * (C + 2))
        assert got == c.nsplit, f"{name}: {got} key splits on {cus} compute units, the case was built for {c.nsplit}"
    cols = (N + 63) // 64 * 64
    vt = torch.full((C, cols + 64), X.POISON, dtype=BF)
    vt[:, :cols] = 0
    vt[:, :N] = c.v[:N].t()
    kd = c.k.cuda()
    out = ops.attention_1head(c.q[X.SUM_FAMILY[("attention_1head", 0)]].cuda(), kd[:N], vt.cuda(), C ** -0.5, split_keys=split)
    assert_exact(out, c.want, f"attention_1head sums {name} split={split}")


@pytest.mark.parametrize("waves", [0, 128], ids=["sp-2-waves-per-simd", "w4-1-wave-per-simd"])
def test_both_softmax_routes_are_walked(waves):
    """Launches without needle rows through the diagnostic library: the jump stair sends its waves through the exact route at the jump
    tile, the rising stair never does - the jump case reports strictly more exact-route hits (what the two share are the tie rows whose
    first set member lies past tile 0)."""
    from chronoedit_amd import ops
    hits = {}
    old, forced = ops.set_attention_waves(waves), ops._force_diag
    ops.force_diagnostics(True)
    try:
        for name in ("route-rising", "route-jump"):
            c = X.sum_named_case(name)
            L = c.B * c.n_k
            kd = c.k.cuda()
            vt = ops.v_transpose(c.v[:L].cuda(), c.H)
            ops.attention_exact_route_hits(reset=True)
            out = ops.attention_vt(c.q["r"].cuda(), kd[:L], vt, c.H, batch=c.B)
            hits[name] = ops.attention_exact_route_hits(reset=True)[0]
            assert_exact(out, c.want, f"attention_vt sums {name} body={waves}")
    finally:
        ops.force_diagnostics(forced)
        ops.set_attention_waves(old)
    print(f"exact-route hits, body {waves}: rising {hits['route-rising']}, jump {hits['route-jump']}")
    assert hits["route-jump"] > hits["route-rising"], hits
