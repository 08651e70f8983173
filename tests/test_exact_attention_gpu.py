"""Attention kernels element by element: needle inputs (tests/exact_util.py) give every query row one winning key per head, chosen by the
test, ahead of every other key by >= 22 nats after the scale, so the output row is V[winner] - exactly: every |V| is in [1, 2), and
the other keys' weights (< e^-22 each) move it by far less than half a bf16 ulp (measured: bit-exact for every form) - no reference SDPA.  Winners cover keys 0 and n - 1, 63 / 64 / 127 / 128, every key of the ragged last tile, a different permutation per head, and
queries in the last, partial query block.  Every key a kernel must not read (rows past the length in a larger buffer, the blocked
layout's padding tokens, the neighbouring samples of a stacked batch) wins outright if it is read, and its V holds a large poison value
- or the zero padding a layout's contract requires.  Needle rows push the online-softmax offset off the speculative route; the
worst-block checks at the end cover that route on smooth random data, per (sample, head, 64-query block)."""
import pytest
import torch

from exact_util import (BF, MIN_MARGIN_NATS, POISON, assert_exact, edge_keys, far_first_tile, needle_k, needle_margins, needle_q, needle_v, seg2_keys,
                        two_segment_q, winners_for)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 64, 8, 4], ids=["auto", "swpipe", "wg8", "wg4"])
def attn_waves(request):
    from chronoedit_amd import ops
    old = ops.set_attention_waves(request.param)
    yield request.param
    ops.set_attention_waves(old)


@pytest.fixture(params=[0, 128, 129], ids=["sp-2-waves-per-simd", "w4-1-wave-per-simd", "w4-persistent"])
def vt_body(request):
    from chronoedit_amd import ops
    old = ops.set_attention_waves(request.param)
    yield request.param
    ops.set_attention_waves(old)


def _stacked(B, n_q, n_k, H, seed, extra_keys=0, positive=False):
    """Needle operands of B stacked samples (CPU): q [B n_q, D], k / v [B n_k + extra_keys, D] (the extra rows: winner-if-read keys
    past the last sample, V = POISON), winners [B, n_q, H]."""
    g = torch.Generator().manual_seed(seed)
    D = H * 128
    qs, ks, vs, ws = [], [], [], []
    for b in range(B):
        win = winners_for(n_q, n_k, H, g, must=edge_keys(n_k))
        qs.append(needle_q(win, sample=b, batch=B))
        ks.append(needle_k(n_k, H, sample=b))
        v = needle_v(n_k, D, g)
        vs.append(v.abs() if positive else v)
        ws.append(win)
    if extra_keys:
        ks.append(needle_k(extra_keys, H, sample=B - 1, invalid=torch.ones(extra_keys, dtype=torch.bool)))
        vs.append(torch.full((extra_keys, D), POISON, dtype=BF))
    q, k, v = torch.cat(qs).to(BF), torch.cat(ks).to(BF), torch.cat(vs)
    for b in range(B if B * n_q * k.shape[0] <= 2 ** 23 else 0):  # the construction itself (tests/test_exact_constructions.py for the big ones)
        forb = torch.ones(k.shape[0], dtype=torch.bool)
        forb[b * n_k:(b + 1) * n_k] = False
        lead, fl = needle_margins(q[b * n_q:(b + 1) * n_q], k, H, ws[b] + b * n_k, forb)
        assert lead.min() >= MIN_MARGIN_NATS and fl.min() >= MIN_MARGIN_NATS, (lead.min(), fl.min())
    return q, k, v, torch.stack(ws)


def _expected(v, winners, n_k, H):
    """out[b n_q + i, h*128:(h+1)*128] = v[b n_k + winners[b, i, h], h*128:(h+1)*128]."""
    B, n_q, _ = winners.shape
    D = H * 128
    out = torch.empty(B * n_q, D, dtype=v.dtype)
    for b in range(B):
        for h in range(H):
            out[b * n_q:(b + 1) * n_q, h * 128:(h + 1) * 128] = v[b * n_k + winners[b, :, h], h * 128:(h + 1) * 128]
    return out


# (n_q, n_k, H, B): the step's 7200 tokens, ragged key / query counts, B >= 3 for the neighbour leaks
ATTN_SHAPES = [(7200, 7200, 2, 1), (333, 257, 3, 3), (1000, 1090, 8, 2), (64, 64, 2, 1), (290, 64, 5, 3), (31, 700, 4, 2)]


@pytest.mark.parametrize("n_q,n_k,H,B", ATTN_SHAPES)
def test_attention_needles(n_q, n_k, H, B, attn_waves):
    from chronoedit_amd import ops
    q, k, v, win = _stacked(B, n_q, n_k, H, seed=n_q + n_k + B, extra_keys=64)
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    L = B * n_k  # rows past L in the same buffers: winner-if-read keys with poison values
    out = ops.attention(qd, kd[:L], vd[:L], H, batch=B)
    assert_exact(out, _expected(v, win, n_k, H), f"attention needles {n_q}x{n_k} H={H} B={B}")


@pytest.mark.parametrize("n_q,L1,L2,H,B", [(7200, 512, 257, 2, 2), (513, 100, 65, 3, 3), (300, 257, 64, 2, 1)])
def test_attention_two_segment_needles(n_q, L1, L2, H, B, attn_waves):
    """Cross-attention over two key segments: the output is the two winners' V rows added at the kernel's rounding point,
    bf16(bf16(o1) + bf16(o2)) - positive V rows, so the sum has no cancellation."""
    from chronoedit_amd import ops
    q1, k1, v1, w1 = _stacked(B, n_q, L1, H, seed=n_q + L1, extra_keys=64, positive=True)
    q2, k2, v2, w2 = _stacked(B, n_q, L2, H, seed=n_q + L2 + 1, extra_keys=64, positive=True)
    # one query row serves both segments: the digit dims of segment 2 move to dims 12..21 (12 + 2p, 13 + 2p), invalid to 104
    q = two_segment_q(q1.float(), q2.float(), H).to(BF)
    k2 = seg2_keys(k2.float(), H).to(BF)
    want = (_expected(v1, w1, L1, H).float() + _expected(v2, w2, L2, H).float()).to(BF)
    out = ops.attention(q.cuda(), k1[:B * L1].cuda(), v1[:B * L1].cuda(), H, k2=k2[:B * L2].cuda(), v2=v2[:B * L2].cuda(), batch=B)
    assert_exact(out, want, f"attention 2-segment needles {n_q}x({L1}+{L2}) H={H} B={B}")
    if attn_waves == 0:  # the V^T form (ce_attention_2seg_vt_bf16): V^T operands with per-sample column strides, zero padding
        def vt_of(v, ln):
            cols = (ln + 63) // 64 * 64
            vt = torch.zeros((H * 128, B * cols), dtype=BF)
            for b in range(B):
                vt[:, b * cols:b * cols + ln] = v[b * ln:(b + 1) * ln].t()
            return vt.cuda()
        out = ops.attention_2seg_vt(q.cuda(), k1[:B * L1].cuda(), vt_of(v1, L1), L1, k2[:B * L2].cuda(), vt_of(v2, L2), L2, H, batch=B)
        assert_exact(out, want, f"attention_2seg_vt needles {n_q}x({L1}+{L2}) H={H} B={B}")


# the last one: 5 x 24 x 5 = 600 (sample, head, query block) items, more than the launcher's 2 x #CUs workgroups - every workgroup of the
# persistent forms walks several items and derives sample, head and block again for each
MANY_ITEMS_VT = (1100, 130, 24, 5)
VT_SHAPES = [(7200, 7200, 2, 2), (333, 258, 3, 3), (1090, 1090, 8, 2), (290, 64, 5, 3), (31, 704, 4, 2), (2000, 200, 16, 3), MANY_ITEMS_VT]


@pytest.mark.parametrize("n_q,n_k,H,B", VT_SHAPES)
def test_attention_vt_needles(n_q, n_k, H, B, vt_body):
    """attention_vt on v_transpose's V^T (its padding columns zero, as the layout's contract requires: a key read past the sample's
    end or past the buffer wins and brings a 0 or a neighbour's row)."""
    from chronoedit_amd import ops
    q, k, v, win = _stacked(B, n_q, n_k, H, seed=n_q * 3 + n_k + B, extra_keys=128)
    if (n_q, n_k, H, B) == MANY_ITEMS_VT:  # fails loudly, not vacuously, on a device with more compute units
        assert (n_q + 255) // 256 * H * B > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    L = B * n_k
    kd = k.cuda()
    vt = ops.v_transpose(v[:L].cuda(), H)
    assert not vt[:, L:].any()
    out = ops.attention_vt(q.cuda(), kd[:L], vt, H, batch=B)
    assert_exact(out, _expected(v, win, n_k, H), f"attention_vt needles {n_q}x{n_k} H={H} B={B}")


def _far_case(H):
    g = torch.Generator().manual_seed(77 + H)
    q, k, v, rows = far_first_tile(70, 130, H, g)
    lead, _ = needle_margins(q, k, H, rows)
    assert lead.min() >= MIN_MARGIN_NATS
    return q, k, v, _expected(v, rows[None], 130, H)


def test_attention_first_tile_far_below_the_winner(attn_waves):
    """Every key of the first tile lies thousands of octaves below the row's winner, which sits in tile 1 or 2: exp2(-first tile's maximum) is
    +inf.  The first tile has nothing to rescale; a body that multiplies l = 0 and O = 0 by that factor returns NaN rows (the
    software-pipelined body did, before alpha = 1 at t == 0)."""
    from chronoedit_amd import ops
    q, k, v, want = _far_case(3)
    assert_exact(ops.attention(q.cuda(), k.cuda(), v.cuda(), 3), want, "attention, first tile far below the winner")


def test_attention_vt_first_tile_far_below_the_winner(vt_body):
    """The same through the V^T bodies: attn_fwd_sp_kernel<.., VT> and both one-wave-per-SIMD forms."""
    from chronoedit_amd import ops
    q, k, v, want = _far_case(3)
    out = ops.attention_vt(q.cuda(), k.cuda(), ops.v_transpose(v.cuda(), 3), 3)
    assert_exact(out, want, "attention_vt, first tile far below the winner")


@pytest.mark.parametrize("N,n,W,H,B", [(300, 128, 3, 2, 3), (7100, 3584, 2, 2, 2), (500, 64, 8, 5, 3), (1000, 256, 4, 8, 2)])
def test_attention_vt_blocked_needles(N, n, W, H, B, vt_body):
    """The all-to-all receive layout [source rank][sample][local token], N valid tokens per sample, the last block padded: padded key
    tokens win if read (their V^T columns are the layout's zero padding), every query row (padded ones included) gets its winner."""
    from chronoedit_amd import ops
    T, D = W * n, H * 128
    g = torch.Generator().manual_seed(N + n + W)
    plain = torch.empty(B, T, 3 * D, dtype=BF)
    wins = []
    for b in range(B):
        win = winners_for(T, N, H, g, must=edge_keys(N))
        invalid = torch.arange(T) >= N
        plain[b, :, :D] = needle_q(win, sample=b, batch=B).to(BF)
        plain[b, :, D:2 * D] = needle_k(T, H, sample=b, invalid=invalid).to(BF)
        plain[b, :, 2 * D:] = needle_v(T, D, g)
        plain[b, N:, 2 * D:] = POISON
        lead, fl = needle_margins(plain[b, :, :D], plain[b, :, D:2 * D], H, win, invalid)
        assert lead.min() >= MIN_MARGIN_NATS and fl.min() >= MIN_MARGIN_NATS
        wins.append(win)
    blocked = plain.view(B, W, n, 3 * D).permute(1, 0, 2, 3).contiguous().view(W * B * n, 3 * D).cuda()
    vt = ops.v_transpose_blocked(blocked[:, 2 * D:], H, B, n, N)
    cols = vt.shape[1] // B
    for b in range(B):
        assert not vt[:, b * cols + N:(b + 1) * cols].any()
    out = ops.attention_vt_blocked(blocked[:, :D], blocked[:, D:2 * D], vt, H, B, n, N)
    got = out.view(W, B, n, D).permute(1, 0, 2, 3).reshape(B * T, D)
    want = _expected(plain[:, :, 2 * D:].reshape(B * T, D), torch.stack(wins), T, H)
    assert_exact(got, want, f"attention_vt_blocked needles N={N} n={n} W={W} H={H} B={B}")


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("N,C", [(3600, 384), (1000, 384), (1000, 128), (777, 128)])
def test_attention_1head_needles(N, C, split):
    """The VAE mid-block attention (one head of C channels, scale C^-1/2): V^T with its contract's zero padding up to 64 ceil(N / 64)
    columns and POISON columns behind that; key rows past N in the buffer win if read."""
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(N + C)
    win = winners_for(N, N, 1, g, must=edge_keys(N))
    extra = 64
    q = torch.zeros(N, C, dtype=torch.float64)
    q[:, :128] = needle_q(win)
    k = torch.zeros(N + extra, C, dtype=torch.float64)
    k[:, :128] = needle_k(N + extra, 1, invalid=torch.arange(N + extra) >= N)
    q, k = q.to(BF), k.to(BF)
    # (scale C^-1/2: at C = 384 the runner-up trails by 512 / sqrt(384) = 26 nats)
    lead, fl = needle_margins(q[:, :128], k[:, :128], 1, win, torch.arange(N + extra) >= N)
    assert (lead * (128 / C) ** 0.5).min() >= MIN_MARGIN_NATS and (fl * (128 / C) ** 0.5).min() >= MIN_MARGIN_NATS
    v = needle_v(N, C, g)
    cols = (N + 63) // 64 * 64
    vt = torch.full((C, cols + 64), POISON, dtype=BF)
    vt[:, :cols] = 0
    vt[:, :N] = v.t()
    out = ops.attention_1head(q.cuda(), k[:N].cuda(), vt.cuda(), C ** -0.5, split_keys=split)
    assert_exact(out, v[win[:, 0]], f"attention_1head needles N={N} C={C} split={split}")


# ---- the speculative route, locally: smooth random data, worst (sample, head, 64-query block) --------------------------------------
def _sdpa(q, k, v, H):
    qh = q.float().view(q.shape[0], H, 128).transpose(0, 1)
    kh = k.float().view(k.shape[0], H, 128).transpose(0, 1)
    vh = v.float().view(v.shape[0], H, 128).transpose(0, 1)
    return torch.nn.functional.scaled_dot_product_attention(qh[None], kh[None], vh[None])[0].transpose(0, 1).reshape(q.shape[0], -1)


def _worst_block(out, ref, B, n, H):
    """max over (sample, head, 64-query block) of the block's rel-L2."""
    o = out.float().view(B, n, H, 128)
    r = ref.float().view(B, n, H, 128)
    worst = 0.0
    for s in range(0, n, 64):
        d = (o[:, s:s + 64] - r[:, s:s + 64]).pow(2).sum((1, 3)).sqrt()
        nr = r[:, s:s + 64].pow(2).sum((1, 3)).sqrt()
        worst = max(worst, float((d / nr).max()))
    return worst


def test_attention_vt_worst_block_on_smooth_data(vt_body):
    from chronoedit_amd import ops
    B, n, H = 2, 7200, 2
    D = H * 128
    g = torch.Generator(device="cuda").manual_seed(41)
    q = torch.randn(B * n, D, device="cuda", generator=g).to(BF)
    k = torch.randn(B * n, D, device="cuda", generator=g).to(BF)
    v = torch.randn(B * n, D, device="cuda", generator=g).to(BF)
    out = ops.attention_vt(q, k, ops.v_transpose(v, H), H, batch=B)
    ref = torch.cat([_sdpa(q[b * n:(b + 1) * n], k[b * n:(b + 1) * n], v[b * n:(b + 1) * n], H) for b in range(B)])
    worst = _worst_block(out, ref, B, n, H)
    print(f"attention_vt body {vt_body}: worst 64-query block rel-L2 {worst:.3e}")
    assert worst < 5e-3, worst  # (measured 3.0e-3 for all three bodies; the whole-tensor bound elsewhere is 1e-2)


def test_attention_mxfp8_worst_block_against_its_contract():
    """attention_mxfp8 (default kernel: lazy offset, speculative) against its contract oracle.dit_oracle.attention_mxfp8 at 7200 keys,
    B = 2, per (sample, head, 64-query block)."""
    from chronoedit_amd import ops
    from oracle import dit_oracle as O
    B, n, H = 2, 7200, 2
    D = H * 128
    g = torch.Generator(device="cuda").manual_seed(43)
    x = torch.randn(B * n, 3 * D, device="cuda", generator=g).to(BF)
    one = torch.ones(D, device="cuda")
    q8, sq = ops.rmsnorm_rope_mxfp8(x[:, :D], one, None, 128, 1e-6, post_scale=ops.MXFP8_Q_SCALE)
    k8, sk = ops.rmsnorm_rope_mxfp8(x[:, D:2 * D], one, None, 128, 1e-6)
    v8t, sv = ops.v_mxfp8_transpose(x[:, 2 * D:], n, B, H)
    out = ops.attention_mxfp8(q8, sq, k8, sk, v8t, sv, H, batch=B)
    ref_in = x.clone()
    ops.rmsnorm_rope_(ref_in[:, :D], one, None, 128, 1e-6, x2=ref_in[:, D:2 * D], w2=one)
    f = lambda t: t.float().cpu().view(B, n, H, 128).permute(0, 2, 1, 3)
    want = O.attention_mxfp8(f(ref_in[:, :D]), f(ref_in[:, D:2 * D]), f(ref_in[:, 2 * D:])).permute(0, 2, 1, 3).reshape(B * n, D)
    worst = _worst_block(out.cpu(), want, B, n, H)
    print(f"attention_mxfp8: worst 64-query block rel-L2 vs its contract {worst:.3e}")
    assert worst < 5e-3, worst  # (measured 3.1e-3)
