"""The padding of a text context attended once, weighted (ChronoEditTransformer3DModel.enable_text_compaction).

Kernel level: `ce_attention_2seg_vt_weighted_bf16` on compacted operands (a sample's n real keys, ONE padding key with log2-weight
log2(192 - n), then garbage rows that the valid count must mask) against `ce_attention_2seg_vt_strided_bf16` on the physically padded
operands (192 keys, the last 192 - n copies of one K row and one V row).  head_dim 128, Nq = 288 (a full 256-row block + a 32-row remainder),
H = 8 (the per-XCD work order) and H = 5 (the other branch), len2 = 257, two samples with different n.
  * multiplicity 1 (n = 191) and no padding at all (valid = len, w = 0): the sample's output is bit-equal;
  * otherwise both kernels are compared with the fp32 reference on the padded operands, on the CPU (the softmax-attention product of
    oracle/dit_oracle.py's `attention`: F.scaled_dot_product_attention per segment, the two outputs added), and the weighted form's
    max-abs and rel-L2 errors must stay within 1.5 x the strided form's (one P entry rounds differently, the row sum is shorter - the
    path must not be worse in kind).  Peaked cases: the padding key as the row maximum far outside the speculative window (the tile
    takes the exact route with the weight applied), and a real key as the maximum with the weighted key far below the window.
    Measured on MI355X (full table: profiles/notes_attention_bf16.md, "Weighted last key"): worst case H = 8, n = (64, 70): strided max-abs
    2.129e-02 rel-L2 2.968e-03, weighted 2.285e-02 / 2.972e-03 (ratios 1.07 / 1.002); the peaked cases agree to all printed digits.
Engine level, on the suite's miniature widths (2 heads x 128, 2 layers), N = 288 tokens, 512 text rows with n = 64 / 37 real ones, 257 image
keys: compaction on against off and both against the fp32 oracle (on <= 1.25 x off; measured rel-L2 5.091e-03 on, 5.078e-03 off); eager against graph replay, context cache on
against off, a prompt without (enough) padding against the uncompacted sequence, a second edit of another length against a fresh engine -
all bit-equal."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NQ, L1, L2, B = 288, 192, 257, 2
pad64 = lambda n: (n + 63) // 64 * 64


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def max_abs(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max())


def _rand(g, *s, scale=1.0):
    return (torch.randn(*s, generator=g) * scale).to(BF)


def _case(H, ns, peaked=None, seed=5):
    """Padded operands (CPU, bf16): q [B NQ, Dm], k1 [B L1, Dm], v1 [B L1, Dm] (rows >= n_b of sample b = one row), k2 / v2 [B L2, Dm]."""
    g = torch.Generator().manual_seed(seed + 100 * H + sum(ns))
    Dm = H * 128
    q, k1, v1 = _rand(g, B * NQ, Dm), _rand(g, B * L1, Dm), _rand(g, B * L1, Dm)
    k2, v2 = _rand(g, B * L2, Dm), _rand(g, B * L2, Dm)
    u = torch.randn(Dm, generator=g)
    if peaked is not None:
        q = (q.float() + u).to(BF)  # every query leans on u: a key +-3 u sits ~ +-49 octaves from the others
    for b, n in enumerate(ns):
        if n < L1:
            kp, vp = _rand(g, Dm), _rand(g, Dm)
            if peaked == "pad":
                kp = (3.0 * u).to(BF)
            elif peaked == "real":
                kp = (-3.0 * u).to(BF)
                k1[b * L1 + 5] = (3.0 * u).to(BF)
            k1[b * L1 + n: (b + 1) * L1] = kp
            v1[b * L1 + n: (b + 1) * L1] = vp
    return q, k1, v1, k2, v2


def _reference(H, q, k1, v1, k2, v2, share_q=False, share2=False):
    """fp32, per sample and head: softmax(q k1^T / sqrt(128)) v1 + softmax(q k2^T / sqrt(128)) v2."""
    f = lambda t, n, b, shared: t.float()[(0 if shared else b) * n: (0 if shared else b) * n + n].view(n, H, 128).transpose(0, 1)
    outs = []
    for b in range(B):
        qb = f(q, NQ, b, share_q)
        o = F.scaled_dot_product_attention(qb, f(k1, L1, b, False), f(v1, L1, b, False)) + \
            F.scaled_dot_product_attention(qb, f(k2, L2, b, share2), f(v2, L2, b, share2))
        outs.append(o.transpose(0, 1).reshape(NQ, H * 128))
    return torch.cat(outs, 0)


def _vt(v, n, cols, width, nb=B):
    """rows [nb n, Dm] -> V^T [Dm, width], sample b at columns [b cols, b cols + n); zero elsewhere."""
    out = torch.zeros(v.shape[1], width, dtype=BF)
    for b in range(nb):
        out[:, b * cols: b * cols + n] = v[b * n: (b + 1) * n].t()
    return out


def _run_pair(H, ns, peaked=None, share=False):
    """(strided on padded operands, weighted on compacted operands, fp32 reference), each [B NQ, Dm] on the CPU."""
    from chronoedit_amd import ops
    q, k1, v1, k2, v2 = _case(H, ns, peaked)
    if share:
        q[NQ:] = q[:NQ]
        k2[L2:], v2[L2:] = k2[:L2], v2[:L2]
    ref = _reference(H, q, k1, v1, k2, v2)
    Dm = H * 128
    c2 = (L2 + 7) // 8 * 8
    nb2 = 1 if share else B
    v1t = _vt(v1, L1, L1, (B - 1) * L1 + pad64(L1)).cuda()
    v2t = _vt(v2, L2, c2, (nb2 - 1) * c2 + pad64(L2), nb2).cuda()
    qd, k1d, k2d = (q[:NQ] if share else q).cuda(), k1.cuda(), (k2[:L2] if share else k2).cuda()
    old = torch.full((B * NQ, Dm), float("nan"), dtype=BF, device="cuda")
    ops.attention_2seg_vt_shared(qd, k1d, v1t, L1, k2d, v2t, L2, H, out=old, batch=B, share_q=share, share2=share, cols1=L1,
                                 cols2=None if share else c2)
    # compacted: n_b real rows, the padding row, then rows of large finite garbage that the valid count has to mask
    valid = [min(n + 1, L1) for n in ns]
    w = [math.log2(L1 - v + 1) for v in valid]
    Lc = (max(valid) + 7) // 8 * 8
    g = torch.Generator().manual_seed(99)
    k1c, v1c = _rand(g, B * Lc, Dm, scale=50.0), _rand(g, B * Lc, Dm, scale=50.0)
    for b, v in enumerate(valid):
        k1c[b * Lc: b * Lc + v] = k1[b * L1: b * L1 + v]
        v1c[b * Lc: b * Lc + v] = v1[b * L1: b * L1 + v]
    v1ct = _vt(v1c, Lc, Lc, (B - 1) * Lc + pad64(Lc)).cuda()
    new = torch.full((B * NQ, Dm), float("nan"), dtype=BF, device="cuda")
    ops.attention_2seg_vt_weighted(qd, k1c.cuda(), v1ct, Lc, k2d, v2t, L2, H, out=new, batch=B,
                                   valid1=torch.tensor(valid, dtype=torch.int32, device="cuda"),
                                   w1=torch.tensor(w, dtype=torch.float32, device="cuda"), share_q=share, share2=share, cols1=Lc,
                                   cols2=None if share else c2)
    return old.cpu(), new.cpu(), ref, valid


def _check(tag, ns, old, new, ref, valid):
    assert torch.isfinite(new.float()).all()
    for b, v in enumerate(valid):
        if v == L1:  # multiplicity 1 or no padding: w = 0, every key walked - the strided kernel's result bit for bit
            rows = slice(b * NQ, (b + 1) * NQ)
            assert torch.equal(new[rows], old[rows]), (tag, ns, b, int((new[rows] != old[rows]).sum()))
    e_old, e_new = (max_abs(old, ref), rel_l2(old, ref)), (max_abs(new, ref), rel_l2(new, ref))
    print(f"{tag} n={ns}: strided max-abs {e_old[0]:.3e} rel-L2 {e_old[1]:.3e} | weighted max-abs {e_new[0]:.3e} rel-L2 {e_new[1]:.3e}")
    assert e_new[0] <= 1.5 * e_old[0] and e_new[1] <= 1.5 * e_old[1], (tag, ns, e_old, e_new)


# n per sample: all padding / a weighted key that ends a tile; alone in a new tile / mid-tile; multiplicity 2 / 1; multiplicity 1 / none
@pytest.mark.parametrize("H", [8, 5])
@pytest.mark.parametrize("ns", [(0, 63), (64, 70), (190, 191), (191, 192)])
def test_weighted_last_key_equals_physical_padding(H, ns):
    old, new, ref, valid = _run_pair(H, ns)
    _check(f"H={H}", ns, old, new, ref, valid)


def test_weighted_last_key_with_shared_queries_and_image_segment():
    old, new, ref, valid = _run_pair(8, (64, 70), share=True)
    _check("shared", (64, 70), old, new, ref, valid)


@pytest.mark.parametrize("peaked", ["pad", "real"])
def test_weighted_last_key_peaked_rows(peaked):
    """pad: the padding key's logit is the row maximum by ~49 octaves - in tile 1 the speculative softmax overflows its window and the exact
    route has to apply the weight again; real: key 5 is the maximum by as much and the weighted key sits ~98 octaves below it."""
    old, new, ref, valid = _run_pair(8, (64, 70), peaked=peaked)
    _check(f"peaked-{peaked}", (64, 70), old, new, ref, valid)
    if peaked == "pad":  # the row IS the padding value (plus the image segment): the weighted key was not lost
        assert rel_l2(new, ref) < 2e-2


def test_weighted_arguments_are_validated():
    from chronoedit_amd import ops
    z = torch.zeros(64, 256, dtype=BF, device="cuda")
    vt = torch.zeros(256, 128, dtype=BF, device="cuda")
    o = torch.zeros(128, 256, dtype=BF, device="cuda")
    va, wa = torch.tensor([32, 1], dtype=torch.int32, device="cuda"), torch.zeros(2, device="cuda")
    args = lambda v, w: (ops._ptr(z), ops._ptr(z), ops._ptr(vt), 32, 256, 128, 32, ops._ptr(z), ops._ptr(vt), 32, 256, 128, 32, ops._ptr(o), 64, 2,
                         128, 256, 256, 0.1, 2, 0, 32, 0, v, w, ops._stream())
    lib = ops.lib()
    assert lib.ce_attention_2seg_vt_weighted_bf16(*args(None, ops._ptr(wa))) == -1
    assert lib.ce_attention_2seg_vt_weighted_bf16(*args(ops._ptr(va), None)) == -1
    assert lib.ce_attention_2seg_vt_weighted_bf16(*args(ops._ptr(va), ops._ptr(wa))) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------------------------------------------------------------------
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
HW, TT, TI = 24, 512, 257  # 12 x 12 patches per frame: N = 288 at T = 2
ORACLE_BOUND = 2e-2        # tests/test_dit_forward_gpu.py's bound for the bf16 path against the fp32 oracle
_PARAMS = {}


def _model(compaction=True, cache=False):
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    if "p" not in _PARAMS:
        _PARAMS["p"] = D.make_synthetic_params(DCFG, dtype=BF)
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in _PARAMS["p"].items()})
    m.enable_text_compaction(compaction)
    m.cache_context = cache
    return m


def _inputs(n_pr=64, n_ng=37, T=2, seed=3):
    """latents, condition, prompt (n_pr real rows, then zero rows, as the reference pads), negative prompt (n_ng), image."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF)
    lat, cond, pr, ng, img = r(1, 16, T, HW, HW).float(), r(1, 20, T, HW, HW), r(1, TT, 128), r(1, TT, 128), r(1, TI, 64)
    pr[:, n_pr:] = 0
    ng[:, n_ng:] = 0
    return lat, cond, pr, ng, img


def _pair_forward(m, inp):
    from chronoedit_amd import pipeline
    lat, cond, pr, ng, img = (t.cuda() for t in inp)
    x = torch.cat([lat.to(BF), cond], 1)
    text2, image2 = pipeline.make_cfg_inputs(pr, ng, img)
    with pipeline._shared_inputs(m):
        out = m(torch.cat([x, x], 0), torch.tensor([500, 500], device="cuda"), text2, image2, return_dict=False)[0]
    return out, text2


def _text_rows(m):
    """Text rows per sample of the engine's transposed-V context buffers (what `_context` last projected)."""
    return sorted(k[2] for k in m.engine()._ctx_bufs)


def _edit(m, inp, steps=3, **kw):
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    lat, cond, pr, ng, img = (t.cuda() for t in inp)
    return denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat.clone(), cond, pr, ng, img, steps, 5.0, **kw).clone()


def test_forward_compacted_vs_full_and_both_vs_oracle():
    inp = _inputs()
    m = _model(True)
    on, text2 = _pair_forward(m, inp)
    on = on.clone()
    assert text2._ce_compact.real == [64, 37] and text2._ce_compact.Lc == 72 and _text_rows(m) == [72]
    assert text2._ce_compact.valid.tolist() == [65, 38]
    m.enable_text_compaction(False)
    off, _ = _pair_forward(m, inp)
    assert _text_rows(m)[-1] == TT
    lat, cond, pr, ng, img = (t.float() for t in inp)
    p = {k: v.float() for k, v in _PARAMS["p"].items()}
    x = torch.cat([lat, cond], 1)
    with torch.no_grad():
        ref = torch.cat([D.dit_forward(p, DCFG, x, torch.tensor([500]), t, img) for t in (pr, ng)], 0)
    e_on, e_off = rel_l2(on, ref), rel_l2(off, ref)
    print(f"forward vs fp32 oracle: compacted {e_on:.3e}, full {e_off:.3e} (bound 1.25 x full); compacted vs full {rel_l2(on, off):.3e}")
    assert e_on <= 1.25 * e_off, (e_on, e_off)
    assert e_on < ORACLE_BOUND and e_off < ORACLE_BOUND, (e_on, e_off)
    assert rel_l2(on[:1], on[1:]) > 1e-3  # the two samples do differ


def test_direct_forward_on_a_full_tensor_never_compacts():
    inp = _inputs()
    lat, cond, pr, ng, img = (t.cuda() for t in inp)
    x = torch.cat([lat.to(BF), cond], 1)
    text2, image2 = torch.cat([pr, ng], 0), torch.cat([img, img], 0)  # nobody examined this tensor
    a, b = _model(True), _model(False)
    ts = torch.tensor([500, 500], device="cuda")
    oa = a(torch.cat([x, x], 0), ts, text2, image2, return_dict=False)[0]
    ob = b(torch.cat([x, x], 0), ts, text2, image2, return_dict=False)[0]
    assert _text_rows(a) == [TT] and torch.equal(oa, ob)


def test_eager_graph_and_context_cache_are_bit_equal():
    inp = _inputs()
    m = _model(True)
    eager = _edit(m, inp)
    assert _text_rows(m) == [72]
    graph = _edit(_model(True), inp, use_graph=True)
    cached = _edit(_model(True, cache=True), inp)
    cached_graph = _edit(_model(True, cache=True), inp, use_graph=True)
    assert torch.equal(eager, graph), max_abs(eager, graph)
    assert torch.equal(eager, cached), max_abs(eager, cached)
    assert torch.equal(eager, cached_graph), max_abs(eager, cached_graph)
    assert torch.isfinite(eager).all()
    full = _edit(_model(False), inp)
    print(f"3-step edit: compacted vs full latents rel-L2 {rel_l2(eager, full):.3e}")
    assert rel_l2(eager, full) < ORACLE_BOUND


@pytest.mark.parametrize("n_pr,n_ng", [(TT, 37), (460, 37)])  # no padding at all in one sample; 52 padding rows: still 8 key tiles
def test_too_little_padding_runs_the_uncompacted_sequence(n_pr, n_ng):
    inp = _inputs(n_pr, n_ng)
    m = _model(True)
    on = _edit(m, inp, steps=2)
    assert _text_rows(m) == [TT]
    off = _edit(_model(False), inp, steps=2)
    assert torch.equal(on, off)


@pytest.mark.parametrize("cache,graph", [(True, False), (False, True)])
def test_second_edit_of_another_length_equals_a_fresh_engine(cache, graph):
    first, second = _inputs(64, 37), _inputs(130, 20, seed=4)
    m = _model(True, cache=cache)
    warm = set()
    _edit(m, first, use_graph=graph, graph_warm=warm)
    again = _edit(m, second, use_graph=graph, graph_warm=warm)  # (graph: a warm shape - the capture must find the new length's buffers)
    assert _text_rows(m)[-1] == 136 or 136 in _text_rows(m)
    fresh = _edit(_model(True, cache=cache), second, use_graph=graph)
    assert torch.equal(again, fresh), max_abs(again, fresh)
