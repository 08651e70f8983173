"""Sparse region edits on the device (chronoedit_amd/sparse_region.py, DiTEngine.sparse_begin / _forward_sparse, pipeline.denoise).
`_forward_sparse` owns the sparse self-attention half (fused q|k|v, the two scatters); its time tables, cross-attention, FFN and head rows
are the dense forward's own methods (`_time_tables`, `_cross_queries`, `_cross_attention`, `_ffn`, `_head_rows`).

Latents 1 x 16 x 2 x 16 x 20 - N = 160 tokens, 2.5 key tiles - with a guidance pair and 6 steps on the tiny model of tests/test_region_gpu.py
(2 heads x 128, 2 layers, ffn 512).  The mask is 128 x 160 with a rectangle over latent rows 4..9 and columns 6..13: with margin 1 that is 60
active tokens, padded to 64.  A grey feathered mask runs through the loop as well.

  1. a "refresh" forward is the plain forward bit for bit;
  2. refresh then sparse on the same input: the active rows against the fp32 oracle at the same positions (rel-L2 <= 2e-2 and <= 3 x the dense
     engine's error there + 2e-3, the bounds of tests/test_dit_forward_gpu.py), exactly 0 elsewhere;
  3. a sparse step reads nothing of the inactive tokens of its input;
  4. stale-cache semantics across two sparse steps against an fp32 second implementation written here from the oracle's pieces;
  5. the loop: refresh_every = 1 is the dense region edit, hipGraph replay equals eager, kept cells end on z_src, also with the 8 -> 2 truncation;
  6. refusals, a second edit with another mask, disable_sparse_region, and ChronoEditPipeline.__call__."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
STEPS, G = 6, 5.0
LH, LW = 16, 20          # latent plane; 8 x 10 patches
H, W = 8 * LH, 8 * LW    # 128 x 160
N = 2 * (LH // 2) * (LW // 2)
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
_PARAMS = {}


def _params():
    if "p" not in _PARAMS:
        _PARAMS["p"] = D.make_synthetic_params(DCFG, dtype=BF)
    return _PARAMS["p"]


def _model():
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in _params().items()})
    return m


def rect_mask():
    m = torch.zeros((H, W), dtype=torch.uint8)
    m[32:80, 48:112] = 255  # latent rows 4..9, columns 6..13
    return m


def feathered_mask():
    """Grey: the rectangle with a ramp of 16 pixels around it, 0 further out."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    d = torch.maximum(torch.maximum(32 - yy, yy - 79), torch.maximum(48 - xx, xx - 111)).clamp(min=0).float()  # pixels outside the rectangle
    return (255.0 * (1.0 - d / 16.0).clamp(0, 1)).round().to(torch.uint8)


def active_ids(mask=None, T=2, margin=1):
    from chronoedit_amd import region, sparse_region
    return sparse_region.active_tokens(region.latent_weights(rect_mask() if mask is None else mask), T, margin)


def test_the_rectangle_gives_60_active_tokens_padded_to_64():
    ids, n = active_ids()
    assert n == 60 and ids.numel() == 64 and ids[:4].tolist() == [0, 1, 2, 3]
    ids_f, n_f = active_ids(feathered_mask())
    assert n_f > n and ids_f.numel() % 8 == 0 and ids_f.numel() < N  # the ramp reaches further; something stays inactive


# ----------------------------------------------------------------------------------------------------------------------------------
# the engine: forwards
# ----------------------------------------------------------------------------------------------------------------------------------
def pair_inputs(seed, shared=True):
    """(hidden [2, 36, 2, 16, 20], timestep [2], text [2, Tt, 128], image [2, 257, 64]) on the CPU, bf16 values in fp32.  shared: the two
    samples differ in the text only (the guidance pair), and the text is 128 rows of which 23 / 30 are real and the rest zero padding - the
    loop's form: compacted text, one image segment for both samples.  Otherwise 40 unpadded rows, and the samples differ in everything."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    hid, txt, img = r(2, 36, 2, LH, LW), r(2, 128 if shared else 40, 128), r(2, 257, 64)
    ts = torch.tensor([700, 400])
    if shared:
        hid[1], img[1], ts = hid[0], img[0], torch.tensor([700, 700])
        txt[0, 23:], txt[1, 30:] = 0, 0
    return hid, ts, txt, img


def run(m, inp, mode=None, shared=True):
    """One forward in the given sparse mode; shared: declared as the loop declares its guidance pair (with the compacted text context)."""
    from chronoedit_amd.pipeline import _shared_inputs, make_cfg_inputs
    hid, ts, txt, img = inp
    hid, ts, txt, img = hid.cuda().to(BF), ts.cuda(), txt.cuda().to(BF), img.cuda().to(BF)
    m._sparse_mode = mode
    try:
        if shared:
            txt, img = make_cfg_inputs(txt[:1], txt[1:], img[:1])
            with _shared_inputs(m):
                return m(hid, ts, txt, img, return_dict=False)[0].clone()
        return m(hid, ts, txt, img, return_dict=False)[0].clone()
    finally:
        m._sparse_mode = None


def begin(m, ids=None):
    ids = active_ids()[0] if ids is None else ids
    m.engine().sparse_begin(ids, 2, 2, LH, LW)
    return ids


def token_rows(out):
    """[B, Cout, T, H, W] -> [B, N, 4 * Cout], column (dh * 2 + dw) * Cout + c: the head's rows."""
    B, C, T = out.shape[:3]
    return out.reshape(B, C, T, LH // 2, 2, LW // 2, 2).permute(0, 2, 3, 5, 4, 6, 1).reshape(B, T * (LH // 2) * (LW // 2), 4 * C)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def oracle(inp, taps=None):
    hid, ts, txt, img = inp
    p32 = {k: v.float() for k, v in _params().items()}
    with torch.no_grad():
        return D.dit_forward(p32, DCFG, hid, ts, txt, img, taps=taps)


@pytest.mark.parametrize("shared", [True, False])
def test_a_refresh_forward_is_the_plain_forward(shared):
    m = _model()
    inp = pair_inputs(1, shared)
    plain = run(m, inp, None, shared)
    begin(m)
    assert torch.equal(run(m, inp, "refresh", shared), plain)
    assert torch.equal(run(m, inp, None, shared), plain)
    # ... and what it stored: every layer's K and V^T of both samples, finite, the padding columns still zero
    st = m.engine()._sparse
    assert st.valid and tuple(st.k.shape) == (2, 2 * N, 256) and tuple(st.vt.shape[:2]) == (2, 256)
    assert torch.isfinite(st.k.float()).all() and bool((st.vt[:, :, 2 * N:] == 0).all()) and bool((st.vt[:, :, : 2 * N] != 0).any())


@pytest.mark.parametrize("shared", [True, False])
def test_fresh_cache_active_rows_against_the_fp32_oracle(shared):
    m = _model()
    inp = pair_inputs(2, shared)
    dense = run(m, inp, None, shared)
    ids = begin(m)
    run(m, inp, "refresh", shared)
    sparse = run(m, inp, "sparse", shared)
    ref = token_rows(oracle(inp))
    got, den = token_rows(sparse.float().cpu()), token_rows(dense.float().cpu())
    e_sparse, e_dense = rel_l2(got[:, ids], ref[:, ids]), rel_l2(den[:, ids], ref[:, ids])
    print(f"shared={shared}: sparse-vs-fp32 {e_sparse:.3e}  dense-vs-fp32 {e_dense:.3e}  sparse-vs-dense {rel_l2(got[:, ids], den[:, ids]):.3e}")
    assert e_sparse <= 2e-2
    assert e_sparse <= 3 * e_dense + 2e-3
    rest = torch.ones(N, dtype=torch.bool)
    rest[ids] = False
    assert bool((got[:, rest] == 0).all()) and bool((got[:, ids] != 0).any())


def test_a_sparse_step_reads_nothing_of_the_inactive_tokens():
    m = _model()
    a = pair_inputs(3)
    ids = begin(m)
    run(m, a, "refresh")
    first = run(m, a, "sparse")
    # A': other values in every latent cell of every inactive token, the active tokens' cells untouched
    cells = torch.zeros(N, dtype=torch.bool)
    cells[ids] = True
    cells = cells.view(2, LH // 2, 1, LW // 2, 1).expand(2, LH // 2, 2, LW // 2, 2).reshape(1, 1, 2, LH, LW)
    hid2 = torch.where(cells, a[0], pair_inputs(33)[0][:1].expand_as(a[0]))
    assert not torch.equal(hid2, a[0])
    assert torch.equal(run(m, (hid2,) + a[1:], "sparse"), first)


def ref_sparse_step(p, inp, ids, cache):
    """The fp32 second implementation of a sparse step, from the oracle's pieces: everything on the active rows; per layer the keys and
    values of the active tokens replace their entries in `cache` (a list of [k, v] per layer, [B, heads, N, 128], from the newest earlier
    step), and the self-attention runs over all of them."""
    hid, ts, txt, img = inp
    cfg = DCFG
    rotary = D.rope_table(cfg, 2, LH, LW)[:, :, ids]
    x = F.conv3d(hid, p["patch_embedding.weight"], p["patch_embedding.bias"], stride=cfg.patch_size).flatten(2).transpose(1, 2)[:, ids]
    temb, tproj, text, image = D.condition_embed(p, cfg, ts, txt, img)
    tproj = tproj.unflatten(1, (6, -1))
    enc = torch.cat([image, text], dim=1)
    Hn = cfg.num_attention_heads
    for i in range(cfg.num_layers):
        b = f"blocks.{i}"
        shift, scale, gate, c_shift, c_scale, c_gate = (p[b + ".scale_shift_table"] + tproj.float()).chunk(6, dim=1)
        h = D.fp32_layer_norm(x, None, None, cfg.eps) * (1 + scale) + shift
        pre = b + ".attn1"
        q = D.rms_norm(D.linear(h, p, pre + ".to_q"), p[pre + ".norm_q.weight"], cfg.eps).unflatten(2, (Hn, -1)).transpose(1, 2)
        k = D.rms_norm(D.linear(h, p, pre + ".to_k"), p[pre + ".norm_k.weight"], cfg.eps).unflatten(2, (Hn, -1)).transpose(1, 2)
        v = D.linear(h, p, pre + ".to_v").unflatten(2, (Hn, -1)).transpose(1, 2)
        q, k = D.apply_rope(q, rotary), D.apply_rope(k, rotary)
        cache[i][0][:, :, ids], cache[i][1][:, :, ids] = k, v
        a = F.scaled_dot_product_attention(q, cache[i][0], cache[i][1]).transpose(1, 2).flatten(2, 3)
        x = x + D.linear(a, p, pre + ".to_out.0") * gate
        h = D.fp32_layer_norm(x, p[b + ".norm2.weight"], p[b + ".norm2.bias"], cfg.eps)
        x = x + D.attention(p, b + ".attn2", cfg, h, enc, None)
        h = D.fp32_layer_norm(x, None, None, cfg.eps) * (1 + c_scale) + c_shift
        x = x + D.feed_forward(p, b + ".ffn", h, "tanh") * c_gate
    shift, scale = (p["scale_shift_table"] + temb.unsqueeze(1)).chunk(2, dim=1)
    return D.linear(D.fp32_layer_norm(x, None, None, cfg.eps) * (1 + scale) + shift, p, "proj_out")  # [B, Na, 4 * Cout]


def test_stale_cache_semantics_across_two_sparse_steps():
    """refresh(A), sparse(B), sparse(C), B and C other inputs than A everywhere: the inactive tokens' keys and values are A's, the active
    ones' those of the newest step - against the fp32 second implementation above, within the bounds of the fresh-cache test.
    Measured on MI355X: sparse(B) 5.1e-3, sparse(C) 5.0e-3 against that reference, the dense engine 5.0e-3 against the dense oracle.  With
    these synthetic weights the fp32 reference itself moves only 5.2e-3 when C's stale keys are swapped for C's own (the dense forward of
    C), which is inside the bound: the tolerance alone would not notice a scatter that went wrong.  So the same semantics are pinned
    exactly as well: the rows of inactive tokens in the cache are bit for bit what the refresh stored, and the result of sparse(C) does not
    depend on the step before it - refresh(A), sparse(C) gives the same bits, which it cannot if any of B's keys or values survived."""
    m = _model()
    a, b, c = pair_inputs(4), pair_inputs(5), pair_inputs(6)
    ids = begin(m)
    run(m, a, "refresh")
    st = m.engine()._sparse
    k_a, vt_a = st.k.clone(), st.vt.clone()
    out_b = run(m, b, "sparse")
    k_b = st.k.clone()
    out_c = run(m, c, "sparse")
    got_b, got_c = token_rows(out_b.float().cpu())[:, ids], token_rows(out_c.float().cpu())[:, ids]
    p32 = {k: v.float() for k, v in _params().items()}
    taps = {}
    oracle(a, taps)
    cache = [[taps[f"blocks.{i}.attn1.k"].clone(), taps[f"blocks.{i}.attn1.v"].clone()] for i in range(DCFG.num_layers)]
    with torch.no_grad():
        ref_b = ref_sparse_step(p32, b, ids, cache)
        ref_c = ref_sparse_step(p32, c, ids, cache)
    dense_c = token_rows(oracle(c))[:, ids]
    e_dense = rel_l2(token_rows(run(_model(), c).float().cpu())[:, ids], dense_c)
    e_b, e_c = rel_l2(got_b, ref_b), rel_l2(got_c, ref_c)
    print(f"sparse(B) {e_b:.3e}  sparse(C) {e_c:.3e}  dense-vs-fp32 {e_dense:.3e}  fp32 stale-vs-dense reading of C {rel_l2(dense_c, ref_c):.3e}")
    for e in (e_b, e_c):
        assert e <= 2e-2
        assert e <= 3 * e_dense + 2e-3
    # the cache, exactly: inactive tokens as the refresh left them, active tokens rewritten by every sparse step
    rows = torch.ones(2 * N, dtype=torch.bool, device="cuda:0")
    for s_ in range(2):
        rows[s_ * N + ids.cuda()] = False
    assert torch.equal(st.k[:, rows], k_a[:, rows]) and torch.equal(st.vt[:, :, : 2 * N][:, :, rows], vt_a[:, :, : 2 * N][:, :, rows])
    assert torch.equal(st.vt[:, :, 2 * N:], vt_a[:, :, 2 * N:])
    for li in range(DCFG.num_layers):
        assert not torch.equal(k_b[li][~rows], k_a[li][~rows]) and not torch.equal(st.k[li][~rows], k_b[li][~rows]), li
    # ... and sparse(C) is a function of A's refresh and C alone
    m2 = _model()
    begin(m2)
    run(m2, a, "refresh")
    assert torch.equal(run(m2, c, "sparse"), out_c)
    assert torch.equal(m2.engine()._sparse.k, st.k) and torch.equal(m2.engine()._sparse.vt, st.vt)
    assert not torch.equal(out_b, out_c)


def test_engine_lifecycle_and_refusals():
    m = _model()
    eng = m.engine()
    inp = pair_inputs(7)
    with pytest.raises(RuntimeError, match="sparse_begin"):
        run(m, inp, "sparse")
    ids = begin(m)
    with pytest.raises(RuntimeError, match="refresh"):
        run(m, inp, "sparse")  # nothing stored yet
    with pytest.raises(ValueError):
        run(m, inp, "sparse-ish")
    for bad in (ids[:-1], torch.cat([ids[:8], ids[:8]]), ids + 100):
        with pytest.raises(ValueError):
            eng.sparse_begin(bad, 2, 2, LH, LW)
    run(m, inp, "refresh")
    assert not eng.sparse_is_warm()
    run(m, inp, "sparse")
    assert eng.sparse_is_warm()
    k_ptr = eng._sparse.k.data_ptr()
    begin(m, ids[8:])  # another list, same geometry: the cache stays where it is, its content is dropped
    assert eng._sparse.k.data_ptr() == k_ptr and not eng._sparse.valid and eng._sparse.Na == 56 and not eng.sparse_is_warm()
    m._tea_mode = "compute"
    try:
        with pytest.raises(ValueError, match="TeaCache"):
            run(m, inp, "refresh")
    finally:
        m._tea_mode = None
    eng.sparse_drop()
    assert eng._sparse is None
    for switch in (lambda x: x.enable_fp8_gemms(), lambda x: x.enable_fp8_attention(), lambda x: x.enable_transposed_v(False)):
        m2 = _model()
        switch(m2)
        with pytest.raises(NotImplementedError):
            m2.engine().sparse_begin(ids, 2, 2, LH, LW)


# ----------------------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------------------
def _inputs(T=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    return r(1, 16, T, LH, LW), r(1, 20, T, LH, LW), r(1, 40, 128), r(1, 40, 128), r(1, 257, 64), r(1, 16, T, LH, LW)


def _scheduler():
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    return FlowUniPCMultistepScheduler(flow_shift=5.0)


def _run(m, inp, mask, sparse=None, use_graph=False, **kw):
    from chronoedit_amd import region
    from chronoedit_amd.pipeline import denoise
    lat0, cond, pr, ng, img, z = (t.cuda() for t in inp)
    cfg = None if mask is None else region.RegionConfig(w=region.latent_weights(mask.cuda()), z_src=z)
    return denoise(m, _scheduler(), lat0, cond.to(BF), pr.to(BF), ng.to(BF), img.to(BF), STEPS, G, use_graph=use_graph, region=cfg,
                   sparse_region=sparse, **kw).clone()


def C(*a, **kw):
    from chronoedit_amd.sparse_region import SparseRegionConfig
    return SparseRegionConfig(*a, **kw)


@pytest.fixture()
def captures(monkeypatch):
    """Records the hipGraph captures of the loop."""
    from chronoedit_amd import pipeline
    n, real = [], pipeline.GraphedDenoiser._capture
    monkeypatch.setattr(pipeline.GraphedDenoiser, "_capture", lambda self, kind="compute": (n.append((tuple(self.latents.shape), kind)), real(self, kind))[1])
    return n


@pytest.fixture(scope="module")
def dense_region_run():
    return _run(_model(), _inputs(), rect_mask())


def kept_cells_hold_the_source(out, mask, z):
    from chronoedit_amd import region
    keep = (region.latent_weights(mask) == 0).cuda()
    assert bool(keep.any()) and not bool(keep.all())
    return torch.equal(out[..., keep], z.cuda()[..., keep]) and not torch.equal(out[..., ~keep], z.cuda()[..., ~keep])


def test_refresh_every_1_is_the_dense_region_edit(dense_region_run):
    for use_graph in (False, True):
        m = _model()
        out = _run(m, _inputs(), rect_mask(), C(1), use_graph=use_graph)
        assert torch.equal(out, dense_region_run), use_graph
        assert m.sparse_report["plan"] == ["compute"] * STEPS and m.sparse_report["sparse"] == 0 and m.engine()._sparse is None
    # an all-255 mask: the whole grid is active, nothing is sparse whatever the config says
    full = torch.full((H, W), 255, dtype=torch.uint8)
    m = _model()
    assert torch.equal(_run(m, _inputs(), full, C(3)), _run(_model(), _inputs(), full))
    assert m.sparse_report["plan"] == ["compute"] * STEPS and m.sparse_report["active"] == N


@pytest.mark.parametrize("mask_name", ["rectangle", "feathered"])
def test_replay_equals_eager_and_kept_cells_end_on_the_source(mask_name, captures, dense_region_run):
    mask = rect_mask() if mask_name == "rectangle" else feathered_mask()
    inp = _inputs()
    m = _model()
    eager = _run(m, inp, mask, C(3))
    assert m.sparse_report["plan"] == ["refresh", "sparse", "sparse"] * 2, m.sparse_report
    assert m.sparse_report["active"] == active_ids(mask)[0].numel() and m.sparse_report["tokens"] == N
    assert torch.isfinite(eager).all() and kept_cells_hold_the_source(eager, mask, inp[5])
    if mask_name == "rectangle":  # sparse steps are another computation than dense ones - and not a far one
        assert not torch.equal(eager, dense_region_run)
        print(f"refresh_every=3 against the dense region edit: rel-L2 {rel_l2(eager.cpu(), dense_region_run.cpu()):.3e}")
    assert not captures
    replay = _run(_model(), inp, mask, C(3), use_graph=True)
    assert torch.equal(replay, eager), float((replay - eager).abs().max())
    kinds = [k for _, k in captures]
    assert sorted(kinds) == sorted(set(kinds)) and set(kinds) <= {"refresh", "sparse"}, captures  # at most one capture per kind


def test_truncation_steps_are_compute_and_the_rest_is_planned_on_two_frames(captures):
    inp, mask = _inputs(T=8), rect_mask()
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    m = _model()
    eager = _run(m, inp, mask, C(3), **kw)
    rep = m.sparse_report
    assert rep["plan"] == ["compute"] * 3 + ["refresh", "sparse", "sparse"] and rep["compute"] == 3 and rep["tokens"] == N and rep["active"] == 64
    assert tuple(m.engine()._sparse.k.shape) == (2, 2 * N, 256)  # the cache exists at the 2-frame shape only
    z2 = inp[5][:, :, [0, -1]]
    assert eager.shape[2] == 2 and torch.isfinite(eager).all() and kept_cells_hold_the_source(eager, mask, z2)
    assert not torch.equal(eager, _run(_model(), inp, mask, **kw))
    assert not captures
    replay = _run(_model(), inp, mask, C(3), use_graph=True, **kw)
    assert torch.equal(replay, eager), float((replay - eager).abs().max())
    assert len(set(captures)) == len(captures) and {k for _, k in captures} <= {"compute", "refresh", "sparse"}, captures


def test_a_callback_that_replaces_the_latents_forces_the_next_step_dense():
    outs = []
    for use_graph in (False, True):
        m = _model()
        out = _run(m, _inputs(), rect_mask(), C(3), use_graph=use_graph, on_step_end=lambda i, t, lat: lat * 0.5 if i == 1 else None)
        assert m.sparse_report["plan"] == ["refresh", "sparse", "compute", "refresh", "sparse", "sparse"], m.sparse_report
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_loop_refusals():
    from chronoedit_amd.guidance import GuidanceReuseConfig
    from chronoedit_amd.teacache import TeaCacheConfig
    inp, mask = _inputs(), rect_mask()
    with pytest.raises(ValueError, match="region"):
        _run(_model(), inp, None, C(3))
    for kw in (dict(teacache=TeaCacheConfig(rel_l1_thresh=0.1, coefficients=(1.0, 0.0))), dict(teacache_measure=True),
               dict(guidance_reuse=GuidanceReuseConfig(pair_every=2)), dict(guidance_measure=2)):
        with pytest.raises(ValueError):
            _run(_model(), inp, mask, C(3), **kw)
    m = _model().enable_teacache(0.1)
    with pytest.raises(ValueError):
        _run(m, inp, mask, C(3))
    m = _model().enable_guidance_reuse(2)
    with pytest.raises(ValueError):
        _run(m, inp, mask, C(3))
    for switch in (lambda x: x.enable_fp8_gemms(), lambda x: x.enable_fp8_attention(), lambda x: x.enable_transposed_v(False)):
        m = _model()
        switch(m)
        with pytest.raises(NotImplementedError):
            _run(m, inp, mask, C(3))
    m = _model()
    m._sp = types.SimpleNamespace(sharded=True, world=2, rank=0, capturable=False)
    with pytest.raises(NotImplementedError):
        _run(m, inp, mask, C(3))
    m._sp, m._cfgp = None, object()
    with pytest.raises(NotImplementedError):
        _run(m, inp, mask, C(3))


def test_a_second_edit_uses_its_own_mask_and_disable_restores_the_dense_edit(dense_region_run):
    inp = _inputs()
    other = torch.zeros((H, W), dtype=torch.uint8)
    other[80:128, 0:48] = 255  # the lower left corner
    m = _model()
    assert m.enable_sparse_region(3) is m  # the transformer-level switch: `denoise` picks it up
    first = _run(m, inp, rect_mask())
    assert m.sparse_report["sparse"] == 4 and torch.equal(first, _run(_model(), inp, rect_mask(), C(3)))
    second = _run(m, inp, other, use_graph=True)
    assert m.sparse_report["active"] == 32
    assert torch.equal(m.engine()._sparse.ids.cpu().long(), active_ids(other)[0])
    assert torch.equal(second, _run(_model(), inp, other, C(3)))
    assert kept_cells_hold_the_source(second, other, inp[5])
    # without a region the switch has no effect
    assert torch.equal(_run(m, inp, None), _run(_model(), inp, None)) and m.sparse_report is None
    assert m.disable_sparse_region() is m and m.engine()._sparse is None
    assert torch.equal(_run(m, inp, rect_mask()), dense_region_run) and m.sparse_report is None


# ----------------------------------------------------------------------------------------------------------------------------------
# the pipeline
# ----------------------------------------------------------------------------------------------------------------------------------
PH, PW = 64, 96


@pytest.fixture(scope="module")
def pipe():
    from transformers import CLIPImageProcessor

    from chronoedit_amd.clip_vision import CLIPVisionModel
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    from chronoedit_amd.vae import AutoencoderKLWan
    from oracle import vae_oracle as V
    dcfg = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320, added_kv_proj_dim=256)
    dp = D.make_synthetic_params(dcfg, dtype=BF)
    vp = V.make_synthetic_params(V.VAEConfig(dim=32, z_dim=16))
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in dp.items()})
    vae = AutoencoderKLWan({k: v.cuda() for k, v in vp.items()}, dim=32, z_dim=16)
    torch.manual_seed(0)
    ie = CLIPVisionModel(hidden_size=320, intermediate_size=640, num_hidden_layers=3, num_attention_heads=4, image_size=56, patch_size=14, device="cuda:0")
    proc = CLIPImageProcessor(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})
    return ChronoEditPipeline(image_encoder=ie, image_processor=proc, transformer=m, vae=vae,
                              scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers"))


def test_pipeline_sparse_edit_keeps_the_source_pixels_where_the_mask_is_0(pipe):
    rgb = np.random.default_rng(9).integers(0, 256, size=(70, 90, 3), dtype=np.uint8)
    image = Image.fromarray(rgb)
    source = np.asarray(image.convert("RGB").resize((PW, PH), Image.LANCZOS))
    mask = np.zeros((PH, PW), dtype=np.uint8)
    mask[16:48, 32:64] = 255  # 4 patches; 16 with the margin, of 24 per frame
    g = torch.Generator().manual_seed(5)
    kw = dict(prompt_embeds=torch.randn(1, 40, 128, generator=g).to(BF).cuda(), negative_prompt_embeds=torch.randn(1, 40, 128, generator=g).to(BF).cuda(),
              height=PH, width=PW, num_frames=5, num_inference_steps=3, guidance_scale=5.0)
    lat = torch.randn(1, 16, 2, PH // 8, PW // 8, generator=g).to(BF).float()
    call = lambda output_type="pil": pipe(image=image, **dict(kw, latents=lat.clone(), output_type=output_type)).frames
    frames_of = lambda fr: np.stack([np.stack([np.asarray(f) for f in sample]) for sample in fr])
    try:
        # the switch alone changes nothing
        plain = call("latent")
        assert pipe.enable_sparse_region(2) is pipe
        assert torch.equal(call("latent"), plain) and pipe.transformer.sparse_report is None
        pipe.set_edit_region(mask)
        frames = frames_of(call())
        rep = pipe.transformer.sparse_report
        assert rep["plan"] == ["refresh", "sparse", "compute"] and rep["active"] == 32 and rep["tokens"] == 48, rep
        keep = mask == 0
        for f in range(frames.shape[1]):
            assert np.array_equal(frames[0, f][keep], source[keep]), f  # the resized source's bytes, exactly, in every returned frame
        assert not np.array_equal(frames[0, -1][~keep], source[~keep])
        sparse_lat = call("latent")
        assert pipe.disable_sparse_region() is pipe
        dense_lat = call("latent")
        assert pipe.transformer.sparse_report is None and not torch.equal(sparse_lat, dense_lat) and torch.isfinite(sparse_lat).all()
        print(f"pipeline: sparse against dense region edit, rel-L2 of the latents {rel_l2(sparse_lat.cpu(), dense_lat.cpu()):.3e}")
    finally:
        pipe.disable_sparse_region()
        pipe.clear_edit_region()
