"""The guidance pair's common work run once (ChronoEditTransformer3DModel.enable_shared_guidance, pipeline._shared_inputs).

Kernel level: the two-segment V^T attention with a shared Q and a shared image segment, and the GEMM's residual row period, against the
existing entry points fed physically duplicated operands - bit-equal (same products, same order).
Engine level, on the miniature widths of the suite (2 heads x 128, ffn 512) with 2 layers (block 1 runs the ordinary path behind a shared
block 0), N = 288 tokens (one full 256-row query block + a 32-row remainder), 128 text keys (two key tiles), 257 image keys (4 tiles + 1):
  * block 0's stream in front of its cross-attention, shared mode, is bit-equal to a B = 1 forward's (same M, same tiles);
  * forward and step, shared against stacked (the A/B switch): bounded by twice the distance between the parent commit's batched B = 2
    forward and its two B = 1 forwards on these inputs, which differ for the same reason (GEMMs at M = N instead of 2 N).  Measured on the
    parent commit on MI355X with exactly these shapes and inputs: rel-L2 0.0 (max abs 0.0) for the forward and 0.0 for the step's latents
    (batched against sequential guidance).  The reason: at these widths every GEMM (M N < 256 x 256 x 128) runs the 128-row-tile kernel,
    which has no split-K and whose sum per output element does not depend on M, and the row and attention kernels work row by row.  Twice
    0.0 is 0.0: the tests assert bit equality of shared against stacked.  (At the full width the dispatcher does change tiles between
    M = 7 200 and 14 400; that distance is what the bench's --dump-outputs comparison shows.)  Both modes stay inside the suite's 2e-2
    rel-L2 bound against the fp32 oracle (measured: 5.1e-3 each);
  * a hipGraph replay of the loop in shared mode, with a TeaCache plan that skips and the 8 -> 2 frame truncation, is bit-equal to the eager loop;
  * a plain forward() with two different latents in the batch is untouched by the switch (nothing is shared unless the loop declares it)."""
import pytest
import torch

from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
HW = 24           # latent height = width: 12 x 12 patches per frame, N = 288 at T = 2
TT, TI = 128, 257
# rel-L2 between the parent commit's batched B = 2 forward (step) and its two B = 1 forwards (sequential step) on the inputs below, measured on MI355X (module docstring)
PARENT_B2_VS_B1_FORWARD = 0.0
PARENT_B2_VS_B1_STEP = 0.0
ORACLE_BOUND = 2e-2  # tests/test_dit_forward_gpu.py's bound for the bf16 path against the fp32 oracle


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rand(g, *s, scale=1.0):
    return (torch.randn(*s, generator=g) * scale).to(BF)


# ----------------------------------------------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share_q,share1,share2", [(True, False, True), (False, False, True), (True, True, True), (False, True, False)])
def test_attention_shared_operands_equal_duplicated_operands(share_q, share1, share2):
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(7)
    H, nq, B = 2, 288, 2
    Dm = H * 128
    c1, c2 = TT, (TI + 7) // 8 * 8
    pad = lambda n: (n + 63) // 64 * 64
    q = _rand(g, B * nq, Dm)
    k1, k2 = _rand(g, B * TT, Dm), _rand(g, B * TI, Dm)
    v1t = torch.zeros(Dm, (B - 1) * c1 + pad(TT), dtype=BF)
    v2t = torch.zeros(Dm, (B - 1) * c2 + pad(TI), dtype=BF)
    for b in range(B):
        v1t[:, b * c1: b * c1 + TT] = _rand(g, Dm, TT)
        v2t[:, b * c2: b * c2 + TI] = _rand(g, Dm, TI)
    if share_q:
        q[nq:] = q[:nq]
    if share1:
        k1[TT:] = k1[:TT]
        v1t[:, c1: c1 + TT] = v1t[:, :TT]
    if share2:
        k2[TI:] = k2[:TI]
        v2t[:, c2: c2 + TI] = v2t[:, :TI]
    q, k1, k2, v1t, v2t = (t.cuda() for t in (q, k1, k2, v1t, v2t))
    want = ops.attention_2seg_vt(q, k1, v1t, TT, k2, v2t, TI, H, batch=B, cols1=c1, cols2=c2)
    s1 = v1t[:, : pad(TT)].contiguous() if share1 else v1t
    s2 = v2t[:, : pad(TI)].contiguous() if share2 else v2t
    out = torch.full((B * nq, Dm), float("nan"), dtype=BF, device="cuda")
    ops.attention_2seg_vt_shared(q[:nq] if share_q else q, k1[:TT] if share1 else k1, s1, TT, k2[:TI] if share2 else k2, s2, TI, H, out=out,
                                 batch=B, share_q=share_q, share1=share1, share2=share2, cols1=None if share1 else c1, cols2=None if share2 else c2)
    assert torch.equal(out.cpu(), want.cpu()), int((out != want).sum())
    assert float(want.float().abs().max()) > 0


def test_attention_strides_are_validated():
    from chronoedit_amd import ops
    z = torch.zeros(64, 256, dtype=BF, device="cuda")
    vt = torch.zeros(256, 128, dtype=BF, device="cuda")
    o = torch.zeros(128, 256, dtype=BF, device="cuda")
    args = lambda qr, k1r, k2r: (ops._ptr(z), ops._ptr(z), ops._ptr(vt), 32, 256, 128, 32, ops._ptr(z), ops._ptr(vt), 32, 256, 128, 32, ops._ptr(o), 64, 2,
                                 128, 256, 256, 0.1, 2, qr, k1r, k2r, ops._stream())
    lib = ops.lib()
    assert lib.ce_attention_2seg_vt_strided_bf16(*args(32, 0, 0)) == -2   # a Q stride below Nq
    assert lib.ce_attention_2seg_vt_strided_bf16(*args(0, 16, 0)) == -2   # a K stride below len
    assert lib.ce_attention_2seg_vt_strided_bf16(*args(0, 0, 0)) == 0
    torch.cuda.synchronize()


# (M, N, K, res_rows, forced kernel; -1 = the dispatcher's choice): the 384-, 288- and 256-row tiles (one-wave-per-SIMD and 8-wave) with period
# boundaries at rows 500 and 1000, inside a tile of each; 270 / 287 tiles on 256 CUs with 16 K-tiles - a last round that is cut along K (fp32
# slabs + the reduce launch); a large product as dispatched; a period shorter than the 384- / 256-row tile forced (their launchers hand it to the 8-wave kernel); small products (the 128-row kernel)
@pytest.mark.parametrize("M,N,K,rr,variant", [(1152, 512, 256, 500, 6), (1152, 512, 256, 500, 7), (1152, 512, 256, 500, 4), (1152, 512, 256, 500, 1),
                                               (10368, 2560, 1024, 5184, 6), (10368, 1792, 1024, 5184, 4), (7200, 5120, 256, 3600, -1),
                                               (1000, 512, 128, 200, 6), (1000, 512, 128, 200, 4), (1000, 512, 128, 200, -1), (576, 256, 256, 288, -1)])
def test_gemm_residual_period_equals_duplicated_residual(M, N, K, rr, variant):
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    a, w = _rand(g, M, K).cuda(), _rand(g, N, K, scale=K ** -0.5).cuda()
    bias = torch.randn(N, generator=g).cuda()
    gate = torch.randn((M + rr - 1) // rr, N, generator=g).cuda()
    res = _rand(g, rr, N).cuda()
    dup = res.repeat((M + rr - 1) // rr, 1)[:M].contiguous()
    old = ops.set_gemm_variant(variant) if variant != -1 else None
    try:
        for gt, gr in ((None, 0), (gate, rr)):
            want = ops.gemm(a, w, bias, epilogue=ops.EPI_GATE_RES, gate=gt, res=dup, gate_rows=gr)
            out = ops.gemm(a, w, bias, epilogue=ops.EPI_GATE_RES, gate=gt, res=res, gate_rows=gr, res_rows=rr)
            assert torch.equal(out.cpu(), want.cpu()), (gr, int((out != want).sum()))
    finally:
        if old is not None:
            ops.set_gemm_variant(old)
    with pytest.raises(ValueError, match="overlap"):
        ops.gemm(a, w[:, :K], bias, out=dup, epilogue=ops.EPI_GATE_RES, res=dup[:rr], res_rows=rr)


# ----------------------------------------------------------------------------------------------------------------------------------
# engine
# ----------------------------------------------------------------------------------------------------------------------------------
_PARAMS = {}


def _model():
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    if "p" not in _PARAMS:
        _PARAMS["p"] = D.make_synthetic_params(DCFG, dtype=BF)
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in _PARAMS["p"].items()})
    return m


def _inputs(T=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF)
    return r(1, 16, T, HW, HW).float(), r(1, 20, T, HW, HW), r(1, TT, 128), r(1, TT, 128), r(1, TI, 64)


def _pair_forward(m, inp, declare, tap=None):
    """One batched guidance forward the way denoise_step builds it; declare = the loop's per-call declaration."""
    from chronoedit_amd import pipeline
    lat, cond, pr, ng, img = (t.cuda() for t in inp)
    x = torch.cat([lat.to(BF), cond], 1)
    text2, image2 = pipeline.make_cfg_inputs(pr, ng, img)
    ts = torch.tensor([500, 500], device="cuda")
    m.engine()._tap = tap
    try:
        if declare:
            with pipeline._shared_inputs(m):
                out = m(torch.cat([x, x], 0), ts, text2, image2, return_dict=False)[0]
        else:
            out = m(torch.cat([x, x], 0), ts, text2, image2, return_dict=False)[0]
    finally:
        m.engine()._tap = None
    assert m._shared_inputs is None
    return out


@pytest.fixture(scope="module")
def forwards():
    """(shared, stacked, taps of the shared run) on the module's inputs - computed once."""
    inp = _inputs()
    m = _model()
    tap = {}
    on = _pair_forward(m, inp, True, tap).clone()
    m.enable_shared_guidance(False)
    off = _pair_forward(m, inp, True).clone()
    return inp, on, off, tap


def test_prefix_is_bit_equal_to_a_single_sample_forward(forwards):
    inp, _, _, tap = forwards
    assert tap["x_pre_cross0"].shape == (288, 256)  # one sample's rows: the prefix ran on N rows
    m = _model()
    lat, cond, pr, ng, img = (t.cuda() for t in inp)
    one = {}
    m.engine()._tap = one
    m(torch.cat([lat.to(BF), cond], 1), torch.tensor([500], device="cuda"), pr, img, return_dict=False)
    m.engine()._tap = None
    assert torch.equal(one["x_pre_cross0"].cpu(), tap["x_pre_cross0"].cpu())


def test_forward_shared_vs_stacked_and_both_vs_oracle(forwards):
    inp, on, off, _ = forwards
    d = rel_l2(on, off)
    print(f"forward: shared vs stacked rel-L2 {d:.3e} (bound {2 * PARENT_B2_VS_B1_FORWARD:.3e})")
    lat, cond, pr, ng, img = (t.float() for t in inp)
    p = {k: v.float() for k, v in _PARAMS["p"].items()}
    x = torch.cat([lat, cond], 1)
    with torch.no_grad():
        ref = torch.cat([D.dit_forward(p, DCFG, x, torch.tensor([500]), t, img) for t in (pr, ng)], 0)
    e_on, e_off = rel_l2(on, ref), rel_l2(off, ref)
    print(f"forward vs fp32 oracle: shared {e_on:.3e}, stacked {e_off:.3e} (bound {ORACLE_BOUND:.1e})")
    assert d <= 2 * PARENT_B2_VS_B1_FORWARD, d
    assert e_on < ORACLE_BOUND and e_off < ORACLE_BOUND, (e_on, e_off)
    assert rel_l2(on[:1], on[1:]) > 1e-3  # the two samples do differ (their text contexts do)


def _step(m, inp, **kw):
    from chronoedit_amd.pipeline import denoise_step
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    lat, cond, pr, ng, img = (t.cuda() for t in inp)
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    sch.set_timesteps(4, device="cuda:0")
    lat = lat.clone()
    denoise_step(m, sch, lat, cond, sch.timesteps[0], pr, ng, img, 5.0, **kw)
    return lat


def test_step_shared_vs_stacked():
    inp = _inputs()
    m = _model()
    tap = {}
    m.engine()._tap = tap
    on = _step(m, inp)
    assert tap["x_pre_cross0"].shape == (288, 256)  # denoise_step declared the pair: block 0's prefix ran on one sample's rows
    m.enable_shared_guidance(False)
    off = _step(m, inp)
    assert tap["x_pre_cross0"].shape == (576, 256)  # the A/B switch: the stacked sequence
    m.engine()._tap = None
    d = rel_l2(on, off)
    print(f"step: shared vs stacked latents rel-L2 {d:.3e} (bound {2 * PARENT_B2_VS_B1_STEP:.3e})")
    assert d <= 2 * PARENT_B2_VS_B1_STEP, d
    assert torch.isfinite(on).all()


def test_graphed_loop_with_skips_and_truncation_is_bit_equal_to_eager():
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    lat, cond, pr, ng, img = (t.cuda() for t in _inputs(T=8))
    outs = []
    for use_graph in (False, True):
        m = _model()
        m.enable_teacache(rel_l1_thresh=2.5, coefficients=(1.0,))  # constant-1 polynomial: skips two of every three free steps
        tap = {}
        m.engine()._tap = tap  # (eager forwards only: with use_graph the first step of each shape, which GraphedDenoiser runs un-captured)
        out = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat.clone(), cond, pr, ng, img, 7, 5.0, enable_temporal_reasoning=True,
                      num_temporal_reasoning_steps=4, use_graph=use_graph)
        m.engine()._tap = None
        assert tap["x_pre_cross0"].shape == (288, 256), (use_graph, tap["x_pre_cross0"].shape)  # the loop declared the pair (2 frames: N = 288, not 2 N)
        plan = m.teacache_report["plan"]
        assert plan[4] and m.teacache_report["skipped"] >= 2 and not all(plan[:4]) and not all(plan[4:]), plan  # skips at both shapes
        assert out.shape[2] == 2 and m._shared_inputs is None
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    assert torch.isfinite(outs[0]).all()


def test_plain_forward_with_two_different_latents_never_shares():
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).cuda()
    x, text, image = r(2, 36, 2, HW, HW), r(2, TT, 128), r(2, TI, 64)
    ts = torch.tensor([300, 700], device="cuda")
    m = _model()
    a = m(x, ts, text, image, return_dict=False)[0].clone()  # the switch at its default (on), nothing declared
    m.enable_shared_guidance(False)
    b = m(x, ts, text, image, return_dict=False)[0]
    assert torch.equal(a, b)
    p = {k: v.float() for k, v in _PARAMS["p"].items()}
    with torch.no_grad():
        ref = D.dit_forward(p, DCFG, x.float().cpu(), ts.cpu(), text.float().cpu(), image.float().cpu())
    assert rel_l2(a, ref) < ORACLE_BOUND
