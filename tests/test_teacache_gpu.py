"""TeaCache step skipping on the device (csrc/ce_tea.hip, chronoedit_amd/teacache.py, the hooks in transformer.py / pipeline.py).

Kernels, element by element: the two token passes against (a.float() -+ b.float()).to(bfloat16), the reduction against float64 sums.
Plan: the engine's plan for a 50-step schedule against the reference's expression restated on CPU bf16 tensors.
Loop: an all-compute plan is bit-identical to the loop without TeaCache; a skipping loop against an fp32 oracle driven by the same
plan (bound: the one tests/test_pipeline_gpu.py::test_edit_end_to_end_vs_oracle holds the latents of this tiny model to, 6e-2 - a
skipped step does strictly less bf16 arithmetic than a computed one); hipGraph replay == eager with skips; state handling.
Shapes: the tiny model of tests/test_pipeline_gpu.py (2 heads x 128, 2 layers, ffn 512), latents 1 x 16 x T x 8 x 12."""
import types

import numpy as np
import pytest
import torch

from oracle import dit_oracle as D

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C, S = True, False
LOOP_PLAN = [C, S, S, C, S, C]            # constant-1 polynomial, threshold 2.5, 6 steps
LOOP_TEA = dict(rel_l1_thresh=2.5, coefficients=(1.0,))
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ----------------------------------------------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------------------------------------------
def _token_operands(count, seed):
    """Two bf16 vectors: random values over 40 binades, and - at fixed places - signed zeros, subnormals, pairs whose sum or difference
    lands on a rounding tie (both parities), and large values whose sum or difference overflows to inf (never inf - inf: every input is finite)."""
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(count, generator=g) * torch.exp2(torch.randint(-20, 21, (count,), generator=g).float())).to(BF)
    b = (torch.randn(count, generator=g) * torch.exp2(torch.randint(-20, 21, (count,), generator=g).float())).to(BF)
    big, sub = 3.0e38, 2.0 ** -130
    special = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (1.0, 2.0 ** -8), (1.0, -(2.0 ** -8)), (1.0078125, 2.0 ** -8), (1.0078125, -(2.0 ** -8)),
               (sub, 3 * sub), (-5 * sub, sub), (sub, -sub), (2.0 ** -126, -sub), (big, big), (big, -big), (-big, big), (-big, -big), (big, 2.0 ** 120)]
    for k, (va, vb) in enumerate(special):
        for pos in (k % count, count - 1 - k % count) if count > 2 * len(special) else ((k % count),):
            a[pos], b[pos] = va, vb
    return a, b


@pytest.mark.parametrize("count", [8, 256 * 97, 5120 * 192])
def test_token_passes_are_exact_in_place(count):
    from chronoedit_amd import ops
    a, b = _token_operands(count, count)
    want_sub = (a.float() - b.float()).to(BF)   # ce_tea_store_bf16: r <- x - r
    want_add = (a.float() + b.float()).to(BF)   # ce_tea_apply_bf16: x <- x + r
    assert not torch.isnan(want_sub.float()).any() and not torch.isnan(want_add.float()).any()
    if count > 64:
        assert torch.isinf(want_sub.float()).any() and torch.isinf(want_add.float()).any()
    x, r = a.cuda(), b.cuda()
    assert ops.tea_store_(x, r) is r
    assert torch.equal(r.cpu(), want_sub), int((r.cpu() != want_sub).sum())
    assert torch.equal(x.cpu(), a)  # the other operand is only read
    x, r = a.cuda(), b.cuda()
    assert ops.tea_apply_(x, r) is x
    assert torch.equal(x.cpu(), want_add), int((x.cpu() != want_add).sum())
    assert torch.equal(r.cpu(), b)


def test_token_passes_refuse_counts_that_are_no_multiple_of_8():
    from chronoedit_amd import ops
    x, r = torch.zeros(16, dtype=BF, device="cuda"), torch.ones(16, dtype=BF, device="cuda")
    lib = ops.lib()
    for n in (12, 1, 7):
        assert lib.ce_tea_store_bf16(ops._ptr(x), ops._ptr(r), n, ops._stream()) == -2
        assert lib.ce_tea_apply_bf16(ops._ptr(x), ops._ptr(r), n, ops._stream()) == -2
    assert lib.ce_tea_store_bf16(ops._ptr(x), ops._ptr(r), 0, ops._stream()) == -1
    assert lib.ce_tea_apply_bf16(ops._ptr(x[1:]), ops._ptr(r), 8, ops._stream()) == -3  # x not 16-byte aligned
    with pytest.raises(ops.HipKernelError, match="unsupported shape"):
        ops.tea_store_(x[:12], r[:12])
    torch.cuda.synchronize()
    assert float(x.float().abs().sum()) == 0 and float(r.float().sum()) == 16  # nothing was written


@pytest.mark.parametrize("n", [1536, 30720])
@pytest.mark.parametrize("S_", [1, 2, 7])
def test_rel_l1_sums_are_exact_on_exactly_summable_rows(S_, n):
    """Integers in [-8, 8] times 2^-3: every difference is a bf16 value, every partial sum a multiple of 2^-3 below 2^24 units - the
    fp32 accumulators hold the float64 answer whatever the order of summation."""
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(S_ * 100000 + n)
    rows = (torch.randint(-8, 9, (S_, n), generator=g).float() * 0.125).to(BF)
    want = torch.zeros(S_, 2, dtype=torch.float64)
    for i in range(1, S_):
        want[i, 0] = (rows[i].double() - rows[i - 1].double()).abs().sum()
        want[i, 1] = rows[i - 1].double().abs().sum()
    out = torch.full((S_, 2), -1.0, dtype=torch.float32, device="cuda")
    ops.tea_rel_l1(rows.cuda(), out=out)
    assert torch.equal(out.cpu().double(), want), (out.cpu(), want)


@pytest.mark.parametrize("n", [1536, 30720])
def test_rel_l1_sums_of_random_rows_are_within_the_fp32_bound_and_repeatable(n):
    """n non-negative fp32 summands in any order: within n 2^-24 relative of the exact sum (9.2e-5 at n = 1536).  The summands of the
    first column are |bf16(a - b)|: the reference subtracts bf16 tensors."""
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(n)
    S_ = 5
    rows = (torch.randn(S_, n, generator=g) * torch.exp2(torch.randint(-3, 4, (S_, 1), generator=g).float())).to(BF)
    dev = rows.cuda()
    out = ops.tea_rel_l1(dev).cpu().double()
    again = ops.tea_rel_l1(dev)
    assert torch.equal(again.cpu().double(), out)  # fixed reduction order: bit-identical from run to run
    assert out[0].abs().sum() == 0
    bound = n * 2.0 ** -24
    for i in range(1, S_):
        d = (rows[i] - rows[i - 1]).abs().double().sum()  # a bf16 difference, summed exactly
        p = rows[i - 1].abs().double().sum()
        e0, e1 = abs(float(out[i, 0] - d) / float(d)), abs(float(out[i, 1] - p) / float(p))
        print(f"rel_l1 n={n} row {i}: relative error {e0:.2e} / {e1:.2e} (bound {bound:.2e})")
        assert e0 <= bound and e1 <= bound, (i, e0, e1, bound)
    with pytest.raises(ops.HipKernelError, match="unsupported shape"):
        ops.tea_rel_l1(torch.zeros(2, 12, dtype=BF, device="cuda"))


# ----------------------------------------------------------------------------------------------------------------------------------
# model, inputs, loops
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


def _inputs(T=2, seed=1):
    """bf16-representable (lat0, cond, prompt, negative, img) on the CPU in fp32."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    return r(1, 16, T, 8, 12), r(1, 20, T, 8, 12), r(1, 40, 128), r(1, 40, 128), r(1, 257, 64)


def _run(m, inp, use_graph=False, steps=6, **kw):
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    lat0, cond, pr, ng, img = inp
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    return denoise(m, sch, lat0.cuda(), cond.cuda().to(BF), pr.cuda().to(BF), ng.cuda().to(BF), img.cuda().to(BF), steps, 5.0,
                   use_graph=use_graph, **kw).clone()


@pytest.fixture(scope="module")
def off_run():
    """The loop without TeaCache on the shared inputs (eager; tests/test_pipeline_gpu.py holds graphed == eager)."""
    return _run(_model(), _inputs())


def test_plan_equals_the_reference_rule_restated_on_cpu_bf16_tensors():
    """wan_video_new_chronoedit.py:1211-1231 on the engine's own time projections of a 50-step schedule: every ratio within one bf16 ulp
    (torch's mean may sum in another order), and - with a threshold no accumulated value comes near - the same plan."""
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    m = _model()
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    sch.set_timesteps(50, device="cuda:0")
    n_steps = len(sch.timesteps)
    rows = m.engine().tea_tproj_rows(sch.timesteps).cpu()
    assert rows.dtype == BF and rows.shape == (n_steps, 6 * 256)
    got = m.teacache_ratios(sch.timesteps)
    coef = (1.0, 0.0)
    want = [0.0]
    for i in range(1, n_steps):
        a, b = rows[i], rows[i - 1]
        want.append(((a - b).abs().mean() / b.abs().mean()).item())
        assert abs(got[i] - want[i]) <= 2.0 ** -8 * abs(want[i]), (i, got[i], want[i])
    rescale = np.poly1d(coef)

    def restated(thresh):
        acc, plan, seen = 0.0, [], []
        for i in range(n_steps):
            if i == 0 or i == n_steps - 1:
                calc, acc = True, 0.0
            else:
                acc += rescale(want[i])
                seen.append(acc)
                calc = not acc < thresh
                if calc:
                    acc = 0.0
            plan.append(calc)
        return plan, seen

    run = np.cumsum(want[1:])
    for k in range(1, 8):  # midway between two adjacent accumulated values; the first candidate that nothing comes near
        thresh = 0.5 * (run[k] + run[k + 1])
        plan, seen = restated(thresh)
        if all(abs(a - thresh) > 2.0 ** -7 * thresh for a in seen):
            break
    else:
        pytest.fail("no threshold candidate clear of every accumulated value")
    assert all(abs(a - thresh) > 2.0 ** -7 * thresh for a in seen)
    assert plan.count(False) >= 1 and plan.count(True) >= 3, plan  # (both kinds of step occur)
    m.enable_teacache(thresh, coef)
    assert m.teacache_plan(sch.timesteps) == plan


def test_all_compute_plan_is_bit_identical_to_the_loop_without_teacache(off_run):
    m = _model()
    m.enable_teacache(0.5, (1.0,))
    for use_graph in (False, True):
        out = _run(m, _inputs(), use_graph=use_graph)
        assert m.teacache_report["plan"] == [C] * 6 and m.teacache_report["skipped"] == 0
        assert torch.equal(out, off_run), (use_graph, float((out - off_run).abs().max()))


def _oracle_loop_with_plan(inp, plan, steps=6, guidance=5.0):
    """The reference loop in fp32 with TeaCache's store / update around the block stack (wan_video_new_chronoedit.py:1233-1239), one
    residual per guidance branch, composed from oracle/dit_oracle.py: taps["patch"], taps["blocks.{L-1}.out"], and the head of
    dit_forward (condition_embed's temb, fp32_layer_norm, linear, the un-patching permutation)."""
    from oracle.unipc_oracle import UniPCOracle
    cfg = DCFG
    p = {k: v.float() for k, v in _PARAMS["p"].items()}
    lat, cond, pr, ng, img = inp
    sch = UniPCOracle()
    sch.set_timesteps(steps, shift=5.0)
    last = f"blocks.{cfg.num_layers - 1}.out"
    res = {}

    def head(x, ts, text, B, T, Hh, Ww):
        temb = D.condition_embed(p, cfg, ts, text, img)[0]
        shift, scale = (p["scale_shift_table"] + temb.unsqueeze(1)).chunk(2, dim=1)
        x = (D.fp32_layer_norm(x.float(), None, None, cfg.eps) * (1 + scale) + shift).type_as(x)
        x = D.linear(x, p, "proj_out")
        pt, ph, pw = cfg.patch_size
        x = x.reshape(B, T // pt, Hh // ph, Ww // pw, pt, ph, pw, -1).permute(0, 7, 1, 4, 2, 5, 3, 6)
        return x.flatten(6, 7).flatten(4, 5).flatten(2, 3)

    with torch.no_grad():
        for i, t in enumerate(sch.timesteps):
            x_in = torch.cat([lat, cond], dim=1)
            ts = t.expand(1)
            outs = {}
            for name, text in (("c", pr), ("u", ng)):
                taps = {}
                full = D.dit_forward(p, cfg, x_in, ts, text, img, taps=taps)
                if plan[i]:
                    res[name] = taps[last] - taps["patch"]
                    outs[name] = full
                    assert torch.equal(head(taps[last], ts, text, *x_in.shape[:1], *x_in.shape[2:]), full)  # the composed head IS dit_forward's
                else:
                    outs[name] = head(taps["patch"] + res[name], ts, text, *x_in.shape[:1], *x_in.shape[2:])
            lat = sch.step(outs["u"] + guidance * (outs["c"] - outs["u"]), lat)
    return lat.float()


def test_skipping_loop_vs_fp32_oracle_with_the_same_plan(off_run):
    m = _model()
    m.enable_teacache(**LOOP_TEA)
    out = _run(m, _inputs())
    assert m.teacache_report["plan"] == LOOP_PLAN and m.teacache_report["computed"] == 3 and m.teacache_report["skipped"] == 3
    assert len(m.teacache_report["ratios"]) == 6
    ref = _oracle_loop_with_plan(_inputs(), LOOP_PLAN)
    e, moved = rel_l2(out, ref), rel_l2(out, off_run)
    print(f"TeaCache C S S C S C: final latents rel-L2 vs the fp32 oracle with the same plan {e:.3e}; vs the loop without TeaCache {moved:.3e}")
    assert torch.isfinite(out).all()
    assert e < 6e-2, e
    assert not torch.equal(out, off_run) and moved > 0  # the plan really skipped


def test_hipgraph_replay_equals_eager_with_skipped_steps():
    m = _model()
    m.enable_teacache(**LOOP_TEA)
    outs = [_run(m, _inputs(), use_graph=g) for g in (False, True)]
    assert m.teacache_report["plan"] == LOOP_PLAN
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    # temporal reasoning: the truncation step (8 -> 2 latent frames) is forced to compute - the 8-frame residual does not fit
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    outs = [_run(m, _inputs(T=8), use_graph=g, **kw) for g in (False, True)]
    assert m.teacache_report["plan"] == [C, S, C, S, S, C]
    assert outs[0].shape == (1, 16, 2, 8, 12)
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


def test_fp8_gemms_replay_skipped_steps():
    m = _model()
    m.enable_fp8_gemms(policy="fast")
    m.enable_teacache(**LOOP_TEA)
    try:
        m.engine()
    except NotImplementedError as e:  # fp8 GEMMs need inner and ffn dims that are multiples of 256
        pytest.skip(str(e))
    outs = [_run(m, _inputs(), use_graph=g) for g in (False, True)]
    assert m.teacache_report["plan"] == LOOP_PLAN
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())


# ----------------------------------------------------------------------------------------------------------------------------------
# state
# ----------------------------------------------------------------------------------------------------------------------------------
def test_disable_teacache_restores_the_plain_loop(off_run):
    m = _model()
    m.enable_teacache(**LOOP_TEA)
    skipped = _run(m, _inputs(), use_graph=True)
    assert not torch.equal(skipped, off_run)
    m.disable_teacache()
    for use_graph in (False, True):
        assert torch.equal(_run(m, _inputs(), use_graph=use_graph), off_run)


def test_a_second_edit_does_not_see_the_first_edits_residual():
    first, second = _inputs(seed=1), _inputs(seed=2)
    fresh = []
    for inp in (first, second):
        m = _model()
        m.enable_teacache(**LOOP_TEA)
        fresh.append(_run(m, inp))
    m = _model()
    m.enable_teacache(**LOOP_TEA)
    warm = set()
    for use_graph in (False, True):
        assert torch.equal(_run(m, first, use_graph=use_graph, graph_warm=warm), fresh[0])
        assert torch.equal(_run(m, second, use_graph=use_graph, graph_warm=warm), fresh[1])
    eng = m.engine()
    assert eng._tea_res is not None and eng._tea_res.shape == (2 * 48, 256)  # one buffer covers the guidance pair
    # a TeaCacheConfig handed to the loop works without enable_teacache()
    from chronoedit_amd.teacache import TeaCacheConfig
    m2 = _model()
    assert torch.equal(_run(m2, first, teacache=TeaCacheConfig(**LOOP_TEA)), fresh[0])
    assert m2.teacache_report["plan"] == LOOP_PLAN


def test_a_direct_forward_runs_the_whole_model_while_teacache_is_enabled():
    lat0, cond, pr, _, img = _inputs()
    x = torch.cat([lat0, cond], dim=1).cuda().to(BF)
    ts = torch.tensor([500], device="cuda:0")
    plain = _model()(x, ts, pr.cuda().to(BF), img.cuda().to(BF), return_dict=False)[0]
    m = _model()
    m.enable_teacache(**LOOP_TEA)
    assert torch.equal(m(x, ts, pr.cuda().to(BF), img.cuda().to(BF), return_dict=False)[0], plain)
    _run(m, _inputs())  # ends on a computed step; the loop leaves no mode behind
    assert m._tea_mode is None
    assert torch.equal(m(x, ts, pr.cuda().to(BF), img.cuda().to(BF), return_dict=False)[0], plain)


def test_skip_mode_without_a_residual_raises():
    lat0, cond, pr, _, img = _inputs()
    x = torch.cat([lat0, cond], dim=1).cuda().to(BF)
    ts = torch.tensor([500], device="cuda:0")
    m = _model()
    m.enable_teacache(**LOOP_TEA)
    m._tea_mode = "skip"
    with pytest.raises(RuntimeError, match="residual"):
        m(x, ts, pr.cuda().to(BF), img.cuda().to(BF), return_dict=False)
    # a residual of another row count (the guidance pair's, 96 rows) does not serve a single sample (48 rows) either
    m._tea_mode = None
    _run(m, _inputs())
    m._tea_mode = "skip"
    with pytest.raises(RuntimeError, match="residual"):
        m(x, ts, pr.cuda().to(BF), img.cuda().to(BF), return_dict=False)
    m._tea_mode = None


def test_sharded_transformer_with_teacache_is_refused():
    m = _model()
    m.enable_teacache(**LOOP_TEA)
    m._sp = types.SimpleNamespace(sharded=True, world=2, rank=0, capturable=False)  # (no process group: the loop must refuse before any forward)
    with pytest.raises(NotImplementedError, match="TeaCache"):
        _run(m, _inputs())
    m._sp = None
    m._cfgp = object()
    with pytest.raises(NotImplementedError, match="TeaCache"):
        _run(m, _inputs())
