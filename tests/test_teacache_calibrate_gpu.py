"""TeaCache calibration on the device: ce_tea_store_dist_bf16 (csrc/ce_tea.hip), the "measure" mode of the engine, `denoise(teacache_measure=True)`
and `calibrate_teacache`.

Kernel: the residual against ops.tea_store_ bit for bit; the two distance sums against integer arithmetic on exactly summable data and
against float64 within a bound derived from the kernel's summation structure; argument errors.
Loop: a measured edit leaves the plain loop's latents; its distances against float64 over snapshots of the engine's residual; the
temporal-reasoning truncation; calibrate -> enable -> edit end to end; what is refused.
Shapes: the tiny model of tests/test_teacache_gpu.py (2 heads x 128, 2 layers, ffn 512), latents 1 x 16 x T x 8 x 12."""
import math
import types

import pytest
import torch

from oracle import dit_oracle as D
from oracle import vae_oracle as V

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U = 2.0 ** -24  # unit roundoff of fp32
TAIL, PAIRED, MANY = 8, 256 * 97, 5120 * 192
CAPPED = 8 * (2 * 2048 * 256 + 3 * 256 + 5)  # the 2048-workgroup cap: the paired loop runs once, then a ragged tail (17 MB per operand)
DCFG = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)


# ----------------------------------------------------------------------------------------------------------------------------------
# kernel
# ----------------------------------------------------------------------------------------------------------------------------------
def _wide_operands(count, seed):
    """Three bf16 vectors over 40 binades; at fixed places signed zeros, subnormals, rounding ties of x - r and differences that overflow."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: (torch.randn(count, generator=g) * torch.exp2(torch.randint(-20, 21, (count,), generator=g).float())).to(BF)
    x, r, prev = rnd(), rnd(), rnd()
    big, sub = 3.0e38, 2.0 ** -130
    special = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (1.0, -(2.0 ** -8)), (1.0078125, -(2.0 ** -8)), (sub, 3 * sub), (2.0 ** -126, -sub), (big, -big)]
    for k, (vx, vr) in enumerate(special):
        x[k % count], r[k % count] = vx, vr
    return x, r, prev


@pytest.mark.parametrize("count", [TAIL, PAIRED, MANY, CAPPED])
def test_store_part_is_bit_identical_to_tea_store(count):
    from chronoedit_amd import ops
    x, r, prev = _wide_operands(count, count)
    xd, pd = x.cuda(), prev.cuda()
    want = ops.tea_store_(xd, r.cuda())
    got = r.cuda()
    sums = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    assert ops.tea_store_dist_(xd, got, pd, sums) is got
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(xd.cpu(), x) and torch.equal(pd.cpu(), prev)  # both are only read
    assert not (sums == -1.0).any()  # both sums were written


@pytest.mark.parametrize("count", [TAIL, PAIRED, MANY])
def test_sums_are_exact_on_exactly_summable_data(count):
    """Multiples of 0.5 up to 4 in magnitude, three in four of them zero: x - r is a bf16 value, every |r_new - prev| and |prev| a multiple of
    0.5, and each total stays below 2^24 half-units - every fp32 partial sum is exact whatever the order."""
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(count + 1)
    half = lambda: torch.randint(-8, 9, (count,), generator=g) * (torch.rand(count, generator=g) < 0.25)  # int64 half-units
    X, R, P = half(), half(), half()
    want = [int((X - R - P).abs().sum()), int(P.abs().sum())]
    assert max(want) < 2 ** 24 and (count == TAIL or min(want) > 0), want
    to_bf = lambda h: (h.float() * 0.5).to(BF).cuda()
    r = to_bf(R)
    sums = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    ops.tea_store_dist_(to_bf(X), r, to_bf(P), sums)
    assert torch.equal(r.cpu().float() * 2, (X - R).float())
    got = (sums.cpu().double() * 2).tolist()
    assert got == [float(w) for w in want], (got, want)


def _summation_depth(count):
    """The most fp32 roundings between an element and the result (csrc/ce_tea.hip): a lane adds its 8 elements per 16-byte vector one by one
    over its ceil(vectors / threads) vectors; 6 butterfly levels join the 64 lanes of a wave; 3 additions join the 4 waves in order; the
    finishing launch gives lane l the workgroup partials l, l + 64, ... to add one by one and joins its 64 lanes with 6 more levels."""
    nv = count // 8
    blocks = min(2048, -(-nv // 256))
    return 8 * -(-nv // (blocks * 256)) + 6 + 3 + -(-blocks // 64) + 6


@pytest.mark.parametrize("count", [PAIRED, CAPPED])
def test_sums_of_random_data_are_within_the_fp32_bound_and_repeatable(count):
    """Non-negative terms added in fp32 through at most k roundings each: |error| <= k u / (1 - k u) * sum of the terms (u = 2^-24).  k is
    _summation_depth for sum |prev| (its terms are exact) and one more for sum |r_new - prev|, whose every term is one fp32 subtraction."""
    from chronoedit_amd import ops
    assert (_summation_depth(PAIRED), _summation_depth(CAPPED)) == (8 + 6 + 3 + 1 + 6, 24 + 6 + 3 + 32 + 6)
    g = torch.Generator().manual_seed(count)
    x, r, prev = (torch.randn(count, generator=g).to(BF) for _ in range(3))
    r_new = (x.float() - r.float()).to(BF)
    want = [float((r_new.double() - prev.double()).abs().sum()), float(prev.double().abs().sum())]
    xd, pd = x.cuda(), prev.cuda()
    runs = []
    for _ in range(2):
        rd, sums = r.cuda(), torch.zeros(2, dtype=torch.float32, device="cuda")
        ops.tea_store_dist_(xd, rd, pd, sums)
        assert torch.equal(rd.cpu(), r_new)
        runs.append(sums.cpu())
    assert torch.equal(runs[0], runs[1])  # a fixed order of summation: the same bits on every run
    for k, name in enumerate(("sum |r_new - prev|", "sum |prev|")):
        depth = _summation_depth(count) + (1 if k == 0 else 0)
        bound = depth * U / (1 - depth * U)
        err = abs(float(runs[0][k].double()) - want[k]) / want[k]
        print(f"store_dist count={count} {name}: relative error {err:.2e} (bound {bound:.2e}, {depth} roundings)")
        assert err <= bound, (name, err, bound)


def test_argument_errors_write_nothing_and_an_aliased_prev_is_refused():
    from chronoedit_amd import ops
    lib = ops.lib()
    x, r, prev = (torch.full((32,), v, dtype=BF, device="cuda") for v in (1.0, 2.0, 3.0))
    sums = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    scratch = torch.full((4096,), -2.0, dtype=torch.float32, device="cuda")
    P, st = ops._ptr, ops._stream()

    def call(x_=x, r_=r, prev_=prev, sums_=sums, scratch_=scratch, scratch_bytes=4096 * 4, n=16):
        return lib.ce_tea_store_dist_bf16(P(x_), P(r_), P(prev_), P(sums_), P(scratch_), scratch_bytes, n, st)

    for missing in ("x_", "r_", "prev_", "sums_", "scratch_"):
        assert call(**{missing: None}) == -1, missing
    assert call(n=0) == -1 and call(n=-8) == -1
    assert call(scratch_bytes=4) == -1  # one workgroup needs 8 bytes
    for n in (12, 1, 7):
        assert call(n=n) == -2
    assert call(x_=x[1:]) == -3 and call(r_=r[1:]) == -3 and call(prev_=prev[1:]) == -3  # 2 bytes past a 16-byte boundary
    assert call(sums_=sums.view(torch.int16)[1:]) == -3 and call(scratch_=scratch.view(torch.int16)[1:]) == -3
    assert call(prev_=r) == -1 and call(prev_=x) == -1 and call(prev_=r[8:]) == -1  # prev overlaps r or x
    with pytest.raises(ops.HipKernelError, match="unsupported shape"):
        ops.tea_store_dist_(x[:12], r[:12], prev[:12], sums)
    for alias in (r, x, r[8:24]):
        with pytest.raises(ValueError, match="alias"):
            ops.tea_store_dist_(x[:16], r[:16], alias[:16], sums)
    with pytest.raises(ValueError, match="prev"):
        ops.tea_store_dist_(x, r, prev[:16], sums)
    with pytest.raises(ValueError, match="sums"):
        ops.tea_store_dist_(x, r, prev, torch.zeros(3, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert all(bool((t.float() == v).all()) for t, v in ((x, 1.0), (r, 2.0), (prev, 3.0), (sums, -1.0), (scratch, -2.0)))  # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert sums.tolist() == [16 * 4.0, 16 * 3.0] and bool((r[:16].float() == -1.0).all()) and bool((r[16:].float() == 2.0).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# model, inputs, loops (the tiny model and inputs of tests/test_teacache_gpu.py: D = 256, 48 tokens per sample, 6 steps, guidance 5)
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
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(BF).float()
    return r(1, 16, T, 8, 12), r(1, 20, T, 8, 12), r(1, 40, 128), r(1, 40, 128), r(1, 257, 64)


def _run(m, inp, steps=6, **kw):
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    lat0, cond, pr, ng, img = inp
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    out = denoise(m, sch, lat0.cuda(), cond.cuda().to(BF), pr.cuda().to(BF), ng.cuda().to(BF), img.cuda().to(BF), steps, 5.0, **kw).clone()
    return out, sch


@pytest.fixture(scope="module")
def measured():
    """ONE measured edit on the shared inputs: (model, final latents, the scheduler, its teacache_measurement, snapshots of engine._tea_res
    after every step)."""
    m = _model()
    snaps = []
    out, sch = _run(m, _inputs(), teacache_measure=True, on_step_end=lambda i, t, lat: snaps.append(m.engine()._tea_res.clone()))
    return m, out, sch, dict(m.teacache_measurement), snaps


def test_measured_loop_keeps_the_latents(measured):
    m, out, sch, meas, _ = measured
    plain, _ = _run(_model(), _inputs())
    assert torch.equal(out, plain), float((out - plain).abs().max())
    graphed, _ = _run(m, _inputs(), teacache_measure=True, use_graph=True)  # use_graph is ignored while measuring
    assert torch.equal(graphed, plain)
    assert m.teacache_measurement["distances"][1:] == meas["distances"][1:]  # the same edit again: the same bits
    assert meas["ratios"] == m.teacache_ratios(sch.timesteps) and len(meas["distances"]) == 6
    assert math.isnan(meas["distances"][0])
    assert all(math.isfinite(d) and d > 0 for d in meas["distances"][1:]), meas["distances"]
    assert m._tea_mode is None and m.teacache_report is None  # no mode is left behind, and no plan was made
    eng = m.engine()
    assert eng._tea_prev is None and eng._tea_sums is None and eng._tea_res.shape == (2 * 48, 256)


def test_distances_agree_with_snapshots_of_the_residual(measured):
    """24 576 elements go through at most 8 + 6 + 3 + 1 + 6 (+ 1 for the subtraction) fp32 roundings: <= 25 * 2^-24 = 1.5e-6 per sum, 3e-6 for
    the quotient; 1e-5 leaves a factor three."""
    _, _, _, meas, snaps = measured
    dist = meas["distances"]
    assert len(snaps) == 6 and all(s.shape == (2 * 48, 256) for s in snaps)
    for i in range(1, 6):
        a, b = snaps[i].double(), snaps[i - 1].double()
        want = float((a - b).abs().sum() / b.abs().sum())
        print(f"step {i}: distance {dist[i]:.9g}, float64 over the snapshots {want:.9g}, relative difference {abs(dist[i] - want) / want:.2e}")
        assert abs(dist[i] - want) <= 1e-5 * want, (i, dist[i], want)


def test_temporal_reasoning_drops_the_previous_residual_at_the_truncation():
    m = _model()
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    out, _ = _run(m, _inputs(T=8), teacache_measure=True, **kw)
    plain, _ = _run(_model(), _inputs(T=8), **kw)
    assert out.shape == (1, 16, 2, 8, 12) and torch.equal(out, plain)
    dist = m.teacache_measurement["distances"]
    assert [math.isnan(d) for d in dist] == [True, False, True, False, False, False], dist
    assert all(math.isfinite(d) and d > 0 for i, d in enumerate(dist) if i not in (0, 2))
    eng = m.engine()
    assert eng._tea_prev is None and eng._tea_res.shape == (2 * 48, 256)  # one residual buffer again, of the 2-frame rows


def test_calibrate_then_enable_end_to_end():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.teacache import TeaCacheCalibration, plan_from_ratios
    from chronoedit_amd.vae import AutoencoderKLWan
    m = _model()
    vp = V.make_synthetic_params(V.VAEConfig(dim=32, z_dim=16))
    pipe = ChronoEditPipeline(vae=AutoencoderKLWan({k: v.cuda() for k, v in vp.items()}, dim=32, z_dim=16), transformer=m,
                              scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0))

    def edit(seed):
        g = torch.Generator().manual_seed(seed)
        dev = lambda t: t.cuda().to(BF)
        return dict(image=dev(torch.rand(1, 3, 64, 96, generator=g) * 2 - 1), prompt_embeds=dev(torch.randn(1, 40, 128, generator=g)),
                    negative_prompt_embeds=dev(torch.randn(1, 40, 128, generator=g)), image_embeds=dev(torch.randn(1, 257, 64, generator=g)),
                    latents=torch.randn(1, 16, 2, 8, 12, generator=g).cuda())

    cal = pipe.calibrate_teacache([edit(1), edit(2)], 6, num_frames=5)
    ratios = m.teacache_measurement["ratios"]
    assert isinstance(cal, TeaCacheCalibration) and len(cal.points) == 10
    assert cal.degree == min(4, len(set(ratios[1:])) - 1) and len(cal.coefficients) == cal.degree + 1
    assert all(math.isfinite(c) for c in cal.coefficients) and math.isfinite(cal.max_residual)
    assert m._teacache is None and m._tea_measure is False  # calibration does not switch TeaCache on, and stops measuring
    thresh = 1.5 * sorted(d for _, d in cal.points)[len(cal.points) // 2]
    pipe.enable_teacache(thresh, cal.coefficients)
    out = pipe.edit_tensors(**edit(3), num_frames=5, num_inference_steps=6, guidance_scale=5.0, output_type="latent")
    assert m.teacache_report["plan"] == plan_from_ratios(ratios, 6, thresh, cal.coefficients)
    assert m.teacache_report["ratios"] == ratios
    assert torch.isfinite(out).all()


def test_measuring_conflicts_are_refused():
    from chronoedit_amd.teacache import TeaCacheConfig
    m = _model()
    with pytest.raises(ValueError, match="TeaCache"):
        _run(m, _inputs(), teacache_measure=True, teacache=TeaCacheConfig(2.5, (1.0,)))
    m.enable_teacache(2.5, (1.0,))
    with pytest.raises(ValueError, match="TeaCache"):
        _run(m, _inputs(), teacache_measure=True)
    with pytest.raises(ValueError, match="TeaCache"):
        m.calibrate_teacache([lambda: _run(m, _inputs())])
    assert m._tea_measure is False
    m.disable_teacache()
    m._sp = types.SimpleNamespace(sharded=True, world=2, rank=0, capturable=False)  # (no process group: the loop must refuse before any forward)
    with pytest.raises(NotImplementedError, match="TeaCache"):
        _run(m, _inputs(), teacache_measure=True)
    m._sp = None
    m._cfgp = object()
    with pytest.raises(NotImplementedError, match="TeaCache"):
        _run(m, _inputs(), teacache_measure=True)
    m._cfgp = None
    m._tea_mode = "measure"  # the mode outside a measured edit: there is no table to write to
    lat0, cond, pr, _, img = _inputs()
    with pytest.raises(RuntimeError, match="measured"):
        m(torch.cat([lat0, cond], dim=1).cuda().to(BF), torch.tensor([500], device="cuda:0"), pr.cuda().to(BF), img.cuda().to(BF), return_dict=False)
    m._tea_mode = None
