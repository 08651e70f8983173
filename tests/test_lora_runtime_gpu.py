"""Switchable LoRA adapters on the device: the merge kernel's accuracy on random data, exact restore of the base, agreement with
fuse_lora, and the paths a switch has to keep valid (history independence, hipGraph edits, the context cache, the per-call scale,
the capture guard).  Small synthetic models (oracle.dit_oracle.make_synthetic_params), as in tests/test_dit_forward_gpu.py."""
import pytest
import torch

import exact_util as X
from oracle import dit_oracle as O
from oracle import vae_oracle as V

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CFG = dict(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
FUSE_FORWARD_TOL = 2e-2  # rel-L2 of tests/test_dit_forward_gpu.py::test_lora_fuse_and_checkpoint_roundtrip_drive_the_engine (fused forward vs the fp32 oracle)


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _model(seed=0):
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    cfg = O.DiTConfig(**CFG)
    p = O.make_synthetic_params(cfg, seed=seed, dtype=BF)
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=cfg.in_channels, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64,
                                     added_kv_proj_dim=256, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in p.items()})
    return cfg, m


def _inputs(cfg, seed=0):
    lat, text, image = O.make_synthetic_inputs(cfg, 2, 16, 16, dtype=BF)
    return lat.cuda(), torch.tensor([500], device="cuda:0"), text.cuda(), image.cuda()


TARGETS_A = ["blocks.0.attn1.to_q", "blocks.0.attn1.to_v", "blocks.1.ffn.net.0.proj", "blocks.1.attn2.to_out.0"]
TARGETS_B = ["blocks.0.attn1.to_q", "blocks.1.ffn.net.2", "blocks.0.attn2.to_q", "blocks.1.attn1.to_out.0"]
TARGETS_K = ["blocks.0.attn2.to_k", "blocks.1.attn2.add_v_proj"]


def _lora(m, targets, r=8, seed=5, alpha=None, amp=0.05):
    """bf16-representable A / B (what an adapter file in bf16 holds): the switchable path keeps them in bf16 on the device."""
    g = torch.Generator().manual_seed(seed)
    mods = dict(m.named_modules())
    sd = {}
    for t in targets:
        sd[f"transformer.{t}.lora_A.weight"] = (torch.randn(r, mods[t].in_features, generator=g) * amp).to(BF).float()
        sd[f"transformer.{t}.lora_B.weight"] = (torch.randn(mods[t].out_features, r, generator=g) * amp).to(BF).float()
        if alpha is not None:
            sd[f"transformer.{t}.alpha"] = torch.tensor(float(alpha))
    return sd


def _weights(m, targets):
    mods = dict(m.named_modules())
    return {t: mods[t].weight.detach().clone() for t in targets}


def test_kernel_accuracy_on_random_data_against_fp64():
    """Bound from the contract, per element: |got - exact| <= half a bf16 ulp of the result (the one rounding) + the fp32 error of what
    is rounded.  The fp32 value is fl(W0 + sum_i fl(s_i * dot_i)) with dot_i a length-r_i fp32 accumulation: standard bounds give
    |fp32 value - exact| <= gamma_(R+2n) * (|W0| + sum_i |s_i| (|B_i| . |A_i|)) with R = the total rank, n adapters (R products and
    additions, n scalings, n additions onto W0), gamma_k = k u / (1 - k u), u = 2^-24; an fp32 error can also move the value across a
    rounding boundary, which the half ulp taken at the EXACT value's binade (ulp of |exact| + the fp32 error) covers."""
    from chronoedit_amd import ops
    g = torch.Generator().manual_seed(3)
    N, K, ranks, scales = 1288, 1344, [32, 96, 512], [0.7, -1.3, 0.05]
    w0 = torch.randn(N, K, generator=g).to(BF)
    ad = [((torch.randn(r, K, generator=g) * 0.2).to(BF), (torch.randn(N, r, generator=g) * 0.2).to(BF), s) for r, s in zip(ranks, scales)]
    got = ops.lora_merge(w0.cuda(), [(a.cuda(), b.cuda(), s) for a, b, s in ad]).cpu()
    exact = w0.double()
    mag = w0.double().abs()
    for a, b, s in ad:
        s32 = float(torch.tensor(s, dtype=torch.float32))  # the scale reaches the kernel as an fp32 number
        exact = exact + s32 * (b.double() @ a.double())
        mag = mag + abs(s32) * (b.double().abs() @ a.double().abs())
    k = sum(ranks) + 2 * len(ranks)
    u = 2.0 ** -24
    e32 = (k * u / (1 - k * u)) * mag
    ulp = torch.exp2(torch.floor(torch.log2((exact.abs() + e32).clamp_min(2.0 ** -126))) - 7)  # bf16: 8 significant bits
    err = (got.double() - exact).abs()
    bound = 0.5 * ulp + e32
    worst_ulps = float((err / ulp).max())
    print(f"lora_merge random data {N}x{K} ranks {ranks}: max error {worst_ulps:.4f} bf16 ulp, at most {float((err / bound).max()):.3f} of the element's bound")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements outside the bound, worst {float((err / bound).max()):.3f} x"


@pytest.mark.parametrize("mode", ["bf16", "mxfp8"])
def test_disable_and_unfuse_return_the_base_exactly(mode):
    cfg, m = _model()
    if mode == "mxfp8":
        m.enable_fp8_gemms()
    args = _inputs(cfg)
    targets = sorted(set(TARGETS_A + TARGETS_B + TARGETS_K))
    base_out = m(*args, return_dict=False)[0].clone()
    base_w = _weights(m, targets)
    eng = m._engine
    q_names = sorted(eng.fp8_set)
    base_q = [[tuple(t.clone() for t in getattr(p, "q_" + n)) for n in q_names] for p in eng.blk]
    assert (mode == "mxfp8") == bool(q_names)
    m.load_lora_weights(_lora(m, TARGETS_A, seed=5), adapter_name="a")
    m.load_lora_weights(_lora(m, TARGETS_B, r=40, seed=6, alpha=20.0), adapter_name="b")
    m.load_lora_weights(_lora(m, TARGETS_K, seed=7, amp=0.2), adapter_name="k")
    for last in ("disable", "unfuse"):
        m.set_adapters(["a", "b", "k"], [1.0, 0.7, 1.0])
        assert m._engine is eng, "a switch on block Linears must keep the packed engine"
        now = _weights(m, targets)
        assert all(not torch.equal(now[t], base_w[t]) for t in targets)
        moved = m(*args, return_dict=False)[0]
        assert rel_l2(moved, base_out) > 1e-3  # the adapters are visible in the forward
        if q_names:  # ... and in the quantised copies the fp8 GEMMs read
            assert any(not torch.equal(getattr(eng.blk[0], "q_" + n)[0], base_q[0][i][0]) for i, n in enumerate(q_names))
        m.disable_lora() if last == "disable" else m.unfuse_lora()
        assert m.get_active_adapters() == []
        now = _weights(m, targets)
        for t in targets:
            assert torch.equal(now[t], base_w[t]), t
        for p, saved in zip(eng.blk, base_q):
            for n, (q0, s0) in zip(q_names, saved):
                q, s = getattr(p, "q_" + n)
                assert torch.equal(q, q0) and torch.equal(s, s0), n
        assert m._engine is eng
        assert torch.equal(m(*args, return_dict=False)[0], base_out)
    assert m._lora_rt.base is None and m._lora_rt.dev == {}  # unfuse_lora gave the memory back


def test_set_adapters_agrees_with_fuse_lora():
    """The same adapter at the same weight through both doors.  fuse_lora forms B @ A in fp32 by the vendor GEMM and rounds once; the
    switchable path does the same sum on the MFMA in another order: at most 1 bf16 ulp apart per element."""
    w = 0.8
    cfg, x = _model()
    _, y = _model()
    args = _inputs(cfg)
    lora = _lora(x, TARGETS_A + TARGETS_K, r=8, seed=5, alpha=4.0)
    x.load_lora_weights(lora, adapter_name="a")
    y.load_lora_weights(lora, adapter_name="a")
    x(*args, return_dict=False)  # x switches with its engine packed, y packs after the fuse
    x.set_adapters(["a"], [w])
    y.fuse_lora(adapter_names=["a"], lora_scale=w)
    wx, wy = _weights(x, TARGETS_A + TARGETS_K), _weights(y, TARGETS_A + TARGETS_K)
    for t in wx:
        X.assert_exact(wx[t], wy[t], t, ulps=1)
    ox, oy = x(*args, return_dict=False)[0], y(*args, return_dict=False)[0]
    e = rel_l2(ox, oy)
    print(f"set_adapters vs fuse_lora: forward rel-L2 {e:.3e}")
    assert e <= FUSE_FORWARD_TOL
    with pytest.raises(ValueError, match="fused"):
        y.set_adapters(["a"])


def _pipeline(m):
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.vae import AutoencoderKLWan
    vp = V.make_synthetic_params(V.VAEConfig(dim=32, z_dim=16))
    vae = AutoencoderKLWan({k: v.cuda() for k, v in vp.items()}, dim=32, z_dim=16)
    return ChronoEditPipeline(vae=vae, transformer=m, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0))


def test_switching_paths(monkeypatch):
    cfg, m = _model()
    targets = sorted(set(TARGETS_A + TARGETS_B + TARGETS_K))
    m.load_lora_weights(_lora(m, TARGETS_A, seed=5), adapter_name="a")
    m.load_lora_weights(_lora(m, TARGETS_B, r=40, seed=6, alpha=20.0), adapter_name="b")
    m.load_lora_weights(_lora(m, TARGETS_K, seed=7, amp=0.2), adapter_name="k")

    # -- the weights depend on the active set and its weights only, not on the history
    m.set_adapters(["a", "b"], [1.0, 0.5])
    both = _weights(m, targets)
    m.set_adapters(["a"])
    only_a = _weights(m, targets)
    m.set_adapters(["b", "a"], [0.5, 1.0])  # the other order of names: the same terms added onto the same base in the other order -
    swapped = _weights(m, targets)          # two fp32 additions commute up to their roundings: at most 1 bf16 ulp after the one rounding
    for t in targets:
        X.assert_exact(swapped[t], both[t], f"{t}: [b, a] against [a, b]", ulps=1)
    assert m.get_active_adapters() == ["b", "a"]
    m.set_adapters(["a", "b"], [1.0, 0.5])
    again = _weights(m, targets)
    assert all(torch.equal(again[t], both[t]) for t in targets)
    m.disable_lora()
    m.set_adapters("a")
    assert all(torch.equal(_weights(m, targets)[t], only_a[t]) for t in targets)
    assert any(not torch.equal(only_a[t], both[t]) for t in targets)

    # -- a switch between two graphed edits: the second edit equals an eager edit with the same adapters
    pipe = _pipeline(m)
    g = torch.Generator().manual_seed(0)
    H, W, F = 64, 96, 5
    image = (torch.rand(1, 3, H, W, generator=g) * 2 - 1).cuda().to(BF)
    prompt = torch.randn(1, 40, 128, generator=g).cuda().to(BF)
    negative = torch.randn(1, 40, 128, generator=g).cuda().to(BF)
    img_emb = torch.randn(1, 257, 64, generator=g).cuda().to(BF)
    lat0 = torch.randn(1, 16, 2, H // 8, W // 8, generator=g).cuda()

    def edit(use_graph):
        pipe.use_graph = use_graph
        return pipe.edit_tensors(image, prompt, negative, img_emb, num_frames=F, num_inference_steps=4, guidance_scale=5.0, latents=lat0.clone(),
                                 output_type="latent").clone()

    first = edit(True)                     # adapter a
    m.set_adapters(["a", "b"], [1.0, 0.5])
    second = edit(True)
    eager = edit(False)
    assert torch.equal(second, eager), float((second - eager).abs().max())
    assert not torch.equal(second, first)

    # -- a switch that touches attn2.to_k / add_v_proj reaches a prompt the context cache has already seen
    cfg_args = _inputs(cfg)
    assert m.cache_context
    before = m(*cfg_args, return_dict=False)[0].clone()
    assert m._engine._ctx_key is not None
    m.set_adapters(["a", "b", "k"], [1.0, 0.5, 1.0])
    assert m._engine._ctx_key is None, "the cached context projections were made with the old to_k / add_v_proj"
    after = m(*cfg_args, return_dict=False)[0].clone()
    m.cache_context = False
    uncached = m(*cfg_args, return_dict=False)[0].clone()
    m.cache_context = True
    assert not torch.equal(after, before) and torch.equal(after, uncached)

    # -- attention_kwargs={"scale": 0.5} == the same adapters at half their weights, and the weights come back afterwards
    m.set_adapters(["a", "b"], [1.0, 0.5])
    held = _weights(m, targets)
    call = dict(image=image, prompt_embeds=prompt, negative_prompt_embeds=negative, image_embeds=img_emb, height=H, width=W, num_frames=F,
                num_inference_steps=2, guidance_scale=5.0, output_type="latent", return_dict=False)
    scaled = pipe(latents=lat0.clone(), attention_kwargs={"scale": 0.5}, **call)[0].clone()
    assert all(torch.equal(_weights(m, targets)[t], held[t]) for t in targets)
    assert m._lora_rt.weights == {"a": 1.0, "b": 0.5}
    plain = pipe(latents=lat0.clone(), **call)[0].clone()
    m.set_adapters(["a", "b"], [0.5, 0.25])
    halved = pipe(latents=lat0.clone(), attention_kwargs={"scale": 1.0}, **call)[0].clone()
    assert torch.equal(scaled, halved) and not torch.equal(scaled, plain)
    # restored when the call raises, too
    m.set_adapters(["a", "b"], [1.0, 0.5])

    def boom(*a, **k):
        raise RuntimeError("stop here")
    with pytest.raises(RuntimeError, match="stop here"):
        pipe(latents=lat0.clone(), attention_kwargs={"scale": 0.5}, callback_on_step_end=boom, **call)
    assert all(torch.equal(_weights(m, targets)[t], held[t]) for t in targets) and m._lora_rt.weights == {"a": 1.0, "b": 0.5}
    # without an active adapter the scale is a no-op
    m.disable_lora()
    off = _weights(m, targets)
    pipe(latents=lat0.clone(), attention_kwargs={"scale": 0.5}, **call)
    assert all(torch.equal(_weights(m, targets)[t], off[t]) for t in targets)

    # -- no switch while the stream is capturing (the flag alone: no capture is started)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for switch in (lambda: m.set_adapters(["a"]), m.enable_lora, m.disable_lora, m.unfuse_lora, lambda: m.delete_adapters(["a"])):
        with pytest.raises(RuntimeError, match="captur"):
            switch()
    monkeypatch.undo()
    assert all(torch.equal(_weights(m, targets)[t], off[t]) for t in targets) and m.get_list_adapters() == ["a", "b", "k"]
