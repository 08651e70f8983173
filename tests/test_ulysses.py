"""Ulysses sequence parallelism (+ CFG parallelism): multi-process tests.
 - CPU / gloo, world 2: the send layout (what ce_rope_scatter_bf16 writes), the two exchanges, the gathered views and the
   K-segmented head merge reproduce un-sharded attention (oracle SDPA), including a token count that does not divide over
   the ranks (zero-padded last shard) and the split k|v-then-q exchange of the engine.
 - CPU / gloo, world 4: CFGParallel builds two Ulysses groups of 2 and hands every rank both predictions.
 - GPU (marker gpu): the HIP kernels of the path against their plain-torch layout contracts (single process); two ranks sharing
   cuda:0 over gloo (host-staged collectives) run the full HIP forward and the CFG denoising loop with the tokens sharded and
   must match the single-process HIP run; four ranks run the 2 x 2 CFG-parallel grouping."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(target, world, *args, timeout=300):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    return sorted(res)


def _init(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _cpu_worker(rank, world, port, q, N, H):
    _init(rank, world, port)
    from chronoedit_amd.parallel import Ulysses
    u = Ulysses()
    hd, D = 128, H * 128
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(N, 3 * D, generator=g)  # replicated "truth"

    def sdpa(qq, kk, vv, heads):
        f = lambda t: t.reshape(-1, heads, hd).transpose(0, 1)[None]
        return torch.nn.functional.scaled_dot_product_attention(f(qq), f(kk), f(vv))[0].transpose(0, 1).reshape(-1, heads * hd)
    ref = sdpa(*qkv.split(D, dim=1), H)
    n_local, start, n_valid = u.shard(N)
    local = u.take_rows(qkv, N)
    Dl, hl = D // world, H // world
    # the engine's order: k|v exchange first (asynchronous), then q
    send_kv = u.send_layout_reference([local[:, D:2 * D], local[:, 2 * D:]])
    recv_kv, w1 = u.all_to_all(send_kv, async_op=True)
    send_q = u.send_layout_reference([local[:, :D]])
    recv_q, w2 = u.all_to_all(send_q, async_op=True)
    w1.wait(), w2.wait()
    kv, qg = u.gathered_view(recv_kv), u.gathered_view(recv_q)
    assert kv.data_ptr() == recv_kv.data_ptr() and qg.shape == (world * n_local, Dl)  # views, no copy
    o = sdpa(qg, kv[:N, :Dl], kv[:N, Dl:], hl)  # [W*n_local, Dl] = the send buffer of the output exchange
    y, _ = u.all_to_all(o.contiguous().view(world, n_local, Dl))
    back = u.merge_heads_reference(y)  # what the K-segmented GEMM operand means
    err = (back[:n_valid] - ref[start:start + n_valid]).abs().max().item() if n_valid else 0.0
    full = u.all_gather_rows(back)[:N]
    err2 = (full - ref).abs().max().item()
    sent = u.stats["all_to_all_bytes_sent_off_rank"]
    q.put((rank, err, err2, sent == (3 * n_local * D + n_local * D) * 4 * (world - 1) // world))
    dist.destroy_process_group()


@pytest.mark.parametrize("N,H", [(64, 4), (50, 2)])
def test_ulysses_layout_roundtrip_gloo(N, H):
    for rank, err, err2, bytes_ok in _spawn(_cpu_worker, 2, N, H):
        assert err < 1e-5 and err2 < 1e-5 and bytes_ok, (rank, err, err2, bytes_ok)


def _cpu_worker_batched(rank, world, port, q, N, H, B):
    """B samples per sharded forward: local rows [sample][local token] (shards rounded up to 64 tokens), receive buffers
    [source rank][sample][local token].  The plain-torch statement of what ce_attention_vt_blocked_bf16 / ce_v_transpose_blocked_bf16
    / the K-segmented out-projection operand read: token g of sample b lives in row (g // n) * B * n + b * n + g % n."""
    _init(rank, world, port)
    from chronoedit_amd.parallel import Ulysses
    u = Ulysses()
    hd, D = 128, H * 128
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, N, 3 * D, generator=g)  # replicated "truth", per sample

    def sdpa(qq, kk, vv, heads):
        f = lambda t: t.reshape(-1, heads, hd).transpose(0, 1)[None]
        return torch.nn.functional.scaled_dot_product_attention(f(qq), f(kk), f(vv))[0].transpose(0, 1).reshape(-1, heads * hd)
    n, start, n_valid = u.shard(N, align=64)
    assert n % 64 == 0 and world * n >= N
    local = torch.cat([u.take_rows(qkv[b], N, align=64) for b in range(B)], 0)  # [B * n, 3D]: rows b * n + i
    Dl, hl = D // world, H // world
    recv_kv, _ = u.all_to_all(u.send_layout_reference([local[:, D:2 * D], local[:, 2 * D:]]))
    recv_q, _ = u.all_to_all(u.send_layout_reference([local[:, :D]]))
    kv, qg = u.gathered_view(recv_kv), u.gathered_view(recv_q)  # [W * B * n, ...]: row (src * B + b) * n + i
    row = lambda b, gtok: (gtok // n) * B * n + b * n + gtok % n
    o = torch.zeros(world * B * n, Dl)
    for b in range(B):
        idx_all = torch.tensor([row(b, t) for t in range(world * n)])
        idx_valid = idx_all[:N]
        o[idx_all] = sdpa(qg[idx_all], kv[idx_valid, :Dl], kv[idx_valid, Dl:], hl)  # queries: every row incl. padding; keys: the N valid tokens
    y, _ = u.all_to_all(o.view(world, B * n, Dl))  # chunk dst = rows [dst * B * n, ...) = [sample][local token] of rank dst
    back = u.merge_heads_reference(y)  # [B * n, D]
    err = 0.0
    for b in range(B):
        ref = sdpa(*qkv[b].split(D, dim=1), H)
        if n_valid:
            err = max(err, (back[b * n:b * n + n_valid] - ref[start:start + n_valid]).abs().max().item())
    q.put((rank, err, n, n_valid))
    dist.destroy_process_group()


@pytest.mark.parametrize("N,H,B,world", [(150, 2, 2, 2), (70, 4, 3, 2), (300, 4, 2, 4)])
def test_ulysses_batched_blocked_layout_gloo(N, H, B, world):
    res = _spawn(_cpu_worker_batched, world, N, H, B)
    for rank, err, n, n_valid in res:
        assert err < 1e-5 and n % 64 == 0, (rank, err, n, n_valid)
    assert sum(nv for *_, nv in res) == N  # the shards cover every token exactly once (some ranks may hold none)


def _cfgp_worker(rank, world, port, q):
    _init(rank, world, port)
    from chronoedit_amd.parallel import CFGParallel, Ulysses
    c = CFGParallel()
    u = Ulysses(c.sp_group)
    # a stand-in forward: every rank of a branch contributes its token shard; the branch result is gathered inside the group
    N = 10
    truth = [torch.arange(N, dtype=torch.float32)[:, None] * (b + 1) + 0.5 * b for b in range(2)]
    mine = u.all_gather_rows(u.take_rows(truth[c.branch], N))[:N]
    cond, uncond = c.exchange(mine)
    ok = torch.equal(cond, truth[0]) and torch.equal(uncond, truth[1])
    q.put((rank, c.branch, u.world, u.rank, bool(ok)))
    dist.destroy_process_group()


def test_cfg_parallel_groups_gloo():
    res = _spawn(_cfgp_worker, 4)
    assert [(r, b, w, ur) for r, b, w, ur, _ in res] == [(0, 0, 2, 0), (1, 0, 2, 1), (2, 1, 2, 0), (3, 1, 2, 1)]
    assert all(ok for *_, ok in res)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: kernels of the path vs their layout contracts (single process)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,H,W", [(37, 4, 2), (200, 40, 8), (90, 40, 4), (64, 2, 1)])
def test_rope_scatter_equals_rmsnorm_rope_plus_layout(M, H, W):
    """ce_rope_scatter_bf16 == ce_rmsnorm_rope_bf16 followed by the send-layout permutation, bit for bit (q, k normalised and
    rotated; v copied), for the fused 3-tensor form and for the split k|v / q form the engine uses."""
    from chronoedit_amd import ops
    dev = torch.device("cuda:0")
    D, hd = H * 128, 128
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(M, 3 * D, generator=g).to(BF).to(dev)
    wq = (1 + 0.05 * torch.randn(D, generator=g)).to(dev)
    wk = (1 + 0.05 * torch.randn(D, generator=g)).to(dev)
    ang = torch.rand(M, 64, generator=g, dtype=torch.float64) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], -1).float().to(dev)
    ref = qkv.clone()
    ops.rmsnorm_rope_(ref[:, :D], wq, cs, hd, 1e-6, x2=ref[:, D:2 * D], w2=wk)
    Dl = D // W
    want = ref.view(M, 3, W, Dl).permute(2, 0, 1, 3).contiguous()  # [W, M, 3, Dl]
    got = ops.rope_scatter(qkv, (0, D, 2 * D), (wq, wk, None), D, W, cs, hd, 1e-6)
    assert torch.equal(got, want)
    got_kv = ops.rope_scatter(qkv, (D, 2 * D), (wk, None), D, W, cs, hd, 1e-6)
    got_q = ops.rope_scatter(qkv, (0,), (wq,), D, W, cs, hd, 1e-6)
    assert torch.equal(got_kv, want[:, :, 1:]) and torch.equal(got_q, want[:, :, :1])
    assert torch.equal(qkv[:, 2 * D:], ref[:, 2 * D:])  # the source is not modified


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,S,epi", [(100, 264, 512, 4, 0), (900, 5120, 5120, 8, 2), (3600, 5120, 5120, 8, 2), (7200, 5120, 5120, 2, 0),
                                          (3600, 5120, 5120, 4, 0)])
def test_gemm_with_k_segmented_operand(M, N, K, S, epi):
    """ce_gemm_bf16 with a_seg_k: A given as [S, M, K/S] (what the output all-to-all leaves) == the same GEMM on the merged [M, K]
    operand, bit for bit, in the 128-tile kernel, the 256-tile kernel and its split-K tail."""
    from chronoedit_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(6)
    a = torch.randn(M, K, generator=g).to(BF).to(dev)
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    res = torch.randn(M, N, generator=g).to(BF).to(dev)
    gate = torch.randn(N, generator=g).to(dev)
    seg = a.view(M, S, K // S).permute(1, 0, 2).contiguous()  # [S, M, K/S]
    kw = dict(epilogue=epi, gate=gate if epi == 2 else None, res=res if epi == 2 else None)
    want = ops.gemm(a, w, b, **kw)
    got = ops.gemm(seg, w, b, **kw)
    assert torch.equal(got, want), (got.float() - want.float()).abs().max()
    for variant in (0, 1, 4, 6):  # every kernel / main loop explicitly
        ops.set_gemm_variant(variant)
        try:
            assert torch.equal(ops.gemm(seg, w, b, **kw), ops.gemm(a, w, b, **kw))
        finally:
            ops.set_gemm_variant(-1)


@pytest.mark.gpu
def test_patchify_row_range():
    from chronoedit_amd import ops
    dev = torch.device("cuda:0")
    x = torch.randn(36, 2, 18, 22, generator=torch.Generator().manual_seed(7)).to(BF).to(dev)
    full = ops.patchify(x, 192)
    N = full.shape[0]  # 198
    nl = (N + 3) // 4
    for r in range(4):
        part = ops.patchify(x, 192, row0=r * nl, nrows=nl)
        valid = max(0, min(nl, N - r * nl))
        assert torch.equal(part[:valid], full[r * nl:r * nl + valid]) and part[valid:].abs().max().item() == 0 if valid < nl else True


# ---------------------------------------------------------------------------------------------------------------------
# GPU: whole forwards / loops with several ranks sharing cuda:0 (gloo, host-staged exchanges)
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_model():
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    from oracle import dit_oracle as O
    cfg = O.DiTConfig(num_attention_heads=4, ffn_dim=1024, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=512)
    p = O.make_synthetic_params(cfg, dtype=BF)
    m = ChronoEditTransformer3DModel(num_attention_heads=4, in_channels=36, ffn_dim=1024, num_layers=2, text_dim=128,
                                     image_dim=64, added_kv_proj_dim=512, device="cuda:0")
    m.load_synthetic_({k: v.cuda() for k, v in p.items()})
    return m, cfg, O


def _gpu_worker(rank, world, port, q):
    _init(rank, world, port)
    torch.cuda.set_device(0)
    m, cfg, O = _tiny_model()
    lat, text, image = O.make_synthetic_inputs(cfg, 2, 18, 22, dtype=BF, text_len=40, real_text=8)  # N = 198: not divisible by 4
    ts = torch.tensor([321], device="cuda:0")
    ref = m(lat.cuda(), ts, text.cuda(), image.cuda()).sample.clone()
    # two samples per forward (the guidance pair batched): different latents / timesteps / prompts per sample
    g = torch.Generator().manual_seed(5)
    lat2 = torch.cat([lat, torch.randn(lat.shape, generator=g).to(BF)], 0).cuda()
    text2 = torch.cat([text, torch.randn(text.shape, generator=g).to(BF)], 0).cuda()
    image2 = torch.cat([image, image], 0).cuda()
    ts2 = torch.tensor([321, 777], device="cuda:0")
    ref2 = m(lat2, ts2, text2, image2).sample.clone()
    m.enable_sequence_parallel()
    out = m(lat.cuda(), ts, text.cuda(), image.cuda()).sample
    calls1 = m._sp.stats["all_to_all_calls"]
    out2 = m(lat2, ts2, text2, image2).sample  # blocked receive layout [source rank][sample][local token], 64-aligned shards
    q.put((rank, bool(torch.equal(out, ref)), float((out.float() - ref.float()).abs().max()), calls1,
           float((out2.float() - ref2.float()).abs().max()), m._sp.stats["all_to_all_calls"] - calls1))
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [4])  # (world 2 of this forward is inside the guidance loops below; round 6: suite time)
def test_ulysses_hip_forward_ranks_sharing_one_gpu(world):
    for rank, equal, err, calls, err2, calls2 in _spawn(_gpu_worker, world):
        assert equal or err < 2e-2, (rank, equal, err)
        assert err2 < 2e-2, (rank, err2)   # B = 2 in one sharded forward == the single-process B = 2 forward
        assert calls == 3 * 2 and calls2 == 3 * 2  # per layer: k|v, q, output - the same number of collectives for two samples


def _fp8_sp_worker(rank, world, port, q):
    """fp8 GEMMs under sequence parallelism with the guidance pair batched: the six large Linears of every block
    run on the e4m3 path with per-row scales of the LOCAL rows, the exchange and the self-attention stay bf16 (attention_path())."""
    _init(rank, world, port)
    torch.cuda.set_device(0)
    import warnings
    m, cfg, O = _tiny_model()
    lat, text, image = O.make_synthetic_inputs(cfg, 2, 18, 22, dtype=BF, text_len=40, real_text=8)
    g = torch.Generator().manual_seed(5)
    lat2 = torch.cat([lat, torch.randn(lat.shape, generator=g).to(BF)], 0).cuda()
    text2 = torch.cat([text, torch.randn(text.shape, generator=g).to(BF)], 0).cuda()
    image2 = torch.cat([image, image], 0).cuda()
    ts2 = torch.tensor([321, 777], device="cuda:0")
    m.enable_fp8_gemms()
    ref2 = m(lat2, ts2, text2, image2).sample.clone()        # single process, fp8 GEMMs, bf16 attention
    m.enable_fp8_attention()
    assert m.attention_path() == "mxfp8"
    m.enable_sequence_parallel()
    assert m.attention_path() == "bf16"                        # the sharded path exchanges bf16 q / k / v
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out2 = m(lat2, ts2, text2, image2).sample
    warned = any("no effect while the tokens are sharded" in str(x.message) for x in w)
    q.put((rank, float((out2.float() - ref2.float()).norm() / ref2.float().norm()), warned, m._sp.stats["all_to_all_calls"]))
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [4])
def test_fp8_gemms_with_the_batched_pair_under_sequence_parallelism(world):
    for rank, err, warned, calls in _spawn(_fp8_sp_worker, world):
        assert err < 2e-2, (rank, err)   # row scales are per token row: sharding the rows does not change them; GEMM tilings differ
        assert warned and calls == 3 * 2  # fp8 attention + sharding is announced, not silently dropped


def _loop_worker(rank, world, port, q, mode):
    """denoise() with guidance 5: single process (batched CFG) vs sharded (the pair batched inside one Ulysses group - blocked receive
    layout, 64-aligned shards, a rank with NO valid token after the frame truncation at world 4 - or the 2 x (world/2) CFG-parallel
    grouping)."""
    _init(rank, world, port)
    torch.cuda.set_device(0)
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    m, cfg, O = _tiny_model()
    g = torch.Generator().manual_seed(11)
    lat0 = torch.randn(1, 16, 8, 8, 12, generator=g).cuda()
    cond = torch.randn(1, 20, 8, 8, 12, generator=g).cuda().to(BF)
    prompt = torch.randn(1, 40, 128, generator=g).cuda().to(BF)
    negative = torch.randn(1, 40, 128, generator=g).cuda().to(BF)
    img = torch.randn(1, 257, 64, generator=g).cuda().to(BF)
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)  # includes the 8 -> 2 frame truncation
    ref = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, prompt, negative, img, 4, 5.0, **kw).clone()
    if mode == "cfgp":
        m.enable_cfg_parallel()
    else:
        m.enable_sequence_parallel()
    out = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, prompt, negative, img, 4, 5.0, **kw)
    err = float((out - ref).norm() / ref.norm())
    q.put((rank, tuple(out.shape), err, bool(torch.isfinite(out).all())))
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world,mode", [(2, "sp"), (4, "sp"), (2, "cfgp"), (4, "cfgp")][1:])  # sp: guidance pair BATCHED inside the Ulysses group; (2, cfgp): the pair split, no token sharding
def test_denoise_loop_with_cfg_sharded_over_ranks(world, mode):
    """`denoise()` must work with the tokens sharded (it used to hand the B = 2 batched-CFG forward to the Ulysses
    path, which raised).  Result vs the single-process loop: identical arithmetic per sample, so rel-L2 <= 5e-3 after 4 steps
    (bit-equal when no GEMM changes its tile decomposition)."""
    for rank, shape, err, finite in _spawn(_loop_worker, world, mode, timeout=600):
        assert shape == (1, 16, 2, 8, 12) and finite and err < 5e-3, (rank, shape, err)


def _full_width_worker(rank, world, port, q):
    """The 8-GPU configuration of BASELINE.json configs[3] as far as one GPU can execute it: world 8, the 14B width (40 heads = 5 per
    rank, D = 5120, F = 13 824), ONE block, the guidance pair batched inside the Ulysses group (blocked receive layout, 64-aligned
    shards) and the 8 -> 2 latent-frame truncation mid-loop (after which ranks 3..7 hold no valid token at all)."""
    _init(rank, world, port)
    torch.cuda.set_device(0)
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    from oracle import dit_oracle as O
    cfg = O.DiTConfig(num_layers=1)
    p = O.make_synthetic_params(cfg, seed=7, dtype=BF)
    m = ChronoEditTransformer3DModel(
        num_attention_heads=cfg.num_attention_heads, attention_head_dim=cfg.attention_head_dim, in_channels=cfg.in_channels,
        out_channels=cfg.out_channels, text_dim=cfg.text_dim, freq_dim=cfg.freq_dim, ffn_dim=cfg.ffn_dim, num_layers=1,
        image_dim=cfg.image_dim, added_kv_proj_dim=cfg.added_kv_proj_dim, rope_temporal_skip_len=cfg.rope_temporal_skip_len,
        device="cuda:0", dtype=BF)
    m.load_synthetic_({k: v.cuda() for k, v in p.items()})
    del p
    g = torch.Generator().manual_seed(11 + 0)  # the same inputs on every rank (replicated)
    lat0 = torch.randn(1, 16, 8, 16, 24, generator=g).cuda()         # 8 latent frames x 8 x 12 tokens = 768
    cond = torch.randn(1, 20, 8, 16, 24, generator=g).cuda().to(BF)
    prompt = torch.randn(1, 512, 4096, generator=g).cuda().to(BF)
    negative = torch.randn(1, 512, 4096, generator=g).cuda().to(BF)
    img = torch.randn(1, 257, 1280, generator=g).cuda().to(BF)
    # one batched forward (B = 2) at 8 frames, single process vs sharded
    x2 = torch.cat([torch.cat([lat0, cond.float()], 1)] * 2).to(BF)
    ts2 = torch.tensor([900, 900], device="cuda:0")
    txt2, img2 = torch.cat([prompt, negative]), torch.cat([img, img])
    ref_fwd = m(x2, ts2, txt2, img2).sample.clone()
    x2s = x2[:, :, [0, -1]].contiguous()  # the post-truncation shape: 2 latent frames = 192 tokens -> 64-row shards, ranks 3..7 all padding
    ref_fwd_s = m(x2s, ts2, txt2, img2).sample.clone()
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    from chronoedit_amd import ops
    ref = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, prompt, negative, img, 4, 5.0, **kw).clone()
    # noise floor of the loop comparison: the SAME single-process loop with another GEMM tile decomposition (128-tile kernel) - four
    # steps of guidance 5 amplify the bf16 summation-order differences of one forward
    old = ops.set_gemm_variant(0)
    alt = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, prompt, negative, img, 4, 5.0, **kw)
    ops.set_gemm_variant(old)
    e_noise = float((alt - ref).norm() / ref.norm())
    m.enable_sequence_parallel()
    out_fwd = m(x2, ts2, txt2, img2).sample
    calls = m._sp.stats["all_to_all_calls"]
    out_fwd_s = m(x2s, ts2, txt2, img2).sample
    out = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, prompt, negative, img, 4, 5.0, **kw)
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    q.put((rank, m._sp.world, m.config.num_attention_heads // m._sp.world, rel(out_fwd, ref_fwd), rel(out_fwd_s, ref_fwd_s), calls, tuple(out.shape),
           rel(out, ref), e_noise, bool(torch.isfinite(out).all())))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_world_8_forty_heads_full_width_block_ranks_sharing_one_gpu():
    """the first 8-GPU run must not be the first time the 8-rank / 5-heads-per-rank path executes.  Eight ranks
    share cuda:0 (collectives host-staged through gloo); forward B = 2 and the 4-step guidance loop incl. the frame truncation equal the
    single-process run up to GEMM tile decomposition (row counts differ per rank): forwards rel-L2 <= 5e-3 at both latent shapes,
    the loop within 3 x what the same single-process loop moves when only its GEMM tiling changes; three collectives per layer."""
    res = _spawn(_full_width_worker, 8, timeout=900)
    assert len(res) == 8
    for rank, world, heads_per_rank, e_fwd, e_fwd_s, calls, shape, e_loop, e_noise, finite in res:
        if rank == 0:
            print(f"world 8 / 5 heads per rank: forward (8 frames) {e_fwd:.2e}, forward (2 frames) {e_fwd_s:.2e}, 4-step loop {e_loop:.2e} "
                  f"(same loop, another GEMM tiling, one process: {e_noise:.2e})")
        assert world == 8 and heads_per_rank == 5
        assert e_fwd < 5e-3 and e_fwd_s < 5e-3, (rank, e_fwd, e_fwd_s)
        assert calls == 3          # one layer: k|v, q, output - for BOTH samples
        assert shape == (1, 16, 2, 16, 24) and finite
        assert e_loop <= 3 * e_noise + 5e-3, (rank, e_loop, e_noise)  # within the loop's own bf16 reordering noise


def _rccl_one_rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world)  # "nccl" IS RCCL on ROCm
    from chronoedit_amd.pipeline import denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    m, cfg, O = _tiny_model()
    lat, text, image = O.make_synthetic_inputs(cfg, 2, 18, 22, dtype=BF, text_len=40, real_text=8)
    ts = torch.tensor([321], device="cuda:0")
    ref = m(lat.cuda(), ts, text.cuda(), image.cuda()).sample.clone()
    m.enable_sequence_parallel(force=True)  # the sharded path with every exchange issued through RCCL (async k|v, q, output, gather)
    out = m(lat.cuda(), ts, text.cuda(), image.cuda()).sample
    g = torch.Generator().manual_seed(11)
    lat0 = torch.randn(1, 16, 2, 8, 12, generator=g).cuda()
    cond = torch.randn(1, 20, 2, 8, 12, generator=g).cuda().to(BF)
    pr, ng = torch.randn(1, 40, 128, generator=g).cuda().to(BF), torch.randn(1, 40, 128, generator=g).cuda().to(BF)
    img = torch.randn(1, 257, 64, generator=g).cuda().to(BF)
    loop = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pr, ng, img, 3, 5.0)
    torch.cuda.synchronize()
    q.put((rank, dist.get_backend(), bool(torch.equal(out, ref)), float((out.float() - ref.float()).abs().max()), m._sp.stats["all_to_all_calls"],
           bool(torch.isfinite(loop).all())))
    dist.destroy_process_group()


def _rccl_eager_default_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    from chronoedit_amd.pipeline import GraphedDenoiser, denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    m, cfg, O = _tiny_model()
    g = torch.Generator().manual_seed(11)
    lat0 = torch.randn(1, 16, 8, 8, 12, generator=g).cuda()
    cond = torch.randn(1, 20, 8, 8, 12, generator=g).cuda().to(BF)
    pr, ng = torch.randn(1, 40, 128, generator=g).cuda().to(BF), torch.randn(1, 40, 128, generator=g).cuda().to(BF)
    img = torch.randn(1, 257, 64, generator=g).cuda().to(BF)
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    ref = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pr, ng, img, 4, 5.0, use_graph=True, **kw).clone()  # un-sharded: graphs
    m.enable_sequence_parallel(force=True)
    refused = False
    try:
        GraphedDenoiser(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0[:, :, :2].clone().contiguous(), cond[:, :, :2].contiguous(), pr, ng, img, 5.0)
    except NotImplementedError:
        refused = True
    out = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pr, ng, img, 4, 5.0, use_graph=True, **kw)  # the pipeline default
    torch.cuda.synchronize()
    q.put((rank, refused, float((out - ref).norm() / ref.norm()), bool(torch.isfinite(out).all())))
    dist.destroy_process_group()


def _owned_comm_graph_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    from chronoedit_amd.pipeline import GraphedDenoiser, denoise
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    m, cfg, O = _tiny_model()
    g = torch.Generator().manual_seed(11)
    lat0 = torch.randn(1, 16, 8, 8, 12, generator=g).cuda()
    cond = torch.randn(1, 20, 8, 8, 12, generator=g).cuda().to(BF)
    pr, ng = torch.randn(1, 40, 128, generator=g).cuda().to(BF), torch.randn(1, 40, 128, generator=g).cuda().to(BF)
    img = torch.randn(1, 257, 64, generator=g).cuda().to(BF)
    kw = dict(enable_temporal_reasoning=True, num_temporal_reasoning_steps=2)
    ref = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pr, ng, img, 4, 5.0, use_graph=False, **kw).clone()  # un-sharded, eager
    m.enable_sequence_parallel(force=True, owned_comm=True)  # every exchange a ce_comm_* call on the library's own RCCL communicator
    eager = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pr, ng, img, 4, 5.0, use_graph=False, **kw).clone()
    calls_eager = m._sp.stats["all_to_all_calls"]
    # two captures in one process (8 latent frames, then 2 after the truncation) and 2 + 2 replays - the sequence that kills the process
    # with torch.distributed's communicator (profiles/r03_rccl_graph_probe.txt)
    graphed = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pr, ng, img, 4, 5.0, use_graph=True, **kw).clone()
    again = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pr, ng, img, 4, 5.0, use_graph=True, **kw).clone()  # a second edit: new captures
    torch.cuda.synchronize()
    accepted = True
    try:
        sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
        sch.set_timesteps(4, device=lat0.device)
        sch._step_index = 0
        GraphedDenoiser(m, sch, lat0[:, :, :2].clone().contiguous(), cond[:, :, :2].contiguous(), pr, ng, img, 5.0)
    except NotImplementedError:
        accepted = False
    torch.cuda.synchronize()
    # the communicator cache.  A second get() for the SAME live group reuses the handle; after the process group was destroyed
    # and re-initialised the default group is another object - the stale ncclComm_t (old world / rank) must not be handed out again
    from chronoedit_amd.parallel import OwnedComm
    c1 = m._sp.comm
    reused = OwnedComm.get() is c1
    c1.close()
    rebuilt_after_close = OwnedComm.get() is not c1
    dist.destroy_process_group()
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=rank, world_size=world)
    c3 = OwnedComm.get()
    fresh = c3 is not c1 and c3.handle is not None and c3.world == world and c3._group_ref is dist.group.WORLD
    snd = torch.arange(64, dtype=torch.float32, device="cuda")
    rcv = torch.zeros_like(snd)
    c3.all_to_all(snd, rcv, async_op=False)
    torch.cuda.synchronize()
    fresh = fresh and bool(torch.equal(snd, rcv))
    q.put((rank, accepted, bool(torch.equal(graphed, eager)), bool(torch.equal(again, eager)), float((eager - ref).norm() / ref.norm()),
           calls_eager, bool(torch.isfinite(graphed).all()), reused, rebuilt_after_close, fresh))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_loop_is_captured_on_the_library_owned_communicator():
    """north_star: the temporal-reasoning loops hipGraph-captured AND sharded.  With `enable_sequence_parallel(owned_comm=True)` the
    exchanges are ce_comm_* calls (csrc/ce_comm.hip: grouped ncclSend / ncclRecv of the librccl.so torch ships, on the capturing stream,
    the k|v exchange forked onto the communicator's side stream and joined by an event) - no Work objects, no watchdog.  One rank over
    RCCL, the most a one-GPU box allows: the sharded 4-step temporal-reasoning loop as TWO captured graphs (8 -> 2 latent frames),
    replayed, equals the eager sharded loop bit for bit, twice in one process; GraphedDenoiser accepts the sharded step."""
    (rank, accepted, same, same_again, err, calls, finite, reused, rebuilt, fresh), = _spawn(_owned_comm_graph_worker, 1, timeout=200)
    assert accepted and finite, (accepted, finite)
    assert reused and rebuilt and fresh, (reused, rebuilt, fresh)  # OwnedComm.get: hit on the live group, never a closed or a stale communicator
    assert same and same_again, (same, same_again)
    assert err < 5e-3, err   # sharded vs un-sharded (different GEMM M splits)
    assert calls == 4 * 2 * 3  # eager loop: 4 steps x ONE batched pass x 2 layers x 3 exchanges


@pytest.mark.gpu
def test_sharded_loop_runs_eagerly_under_the_graph_default():
    """`use_graph=True` is the pipeline default; a step that holds RCCL exchanges cannot be captured on this torch / RCCL build
    (tools/rccl_graph_probe.py, profiles/r03_rccl_graph_probe.txt: the process-group watchdog polls the events of Works created under
    capture and takes the process down), so GraphedDenoiser refuses it and `denoise` runs that loop eagerly - same result as the
    graphed un-sharded loop."""
    (rank, refused, err, finite), = _spawn(_rccl_eager_default_worker, 1, timeout=300)
    assert refused and finite and err < 5e-3, (refused, err)


@pytest.mark.gpu
def test_sharded_path_over_rccl_on_one_rank():
    """The Ulysses code path with its collectives issued through RCCL (backend "nccl") in a group of one rank - the only RCCL
    exercise a one-GPU box allows: asynchronous all_to_all_single + work.wait() ordering against the compute stream, the
    exchange buffers as strided kernel operands, all_gather_into_tensor; the result must equal the un-sharded forward."""
    (rank, backend, equal, err, calls, finite), = _spawn(_rccl_one_rank_worker, 1, timeout=300)
    assert backend == "nccl" and (equal or err < 2e-2) and finite, (backend, equal, err, finite)
    assert calls == 3 * 2 + 3 * 1 * 2 * 3  # forward: 2 layers x 3; loop: 3 steps x ONE batched pass x 2 layers x 3
