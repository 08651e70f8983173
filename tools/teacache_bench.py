"""What TeaCache step skipping (chronoedit_amd/teacache.py) costs and saves at the bench shape: the 14B transformer with synthetic weights,
720p (2 latent frames, 7 200 tokens per sample), guidance 5 (the pair batched: 14 400 token rows), 50 steps, hipGraph replay,
context cache on - `pipeline.denoise` as the pipeline drives it.

Prints: the achieved TB/s of the two token passes (ce_tea_store_bf16 / ce_tea_apply_bf16: 2 reads + 1 write of the [rows, D] bf16
matrix) next to torch's copy of the same matrix; the ms of building the plan; then one edit without TeaCache and one per threshold -
the plan, the skipped count, sec / edit, the median ms of a computed and of a skipped step (device time between the ends of consecutive
steps) and the relative L2 of the final latents against the run without TeaCache from the same seed.  The weights are synthetic: the
drift figures say what the mechanism does to THIS network, nothing about image quality on the real checkpoint.

Thresholds: --thresholds a,b,c, or (default) 1.5, 3 and 6 times the median per-step ratio of the schedule - about one, two and five
skipped steps per computed one where the ratios are level.  The rescaling polynomial is the identity.

    timeout 900 python tools/teacache_bench.py [--steps 50] [--layers 40] [--out FILE.json]

(--time-limit: the script also ends itself after that many seconds.)"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd import ops  # noqa: E402
from chronoedit_amd.pipeline import denoise  # noqa: E402
from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler  # noqa: E402
from chronoedit_amd.transformer import ChronoEditTransformer3DModel  # noqa: E402

D = 5120


def build_model(layers, dev):
    """The synthetic 14B network of bench.py (same seed, same initialisation)."""
    m = ChronoEditTransformer3DModel(num_attention_heads=40, attention_head_dim=128, in_channels=36, out_channels=16, text_dim=4096,
                                     freq_dim=256, ffn_dim=13824, num_layers=layers, image_dim=1280, added_kv_proj_dim=5120, device=dev,
                                     dtype=torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("scale_shift_table"):
                p.copy_(torch.randn(p.shape, generator=g, device=dev) / D ** 0.5)
            elif "norm" in name and name.endswith(".weight"):
                p.fill_(1.0)
            elif name.endswith(".bias"):
                p.zero_()
            else:
                p.normal_(0.0, 0.02, generator=g)
    return m


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        fn()
        en.record()
        en.synchronize()
        ts.append(st.elapsed_time(en))
    return statistics.median(ts)


def row_passes(rows, dev, reps):
    """Four distinct operand pairs walked in turn (1.2 GB: nothing is served from the 256 MB Infinity Cache)."""
    xs = [torch.randn(rows, D, device=dev).to(torch.bfloat16) for _ in range(4)]
    rs = [torch.randn(rows, D, device=dev).to(torch.bfloat16) for _ in range(4)]
    nbytes = rows * D * 2
    out = {}
    for name, fn, moved in (("torch copy", lambda x, r: r.copy_(x), 2 * nbytes), ("ce_tea_store_bf16", ops.tea_store_, 3 * nbytes),
                            ("ce_tea_apply_bf16", ops.tea_apply_, 3 * nbytes)):
        ms = _median_ms(lambda: [fn(x, r) for x, r in zip(xs, rs)], reps) / len(xs)
        out[name] = {"ms": ms, "TB_per_s": moved / ms / 1e9}
        print(f"{name:18s} [{rows}, {D}] bf16: {ms * 1e3:7.1f} us  {moved / 1e6:6.0f} MB moved  {moved / ms / 1e9:5.2f} TB/s", flush=True)
    return out


def one_edit(m, wl, steps, warm):
    """-> (final latents, sec / edit, per-step device ms)."""
    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]

    def mark(i, t, latents):
        marks[i + 1].record()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks[0].record()
    out = denoise(m, sch, wl["latents"].clone(), wl["condition"], wl["prompt"], wl["negative"], wl["image"], steps, 5.0, use_graph=True,
                  on_step_end=mark, graph_warm=warm)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    return out.clone(), sec, [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--thresholds", type=str, default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--time-limit", type=int, default=840)
    a = ap.parse_args()
    signal.alarm(a.time_limit)
    dev = torch.device("cuda", 0)
    h, w = a.height // 8, a.width // 8
    rows = 2 * 2 * (h // 2) * (w // 2)
    result = {"shape": {"layers": a.layers, "height": a.height, "width": a.width, "steps": a.steps, "token_rows": rows}}
    result["row_passes"] = row_passes(rows, dev, a.reps)
    torch.cuda.empty_cache()

    m = build_model(a.layers, dev)
    m.cache_context = True  # as ChronoEditPipeline sets it
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    prompt, negative = rnd(1, 512, 4096), rnd(1, 512, 4096)
    prompt[:, 64:] = 0
    negative[:, 64:] = 0
    bf = torch.bfloat16
    wl = {"latents": rnd(1, 16, 2, h, w), "condition": rnd(1, 20, 2, h, w).to(bf), "prompt": prompt.to(bf), "negative": negative.to(bf),
          "image": rnd(1, 257, 1280).to(bf)}
    warm = set()
    one_edit(m, wl, 3, warm)  # packs the weights, allocates the workspaces

    sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
    sch.set_timesteps(a.steps, device=dev)
    m.teacache_ratios(sch.timesteps)
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ratios = m.teacache_ratios(sch.timesteps)
        ts.append((time.perf_counter() - t0) * 1e3)
    result["plan_ms"] = statistics.median(ts)
    result["ratios"] = ratios
    med = statistics.median(ratios[1:])
    print(f"plan of {a.steps} steps: {result['plan_ms']:.2f} ms (time projections of every step + one reduction + one read-back); "
          f"ratios min {min(ratios[1:]):.4g} median {med:.4g} max {max(ratios[1:]):.4g}", flush=True)
    thresholds = [float(t) for t in a.thresholds.split(",") if t] or [1.5 * med, 3.0 * med, 6.0 * med]

    off, sec, per = one_edit(m, wl, a.steps, warm)
    off2, sec2, _ = one_edit(m, wl, a.steps, warm)
    result["off"] = {"sec_per_edit": [sec, sec2], "step_ms_median": statistics.median(per), "repeat_bit_identical": bool(torch.equal(off, off2))}
    print(f"TeaCache off: {sec:.2f} / {sec2:.2f} s per edit (two runs), median step {statistics.median(per):.1f} ms, "
          f"second run bit-identical: {torch.equal(off, off2)}", flush=True)
    result["runs"] = []
    for th in thresholds:
        m.enable_teacache(th)
        one_edit(m, wl, a.steps, warm)  # (a first edit under this plan: the residual buffer is allocated here, not in the timed edit)
        out, sec, per = one_edit(m, wl, a.steps, warm)
        rep = m.teacache_report
        comp = [p for p, c in zip(per, rep["plan"]) if c]
        skip = [p for p, c in zip(per, rep["plan"]) if not c]
        drift = float((out - off).norm() / off.norm())
        run = {"threshold": th, "plan": "".join("C" if c else "s" for c in rep["plan"]), "computed": rep["computed"], "skipped": rep["skipped"],
               "sec_per_edit": sec, "compute_step_ms": statistics.median(comp), "skip_step_ms": statistics.median(skip) if skip else None,
               "rel_l2_vs_off": drift, "finite": bool(torch.isfinite(out).all())}
        result["runs"].append(run)
        print(f"threshold {th:.5g}: plan {run['plan']}  skipped {run['skipped']} / {a.steps}  {sec:.2f} s per edit  computed step "
              f"{run['compute_step_ms']:.1f} ms  skipped step {run['skip_step_ms'] if skip else float('nan'):.2f} ms  rel-L2 of the final latents vs off {drift:.3e}",
              flush=True)
        m.disable_teacache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
