"""Fit TeaCache's rescaling polynomial (chronoedit_amd/teacache.py) on a checkpoint: N seeded edits run measured - every step computes and
the pass that stores the block stack's residual also measures its relative L1 distance to the previous step's residual, on the device
(ce_tea_store_dist_bf16) - and the pooled (ratio, distance) points are fitted.  Writes one JSON:

    {"coefficients": [...], "degree": d, "points": [[ratio, distance], ...], "max_residual": .., "rms_residual": .., "shape": {...}, "plans": {...}}

`pipe.enable_teacache(thresh, json["coefficients"])` takes the coefficients as they are.  "plans": for --thresholds (default: 1.5, 3 and 6
times the median fitted distance) the compute / skip plan of the schedule under the fitted polynomial.

The transformer: --checkpoint DIR (a diffusers layout, its `transformer/` is loaded), or the synthetic 14B network of bench.py
(--layers, default 40).  The conditioning of the edits is seeded noise of the right shapes: with a real checkpoint that calibrates the
mechanism, not the prompts a user runs - for those call `ChronoEditPipeline.calibrate_teacache(edits, steps)` with real edits.
With synthetic weights the coefficients say nothing about a trained network.

    timeout 900 python tools/teacache_calibrate.py [--checkpoint DIR] [--steps 50] [--edits 2] [--out FILE.json] [--time-steps]

--time-steps: also the median device ms of a measured step next to a computed TeaCache step (an all-compute plan, eager), alternating,
and the achieved TB/s of ce_tea_store_dist_bf16 (3 reads + 1 write) next to ce_tea_store_bf16 (2 reads + 1 write) on the edit's token matrix.
(--time-limit: the script also ends itself after that many seconds.)"""
import argparse
import json
import os
import signal
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd import ops  # noqa: E402
from chronoedit_amd.pipeline import denoise  # noqa: E402
from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler  # noqa: E402
from chronoedit_amd.teacache import plan_from_ratios  # noqa: E402
from chronoedit_amd.transformer import ChronoEditTransformer3DModel  # noqa: E402

BF = torch.bfloat16


def synthetic_model(layers, dev):
    """The synthetic 14B network of bench.py (same seed, same initialisation)."""
    m = ChronoEditTransformer3DModel(num_attention_heads=40, attention_head_dim=128, in_channels=36, out_channels=16, text_dim=4096,
                                     freq_dim=256, ffn_dim=13824, num_layers=layers, image_dim=1280, added_kv_proj_dim=5120, device=dev, dtype=BF)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("scale_shift_table"):
                p.copy_(torch.randn(p.shape, generator=g, device=dev) / 5120 ** 0.5)
            elif "norm" in name and name.endswith(".weight"):
                p.fill_(1.0)
            elif name.endswith(".bias"):
                p.zero_()
            else:
                p.normal_(0.0, 0.02, generator=g)
    return m


def seeded_edit(m, seed, frames, h, w, dev):
    cfg = m.config
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *s: torch.randn(s, generator=g, device=dev)
    prompt, negative = rnd(1, 512, cfg.text_dim), rnd(1, 512, cfg.text_dim)
    prompt[:, 64:] = 0
    negative[:, 64:] = 0
    return {"latents": rnd(1, 16, frames, h, w), "condition": rnd(1, 20, frames, h, w).to(BF), "prompt": prompt.to(BF), "negative": negative.to(BF),
            "image": rnd(1, 257, cfg.image_dim).to(BF)}


def run_edit(m, wl, steps, guidance, step_ms=None, **kw):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), wl["latents"].clone(), wl["condition"], wl["prompt"], wl["negative"], wl["image"],
            steps, guidance, on_step_end=lambda i, t, lat: marks[i + 1].record(), **kw)
    torch.cuda.synchronize()
    if step_ms is not None:
        step_ms.extend(marks[i].elapsed_time(marks[i + 1]) for i in range(1, steps))  # (step 0 of a measured edit has no distance pass)


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


def store_passes(rows, D, dev, reps):
    """Four distinct operand sets walked in turn (nothing is served from the Infinity Cache at the bench shape), the two passes alternating."""
    xs, rs, ps = ([torch.randn(rows, D, device=dev).to(BF) for _ in range(4)] for _ in range(3))
    sums = torch.zeros(2, dtype=torch.float32, device=dev)
    nbytes = rows * D * 2
    passes = {"ce_tea_store_bf16": (lambda: [ops.tea_store_(x, r) for x, r in zip(xs, rs)], 3 * nbytes),
              "ce_tea_store_dist_bf16": (lambda: [ops.tea_store_dist_(x, r, p, sums) for x, r, p in zip(xs, rs, ps)], 4 * nbytes)}
    ms = {k: [] for k in passes}
    for _ in range(3):
        for k, (fn, _) in passes.items():
            ms[k].append(_median_ms(fn, reps) / len(xs))
    out = {}
    for k, (_, moved) in passes.items():
        t = statistics.median(ms[k])
        out[k] = {"ms": t, "TB_per_s": moved / t / 1e9, "ms_runs": ms[k]}
        print(f"{k:24s} [{rows}, {D}] bf16: {t * 1e3:7.1f} us  {moved / 1e6:6.0f} MB moved  {moved / t / 1e9:5.2f} TB/s", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", type=str, default="")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=2, help="latent frames")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--guidance", type=float, default=5.0)
    ap.add_argument("--edits", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--thresholds", type=str, default="")
    ap.add_argument("--time-steps", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--time-limit", type=int, default=840)
    a = ap.parse_args()
    signal.alarm(a.time_limit)
    dev = torch.device("cuda", 0)
    h, w = a.height // 8, a.width // 8
    if a.checkpoint:
        m = ChronoEditTransformer3DModel.from_pretrained(a.checkpoint, subfolder="transformer", torch_dtype=BF, device=dev)
    else:
        m = synthetic_model(a.layers, dev)
    m.cache_context = True  # as ChronoEditPipeline sets it
    edits = [seeded_edit(m, a.seed + k, a.frames, h, w, dev) for k in range(a.edits)]
    result = {"shape": {"checkpoint": a.checkpoint or f"synthetic, {a.layers} layers", "height": a.height, "width": a.width, "latent_frames": a.frames,
                        "steps": a.steps, "guidance": a.guidance, "edits": a.edits, "seed": a.seed}}

    cal = m.calibrate_teacache([lambda wl=wl: run_edit(m, wl, a.steps, a.guidance) for wl in edits], degree=a.degree)
    result.update(coefficients=list(cal.coefficients), degree=cal.degree, points=[list(p) for p in cal.points],
                  max_residual=cal.max_residual, rms_residual=cal.rms_residual)
    ratios = m.teacache_measurement["ratios"]
    dist = [d for _, d in cal.points]
    print(f"{len(cal.points)} points of {a.edits} edits x {a.steps} steps: ratios {min(ratios[1:]):.4g} .. {max(ratios[1:]):.4g}, distances "
          f"{min(dist):.4g} .. {max(dist):.4g}; degree {cal.degree}, fit residual max {cal.max_residual:.3e} rms {cal.rms_residual:.3e}", flush=True)
    print("coefficients (highest power first):", ", ".join(f"{c:.9g}" for c in cal.coefficients), flush=True)
    med = statistics.median(dist)
    thresholds = [float(t) for t in a.thresholds.split(",") if t] or [1.5 * med, 3.0 * med, 6.0 * med]
    result["plans"] = {}
    for th in thresholds:
        plan = plan_from_ratios(ratios, a.steps, th, cal.coefficients)
        result["plans"][f"{th:.6g}"] = "".join("C" if c else "s" for c in plan)
        print(f"threshold {th:.5g}: plan {result['plans'][f'{th:.6g}']}  skipped {plan.count(False)} / {a.steps}", flush=True)

    if a.time_steps:
        steps = min(a.steps, 8)
        measured, computed = [], []
        for _ in range(2):  # alternating; the first edit of each kind is the warm-up of that kind's buffers
            for timed in (False, True):
                m.enable_teacache(0.0)  # an all-compute plan: every step saves the tokens and stores the residual
                run_edit(m, edits[0], steps, a.guidance, computed if timed else None)
                m.disable_teacache()
                run_edit(m, edits[0], steps, a.guidance, measured if timed else None, teacache_measure=True)
        result["step_ms"] = {"computed_teacache_step": statistics.median(computed), "measured_step": statistics.median(measured),
                             "computed_runs": computed, "measured_runs": measured}
        print(f"eager step, median of {len(computed)}: computed TeaCache step {statistics.median(computed):.2f} ms, measured step "
              f"{statistics.median(measured):.2f} ms", flush=True)
        m.engine().tea_release()
        torch.cuda.empty_cache()
        result["store_passes"] = store_passes((2 if a.guidance > 1 else 1) * a.frames * (h // 2) * (w // 2), m.config.num_attention_heads * m.config.attention_head_dim,
                                              dev, a.reps)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
