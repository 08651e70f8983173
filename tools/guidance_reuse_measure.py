"""Guidance reuse (chronoedit_amd/guidance.py) on a checkpoint: how fast the guidance direction bf16(c - u) moves from step to step, and
what the planned loop costs.  N seeded edits run measured - every step runs the pair, and the pass that stores the direction also sums its
squared distance to the directions of the 1..max_age steps before, on the device (ce_cfg_unipc_step_delta) - one read-back per edit.  Writes

    {"shape": {...}, "edits": [{"timesteps": [...], "rel_l2": [[age 1, .., age A] per step]}, ...], "median_rel_l2_per_age": [...]}

rel_l2[i][a-1] = ||d_i - d_(i-a)|| / ||d_i|| (NaN where no direction of that age exists): on a real checkpoint this table is what tells how
large `pair_every` may be (a "reuse" step a steps after its pair uses a direction that is rel_l2[.][a-1] off).  With synthetic weights it
says nothing about a trained network.

The transformer: --checkpoint DIR (a diffusers layout, its `transformer/` is loaded), or the synthetic 14B network of bench.py (--layers).
The conditioning is seeded noise of the right shapes; for real edits call `ChronoEditPipeline.measure_guidance_reuse(edits, steps)`.

    timeout 900 python tools/guidance_reuse_measure.py [--checkpoint DIR] [--steps 50] [--edits 1] [--max-age 3] [--out FILE.json] [--bench]

--bench: also (hipGraph replay, alternating order, --runs each) the median device ms of a "pair" step next to the plain guided step and of a
"reuse" step next to the plain unguided step over --bench-steps steps, then seconds per --steps edit and the relative L2 of the final
latents against the plain edit for pair_every 2 and 3 and for interval (0, 0.8) with pair_every 1.
(--time-limit: the script also ends itself after that many seconds.)"""
import argparse
import json
import math
import os
import signal
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd.guidance import GuidanceReuseConfig  # noqa: E402
from chronoedit_amd.pipeline import denoise  # noqa: E402
from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler  # noqa: E402
from chronoedit_amd.transformer import ChronoEditTransformer3DModel  # noqa: E402
from teacache_calibrate import seeded_edit, synthetic_model  # noqa: E402

BF = torch.bfloat16


def run_edit(m, wl, steps, guidance, warm, guided=True, **kw):
    """One graphed edit; returns (final latents, device ms per step, seconds of the whole loop on the host clock)."""
    import time
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    marks[0].record()
    out = denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), wl["latents"].clone(), wl["condition"], wl["prompt"],
                  wl["negative"] if guided else None, wl["image"], steps, guidance, use_graph=True, graph_warm=warm,
                  on_step_end=lambda i, t, lat: marks[i + 1].record(), **kw)
    torch.cuda.synchronize()
    return out.clone(), [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)], time.perf_counter() - t0


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def bench(m, wl, a, result):
    warm = set()
    legs = {"plain_guided": dict(), "plain_unguided": dict(guided=False), "pair_every_2": dict(guidance_reuse=GuidanceReuseConfig(2))}
    per = {"plain_guided": [], "plain_unguided": [], "pair": [], "reuse": []}
    for name, kw in legs.items():  # the first edit of each leg: lazy initialisations, both forms' workspaces
        run_edit(m, wl, 4, a.guidance, warm, **kw)
    for _ in range(a.runs):
        for name, kw in legs.items():
            _, ms, _ = run_edit(m, wl, a.bench_steps, a.guidance, warm, **kw)
            if name == "pair_every_2":
                kinds = m.guidance_report["plan"]
                # (steps 0-3 hold the captures of the two graphs: left out of every leg alike)
                per["pair"].append(statistics.median(t for t, k in list(zip(ms, kinds))[4:] if k == "pair"))
                per["reuse"].append(statistics.median(t for t, k in list(zip(ms, kinds))[4:] if k == "reuse"))
            else:
                per[name].append(statistics.median(ms[4:]))
    result["step_ms"] = {k: {"median": statistics.median(v), "runs": v, "spread": max(v) - min(v)} for k, v in per.items()}
    for k, v in result["step_ms"].items():
        print(f"{k:15s} step: median {v['median']:8.2f} ms  runs {', '.join(f'{t:.2f}' for t in v['runs'])}  spread {v['spread']:.2f} ms", flush=True)
    plans = {"plain": None, "pair_every_2": GuidanceReuseConfig(2), "pair_every_3": GuidanceReuseConfig(3), "interval_0_0.8_pair_every_1": GuidanceReuseConfig(1, (0.0, 0.8))}
    result["edits_s"] = {}
    ref = None
    for name, cfg in plans.items():
        out, _, secs = run_edit(m, wl, a.steps, a.guidance, warm, **({} if cfg is None else {"guidance_reuse": cfg}))
        ref = out if ref is None else ref
        rep = m.guidance_report
        result["edits_s"][name] = {"seconds": secs, "rel_l2_vs_plain": rel_l2(out, ref), "counts": None if rep is None else {k: rep[k] for k in ("pair", "reuse", "off")}}
        print(f"{name:28s}: {secs:6.2f} s per {a.steps}-step edit, final latents rel-L2 vs plain {rel_l2(out, ref):.3e}  {result['edits_s'][name]['counts']}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", type=str, default="")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=2, help="latent frames")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--guidance", type=float, default=5.0)
    ap.add_argument("--edits", type=int, default=1)
    ap.add_argument("--max-age", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=12)
    ap.add_argument("--runs", type=int, default=3)
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
                        "steps": a.steps, "guidance": a.guidance, "edits": a.edits, "seed": a.seed, "max_age": a.max_age}, "edits": []}
    for wl in edits:
        denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), wl["latents"].clone(), wl["condition"], wl["prompt"], wl["negative"], wl["image"],
                a.steps, a.guidance, guidance_measure=a.max_age)
        result["edits"].append({k: m.guidance_measurement[k] for k in ("timesteps", "rel_l2")})
    med = []
    for age in range(a.max_age):
        vals = [r[age] for e in result["edits"] for r in e["rel_l2"] if math.isfinite(r[age])]
        med.append(statistics.median(vals) if vals else float("nan"))
    result["median_rel_l2_per_age"] = med
    print("median rel-L2 of the direction per age:", ", ".join(f"{a_ + 1}: {v:.4g}" for a_, v in enumerate(med)), flush=True)
    if a.bench:
        bench(m, edits[0], a, result)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
