"""Automatic edit regions (chronoedit_amd/auto_region.py) on a checkpoint: how early the region of an edit shows.  N seeded edits run the
plain loop measured - every step also writes its change map d = mean over channels of (x0 - z_src)^2 on the last latent frame into a
[steps, h, w] device table (ce_auto_region_change_f32), read back once per edit.  Writes

    {"shape": {...}, "edits": [{"timesteps": [...], "steps": [{"step", "threshold", "active_fraction", "iou"}, ...]}, ...],
     "median_iou_per_step": [...], "first_step_with_median_iou_at_least": {"0.5": k, "0.8": k, "0.9": k}}

iou = the IoU of that step's seed set (d > threshold) with the LAST step's: on a real checkpoint this table is what tells which
`detect_step` is early enough, and active_fraction which `max_area` separates local edits from global ones.  With synthetic weights, or
with the seeded-noise source latents this tool uses without --checkpoint's VAE, it says nothing about a trained network.

The transformer: --checkpoint DIR (a diffusers layout, its `transformer/` is loaded), or the synthetic 14B network of bench.py (--layers).
The conditioning and the source latents are seeded noise of the right shapes; for real edits call
`ChronoEditPipeline.measure_auto_region(edits, steps)`.

    timeout 900 python tools/auto_region_measure.py [--checkpoint DIR] [--steps 8] [--edits 1] [--threshold otsu] [--floor 0] [--out FILE.json]
(--time-limit: the script also ends itself after that many seconds.)"""
import argparse
import json
import os
import signal
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd.auto_region import AutoRegion, AutoRegionConfig  # noqa: E402
from chronoedit_amd.pipeline import denoise  # noqa: E402
from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler  # noqa: E402
from chronoedit_amd.transformer import ChronoEditTransformer3DModel  # noqa: E402
from teacache_calibrate import seeded_edit, synthetic_model  # noqa: E402

BF = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", type=str, default="")
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--frames", type=int, default=2, help="latent frames")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--guidance", type=float, default=5.0)
    ap.add_argument("--edits", type=int, default=1)
    ap.add_argument("--threshold", type=str, default="otsu", help="'otsu' or a number in RMS units of the normalised latents")
    ap.add_argument("--floor", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
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
    cfg = AutoRegionConfig(0, threshold=a.threshold if a.threshold == "otsu" else float(a.threshold), floor=a.floor)
    result = {"shape": {"checkpoint": a.checkpoint or f"synthetic, {a.layers} layers", "height": a.height, "width": a.width, "latent_frames": a.frames,
                        "steps": a.steps, "guidance": a.guidance, "edits": a.edits, "seed": a.seed, "threshold": a.threshold, "floor": a.floor}, "edits": []}
    for k in range(a.edits):
        wl = seeded_edit(m, a.seed + k, a.frames, h, w, dev)
        z_src = torch.randn(wl["latents"].shape, generator=torch.Generator(device=dev).manual_seed(1000 + a.seed + k), device=dev)
        denoise(m, FlowUniPCMultistepScheduler(flow_shift=5.0), wl["latents"].clone(), wl["condition"], wl["prompt"], wl["negative"], wl["image"],
                a.steps, a.guidance, auto_region=AutoRegion(cfg, z_src, measure=True))
        result["edits"].append(m.auto_region_measurement)
    med = [statistics.median(e["steps"][i]["iou"] for e in result["edits"]) for i in range(a.steps)]
    result["median_iou_per_step"] = med
    result["first_step_with_median_iou_at_least"] = {str(b): next((i for i, v in enumerate(med) if v >= b), None) for b in (0.5, 0.8, 0.9)}
    print("median IoU with the last step's seed set, per step:", ", ".join(f"{i}: {v:.3f}" for i, v in enumerate(med)), flush=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
