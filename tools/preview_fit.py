"""Fit the live previews' latent -> RGB map (chronoedit_amd/preview.py) on a VAE: every image goes through the ordinary pre-processing, one
single-frame encode and a decode; ce_preview_gram_f64 sums the products over all latent cells on the device; `preview.solve_factors` solves
the 17 x 3 least-squares problem.  Writes one JSON:

    {"factors": [[r, g, b] x 17], "report": {"rms": [..], "r2": [..]}, "shape": {...}}

`pipe.enable_preview(on_preview, factors=json["factors"])` takes the factors as they are (rows 0..15 the channel weights, row 16 the bias).

The VAE: --checkpoint DIR (a diffusers layout, its `vae/` is loaded), or the architecture with seeded random weights.  The images: files
(--images a.png b.jpg ...), or --synthetic N seeded gradient-plus-noise pictures.  "report" says how well a linear map explains the 8 x 8
box means of THIS VAE's decoded pixels: with random weights it says nothing about a trained checkpoint.

    timeout 600 python tools/preview_fit.py [--checkpoint DIR] [--images ...] [--synthetic 4] [--height 720 --width 1280] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402
from chronoedit_amd.vae import AutoencoderKLWan  # noqa: E402


def synthetic_images(n, height, width, seed=0):
    """Smooth colour gradients with noise on top: pictures with both low and high frequencies, no two alike."""
    from PIL import Image
    yy, xx = np.mgrid[0:height, 0:width]
    out = []
    for k in range(n):
        rng = np.random.default_rng(seed + k)
        a, b, c = rng.uniform(0.3, 1.0, 3)
        base = np.stack([xx * 255.0 * a / width, yy * 255.0 * b / height, (xx + yy) * 255.0 * c / (width + height)], axis=2)
        base = np.roll(base, k, axis=2)
        out.append(Image.fromarray(np.clip(base + rng.normal(0, 25, base.shape), 0, 255).astype(np.uint8)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", type=str, default="")
    ap.add_argument("--images", nargs="*", default=[])
    ap.add_argument("--synthetic", type=int, default=4)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.checkpoint:
        vae = AutoencoderKLWan.from_pretrained(a.checkpoint, subfolder="vae", torch_dtype=torch.bfloat16, device=dev)
    else:
        vae = AutoencoderKLWan.random_init(dev, seed=4321)
    if a.images:
        from PIL import Image
        images = [Image.open(p).convert("RGB") for p in a.images]
    else:
        images = synthetic_images(a.synthetic, a.height, a.width, a.seed)
    pipe = ChronoEditPipeline(vae=vae)
    factors = pipe.fit_preview_factors(images, height=a.height, width=a.width)
    result = {"factors": [[float(v) for v in row] for row in factors.tolist()], "report": pipe.preview_fit_report,
              "shape": {"checkpoint": a.checkpoint or "synthetic (seeded random weights)", "height": a.height, "width": a.width,
                        "images": a.images or f"{a.synthetic} synthetic, seed {a.seed}", "cells": int(pipe.preview_fit_gram[16, 16])}}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
