"""What the image pre- and post-processing around an edit costs on the host (PIL, numpy, CLIPImageProcessor) and on the device
(chronoedit_amd/image_io.py, csrc/ce_image.hip) - the two settings of `ChronoEditPipeline.enable_device_image_io`, which produce the same bits.

Stages, each for a 1280x720 and a 4032x3024 input going to 1280x720:
    preprocess   PIL image -> bf16 [1, 3, 720, 1280] on the device           (Lanczos resize, / 255, 2x - 1)
    clip         PIL image -> fp32 [1, 3, 224, 224] on the device             (bicubic shortest-edge resize, centre crop, rescale, normalise)
and for 2 and 29 frames:
    pil frames   bf16 [1, 3, F, 720, 1280] on the device -> F PIL images
then whole `__call__` edits (PIL in, PIL out) of the 14B architecture with seeded random weights, 8 steps, guidance 5, for both inputs.

One process; the two settings alternate repetition by repetition; wall time per call with the device synchronised.  Prints mean and
spread (sample standard deviation) and writes the table as markdown.  "first" is the first call of the process (for the device path
it includes building the resize tables for a new pair of sizes: pure Python, cached per (in, out, filter, device)).

    timeout 900 python tools/image_io_bench.py [--reps 10] [--layers 40] [--no-edit] [--out profiles/notes_image_io.md]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd import image_io  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402

H, W = 720, 1280
INPUTS = {"1280x720": (1280, 720), "4032x3024": (4032, 3024)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab(name, host, device, reps, rows):
    """host / device alternate; the first call of each is reported apart."""
    first = {"host": timed(host), "device": timed(device)}
    ts = {"host": [], "device": []}
    for _ in range(reps):
        ts["host"].append(timed(host))
        ts["device"].append(timed(device))
    mh, sh = statistics.mean(ts["host"]), statistics.stdev(ts["host"])
    md, sd = statistics.mean(ts["device"]), statistics.stdev(ts["device"])
    verdict = "device" if md < mh - 2 * sh else "host"
    rows.append((name, mh, sh, first["host"], md, sd, first["device"], verdict))
    print(f"{name:34s} host {mh:9.2f} +- {sh:7.2f} ms (first {first['host']:9.2f})   device {md:9.2f} +- {sd:7.2f} ms (first {first['device']:9.2f})"
          f"   -> {verdict}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-edit", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "notes_image_io.md"))
    a = ap.parse_args()
    from PIL import Image
    from transformers import CLIPImageProcessor
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    # a smooth picture plus noise, not pure noise: neither path's time depends on the content, but the frames stay plausible
    images = {}
    for name, (w, h) in INPUTS.items():
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255.0 / w, yy * 255.0 / h, (xx + yy) * 255.0 / (w + h)], axis=2)
        images[name] = Image.fromarray(np.clip(base + rng.normal(0, 20, base.shape), 0, 255).astype(np.uint8))
    proc = CLIPImageProcessor()
    rows = []
    for name, im in images.items():
        ab(f"preprocess {name} -> {W}x{H}", lambda: ChronoEditPipeline.preprocess_image(im, H, W).to(device=dev, dtype=torch.bfloat16),
           lambda: image_io.preprocess_pil(im, H, W, dev), a.reps, rows)
        ab(f"clip {name} -> 224x224", lambda: proc(images=im, return_tensors="pt")["pixel_values"].to(dev),
           lambda: image_io.clip_pixel_values(proc, im, dev), a.reps, rows)
    for F in (2, 29):
        video = (torch.rand((1, 3, F, H, W), device=dev) * 2.2 - 1.1).to(torch.bfloat16)
        ab(f"pil frames x{F} {W}x{H}", lambda: ChronoEditPipeline.postprocess_video(video, "pil"), lambda: image_io.frames_to_pil(video), a.reps, rows)
        del video
    if not a.no_edit:
        import bench  # build_model: the 14B architecture with seeded random weights
        from chronoedit_amd.clip_vision import CLIPVisionModel
        from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
        from chronoedit_amd.vae import AutoencoderKLWan
        torch.manual_seed(0)
        pipe = ChronoEditPipeline(vae=AutoencoderKLWan.random_init(dev, seed=4321), transformer=bench.build_model(a.layers, dev),
                                  scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0), image_encoder=CLIPVisionModel(device=dev), image_processor=proc)
        g = torch.Generator(device=dev).manual_seed(42)
        pos = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        neg = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        lat = torch.randn((1, 16, 2, H // 8, W // 8), generator=g, device=dev)
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=5, num_inference_steps=a.steps, guidance_scale=5.0,
                  output_type="pil")

        def edit(im, flag):
            pipe.enable_device_image_io(flag)
            return pipe(image=im, latents=lat.clone(), **kw).frames

        im0 = images["1280x720"]
        edit(im0, True)  # warm-up: packs every engine, sizes the workspaces, captures the graphs
        same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(edit(im0, True)[0], edit(im0, False)[0]))
        print(f"__call__ frames with the switch on and off identical: {same}", flush=True)
        for name, im in images.items():
            ab(f"__call__ {a.steps} steps, {name} in, PIL out", lambda: edit(im, False), lambda: edit(im, True), a.reps, rows)
        pipe.enable_device_image_io(True)
    lines = ["# Image pre- and post-processing: host path against device path", "",
             f"`tools/image_io_bench.py --reps {a.reps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {os.cpu_count()} host CPUs visible.",
             "One process, the two settings of `enable_device_image_io` alternating; wall ms per call with the device synchronised: mean +- sample",
             "standard deviation over the repetitions, and the first call of the process apart (on the device path it builds the resize tables",
             "for a new pair of sizes).  Verdict `device`: the device mean lies below the host mean by more than twice the host's spread.", "",
             "| stage | host ms | host first | device ms | device first | verdict |", "|---|---|---|---|---|---|"]
    for name, mh, sh, fh, md, sd, fd, verdict in rows:
        lines.append(f"| {name} | {mh:.2f} +- {sh:.2f} | {fh:.2f} | {md:.2f} +- {sd:.2f} | {fd:.2f} | {verdict} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
