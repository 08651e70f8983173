"""What tiled edits (chronoedit_amd/tiles.py, csrc/ce_tiles.hip; `ChronoEditPipeline.enable_tiled_edit`) cost: a 4032x3024 photo, tiles of
1280x720, 5 frames, the 14B architecture with seeded random weights.

A 4032x3024 canvas plans 4 x 6 = 24 tiles of 1280x720 at the default overlap (at least 4 x 5 = 20 at any), more than the 16 a pass takes, so the photo is edited at a
scale whose plan fits (`--scale`, default 0.75: 3024x2268, 3 x 4 = 12 tiles at the default overlap).

    passes     ce_tiles_fuse_f32 and ce_tiles_scatter_f32 on the plan's latents (2 latent frames), ce_tiles_blend_u8 on the decoded tiles'
               bytes next to ce_focus_paste_u8 writing the same target (a whole-photo box, no mask): device time per launch
    step       the tiled step - all tiles as one batched pass, fused - against the steps of `__call__` on a list of the same number of
               tile-size images (which runs its samples one after the other: per step index the samples' step times are added up).  Wall
               time between the calls' `callback_on_step_end`, each behind a device synchronise; the first step of a call is left out
    __call__   a whole tiled edit, PIL in, PIL out: 8 steps at guidance 1, and `--long-steps` (50) at guidance 5

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 1100 python tools/tiled_bench.py [--reps 3] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_tiled.md]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from region_focus_bench import H, W, SH, SW, alternate, commit, device_ms, fmt, photo_and_mask, wall  # noqa: E402

from chronoedit_amd import ops, tiles  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402


def step_times(pipe, kw, n_samples, **call):
    """One call -> per step index 1.. the wall time of that step over all samples, in ms (step 0 of every sample is left out: it follows the
    encoders)."""
    marks = []

    def cb(p, i, t, tensors):
        torch.cuda.synchronize()
        marks.append((i, time.perf_counter()))
        return {}

    pipe(callback_on_step_end=cb, **kw, **call)
    steps = kw["num_inference_steps"]
    assert len(marks) == steps * n_samples
    per = [0.0] * (steps - 1)
    for k in range(1, len(marks)):
        if marks[k][0] > 0:
            per[marks[k][0] - 1] += (marks[k][1] - marks[k - 1][1]) * 1e3
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=6, help="steps of the calls the step times are read from")
    ap.add_argument("--long-steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=0.75)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_tiled.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tiled_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    im, _ = photo_and_mask()
    p = tiles.plan(im.size, H, W, size=a.scale)
    n, (TW_, TH_), (Wt, Ht) = p.count, p.tile, p.target
    whole = tiles.plan(im.size, H, W, max_tiles=1 << 30)  # (what the photo's own size would take)
    full = f"{len(whole.xs)} x {len(whole.ys)} = {whole.count}"
    xs, ys, th, tw, ch, cw = p.cells
    lines = ["# Tiled edits: what a whole photo at full size costs", "",
             f"`tools/tiled_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps} --long-steps {a.long_steps} --scale {a.scale}` on "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}, commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo plans {full} tiles of {W}x{H} at overlap 0.25 (at least 4 x 5 = 20 at any overlap), more than the 16 one pass takes: it is edited at scale {a.scale}, target {Wt}x{Ht}, "
             f"canvas {p.canvas[0]}x{p.canvas[1]}, {len(p.xs)} x {len(p.ys)} = {n} tiles at x {list(p.xs)}, y {list(p.ys)} (overlap 0.25).",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------
    F = 5
    lat = torch.randn((n, 16, 2, th, tw), generator=g, device=dev)
    canvas = torch.empty((16, 2, ch, cw), device=dev)
    frames = torch.randint(0, 256, (n, F, TH_, TW_, 3), generator=g, device=dev, dtype=torch.uint8)
    out = torch.empty((F, Ht, Wt, 3), dtype=torch.uint8, device=dev)
    photo = torch.randint(0, 256, (Ht, Wt, 3), generator=g, device=dev, dtype=torch.uint8)
    edit = torch.randint(0, 256, (F, Ht, Wt, 3), generator=g, device=dev, dtype=torch.uint8)
    passes = {
        "ce_tiles_fuse_f32": (lambda: ops.tiles_fuse(lat, canvas, xs, ys), 4 * (lat.numel() + canvas.numel())),
        "ce_tiles_scatter_f32": (lambda: ops.tiles_scatter(canvas, lat, xs, ys), 8 * lat.numel()),
        f"ce_tiles_blend_u8, {F} frames": (lambda: ops.tiles_blend_u8(frames, p.xs, p.ys, p.target, out=out), frames.numel() + out.numel()),
        f"ce_focus_paste_u8, {F} frames, whole-photo box, no mask": (lambda: ops.focus_paste_u8(edit, photo, None, 0, 0, out=out),
                                                                    photo.numel() + edit.numel() + out.numel()),
    }
    ts = alternate({k: v[0] for k, v in passes.items()}, max(a.reps, 10), device_ms)
    lines += ["## The passes", "", "Device time per launch (events on the stream around 10 launches back to back, divided).  The rate is the bytes the pass has to",
              "move over that time: for the fusion the tiles and the canvas, for the blend the tiles' bytes and the target, for the paste src + edit + out.", "",
              "| pass | bytes | us | GB/s |", "|---|---|---|---|"]
    for k, (_, nbytes) in passes.items():
        med = statistics.median(ts[k])
        print(f"{k:60s} {nbytes / 1e6:9.2f} MB  {fmt(ts[k], 1e3)} us  {nbytes / med / 1e6:8.1f} GB/s", flush=True)
        lines.append(f"| `{k}` | {nbytes / 1e6:.1f} MB | {fmt(ts[k], 1e3)} | {nbytes / med / 1e6:.0f} |")
    del lat, canvas, frames, out, photo, edit

    # ---- the step and the whole edit ---------------------------------------------------------------------------------------------------
    if not a.no_edit:
        import bench  # build_model: the 14B architecture with seeded random weights
        from transformers import CLIPImageProcessor

        from chronoedit_amd.clip_vision import CLIPVisionModel
        from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
        from chronoedit_amd.vae import AutoencoderKLWan
        torch.manual_seed(0)
        model = bench.build_model(a.layers, dev)
        vae = AutoencoderKLWan.random_init(dev, seed=4321)
        pipe = ChronoEditPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0),
                                  image_encoder=CLIPVisionModel(device=dev), image_processor=CLIPImageProcessor())
        pos = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        neg = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        noise = torch.randn((1, 16, 2, ch, cw), generator=g, device=dev)
        target = tiles.target_image(im, p.target, dev)
        crops = tiles.tile_images(target, p)
        cut = tiles.reference_scatter(noise[0].cpu(), xs, ys, th, tw).to(dev)
        base = dict(height=H, width=W, num_frames=5)

        def tiled_kw(steps, guidance, output_type):
            return dict(base, image=im, latents=noise.clone(), prompt_embeds=pos, negative_prompt_embeds=neg, num_inference_steps=steps,
                        guidance_scale=guidance, output_type=output_type)

        def switched(fn):
            pipe.enable_tiled_edit(size=a.scale)
            try:
                return fn()
            finally:
                pipe.disable_tiled_edit()

        def run_tiled(steps, guidance, output_type="latent"):
            return switched(lambda: pipe(**tiled_kw(steps, guidance, output_type)).frames)

        def steps_tiled():
            kw = tiled_kw(a.steps, 5.0, "latent")
            call = {k: kw.pop(k) for k in ("image", "latents")}
            return switched(lambda: step_times(pipe, kw, 1, **call))

        def steps_list():
            kw = dict(base, prompt_embeds=pos.repeat(n, 1, 1), negative_prompt_embeds=neg.repeat(n, 1, 1), num_inference_steps=a.steps, guidance_scale=5.0,
                      output_type="latent")
            return step_times(pipe, kw, n, image=crops, latents=cut.clone())

        for fn in (steps_tiled, steps_list):  # warm-up: packs the engine, captures the graphs of both shapes
            fn(), fn()
        t_tiled, t_list = [], []
        for _ in range(a.reps):
            t_tiled += steps_tiled()
            t_list += steps_list()
        ratio = statistics.median(t_tiled) / statistics.median(t_list)
        spread = lambda v: (max(v) - min(v)) / statistics.median(v)
        print(f"step, {n} tiles, guidance 5: tiled {fmt(t_tiled)} ms | list call, samples added up {fmt(t_list)} ms | ratio {ratio:.3f}", flush=True)
        lines += ["", f"## The step: {n} tiles of {W}x{H}, guidance 5, 2 latent frames", "",
                  f"Steps 1 .. {a.steps - 1} of {a.reps} calls each, graph replay.  The tiled step runs the {n} tiles as one batched pass of {2 * n} samples and ends with",
                  f"the two fusion launches; the list call runs the same {n} tile images one after the other, two samples per step, and its row adds the {n}",
                  "samples' times of a step index up.", "",
                  "| form | ms per step of all tiles | spread (max - min) / median |", "|---|---|---|",
                  f"| tiled: one batched pass + fusion | {fmt(t_tiled)} | {spread(t_tiled):.3f} |",
                  f"| `__call__` on the list of the {n} tile images (the parent commit's call) | {fmt(t_list)} | {spread(t_list):.3f} |", "",
                  f"Tiled over list: **{ratio:.3f}**."]
        lines += ["", "## A whole tiled `__call__`, PIL in, PIL out, 5 frames", "", "| edit | frame size | s |", "|---|---|---|"]
        for steps, guidance, reps in ((8, 1.0, max(2, a.reps)), (a.long_steps, 5.0, 1)):
            if steps <= 0:
                continue
            run_tiled(2, guidance, "pil")  # warm-up of this guidance form and of the decode's shape
            tt = [wall(lambda: run_tiled(steps, guidance, "pil")) for _ in range(reps)]
            size = run_tiled(2, guidance, "pil")[0][0].size
            print(f"__call__ {steps} steps guidance {guidance}: {fmt(tt, 1e-3, 2)} s, frames {size}", flush=True)
            lines.append(f"| {steps} steps, guidance {guidance:g}, {n} tiles ({reps} run{'s' if reps > 1 else ''}) | {size[0]}x{size[1]} | {fmt(tt, 1e-3, 2)} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
