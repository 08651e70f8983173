"""What one crop per group of stroke clusters costs and buys (chronoedit_amd/clusters.py, csrc/ce_clusters.hip;
`ChronoEditPipeline.enable_sketch_region(max_crops=)`): a 4032x3024 photo with two stroke clusters in opposite corners, (grow, feather) =
(32, 16), the edit at 1280x720, hipGraph replay on, the 14B architecture with seeded random weights.

    passes     ce_clusters_table_i32, ce_clusters_select_u8 and ce_clusters_paste_u8 at the photo's size: device time per call
    plan       from the first read to the crops' plans (`clusters.plan`: grouping on the host, per-group masks, the second read), and all
               that runs in front of the edit (`sketch.masks` + `clusters.plan`) against `sketch.masks` of the single-box call
    __call__   a whole 8-step edit, PIL in, PIL out, at guidance 5: max_crops = 1 (the single-box call: the parent's code path, bit for
               bit) against max_crops = 2, and both again under `enable_sparse_region(refresh_every=2)` with the active token counts

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 1100 python tools/sketch_crops_bench.py [--reps 3] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_sketch_crops.md]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sketch_bench import alternate, commit, device_ms, fmt, wall  # noqa: E402

from chronoedit_amd import autofocus, clusters, image_io, ops, sketch  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402

H, W = 720, 1280
SW, SH = 4032, 3024
GROW, FEATHER = 32, 16


def photo_and_composite():
    """A seeded photo, and the editor's composite: a mug-sized blob with a handle in the top left corner, a hat-sized one with a brim in the
    bottom right one, in flat colours."""
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:SH, 0:SW].astype(np.float32)
    base = np.stack([xx * (255.0 / SW), yy * (255.0 / SH), (xx + yy) * (255.0 / (SW + SH))], axis=2)
    im = Image.fromarray(np.clip(base + rng.normal(0, 20, base.shape).astype(np.float32), 0, 255).astype(np.uint8))
    cp = im.copy()
    d = ImageDraw.Draw(cp)
    d.ellipse((300, 260, 760, 820), fill=(250, 40, 40))
    d.arc((700, 380, 940, 700), -90, 90, fill=(250, 40, 40), width=30)
    d.ellipse((3200, 2300, 3700, 2640), fill=(40, 60, 240))
    d.line((3080, 2660, 3820, 2660), fill=(40, 60, 240), width=36)
    return im, cp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes and the plan only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_sketch_crops.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sketch_crops_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    im, cp = photo_and_composite()
    cfg1 = sketch.SketchConfig(GROW, FEATHER)
    cfg2 = sketch.SketchConfig(GROW, FEATHER, max_crops=2)
    lines = ["# Sketch edits with one crop per group of stroke clusters: what the table, the masks and the crops cost", "",
             f"`tools/sketch_crops_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
             f"commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, two stroke clusters in opposite corners, (grow, feather) = ({GROW}, {FEATHER}), the edit at {W}x{H}.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------
    bg_u8, cp_u8 = image_io.upload_rgb(im, dev), image_io.upload_rgb(cp, dev)
    ch, _, roots, sums, kept, m, _ = sketch.labelled_stages(bg_u8, cp_u8, GROW, FEATHER, 0, 0)
    table, counters = ops.clusters_table_i32(roots, sums, kept)
    count = int(counters[0])
    rows = table.tolist()
    groups = clusters.group(rows[:count], (SW, SH), (W, H), 0.25, FEATHER, 2)
    gor = clusters.group_of_row(groups).to(dev)
    sel = ops.clusters_select_u8(roots, kept, table, gor, 0)
    masks = clusters.group_masks(roots, kept, table, rows, groups, FEATHER)
    boxes = [clusters.focus_box(autofocus.mask_box(x)[0], (SW, SH), (W, H), 0.25)[0] for x in masks]
    l, t, r, b = boxes[-1]
    frames = torch.randint(0, 256, (5, b - t, r - l, 3), dtype=torch.uint8, device=dev)
    canvas = bg_u8.unsqueeze(0).repeat(5, 1, 1, 1).contiguous()
    host = clusters.table(roots.cpu(), sums.cpu(), kept.cpu())
    same = bool(int(host[0]) == count and torch.equal(host[1], table.cpu()) and torch.equal(sel.cpu(), clusters.select(roots.cpu(), kept.cpu(), [rows[i][0] for i in groups[0]])))
    fns = {"table": lambda: ops.clusters_table_i32(roots, sums, kept, table, counters), "select": lambda: ops.clusters_select_u8(roots, kept, table, gor, 0, sel),
           "paste (5 frames, masked)": lambda: ops.clusters_paste_u8(frames, masks[-1], canvas, l, t),
           "paste (5 frames, whole box)": lambda: ops.clusters_paste_u8(frames, None, canvas, l, t),
           "roots + sums (the labelling, for scale)": lambda: clusters._cc.sums(clusters._cc.roots(kept), ch)}
    ts = alternate(fns, max(a.reps, 10), device_ms)
    plane = SH * SW
    lines += ["## The three passes on the device", "",
              f"Device time per call (events on the stream around 10 calls back to back, divided).  {count} clusters, {int((kept != 0).sum())} kept pixels of {plane}; the",
              f"second crop's box is {r - l}x{b - t}.  The table and the first group's selected plane equal the host forms: **{same}**.", "", "| pass | us |", "|---|---|"]
    for k in fns:
        print(f"{k:45s} {fmt(ts[k], 1e3)} us", flush=True)
        lines.append(f"| {k} | {fmt(ts[k], 1e3)} |")

    # ---- the plan ----------------------------------------------------------------------------------------------------------------------
    entry = sketch.masks(cfg2, [im], [cp], dev)[0]
    plan_ts = alternate({"plan": lambda: clusters.plan(entry, 2, W, H, 0.25), "masks1": lambda: sketch.masks(cfg1, [im], [cp], dev),
                         "masks2": lambda: clusters.plan(sketch.masks(cfg2, [im], [cp], dev)[0], 2, W, H, 0.25)}, max(a.reps, 5), wall)
    crops = clusters.plan(entry, 2, W, H, 0.25)
    single = sketch.focus_plan(entry, W, H, 0.25).report
    lines += ["", "## From the read to the plans", "",
              f"`clusters.plan` from the first read's integers to the crops' plans (the grouping, {len(groups)} x (select + two box passes + a reduction), the second read): "
              f"{fmt(plan_ts['plan'])} ms.", f"All that runs in front of the edit - both uploads, the chain, the reads, the plan: {fmt(plan_ts['masks2'])} ms with max_crops = 2 against "
              f"{fmt(plan_ts['masks1'])} ms for the single-box call (`sketch.masks`).", "",
              f"The single box: {single['box']}, reason {single['reason']!r}, scale {single['scale']:.3f}.  The crops ({crops.reason!r}): "
              + "; ".join(f"{p.report['box']}, scale {p.report['scale']:.3f}, the mask covers {p.report['mask_fraction_of_box']:.3f} of the box" for p in crops.plans) + "."]
    print(f"plan {fmt(plan_ts['plan'])} ms; in front of the edit {fmt(plan_ts['masks2'])} ms against {fmt(plan_ts['masks1'])} ms", flush=True)
    print(f"single {single['box']} scale {single['scale']:.3f}; crops {[(p.report['box'], round(p.report['scale'], 3)) for p in crops.plans]}", flush=True)
    del entry, crops, masks, canvas, frames, bg_u8, cp_u8, roots, sums, kept, ch, m, sel

    # ---- the whole edit ----------------------------------------------------------------------------------------------------------
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
        lat0 = torch.randn((1, 16, 2, H // 8, W // 8), generator=g, device=dev)
        value = {"background": im, "composite": cp}
        seen = {}

        def edit(max_crops):
            pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=max_crops)
            try:
                out = pipe(image=value, prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=5, num_inference_steps=a.steps,
                           guidance_scale=5.0, output_type="pil", latents=lat0.clone()).frames
                seen[max_crops] = (pipe.sketch_report[0], getattr(pipe.transformer, "sparse_report", None))
            finally:
                pipe.disable_sketch_region()
            return out

        lines += ["", f"## A whole {a.steps}-step `__call__` at guidance 5, PIL in, PIL out, 5 frames", "",
                  "max_crops = 1 is the single-box call: the code path of the commit before this change, bit for bit (tests/test_clusters_gpu.py).", ""]
        for sparse in (False, True):
            if sparse:
                pipe.enable_sparse_region(refresh_every=2)
            try:
                for k in (1, 2):  # warm-up: packs the engine, captures the graphs of every form
                    edit(k), edit(k)
                ts = alternate({k: (lambda k=k: edit(k)) for k in (1, 2)}, max(2, a.reps), wall)
            finally:
                pipe.disable_sparse_region()
            lines += [("With `enable_sparse_region(refresh_every=2)`:" if sparse else "Dense steps:"), "", "| edit | scale(s) | ms |" + (" active / all tokens (last sample) |" if sparse else ""),
                      "|---|---|---|" + ("---|" if sparse else "")]
            for k in (1, 2):
                rep, srep = seen[k]
                scales = ", ".join(f"{c['scale']:.3f}" for c in rep["crops"]) if k > 1 else f"{rep['scale']:.3f}"
                tokens = f" {srep['active']} / {srep['tokens']} |" if sparse and srep else (" - |" if sparse else "")
                name = "single box (max_crops = 1)" if k == 1 else f"{len(rep['crops'])} crops (max_crops = 2, {rep['crops_reason']!r})"
                print(f"__call__ sparse={sparse} {name:45s} scales {scales:16s} {fmt(ts[k])} ms{tokens}", flush=True)
                lines.append(f"| {name} | {scales} | {fmt(ts[k])} |{tokens}")
            lines.append("")
    lines += ["## What these numbers do not say", "",
              "The weights are random: nothing here judges how a checkpoint edits two crops of one photo consistently - each crop is denoised on its",
              "own, from its value's noise row, and sees only itself.  The default of max_crops = 1 is a choice, not a measurement.  What the feature",
              "guarantees is arithmetic: the table, the selected planes and the paste bit-equal to their host forms (tests/test_exact_clusters_gpu.py), and",
              "a call with crops equal to the explicit-mask focused call on the crops' masks and PIL's chained paste into the background",
              "(tests/test_clusters_gpu.py)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
