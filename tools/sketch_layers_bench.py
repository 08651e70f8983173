"""What sketch edits from the editor's layers (chronoedit_amd/layers.py, csrc/ce_layers.hip; `enable_sketch_region(strokes="layers",
layer_prompts=)`) cost: the 4032x3024 photo of tools/sketch_bench.py with its strokes - over about 1/16 of it - drawn into two RGBA layers,
(grow, feather) = (32, 16), the edit at 1280x720, hipGraph replay on, the 14B architecture with seeded random weights.

    passes     ce_layers_strokes_u8 and ce_layers_over_u8 on each layer's alpha bounding box, and on the whole layer: device time per launch;
               ce_sketch_changed_u8 on the whole photo next to them (what the difference mode runs in their place)
    upload     a layer's box against the whole layer (the crop on the host and the copy)
    in front   everything in front of the edit (`sketch.masks`: uploads, chain, the one read): strokes by difference - the code path of
               the commit before this change - against strokes from the layers with the editor's composite, and without one (built)
    __call__   a whole 8-step edit at guidance 5 on the two-corner strokes of tools/sketch_crops_bench.py: the two-crop call (max_crops = 2,
               one prompt) against two layers with two prompts (max_crops = 1, layer_prompts)

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 900 python tools/sketch_layers_bench.py [--reps 5] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_sketch_layers.md]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sketch_bench as SB  # noqa: E402
import sketch_crops_bench as CB  # noqa: E402
from sketch_bench import alternate, commit, device_ms, fmt, wall  # noqa: E402

from chronoedit_amd import image_io, layers, ops, sketch  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402

H, W, SW, SH = SB.H, SB.W, SB.SW, SB.SH
GROW, FEATHER = 32, 16


def replayed_ms(fn, inner=20):
    """Device time per launch without the host in between: `inner` launches captured into one graph, the replay timed by events."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    graph.replay()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    graph.replay()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / inner


def drawn_layers(size, shapes):
    """Per entry of `shapes` one RGBA layer, transparent except for what its callable draws (opaque, flat colours, hard edges)."""
    from PIL import Image, ImageDraw
    out = []
    for draw in shapes:
        ly = Image.new("RGBA", size)
        draw(ImageDraw.Draw(ly))
        out.append(ly)
    return out


def one_sixteenth():
    """sketch_bench's photo; its ellipse (1/16 of the photo) and first line in layer 0, its second line in layer 1."""
    im, _ = SB.photo_and_composite()
    a, b = SW / 8 * 1.128, SH / 8 * 1.128
    cx, cy = SW * 0.62, SH * 0.4

    def first(d):
        d.ellipse((cx - a, cy - b, cx + a, cy + b), fill=(250, 40, 40, 255))
        d.line((cx - a, cy + b + 60, cx + a, cy + b + 140), fill=(30, 220, 60, 255), width=24)

    return im, drawn_layers(im.size, [first, lambda d: d.line((cx - a - 80, cy - b, cx - a - 120, cy + b), fill=(40, 60, 240, 255), width=24)])


def two_corners():
    """sketch_crops_bench's photo; its mug in layer 0, its hat in layer 1."""
    im, _ = CB.photo_and_composite()

    def mug(d):
        d.ellipse((300, 260, 760, 820), fill=(250, 40, 40, 255))
        d.arc((700, 380, 940, 700), -90, 90, fill=(250, 40, 40, 255), width=30)

    def hat(d):
        d.ellipse((3200, 2300, 3700, 2640), fill=(40, 60, 240, 255))
        d.line((3080, 2660, 3820, 2660), fill=(40, 60, 240, 255), width=36)

    return im, drawn_layers(im.size, [mug, hat])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes, the uploads and the front of the edit only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_sketch_layers.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sketch_layers_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    im, ls = one_sixteenth()
    host = layers.boxes(ls)
    lbs = layers.uploaded(host, dev)
    whole = [layers.LayerBox(k, (0, 0, SW, SH), torch.from_numpy(np.array(ly, dtype=np.uint8)).to(dev)) for k, ly in enumerate(ls)]
    bg_u8 = image_io.upload_rgb(im, dev)
    cp = layers.composite(im, host)
    cp_u8 = layers.composite_u8(bg_u8, lbs)
    ch = layers.strokes(lbs, im.size, 0, dev)
    n_changed = int((ch != 0).sum())
    same = bool(torch.equal(ch.cpu(), layers.strokes(host, im.size))) and bool(torch.equal(cp_u8.cpu(), torch.from_numpy(np.array(cp))))
    by_difference = bool(torch.equal(ch, sketch.changed(bg_u8, cp_u8, 0)))
    lines = ["# Sketch edits from the editor's layers: what the two passes, the uploads and a prompt per layer cost", "",
             f"`tools/sketch_layers_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
             f"commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, opaque strokes over {n_changed / (SW * SH):.3f} of it ({n_changed} pixels) in two layers whose alpha boxes are "
             + " and ".join(f"{lb.box[2] - lb.box[0]}x{lb.box[3] - lb.box[1]}" for lb in host) + f", (grow, feather) = ({GROW}, {FEATHER}), the edit at {W}x{H}.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.",
             f"The device's strokes plane and composite are the host forms' bytes: **{same}**; the strokes by alpha are the strokes by difference here: **{by_difference}**.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------
    plane, canvas, out = torch.zeros((SH, SW), dtype=torch.uint8, device=dev), bg_u8.clone(), torch.empty((SH, SW), dtype=torch.uint8, device=dev)
    fns = {}
    for name, boxes in (("box", lbs), ("whole layer", whole)):
        for lb in boxes:
            l, t, r, b = lb.box
            fns[f"`ce_layers_strokes_u8`, layer {lb.index}, {name} {r - l}x{b - t}"] = (lambda lb=lb: ops.layers_strokes_u8(lb.rgba, lb.box[0], lb.box[1], plane, 0), 5 * (r - l) * (b - t))
            fns[f"`ce_layers_over_u8`, layer {lb.index}, {name} {r - l}x{b - t}"] = (lambda lb=lb: ops.layers_over_u8(lb.rgba, lb.box[0], lb.box[1], canvas), 10 * (r - l) * (b - t))
    fns[f"`ce_sketch_changed_u8`, the photo {SW}x{SH} (the difference mode's pass)"] = (lambda: ops.sketch_changed_u8(bg_u8, cp_u8, 0, out=out), 7 * SW * SH)
    fns[f"memset of the strokes plane, {SW}x{SH}"] = (lambda: plane.zero_(), SW * SH)
    ts = alternate({k: v[0] for k, v in fns.items()}, max(a.reps, 10), device_ms)
    rs = alternate({k: v[0] for k, v in fns.items()}, max(a.reps, 10), replayed_ms)
    lines += ["## The two passes", "",
              "`launched`: events on the stream around 10 launches from Python back to back, divided - the figure the other notes give, and here the host's",
              "rate of launching, not the device's: the smallest box costs what the whole layer costs.  `replayed`: 20 launches captured into one graph, the",
              "replay timed by events, divided: the device's time per launch, the launch gaps of a graph included.  The bytes are those of an opaque stroke:",
              "4 read and 1 written per pixel for the strokes, 4 + 3 read and 3 written for the composite; where the alpha is 0 the passes read the layer only,",
              "and the same buffers are read again launch after launch (the 256 MiB Infinity Cache holds them), so the last column is an upper",
              "bound of a rate, not a bandwidth measurement.", "", "| pass | launched, us | replayed, us | MB at most | GB/s at most (replayed) |", "|---|---|---|---|---|"]
    for k, (_, nbytes) in fns.items():
        print(f"{k:90s} launched {fmt(ts[k], 1e3)} us, replayed {fmt(rs[k], 1e3, 2)} us", flush=True)
        lines.append(f"| {k} | {fmt(ts[k], 1e3)} | {fmt(rs[k], 1e3, 2)} | {nbytes / 1e6:.1f} | {nbytes / statistics.median(rs[k]) / 1e6:.0f} |")
    del plane, canvas, out, whole

    # ---- the uploads -----------------------------------------------------------------------------------------------------------------
    ups = {"the layers' boxes (`layers.boxes` on the host + `layers.uploaded`)": lambda: layers.uploaded(layers.boxes(ls), dev),
           "the whole layers (`np.array(layer)` + the copy)": lambda: [torch.from_numpy(np.array(ly, dtype=np.uint8)).to(dev) for ly in ls],
           "the photo (`image_io.upload_rgb`, for scale)": lambda: image_io.upload_rgb(im, dev)}
    ts = alternate(ups, a.reps, wall)
    lines += ["", "## The upload of the layers", "", f"Both layers, from pageable memory; the boxes hold {sum(lb.rgba.numel() for lb in host) / 1e6:.1f} MB, the whole layers "
              f"{2 * 4 * SW * SH / 1e6:.1f} MB.  `getbbox()` and the crop are part of the first row.", "", "| upload | ms |", "|---|---|"]
    for k in ups:
        print(f"{k:70s} {fmt(ts[k])} ms", flush=True)
        lines.append(f"| {k} | {fmt(ts[k])} |")

    # ---- in front of the edit --------------------------------------------------------------------------------------------------------
    front = {}
    for kw, tag in (({}, ""), ({"min_stroke": 64, "max_crops": 2}, ", min_stroke 64, max_crops 2")):
        d_cfg, l_cfg = sketch.SketchConfig(GROW, FEATHER, **kw), sketch.SketchConfig(GROW, FEATHER, strokes="layers", **kw)
        front[f"strokes by difference (the commit before this change){tag}"] = lambda c=d_cfg: sketch.masks(c, [im], [cp], dev)
        front[f"strokes from the layers, the editor's composite{tag}"] = lambda c=l_cfg: sketch.masks(c, [im], [cp], dev, [ls])
        front[f"strokes from the layers, no composite (built on the device; PIL's copy for CLIP by the host form){tag}"] = lambda c=l_cfg: sketch.masks(c, [im], [None], dev, [ls])
    ts = alternate(front, a.reps, wall)
    e_d, e_l = sketch.masks(sketch.SketchConfig(GROW, FEATHER), [im], [cp], dev)[0], sketch.masks(sketch.SketchConfig(GROW, FEATHER, strokes="layers"), [im], [None], dev, [ls])[0]
    same_mask = bool(torch.equal(e_d["mask_dev"], e_l["mask_dev"])) and bool(torch.equal(e_d["cp_u8"], e_l["cp_u8"]))
    lines += ["", "## Everything in front of the edit", "", "`sketch.masks` for one value: the uploads, the chain, the reductions and the one read, wall clock.  The first row of each "
              f"group is the difference mode: the code path of the commit before this change, measured in this run.  The mask and the composite of the last row are the first row's bytes: **{same_mask}**.",
              "", "| form | ms |", "|---|---|"]
    for k in front:
        print(f"{k:120s} {fmt(ts[k])} ms", flush=True)
        lines.append(f"| {k} | {fmt(ts[k])} |")
    del e_d, e_l, bg_u8, cp_u8, ch, lbs

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
        pos = torch.randn((2, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        neg = torch.randn((2, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        lat0 = torch.randn((1, 16, 2, H // 8, W // 8), generator=g, device=dev)
        im2, ls2 = two_corners()
        value = {"background": im2, "layers": ls2, "composite": layers.composite(im2, layers.boxes(ls2))}
        seen = {}

        def edit(form):
            switch, rows = {"crops": (dict(max_crops=2), 1), "crops, layers": (dict(max_crops=2, strokes="layers"), 1),
                            "prompts": (dict(strokes="layers", layer_prompts=True), 2)}[form]
            pipe.enable_sketch_region(grow=GROW, feather=FEATHER, **switch)
            try:
                out = pipe(image=value, prompt_embeds=pos[:rows], negative_prompt_embeds=neg[:rows], height=H, width=W, num_frames=5,
                           num_inference_steps=a.steps, guidance_scale=5.0, output_type="pil", latents=lat0.clone()).frames
                seen[form] = pipe.sketch_report[0]
            finally:
                pipe.disable_sketch_region()
            return out

        names = {"crops": "two crops, one prompt, strokes by difference (`max_crops=2`: the commit before this change)",
                 "crops, layers": "two crops, one prompt, strokes from the layers (`max_crops=2, strokes=\"layers\"`)",
                 "prompts": "two layers, two prompts (`strokes=\"layers\", layer_prompts=True`)"}
        for k in names:  # warm-up: packs the engine, captures the graphs of every form
            edit(k), edit(k)
        fd, fl = edit("crops"), edit("crops, layers")
        same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(fd[0], fl[0]))
        del fd, fl
        ts = alternate({k: (lambda k=k: edit(k)) for k in names}, max(2, a.reps // 2 + 1), wall)
        lines += ["", f"## A whole {a.steps}-step `__call__` at guidance 5, PIL in, PIL out, 5 frames", "",
                  "The two-corner strokes of tools/sketch_crops_bench.py, the mug in layer 0 and the hat in layer 1.  All three forms run two crops; "
                  f"the two-crop call's frames with the strokes from the layers are those by difference, byte for byte: **{same}**.", "", "| edit | boxes | ms |", "|---|---|---|"]
        for k, name in names.items():
            print(f"__call__ {name:100s} {fmt(ts[k])} ms", flush=True)
            lines.append(f"| {name} | {', '.join(str(c['box']) for c in seen[k]['crops'])} | {fmt(ts[k])} |")
    lines += ["", "## What these numbers do not say", "",
              "The weights are random: nothing here judges what a checkpoint makes of a composite that holds one layer's strokes only, or of two prompts in",
              "one photo.  What the feature guarantees is arithmetic - the two passes bit-equal to PIL's `alpha_composite` and `point` / `lighter`",
              "(tests/test_layers_cpu.py, tests/test_exact_layers_gpu.py), a layers call equal to the difference call where the strokes are opaque and differ from",
              "the photo, a black stroke on a black patch found, two layers with two prompts equal to the explicit-mask call with PIL's chained paste",
              "(tests/test_sketch_layers_gpu.py).  Not measured: translucent or anti-aliased strokes (the passes' cost does not depend on the alpha's value,",
              "except that a run of four pixels with alpha 0 is not written), more than two layers, `enable_sparse_region` under a prompt per layer."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
