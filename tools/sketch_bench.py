"""What a sketch edit (chronoedit_amd/sketch.py, csrc/ce_sketch.hip; `ChronoEditPipeline.enable_sketch_region`) costs: a 4032x3024 photo, strokes
over about 1/16 of it, the edit at 1280x720, hipGraph replay on, the 14B architecture with seeded random weights.

    passes     ce_sketch_changed_u8, ce_sketch_dilate_u8 and ce_sketch_box_u8 (both axes each) at (grow, feather) = (8, 8), (32, 16) and
               (128, 64): device time per launch, and the whole build back to back
    host       sketch.reference on the CPU at the same settings, and PIL's own recipe (MaxFilter, BoxBlur) at (8, 8) only - larger windows
               take minutes
    __call__   a whole 8-step edit, PIL in, PIL out, at guidance 1 (the paint-brush caller's) and 5: the sketch edit, the explicit-mask
               focused call with the same mask, the plain call on the composite resized to the edit's size

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 1100 python tools/sketch_bench.py [--reps 5] [--layers 40] [--no-edit] [--no-pil] [--commit HASH] [--out profiles/notes_sketch.md]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chronoedit_amd import image_io, ops, sketch  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402

H, W = 720, 1280
SW, SH = 4032, 3024
SETTINGS = [(8, 8), (32, 16), (128, 64)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, inner=10):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(inner):
        fn()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / inner


def alternate(fns, reps, timer):
    """{name: [ms]}: one warm-up call each, then the callables in turn, repetition by repetition."""
    for fn in fns.values():
        timer(fn)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timer(fn))
    return ts


def fmt(ts, unit=1.0, digits=1):
    return f"{statistics.median(ts) * unit:.{digits}f} ({min(ts) * unit:.{digits}f} .. {max(ts) * unit:.{digits}f})"


def photo_and_composite():
    """A seeded photo, and the editor's composite: a filled ellipse of about 1/16 of the photo and two brush lines next to it, in flat colours."""
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:SH, 0:SW].astype(np.float32)
    base = np.stack([xx * (255.0 / SW), yy * (255.0 / SH), (xx + yy) * (255.0 / (SW + SH))], axis=2)
    im = Image.fromarray(np.clip(base + rng.normal(0, 20, base.shape).astype(np.float32), 0, 255).astype(np.uint8))
    cp = im.copy()
    d = ImageDraw.Draw(cp)
    a, b = SW / 8 * 1.128, SH / 8 * 1.128  # pi a b = SW SH / 16
    cx, cy = SW * 0.62, SH * 0.4
    d.ellipse((cx - a, cy - b, cx + a, cy + b), fill=(250, 40, 40))
    d.line((cx - a, cy + b + 60, cx + a, cy + b + 140), fill=(30, 220, 60), width=24)
    d.line((cx - a - 80, cy - b, cx - a - 120, cy + b), fill=(40, 60, 240), width=24)
    return im, cp


def pil_recipe(bg, cp, grow, feather, threshold=0):
    from PIL import ImageChops, ImageFilter
    r, g, b = ImageChops.difference(cp, bg).split()
    m = ImageChops.lighter(ImageChops.lighter(r, g), b).point(lambda v: 255 if v > threshold else 0)
    return m.filter(ImageFilter.MaxFilter(2 * (grow + feather) + 1)).filter(ImageFilter.BoxBlur(feather))


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes and the host forms only")
    ap.add_argument("--no-pil", action="store_true", help="skip PIL's own recipe (18 s on the CPU at (8, 8))")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_sketch.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sketch_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    im, cp = photo_and_composite()
    bg_u8, cp_u8 = image_io.upload_rgb(im, dev), image_io.upload_rgb(cp, dev)
    n_changed = int((sketch.changed(bg_u8, cp_u8, 0) > 0).sum())
    lines = ["# Sketch edits: what the mask at the photo's size and the second source cost", "",
             f"`tools/sketch_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
             f"commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, strokes over {n_changed / (SW * SH):.3f} of it ({n_changed} changed pixels), the edit at {W}x{H}.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------
    plane = SH * SW
    floor = 2 * 3 * plane + plane + 4 * 2 * plane  # two photos read, the changed plane written, four passes over a plane
    lines += ["## The mask build on the device", "",
              "Device time per launch (events on the stream around 10 launches back to back, divided).  `whole build` is `sketch.mask`: the five launches",
              f"and their four intermediate planes.  The bytes a build has to move are two {3 * plane / 1e6:.1f} MB reads, one {plane / 1e6:.1f} MB write and four passes",
              f"that read and write a plane: {floor / 1e6:.0f} MB.", "",
              "| (grow, feather) | changed, us | dilate h | dilate v | box h | box v | sum of the five | whole build, us | GB/s of the floor | same bytes as the host |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    totals, host_masks = {}, {}
    for grow, feather in SETTINGS:
        R = grow + feather
        ch = ops.sketch_changed_u8(bg_u8, cp_u8, 0)
        dh = ops.sketch_dilate_u8(ch, 0, R)
        dv = ops.sketch_dilate_u8(dh, 1, R)
        bh = ops.sketch_box_u8(dv, 0, feather)
        bv = ops.sketch_box_u8(bh, 1, feather)
        fns = {"changed": lambda: ops.sketch_changed_u8(bg_u8, cp_u8, 0, out=ch), "dilate h": lambda: ops.sketch_dilate_u8(ch, 0, R, out=dh),
               "dilate v": lambda: ops.sketch_dilate_u8(dh, 1, R, out=dv), "box h": lambda: ops.sketch_box_u8(dv, 0, feather, out=bh),
               "box v": lambda: ops.sketch_box_u8(bh, 1, feather, out=bv), "whole": lambda: sketch.mask(bg_u8, cp_u8, grow, feather, 0)}
        ts = alternate(fns, max(a.reps, 10), device_ms)
        host_masks[(grow, feather)] = sketch.reference(im, cp, grow, feather, 0)
        same = bool(torch.equal(bv.cpu(), host_masks[(grow, feather)]))
        five = sum(statistics.median(ts[k]) for k in list(fns)[:5])
        whole = statistics.median(ts["whole"])
        totals[(grow, feather)] = whole
        print(f"({grow}, {feather}): " + ", ".join(f"{k} {fmt(ts[k], 1e3)} us" for k in fns) + f"; same bytes {same}", flush=True)
        lines.append(f"| ({grow}, {feather}) | " + " | ".join(fmt(ts[k], 1e3) for k in list(fns)[:5]) + f" | {five * 1e3:.1f} | {fmt(ts['whole'], 1e3)} | "
                     f"{floor / whole / 1e6:.0f} | {same} |")
    ratio = totals[SETTINGS[-1]] / totals[SETTINGS[0]]
    lines += ["", f"The build at {SETTINGS[-1]} takes **{ratio:.2f}** times the build at {SETTINGS[0]}."]
    print(f"build ratio {SETTINGS[-1]} / {SETTINGS[0]}: {ratio:.2f}", flush=True)

    # ---- the vertical passes away from the common case: the radii the API admits beyond any sensible brush, and a width that is no multiple of 4 ----
    ch = ops.sketch_changed_u8(bg_u8, cp_u8, 0)
    odd = ch[:, :SW - 2].contiguous()  # a cropped photo's width: the byte path, four columns per lane, the last lane's masked
    tmp, tmp_odd = torch.empty_like(ch), torch.empty_like(odd)
    extra = {}
    for r in (16, 48, 63, 64, 192, 512, 1536, 4096):
        extra[f"`ce_sketch_dilate_u8` vertical, R = {r}, {SW} wide"] = (lambda r=r: ops.sketch_dilate_u8(ch, 1, r, out=tmp), r)
    for r in (16, 1024):
        extra[f"`ce_sketch_box_u8` vertical, feather {r}, {SW} wide"] = (lambda r=r: ops.sketch_box_u8(ch, 1, r, out=tmp), r)
    for r in (16, 48, 192):
        extra[f"`ce_sketch_dilate_u8` vertical, R = {r}, {SW - 2} wide (byte path)"] = (lambda r=r: ops.sketch_dilate_u8(odd, 1, r, out=tmp_odd), r)
    extra[f"`ce_sketch_box_u8` vertical, feather 16, {SW - 2} wide (byte path)"] = (lambda: ops.sketch_box_u8(odd, 1, 16, out=tmp_odd), 16)
    extra[f"`ce_sketch_dilate_u8` horizontal, R = 4096, {SW} wide (52 KiB of LDS)"] = (lambda: ops.sketch_dilate_u8(ch, 0, 4096, out=tmp), 4096)
    ts = alternate({k: v[0] for k, v in extra.items()}, max(a.reps, 10), device_ms)
    lines += ["", "## The passes away from the common case", "",
              "A vertical pass keeps a running sum (two loads per output) over segments of 32 rows.  Up to radius 63 a segment's first window is summed row",
              "by row (2 + (2 r + 1) / 32 loads per output); from radius 64 on it is gathered from per-segment sums that a first launch writes to the scratch",
              "(one more load per output, then fewer than 64 rows and (2 r + 1) / 32 eight-byte entries per segment).  The grid is the same at every radius.",
              "A width that is no multiple of 4 takes the byte path: the same four columns per lane, four byte accesses in place of one dword.", "",
              "| pass | first window | us |", "|---|---|---|"]
    for k, (_, r) in extra.items():
        how = "-" if "horizontal" in k else "segment sums" if r >= 64 else "row by row"
        print(f"{k:80s} {fmt(ts[k], 1e3)} us", flush=True)
        lines.append(f"| {k} | {how} | {fmt(ts[k], 1e3)} |")
    del ch, odd, tmp, tmp_odd

    # ---- the host forms ---------------------------------------------------------------------------------------------------------------
    lines += ["", "## The same mask on the host", "", "`sketch.reference` (torch on the CPU: running sums) from the two PIL images, and PIL's own recipe "
              "(`ImageChops.difference` -> `point` -> `MaxFilter` -> `BoxBlur`) at the smallest setting only.", "", "| (grow, feather) | sketch.reference, ms | PIL's recipe, ms | same bytes |",
              "|---|---|---|---|"]
    for grow, feather in SETTINGS:
        ts = [wall(lambda: sketch.reference(im, cp, grow, feather, 0)) for _ in range(3)]
        pil_ms, same = "-", "-"
        if (grow, feather) == SETTINGS[0] and not a.no_pil:
            t0 = time.perf_counter()
            m = pil_recipe(im, cp, grow, feather)
            pil_ms = f"{(time.perf_counter() - t0) * 1e3:.0f}"
            same = str(bool(np.array_equal(np.asarray(m), host_masks[(grow, feather)].numpy())))
        print(f"host ({grow}, {feather}): reference {fmt(ts)} ms, PIL {pil_ms} ms, same {same}", flush=True)
        lines.append(f"| ({grow}, {feather}) | {fmt(ts)} | {pil_ms} | {same} |")

    # ---- the whole edit ----------------------------------------------------------------------------------------------------------
    if not a.no_edit:
        from PIL import Image

        import bench  # build_model: the 14B architecture with seeded random weights
        from transformers import CLIPImageProcessor

        from chronoedit_amd.clip_vision import CLIPVisionModel
        from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
        from chronoedit_amd.vae import AutoencoderKLWan
        del bg_u8, cp_u8
        torch.manual_seed(0)
        model = bench.build_model(a.layers, dev)
        vae = AutoencoderKLWan.random_init(dev, seed=4321)
        pipe = ChronoEditPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0),
                                  image_encoder=CLIPVisionModel(device=dev), image_processor=CLIPImageProcessor())
        pos = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        neg = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        lat0 = torch.randn((1, 16, 2, H // 8, W // 8), generator=g, device=dev)
        grow, feather = SETTINGS[1]
        value = {"background": im, "composite": cp}
        mask = Image.fromarray(host_masks[(grow, feather)].numpy(), mode="L")
        small = cp.resize((W, H), Image.LANCZOS)
        reports = {}

        def edit(form, scale):
            kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=5, num_inference_steps=a.steps, guidance_scale=scale,
                      output_type="pil", latents=lat0.clone())
            if form == "sketch":
                pipe.enable_sketch_region(grow=grow, feather=feather)
                try:
                    out = pipe(image=value, **kw).frames
                    reports["sketch"] = pipe.sketch_report[0]
                finally:
                    pipe.disable_sketch_region()
            elif form == "explicit":
                pipe.enable_region_focus(0.25).set_edit_region(mask)
                try:
                    out = pipe(image=cp, **kw).frames
                finally:
                    pipe.disable_region_focus().clear_edit_region()
            else:
                out = pipe(image=small, **kw).frames
            return out

        names = {"sketch": f"sketch edit (grow {grow}, feather {feather})", "explicit": "explicit-mask focused call, the same mask", "plain": f"plain call on the composite at {W}x{H}"}
        lines += ["", f"## A whole {a.steps}-step `__call__`, PIL in, PIL out, 5 frames", ""]
        for scale in (1.0, 5.0):
            for form in names:  # warm-up: packs the engine, captures the graphs of every form
                edit(form, scale), edit(form, scale)
            fs, fe = edit("sketch", scale), edit("explicit", scale)
            same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(fs[0], fe[0]))
            keep = host_masks[(grow, feather)].numpy() == 0
            exact = fs[0][0].size == im.size and all(np.array_equal(np.asarray(f)[keep], np.asarray(im)[keep]) for f in fs[0])
            del fs, fe
            ts = alternate({k: (lambda k=k: edit(k, scale)) for k in names}, max(3, a.reps // 2 + 1), wall)
            lines += [f"Guidance {scale:g}: the sketch call's frames are the explicit-mask call's, byte for byte (threshold 0): **{same}**; they have the photo's size and "
                      f"its bytes where the mask is 0: **{exact}**.", "", "| edit | ms |", "|---|---|"]
            for k, name in names.items():
                print(f"__call__ guidance {scale:g} {name:55s} {fmt(ts[k])} ms", flush=True)
                lines.append(f"| {name} | {fmt(ts[k])} |")
            d = statistics.median(ts["sketch"]) - statistics.median(ts["explicit"])
            lines += ["", f"Sketch minus explicit: {d:.1f} ms (medians).", ""]
            print(f"guidance {scale:g}: sketch - explicit = {d:.1f} ms, same frames {same}, photo kept {exact}", flush=True)
        # what the difference is made of: one more upload, and the build with its reductions and its one read
        up = [wall(lambda: image_io.upload_rgb(im, dev)) for _ in range(5)]
        pipe.enable_sketch_region(grow=grow, feather=feather)
        masks = [wall(lambda: sketch.masks(pipe._sketch_region, [im], [cp], dev)) for _ in range(5)]
        entry = sketch.masks(pipe._sketch_region, [im], [cp], dev)[0]
        copies = [wall(lambda: entry["mask_dev"].cpu()) for _ in range(5)]
        pipe.disable_sketch_region()
        rep = reports["sketch"]
        lines += [f"One upload of the photo ({3 * plane / 1e6:.1f} MB from pageable memory, `convert(\"RGB\")` and the copy included): {fmt(up)} ms.  Both uploads, the build, the two "
                  f"reductions and the read of ten integers (`sketch.masks`: all that runs in front of the edit): {fmt(masks)} ms.  The report's copy of the "
                  f"mask to the host, behind the edit: {fmt(copies)} ms.",
                  f"The plan: box {rep['box']}, scale {rep['scale']:.3f}, the mask covers {rep['mask_fraction_of_box']:.3f} of the box; {rep['changed_pixels']} changed pixels."]
        print(f"upload {fmt(up)} ms, sketch.masks {fmt(masks)} ms, mask copy {fmt(copies)} ms", flush=True)
    lines += ["", "## What these numbers do not say", "",
              "The weights are random: nothing here judges what the paint-brush LoRA makes of a sketch inside a crop.  What the feature guarantees is",
              "arithmetic - the mask equal to PIL's recipe (tests/test_sketch_cpu.py), the three passes bit-equal to it (tests/test_exact_sketch_gpu.py), a",
              "sketch call equal to the explicit-mask focused call and to PIL's paste into the background (tests/test_sketch_gpu.py)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
