"""What a focused region edit (chronoedit_amd/focus.py, csrc/ce_focus.hip; `ChronoEditPipeline.enable_region_focus`) costs: a 4032x3024 photo,
a mask of about 1/16 of its area, the edit at 1280x720, guidance 5, hipGraph replay on, the 14B architecture with seeded random weights.

    passes     ce_focus_resample_l8 (both axes of the mask's crop) and ce_focus_paste_u8 (2 and 29 frames): device time per launch
    in         the pre-processing of a focused call (plan, upload, crop, Lanczos, table lookup, the mask's bilinear resize), device passes
               against the host form (PIL itself, then one upload)
    out        the paste-back behind the decode for 2 and 29 frames (uint8, Lanczos to the box, paste, PIL frames of the photo's size),
               device passes against the host form
    __call__   a whole 8-step edit, PIL in, PIL out: the unfocused region call (the parent commit's, launch for launch) and the focused one,
               each with and without sparse steps

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 1100 python tools/region_focus_bench.py [--reps 7] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_region_focus.md]"""
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

from chronoedit_amd import focus, image_io, ops  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402

H, W, G = 720, 1280, 5.0
SW, SH = 4032, 3024


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


def photo_and_mask():
    """A seeded photo and an elliptic mask of 1/16 of its area, feathered over 48 pixels: 0, 255 and greys."""
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:SH, 0:SW].astype(np.float32)
    base = np.stack([xx * (255.0 / SW), yy * (255.0 / SH), (xx + yy) * (255.0 / (SW + SH))], axis=2)
    im = Image.fromarray(np.clip(base + rng.normal(0, 20, base.shape).astype(np.float32), 0, 255).astype(np.uint8))
    a, b = SW / 8 * 1.128, SH / 8 * 1.128  # pi a b = SW SH / 16
    d = np.sqrt(((xx - SW * 0.62) / a) ** 2 + ((yy - SH * 0.4) / b) ** 2)
    m = np.clip((1.0 - d) * (a / 48.0) + 0.5, 0, 1)
    return im, Image.fromarray(np.round(m * 255).astype(np.uint8))


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--context", type=float, default=0.25)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes, the pre-processing and the paste-back only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_region_focus.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("region_focus_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    im, mask = photo_and_mask()
    rep = focus.plan(im.size, mask, H, W, a.context)
    box = rep["box"]
    l, t, r, b = box
    bw, bh = r - l, b - t
    area = float((np.asarray(mask) > 0).mean())
    print(f"plan: {rep}", flush=True)
    lines = ["# Focused region edits: what the crop and the source-size paste-back cost", "",
             f"`tools/region_focus_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
             f"commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, an elliptic mask over {area:.3f} of it, the edit at {W}x{H}, context {a.context:g}: box {box} ({bw}x{bh}, scale {rep['scale']:.3f}, "
             f"the mask covers {rep['mask_fraction_of_box']:.3f} of it).",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------
    src_u8, mask_dev = image_io.upload_rgb(im, dev), torch.from_numpy(np.asarray(mask)).to(dev)
    view = mask_dev[t:b, l:r]
    th = image_io._device_tables(bw, W, image_io.BILINEAR, dev)
    tv = image_io._device_tables(bh, H, image_io.BILINEAR, dev)
    mh = ops.focus_resample_l8(view, 0, *th)
    mv = torch.empty((H, W), dtype=torch.uint8, device=dev)
    passes = {"ce_focus_resample_l8 horizontal (the mask's crop through the pitch)": (lambda: ops.focus_resample_l8(view, 0, *th, out=mh), bw * bh + W * bh),
              "ce_focus_resample_l8 vertical": (lambda: ops.focus_resample_l8(mh, 1, *tv, out=mv), W * bh + W * H)}
    for F in (2, 29):
        edit = torch.randint(0, 256, (F, bh, bw, 3), generator=g, device=dev, dtype=torch.uint8)
        out = torch.empty((F, SH, SW, 3), dtype=torch.uint8, device=dev)
        nbytes = F * SH * SW * 3 + SH * SW * 3 + F * bh * bw * 4
        passes[f"ce_focus_paste_u8, {F} frames, mask"] = (lambda e=edit, o=out: ops.focus_paste_u8(e, src_u8, mask_dev, l, t, out=o), nbytes)
        passes[f"ce_focus_paste_u8, {F} frames, no mask"] = (lambda e=edit, o=out: ops.focus_paste_u8(e, src_u8, None, l, t, out=o), nbytes - F * bh * bw)
    ts = alternate({k: v[0] for k, v in passes.items()}, max(a.reps, 10), device_ms)
    lines += ["## The passes", "", "Device time per launch (events on the stream around 10 launches back to back, divided) and the rate that makes of the bytes the pass",
              "has to move.  The paste writes every frame at the photo's size (36.6 MB each); the 29-frame working set (1.1 GB) exceeds the last-level cache.", "",
              "| pass | bytes | us | GB/s |", "|---|---|---|---|"]
    for k, (_, nbytes) in passes.items():
        med = statistics.median(ts[k])
        print(f"{k:75s} {nbytes / 1e6:9.2f} MB  {fmt(ts[k], 1e3)} us  {nbytes / med / 1e6:8.1f} GB/s", flush=True)
        lines.append(f"| `{k}` | {nbytes / 1e6:.2f} MB | {fmt(ts[k], 1e3)} | {nbytes / med / 1e6:.0f} |")
    del passes, edit, out

    # ---- the pre-processing and the paste-back: device passes against PIL on the host ---------------------------------------------
    def pre(flag):
        plans = focus.setup(im, mask, H, W, a.context, "pil", dev if flag else None)
        return plans, focus.inputs(plans, H, W, dev)

    (plans_d, (img_d, m_d)), (plans_h, (img_h, m_h)) = pre(True), pre(False)
    same_in = bool(torch.equal(img_d, img_h)) and bool(torch.equal(m_d[0], m_h[0]))
    ts = alternate({"device": lambda: pre(True), "host": lambda: pre(False)}, a.reps, wall)
    lines += ["", "## The pre-processing of a focused call", "",
              "Mask normalisation and bounding box (host, both forms), then crop -> Lanczos -> table lookup and the mask's crop -> bilinear, ending in a",
              f"device synchronise.  Device form: the photo and the mask are uploaded whole (36.6 + 12.2 MB).  Both forms give the same bits: **{same_in}**.", "",
              "| form | ms |", "|---|---|", f"| device passes | {fmt(ts['device'])} |", f"| host (PIL), then one upload | {fmt(ts['host'])} |"]
    print(f"pre-processing: device {fmt(ts['device'])} ms, host {fmt(ts['host'])} ms, same bits {same_in}", flush=True)
    lines += ["", "## The paste-back behind the decode", "",
              "`ce_video_to_u8` -> per frame Lanczos to the box -> `ce_focus_paste_u8` -> one device-to-host copy -> `Image.fromarray` per frame, against",
              "`postprocess_video(..., \"pil\")` -> per frame `resize` and `paste` in PIL.  PIL frames of the photo's size come out of both.", "",
              "| frames | device passes, ms | per frame | host (PIL), ms | per frame | same bytes |", "|---|---|---|---|---|---|"]
    for F in (2, 29):
        video = (torch.rand((1, 3, F, H, W), generator=g, device=dev) * 2.2 - 1.1).to(torch.bfloat16)
        post = lambda plans: focus.paste(video, plans, lambda b_: 0, "pil", True)
        fd, fh = post(plans_d), post(plans_h)
        same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(fd[0], fh[0]))
        del fd, fh
        ts = alternate({"device": lambda: post(plans_d), "host": lambda: post(plans_h)}, max(3, a.reps // 2), wall)
        md, mh_ = statistics.median(ts["device"]), statistics.median(ts["host"])
        print(f"paste-back {F} frames: device {fmt(ts['device'])} ms, host {fmt(ts['host'])} ms, same bytes {same}", flush=True)
        lines.append(f"| {F} | {fmt(ts['device'])} | {md / F:.1f} | {fmt(ts['host'])} | {mh_ / F:.1f} | {same} |")
        del video
    del plans_d, plans_h, img_d, img_h

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
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=5, num_inference_steps=a.steps, guidance_scale=G, output_type="pil")
        pipe.set_edit_region(mask)
        reports = {}

        def edit(focused, sparse):
            pipe.enable_region_focus(a.context) if focused else pipe.disable_region_focus()
            pipe.enable_sparse_region(2) if sparse else pipe.disable_sparse_region()
            frames = pipe(image=im, latents=lat0.clone(), **kw).frames
            reports[(focused, sparse)] = pipe.transformer.sparse_report
            return frames

        forms = {"region, unfocused (the parent commit's call)": (False, False), "region, unfocused, sparse steps (refresh_every 2)": (False, True),
                 "focused": (True, False), "focused, sparse steps (refresh_every 2)": (True, True)}
        for fs in forms.values():  # warm-up: packs the engine, captures the graphs of every form
            edit(*fs), edit(*fs)
        frames = edit(True, False)
        keep = np.asarray(mask) == 0
        exact = frames[0][0].size == im.size and all(np.array_equal(np.asarray(f)[keep], np.asarray(im)[keep]) for f in frames[0])
        print(f"focused frames have the photo's size and its bytes where the mask is 0: {exact}", flush=True)
        del frames
        ts = alternate({k: (lambda fs=fs: edit(*fs)) for k, fs in forms.items()}, max(3, a.reps // 2), wall)
        lines += ["", f"## A whole {a.steps}-step `__call__`, PIL in, PIL out, 5 frames", "",
                  f"The same {SW}x{SH} photo and mask go into every form.  Unfocused, the photo is resized to {W}x{H} and {W}x{H} frames come back (the parent",
                  f"commit's call, launch for launch); focused, the model sees the {bw}x{bh} box and frames of {SW}x{SH} come back - the photo's bytes exactly",
                  f"where the mask is 0, in every frame: **{exact}**.  The mask covers {area:.3f} of the photo and {rep['mask_fraction_of_box']:.3f} of the box, so",
                  "the focused edit's sparse steps carry more active tokens than the unfocused one's: that is the point of the crop, not an overhead.", "",
                  "| edit | ms | active / tokens of a sparse step |", "|---|---|---|"]
        for k, fs in forms.items():
            sr = reports[fs]
            act = "-" if not sr else f"{sr['active']} / {sr['tokens']}"
            print(f"__call__ {k:55s} {fmt(ts[k])} ms  {act}", flush=True)
            lines.append(f"| {k} | {fmt(ts[k])} | {act} |")
        pipe.disable_region_focus().disable_sparse_region().clear_edit_region()
    lines += ["", "## What these numbers do not say", "",
              "The weights are random: nothing here judges how well the checkpoint edits a crop, or how its seam blends.  What the feature guarantees is",
              "arithmetic - the box (tests/test_focus_cpu.py), the two passes bit-equal to PIL (tests/test_exact_focus_gpu.py), a focused call equal to",
              "the plain region call on `image.crop(box)` followed by PIL's resize and paste (tests/test_focus_gpu.py)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
