"""What an auto-focused edit (chronoedit_amd/autofocus.py, csrc/ce_autofocus.hip; `ChronoEditPipeline.enable_auto_focus`) costs next to the calls
it is made of: a 4032x3024 photo, the edit at 1280x720, 8 steps, detect_step 1, guidance 5, hipGraph replay on, the 14B architecture with
seeded random weights.

    passes     ce_autofocus_bbox_u8 (the photo-size mask, and the box's view of it) and ce_autofocus_restart_f32 (the 720p latents): device
               time per launch
    decision   the mask lift and both reductions of an accepted detection, against the host form (the lifted mask read to the host, then
               focus.mask_bbox and a count)
    __call__   a whole edit, PIL in, PIL out: plain, auto region (the parent commit's calls, launch for launch), explicit-mask focused (the
               mask the auto-focused call reports), auto focus cold and warm - the focused forms with and without sparse steps.
               Random weights have no region, so - as in tools/region_auto_bench.py - the scout's source latents are x0 behind step 1 of
               the plain edit, + 2.0 on a rectangle of 1/16 of the last latent frame: exactly that rectangle is detected.

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the tables as markdown.

    timeout 1100 python tools/auto_focus_bench.py [--reps 7] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_auto_focus.md]"""
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

from chronoedit_amd import autofocus, focus, ops, region  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402

H, W, G, FRAMES = 720, 1280, 5.0, 5
SW, SH = 4032, 3024
K = 1  # detect_step


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, inner=20):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(inner):
        fn()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / inner


def alternate(fns, reps, timer, warm=1):
    """{name: [ms]}: warm-up calls, then the callables in turn, repetition by repetition."""
    for _ in range(warm):
        for fn in fns.values():
            timer(fn)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timer(fn))
    return ts


def fmt(ts, unit=1.0, digits=1):
    return f"{statistics.median(ts) * unit:.{digits}f} ({min(ts) * unit:.{digits}f} .. {max(ts) * unit:.{digits}f})"


def photo():
    from PIL import Image
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:SH, 0:SW].astype(np.float32)
    base = np.stack([xx * (255.0 / SW), yy * (255.0 / SH), (xx + yy) * (255.0 / (SW + SH))], axis=2)
    return Image.fromarray(np.clip(base + rng.normal(0, 20, base.shape).astype(np.float32), 0, 255).astype(np.uint8))


def sixteenth_rect(h, w):
    """Rows and columns of a rectangle of 1/16 of an h x w plane, on even cells, right of and above the centre."""
    hh, ww = h // 4 // 2 * 2, w // 4 // 2 * 2
    y0, x0 = int(h * 0.4 - hh / 2) // 2 * 2, int(w * 0.62 - ww / 2) // 2 * 2
    return slice(y0, y0 + hh), slice(x0, x0 + ww)


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
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes and the decision only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_auto_focus.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("auto_focus_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    T, h, w = (FRAMES - 1) // 4 + 1, H // 8, W // 8
    rect = sixteenth_rect(h, w)
    lines = ["# Auto-focused edits: what the scout, the decision and the two starts cost", "",
             f"`tools/auto_focus_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
             f"commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, the edit at {W}x{H} ({FRAMES} frames, {T} latent frames), detect_step {K}, context {a.context:g}, guidance {G:g}, graph replay on.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]

    # ---- the passes --------------------------------------------------------------------------------------------------------------------
    # the detection's edit-size mask of the 1/16 rectangle (dilate 1, feather 1), as auto_region.detect leaves it
    wts = torch.zeros((h, w), dtype=torch.float32, device=dev)
    wts[rect[0].start - 2:rect[0].stop + 2, rect[1].start - 2:rect[1].stop + 2] = 0.5
    wts[rect[0].start - 1:rect[0].stop + 1, rect[1].start - 1:rect[1].stop + 1] = 1.0
    mask_edit = ops.auto_region_mask_u8(wts)
    mask_src = autofocus.lift_mask(mask_edit, (SW, SH))
    rep = autofocus.plan(mask_src, (W, H), a.context)
    l, t, r, b = box = rep["box"]
    print(f"plan: {rep}", flush=True)
    view, out5 = mask_src[t:b, l:r], torch.empty(5, dtype=torch.int32, device=dev)
    x0 = torch.randn((1, 16, T, h, w), generator=g, device=dev)
    eps, mixed = torch.randn_like(x0), torch.empty_like(x0)
    tabs = autofocus.restart_tables(box, (SW, SH), (h, w), dev)
    passes = {f"ce_autofocus_bbox_u8, the {SW}x{SH} mask": (lambda: ops.autofocus_bbox_u8(mask_src, out=out5), SW * SH),
              f"ce_autofocus_bbox_u8, the box's {r - l}x{b - t} view (pitch {SW})": (lambda: ops.autofocus_bbox_u8(view, out=out5), (r - l) * (b - t)),
              f"ce_autofocus_restart_f32, 16 x {T} x {h} x {w}": (lambda: ops.autofocus_restart(x0, eps, tabs, 0.9, out=mixed), 12 * x0.numel()),
              "ce_autofocus_restart_f32, bf16 state": (lambda: ops.autofocus_restart(x0, eps, tabs, 0.9, True, out=mixed), 12 * x0.numel())}
    ts = alternate({k: v[0] for k, v in passes.items()}, max(a.reps, 10), device_ms)
    lines += ["## The passes", "", "Device time per call (events on the stream around 20 calls back to back, divided) and the rate that makes of the bytes the pass has",
              "to move.  A bbox call is two launches (the five integers are initialised by the call itself).", "", "| pass | bytes | us | GB/s |", "|---|---|---|---|"]
    for k_, (_, nbytes) in passes.items():
        med = statistics.median(ts[k_])
        print(f"{k_:75s} {nbytes / 1e6:9.2f} MB  {fmt(ts[k_], 1e3)} us  {nbytes / med / 1e6:8.1f} GB/s", flush=True)
        lines.append(f"| `{k_}` | {nbytes / 1e6:.2f} MB | {fmt(ts[k_], 1e3)} | {nbytes / med / 1e6:.0f} |")

    # ---- the decision: lift and two reductions, against the host form ---------------------------------------------------------------
    def decide_device():
        return autofocus.plan(autofocus.lift_mask(mask_edit, (SW, SH)), (W, H), a.context)

    def decide_host():
        m = autofocus.lift_mask(mask_edit, (SW, SH)).cpu()  # the 12 MB read
        bx, why = focus.focus_box(focus.mask_bbox(m), (SW, SH), (W, H), a.context)
        return {"box": bx, "reason": why, "mask_fraction_of_box": float((m[bx[1]:bx[3], bx[0]:bx[2]] > 0).sum()) / ((bx[2] - bx[0]) * (bx[3] - bx[1]))}

    dd, dh = decide_device(), decide_host()
    same = all(dd[k_] == dh[k_] for k_ in dh)
    ts = alternate({"device": decide_device, "host": decide_host}, max(a.reps, 10), wall, warm=2)
    lines += ["", "## The decision of an accepted detection", "",
              f"The {W}x{H} mask -> `focus.resize_l8` to {SW}x{SH} -> the bounding box and the mask's share of the box.  Device form: two reductions, five integers",
              f"read each.  Host form: the lifted mask read to the host ({SW * SH / 1e6:.1f} MB), `focus.mask_bbox`, a count.  Host clock, device idle before; both give the",
              f"same plan: **{same}**.", "", "| form | ms |", "|---|---|", f"| device reductions | {fmt(ts['device'], digits=2)} |",
              f"| `.cpu()` + `focus.mask_bbox` | {fmt(ts['host'], digits=2)} |"]
    print(f"decision: device {fmt(ts['device'], digits=2)} ms, host {fmt(ts['host'], digits=2)} ms, same plan {same}", flush=True)
    del passes, view, x0, eps, mixed

    # ---- the whole edit -------------------------------------------------------------------------------------------------------------
    if not a.no_edit:
        import bench  # build_model: the 14B architecture with seeded random weights
        from transformers import CLIPImageProcessor

        from chronoedit_amd.clip_vision import CLIPVisionModel
        from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
        from chronoedit_amd.vae import AutoencoderKLWan
        torch.manual_seed(0)
        im = photo()
        model = bench.build_model(a.layers, dev)
        vae = AutoencoderKLWan.random_init(dev, seed=4321)
        pipe = ChronoEditPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0),
                                  image_encoder=CLIPVisionModel(device=dev), image_processor=CLIPImageProcessor())
        pos = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        neg = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        lat0 = torch.randn((1, 16, T, h, w), generator=g, device=dev)
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=FRAMES, num_inference_steps=a.steps, guidance_scale=G)
        seen = {}

        def grab(p, i, t_, kws):
            if i == K:
                seen["x0"] = p.scheduler.model_outputs[-1].clone()
            return {}

        pipe(image=im, latents=lat0.clone(), output_type="latent", callback_on_step_end=grab, **kw)
        z_e = seen["x0"].clone()
        z_e[:, :, -1, rect[0], rect[1]] += 2.0
        real, scout = region.static_source_latents, {"next": False}

        def source_latents(vae_, image, nf):
            """The VAE encode still runs (its cost belongs to the edit); for the whole-photo pass of a detecting call what it returns is replaced
            by the source latents that have a region.  The crop's pass keeps its own."""
            lat = real(vae_, image, nf)
            if scout["next"]:
                scout["next"] = False
                return z_e
            return lat

        region.static_source_latents = source_latents
        reports, found = {}, {}

        def edit(form, sparse=False, output_type="pil"):
            pipe.disable_auto_region().disable_auto_focus().disable_region_focus().clear_edit_region().disable_sparse_region()
            if sparse:
                pipe.enable_sparse_region(2)
            if form in ("auto region", "auto focus, cold", "auto focus, warm"):
                pipe.enable_auto_region(K)
                scout["next"] = True
            if form.startswith("auto focus"):
                pipe.enable_auto_focus(a.context, warm_start=form.endswith("warm"))
            if form == "explicit-mask focused":
                pipe.set_edit_region(found["mask"]).enable_region_focus(a.context)
            frames = pipe(image=im, latents=lat0.clone(), output_type=output_type, **kw).frames
            reports[(form, sparse)] = (pipe.focus_report, model.sparse_report)
            return frames

        frames = edit("auto focus, cold")
        fr = pipe.focus_report[0]
        assert fr["reason"] == "ok" and fr["detect"]["accepted"], fr
        found["mask"] = fr["mask"]
        keep = np.asarray(fr["mask"]) == 0
        exact = frames[0][0].size == im.size and all(np.array_equal(np.asarray(f)[keep], np.asarray(im)[keep]) for f in frames[0])
        same_frames = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(frames[0], edit("explicit-mask focused")[0]))
        print(f"auto focus: box {fr['box']} scale {fr['scale']:.3f}, the mask covers {fr['mask_fraction_of_box']:.3f} of it; the photo's bytes where the mask is 0: "
              f"{exact}; cold start equals the explicit-mask focused call: {same_frames}", flush=True)
        del frames
        forms = [("plain", False), ("auto region", False), ("auto region", True), ("explicit-mask focused", False), ("explicit-mask focused", True),
                 ("auto focus, cold", False), ("auto focus, cold", True), ("auto focus, warm", False), ("auto focus, warm", True)]
        for fs in forms:  # warm-up: packs the engine, captures the graphs of every form
            edit(*fs)
        ts = alternate({fs: (lambda fs=fs: edit(*fs)) for fs in forms}, max(3, a.reps // 2), wall)
        med = {fs: statistics.median(ts[fs]) for fs in forms}
        bw, bh = fr["box"][2] - fr["box"][0], fr["box"][3] - fr["box"][1]
        lines += ["", f"## A whole {a.steps}-step `__call__`, PIL in, PIL out, {FRAMES} frames", "",
                  f"`plain` and `auto region` are the parent commit's calls, launch for launch: the photo is resized to {W}x{H} and {W}x{H} frames come back.  The",
                  f"focused forms edit the {bw}x{bh} box (scale {fr['scale']:.3f}, the mask covers {fr['mask_fraction_of_box']:.3f} of it) and return {SW}x{SH} frames - the",
                  f"photo's bytes exactly where the mask is 0, in every frame: **{exact}**.  The explicit-mask focused call is given the mask the auto-focused",
                  f"call reports; the cold start returns its frames bit for bit: **{same_frames}**.  Sparse: `enable_sparse_region(refresh_every=2)`.", "",
                  "| edit | sparse steps | plan of the (last) loop | active / tokens | ms | against plain |", "|---|---|---|---|---|---|"]
        for fs in forms:
            sr = reports[fs][1]
            plan = "" if not sr else "".join(k_[0] for k_ in sr["plan"])
            act = "" if not sr else f"{sr['active']} / {sr['tokens']}"
            print(f"__call__ {fs[0]:25s} sparse={fs[1]!s:5s} {plan:10s} {act:14s} {fmt(ts[fs])} ms  x{med[fs] / med[('plain', False)]:.3f}", flush=True)
            lines.append(f"| {fs[0]} | {'yes' if fs[1] else 'no'} | {plan} | {act} | {fmt(ts[fs])} | x {med[fs] / med[('plain', False)]:.3f} |")
        step = med[("plain", False)] / a.steps
        lines += ["", "Plan letters: c = compute, r = refresh, s = sparse (of the focused pass where there is one; a warm start's plan covers the tail only).", "",
                  "## The two expectations", "",
                  f"A dense step of the whole photo is at most {step:.0f} ms (the plain call over its {a.steps} steps, encoders and decode included).", "",
                  "| difference | dense | sparse |", "|---|---|---|"]
        for name, x, y in (("cold - explicit-mask focused (expected: k + 1 dense steps and one encode pair)", "auto focus, cold", "explicit-mask focused"),
                           ("cold - warm (expected: k + 1 steps of the focused pass)", "auto focus, cold", "auto focus, warm")):
            lines.append(f"| {name} | {med[(x, False)] - med[(y, False)]:.0f} ms | {med[(x, True)] - med[(y, True)]:.0f} ms |")
            print(f"{name}: dense {med[(x, False)] - med[(y, False)]:.0f} ms, sparse {med[(x, True)] - med[(y, True)]:.0f} ms", flush=True)
        region.static_source_latents = real
        pipe.disable_auto_region().disable_auto_focus().disable_region_focus().clear_edit_region().disable_sparse_region()
    lines += ["", "## What these numbers do not say", "",
              "The weights are random and the region is planted in the source latents: nothing here judges whether step k's estimate locates a real edit,",
              "whether a checkpoint rebuilds detail from a bilinearly resampled estimate at sigma k + 1, or which `detect_step` makes the warm start",
              "acceptable - `measure_auto_region` on the loaded checkpoint is the tool for that.  What the feature guarantees is arithmetic: the tables and",
              "the tail schedule (tests/test_autofocus_cpu.py), the two passes bit-equal to their CPU expressions (tests/test_exact_autofocus_gpu.py), the",
              "cold start equal to the explicit-mask focused call and the warm start to a second implementation (tests/test_autofocus_gpu.py)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
