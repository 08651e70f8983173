"""What the guided detail lift (chronoedit_amd/lift.py, csrc/ce_lift.hip; `ChronoEditPipeline.enable_detail_lift`) costs: a 4032x3024 photo, the
edit at 1280x720, radius 4, 2 and 29 frames, the 14B architecture with seeded random weights.

    passes     ce_lift_fit_q16, ce_lift_smooth_f32, ce_lift_gate_f32 and ce_lift_apply_u8 (g = 0 / mixed / 1 everywhere, and without a fallback
               plane): device time per launch; the apply's rate over P + U + out next to ce_focus_paste_u8's on the same photo (a whole-photo
               box, no mask: the same bytes written, the same bytes read)
    out        the whole output stage behind the decode (`lift.output`: uint8, the Lanczos upsample of every frame, the four passes, one copy
               to the host, PIL frames) for 2 and 29 frames, with and without the gate, next to the focused call's paste-back
    __call__   a whole 8-step edit, PIL in, PIL out: plain (edit-size frames), lifted, lifted with gate=None, and the focused call

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 1100 python tools/lift_bench.py [--reps 7] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_lift.md]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from region_focus_bench import H, W, SH, SW, G, alternate, commit, device_ms, fmt, photo_and_mask, wall  # noqa: E402

from chronoedit_amd import focus, image_io, lift, ops  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402


def edited_frames(L: torch.Tensor, F: int, g: torch.Generator) -> torch.Tensor:
    """F edit-size frames the lift has something to do with: a tone curve and a tint that drift from frame to frame (the affine model
    explains them), and one rectangle of noise (it does not: the gate opens there)."""
    x = L.float() / 255.0
    out = []
    for f in range(F):
        e = x ** (0.7 + 0.01 * f) * torch.tensor([1.05, 0.95, 0.85], device=L.device) * 255.0
        e[H // 3:H // 3 + H // 6, W // 2:W // 2 + W // 5] = torch.rand((H // 6, W // 5, 3), generator=g, device=L.device) * 255.0
        out.append(e.clamp(0, 255).round().to(torch.uint8))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes and the output stage only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_lift.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lift_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    im, mask = photo_and_mask()
    cfg = lift.LiftConfig(radius=a.radius)
    lines = ["# Guided detail lift: what returning a whole-image edit at the photo's size costs", "",
             f"`tools/lift_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps} --radius {a.radius}` on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}, commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, the edit at {W}x{H}, radius {cfg.radius}, eps {cfg.eps:g}, gate {cfg.gate}, max_gain {cfg.max_gain:g}.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------
    P = image_io.upload_rgb(im, dev)
    L = image_io.resize_u8(P, (W, H), image_io.LANCZOS)
    tabs = lift.tables((SW, SH), (H, W), dev)
    lines += ["## The passes", "", "Device time per launch (events on the stream around 10 launches back to back, divided).  The rate is the bytes the pass has to move",
              "over that time: for the apply P + U + out (U only where it is read), for the paste src + edit + out - with a whole-photo box and no mask the",
              "same volume.  The coefficient grid (29.5 MB per frame) is not counted.", "",
              "| pass | frames | bytes | us | GB/s |", "|---|---|---|---|---|"]
    ratio = {}
    for F in (2, 29):
        E = edited_frames(L, F, g)
        U = torch.stack([image_io.resize_u8(f, (SW, SH), image_io.LANCZOS) for f in E])
        AB = ops.lift_fit_q16(L, E, cfg.radius, cfg.eps_q, cfg.max_gain)
        coef, R = ops.lift_smooth(L, E, AB, cfg.radius)
        ops.lift_gate(R, coef, cfg.radius, *cfg.gate)
        gmean = float(coef[..., 6].mean())
        c0, c1 = coef.clone(), coef.clone()
        c0[..., 6], c1[..., 6] = 0.0, 1.0
        out = torch.empty((F, SH, SW, 3), dtype=torch.uint8, device=dev)
        frame, cells = SH * SW * 3, F * H * W
        passes = {
            "ce_lift_fit_q16": (lambda: ops.lift_fit_q16(L, E, cfg.radius, cfg.eps_q, cfg.max_gain, out=AB), cells * 3 + H * W * 3 + cells * 24),
            "ce_lift_smooth_f32": (lambda: ops.lift_smooth(L, E, AB, cfg.radius, coef=coef, R=R), cells * (24 + 3 + 32 + 4)),
            "ce_lift_gate_f32": (lambda: ops.lift_gate(R, coef, cfg.radius, *cfg.gate), cells * 8),
            f"ce_lift_apply_u8, the fitted gate (mean g {gmean:.3f})": (lambda: ops.lift_apply_u8(P, coef, tabs, U, out=out), frame * (2 * F + 1)),
            "ce_lift_apply_u8, g = 1 everywhere": (lambda: ops.lift_apply_u8(P, c1, tabs, U, out=out), frame * (2 * F + 1)),
            "ce_lift_apply_u8, g = 0 everywhere (U given, never read)": (lambda: ops.lift_apply_u8(P, c0, tabs, U, out=out), frame * (F + 1)),
            "ce_lift_apply_u8, no fallback plane": (lambda: ops.lift_apply_u8(P, c0, tabs, None, out=out), frame * (F + 1)),
            "ce_focus_paste_u8, whole-photo box, no mask": (lambda: ops.focus_paste_u8(U, P, None, 0, 0, out=out), frame * (2 * F + 1)),
        }
        ts = alternate({k: v[0] for k, v in passes.items()}, max(a.reps, 10), device_ms)
        med = {k: statistics.median(v) for k, v in ts.items()}
        for k, (_, nbytes) in passes.items():
            print(f"F={F:2d} {k:60s} {nbytes / 1e6:9.2f} MB  {fmt(ts[k], 1e3)} us  {nbytes / med[k] / 1e6:8.1f} GB/s", flush=True)
            lines.append(f"| `{k}` | {F} | {nbytes / 1e6:.1f} MB | {fmt(ts[k], 1e3)} | {nbytes / med[k] / 1e6:.0f} |")
        ratio[F] = med["ce_focus_paste_u8, whole-photo box, no mask"] / med["ce_lift_apply_u8, g = 1 everywhere"]
        del passes, E, U, AB, coef, R, c0, c1, out
    lines += ["", "The apply's rate with every byte of U read, over the paste's on the same photo in the same run: "
              + ", ".join(f"**{ratio[F]:.2f}** at {F} frames" for F in ratio) + "."]

    # ---- the output stage behind the decode ------------------------------------------------------------------------------------------
    kept = [(P, L)]
    plans = focus.setup(im, mask, H, W, 0.25, "pil", dev)
    lines += ["", "## The output stage behind the decode", "",
              "`ce_video_to_u8` -> (with a gate) per frame the Lanczos upsample to the photo's size -> the four passes -> one device-to-host copy ->",
              "`Image.fromarray` per frame, ending with PIL frames of the photo's size; next to it the focused call's paste-back of the same frames",
              "(`focus.paste`: Lanczos to the box, paste).  The host form (`lift.reference`) is not measured at this size.", "",
              "| frames | lifted, ms | per frame | lifted, gate=None, ms | per frame | focused paste-back, ms | per frame |", "|---|---|---|---|---|---|---|"]
    for F in (2, 29):
        video = (torch.rand((1, 3, F, H, W), generator=g, device=dev) * 2.2 - 1.1).to(torch.bfloat16)
        post = lambda c: lift.output(video, c, kept, [im], lambda b_: 0, H, W, "pil")[0]
        forms = {"lift": lambda: post(cfg), "nogate": lambda: post(lift.LiftConfig(radius=a.radius, gate=None)),
                 "focus": lambda: focus.paste(video, plans, lambda b_: 0, "pil", True)}
        ts = alternate(forms, max(3, a.reps // 2), wall)
        m = {k: statistics.median(v) for k, v in ts.items()}
        print(f"output stage {F} frames: lifted {fmt(ts['lift'])} ms, gate=None {fmt(ts['nogate'])} ms, focused paste-back {fmt(ts['focus'])} ms", flush=True)
        lines.append(f"| {F} | {fmt(ts['lift'])} | {m['lift'] / F:.1f} | {fmt(ts['nogate'])} | {m['nogate'] / F:.1f} | {fmt(ts['focus'])} | {m['focus'] / F:.1f} |")
        del video
    del plans

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
        reports = {}

        def edit(form):
            pipe.disable_detail_lift().disable_region_focus().clear_edit_region()
            if form == "focused":
                pipe.enable_region_focus(0.25).set_edit_region(mask)
            elif form != "plain":
                pipe.enable_detail_lift(radius=a.radius, gate=None if form == "nogate" else cfg.gate)
            frames = pipe(image=im, latents=lat0.clone(), **kw).frames
            reports[form] = pipe.lift_report
            return frames

        names = {"plain": f"plain: {W}x{H} frames (the parent commit's call)", "lift": f"lifted: {SW}x{SH} frames", "nogate": f"lifted, gate=None: {SW}x{SH} frames",
                 "focused": f"focused region edit (a mask over 1/16 of the photo): {SW}x{SH} frames"}
        for form in names:  # warm-up: packs the engine, captures the graphs
            edit(form), edit(form)
        sizes = {form: edit(form)[0][0].size for form in names}
        print(f"frame sizes: {sizes}; lift report {reports['lift']}", flush=True)
        ts = alternate({form: (lambda form=form: edit(form)) for form in names}, max(3, a.reps // 2), wall)
        lines += ["", f"## A whole {a.steps}-step `__call__`, PIL in, PIL out, 5 frames", "",
                  f"The same {SW}x{SH} photo goes into every form.  The synthetic VAE decodes noise, so the fitted gate is nearly 1 everywhere",
                  f"(fallback_fraction {reports['lift'][0]['fallback_fraction']:.3f}): every byte of U is read - the expensive end of the apply.", "",
                  "| edit | frame size | ms |", "|---|---|---|"]
        for form, name in names.items():
            print(f"__call__ {name:75s} {fmt(ts[form])} ms", flush=True)
            lines.append(f"| {name} | {sizes[form][0]}x{sizes[form][1]} | {fmt(ts[form])} |")
        pipe.disable_detail_lift().disable_region_focus().clear_edit_region()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
