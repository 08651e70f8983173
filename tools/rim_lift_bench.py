"""What the mask-aware detail lift (chronoedit_amd/rimlift.py, csrc/ce_rimlift.hip; `enable_detail_lift(focus=True, mask_aware=True)`) costs:
the 4032x3024 bench photo with the elliptic mask of region_focus_bench.py, the edit at 1280x720, radius 4, the 14B architecture with seeded
random weights.

    passes     ce_rimlift_fit_q16 / ce_rimlift_smooth_f32 next to ce_lift_fit_q16 / ce_lift_smooth_f32 on the same crop, in the same run, for
               2 and 29 frames - and ce_lift_gate_f32, which both chains share
    __call__   a whole 8-step focused edit, PIL in, PIL out, with the switch off and on

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the tables as markdown.

    timeout 900 python tools/rim_lift_bench.py [--reps 7] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_rim_lift.md]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lift_bench import edited_frames  # noqa: E402
from region_focus_bench import H, W, SH, SW, G, alternate, commit, device_ms, fmt, photo_and_mask, wall  # noqa: E402

from chronoedit_amd import focus, lift, ops, rimlift  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402


def passes(plan, F, cfg, g, reps, lines):
    """One crop, F frames blended by the edit-size mask: the two pairs of passes and the gate -> {form: median ms}."""
    L, M = plan.lift_L, plan.lift_M
    T = edited_frames(L, F, g).float()
    w = (M.float() / 255.0)[None, ..., None]
    E = (L.float() + w * (T - L.float())).round().clamp(0, 255).to(torch.uint8).contiguous()
    AB, ABm = ops.lift_fit_q16(L, E, cfg.radius, cfg.eps_q, cfg.max_gain), ops.rimlift_fit_q16(L, E, M, cfg.radius, cfg.eps_q, cfg.max_gain)
    (coef, R), (coefm, Rm) = ops.lift_smooth(L, E, AB, cfg.radius), ops.rimlift_smooth(L, E, M, ABm, cfg.radius)
    means = [float(ops.lift_gate(r_, c_, cfg.radius, *cfg.gate)[..., 6].mean()) for r_, c_ in ((R, coef), (Rm, coefm))]
    fns = {"ce_lift_fit_q16": lambda: ops.lift_fit_q16(L, E, cfg.radius, cfg.eps_q, cfg.max_gain, out=AB),
           "ce_rimlift_fit_q16": lambda: ops.rimlift_fit_q16(L, E, M, cfg.radius, cfg.eps_q, cfg.max_gain, out=ABm),
           "ce_lift_smooth_f32": lambda: ops.lift_smooth(L, E, AB, cfg.radius, coef=coef, R=R),
           "ce_rimlift_smooth_f32": lambda: ops.rimlift_smooth(L, E, M, ABm, cfg.radius, coef=coefm, R=Rm),
           "ce_lift_gate_f32": lambda: ops.lift_gate(R, coef, cfg.radius, *cfg.gate)}
    ts = alternate(fns, max(reps, 10), device_ms)
    med = {k: statistics.median(v) for k, v in ts.items()}
    for k in fns:
        print(f"F={F:2d} {k:24s} {fmt(ts[k], 1e3)} us", flush=True)
    plain = med["ce_lift_fit_q16"] + med["ce_lift_smooth_f32"] + med["ce_lift_gate_f32"]
    masked = med["ce_rimlift_fit_q16"] + med["ce_rimlift_smooth_f32"] + med["ce_lift_gate_f32"]
    lines.append(f"| {F} | {fmt(ts['ce_lift_fit_q16'], 1e3)} | {fmt(ts['ce_rimlift_fit_q16'], 1e3)} | {fmt(ts['ce_lift_smooth_f32'], 1e3)} | "
                 f"{fmt(ts['ce_rimlift_smooth_f32'], 1e3)} | {fmt(ts['ce_lift_gate_f32'], 1e3)} | {plain * 1e3:.1f} | {masked * 1e3:.1f} | {masked / plain:.2f} | "
                 f"{means[0]:.3f} / {means[1]:.3f} |")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_rim_lift.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rim_lift_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    cfg = lift.LiftConfig(radius=a.radius)
    im, mask = photo_and_mask()
    lines = ["# Mask-aware detail lift: what fitting under the region's weights costs", "",
             f"`tools/rim_lift_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps} --radius {a.radius}` on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}, commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, the edit at {W}x{H}, radius {cfg.radius}, eps {cfg.eps:g}, gate {cfg.gate}, max_gain {cfg.max_gain:g}.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]
    plans = focus.setup(im, mask, H, W, 0.25, "pil", dev)
    focus.inputs(plans, H, W, dev, keep_L=True)
    p = plans[0]
    lines += [f"The box: {p.box} = {p.box[2] - p.box[0]}x{p.box[3] - p.box[1]}, scale {p.report['scale']:.3f}; the edit-size weight plane is non-zero over "
              f"{float((p.lift_M > 0).float().mean()):.3f} of the crop and between 1 and 254 over {float(((p.lift_M > 0) & (p.lift_M < 255)).float().mean()):.3f} of it.", "",
              "## The two masked passes next to the plain ones", "",
              "Device time per call (events on the stream around 10 calls back to back, divided), in us.  The frames are `lift_bench.py`'s drifting tone",
              "curve with one rectangle of noise, blended with the source by the weight plane.  The chains are fit + smooth + gate; the gate pass is shared.", "",
              "| frames | `ce_lift_fit_q16` | `ce_rimlift_fit_q16` | `ce_lift_smooth_f32` | `ce_rimlift_smooth_f32` | `ce_lift_gate_f32` | plain chain | masked chain | "
              "masked / plain | mean g, plain / masked |", "|---|---|---|---|---|---|---|---|---|---|"]
    for F in (2, 29):
        passes(p, F, cfg, g, a.reps, lines)
    del plans, p

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

        def edit(masked):
            pipe.enable_detail_lift(radius=a.radius, focus=True, mask_aware=masked).enable_region_focus(0.25).set_edit_region(mask)
            frames = pipe(image=im, latents=lat0.clone(), **kw).frames
            reports[masked] = pipe.lift_report
            return frames

        names = {False: "focused region edit + lift inside the box", True: "... with `mask_aware=True`"}
        for form in names:  # warm-up: packs the engine, captures the graphs
            edit(form), edit(form)
        ts = alternate({form: (lambda form=form: edit(form)) for form in names}, max(2, a.reps // 2), wall)
        lines += ["", f"## A whole {a.steps}-step focused `__call__`, PIL in, PIL out, 5 frames, {a.layers} layers", "",
                  "The synthetic VAE decodes noise, so the gate is nearly 1 with either fit (fallback_fraction "
                  + " / ".join(f"{reports[f_][0]['fallback_fraction']:.3f}" for f_ in names) + ").", "", "| edit | ms |", "|---|---|"]
        for form, name in names.items():
            print(f"__call__ {name:50s} {fmt(ts[form])} ms", flush=True)
            lines.append(f"| {name} | {fmt(ts[form])} |")
        pipe.disable_detail_lift().disable_region_focus().clear_edit_region()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
