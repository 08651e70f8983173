"""What the detail lift inside focus boxes (chronoedit_amd/boxlift.py, csrc/ce_boxlift.hip; `enable_detail_lift(focus=True)`) costs: the
4032x3024 bench photo, the edit at 1280x720, radius 4, 2 and 29 frames, the 14B architecture with seeded random weights.  Two kinds of boxes:
the elliptic mask of region_focus_bench.py (one box) and the two-corner strokes of sketch_crops_bench.py (two crops of one photo).

    fused      ce_boxlift_apply_paste_u8 against the composition it replaces, in the same run: ce_lift_apply_u8 on the contiguous crop, then
               ce_clusters_paste_u8 of the lifted box - with mask NULL, with the bench's mask, and with an all-zero mask
    out        the whole output stage behind the decode: the focused call's paste-back (`focus.paste` / `clusters.paste`) against
               the same calls with `lift=` (`boxlift.output`), for 2 and 29 frames
    __call__   a whole 8-step edit, PIL in, PIL out: focused against focused + lift, for the one box and for the two crops

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 1100 python tools/focus_lift_bench.py [--reps 7] [--layers 40] [--no-edit] [--commit HASH] [--out profiles/notes_focus_lift.md]"""
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
from sketch_crops_bench import FEATHER, GROW, photo_and_composite  # noqa: E402

from chronoedit_amd import clusters, focus, image_io, lift, ops, sketch  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline  # noqa: E402


def fused_against_composition(name, plan, F, cfg, g, reps, lines):
    """One box, F frames: the cells of a real fit, then the fused pass and the composition with three masks -> {form: median ms}."""
    dev = plan.src_u8.device
    P, L, (l, t, r, b) = plan.src_u8, plan.lift_L, plan.box
    bw, bh = r - l, b - t
    E = edited_frames(L, F, g)
    AB = ops.lift_fit_q16(L, E, cfg.radius, cfg.eps_q, cfg.max_gain)
    coef, R = ops.lift_smooth(L, E, AB, cfg.radius)
    ops.lift_gate(R, coef, cfg.radius, *cfg.gate)
    U = torch.stack([image_io.resize_u8(f, (bw, bh), image_io.LANCZOS) for f in E]).contiguous()
    tabs = lift.tables((bw, bh), (H, W), dev)
    Pc = P[t:b, l:r].contiguous()
    Q = torch.empty((F, bh, bw, 3), dtype=torch.uint8, device=dev)
    src = P if plan.paste_u8 is None else plan.paste_u8
    canvas = src.unsqueeze(0).repeat(F, 1, 1, 1).contiguous()
    masks = {"mask NULL": None, "the bench's mask": plan.mask_dev, "an all-zero mask": torch.zeros_like(plan.mask_dev)}
    share = float((plan.mask_dev[t:b, l:r] > 0).float().mean())
    # the two give the same canvas (each from a fresh one)
    same = True
    for m in masks.values():
        a, c = canvas.clone(), canvas.clone()
        ops.boxlift_apply_paste_u8(P, coef, tabs, U, m, a, l, t, bw, bh)
        ops.clusters_paste_u8(ops.lift_apply_u8(Pc, coef, tabs, U, out=Q), m, c, l, t)
        same = same and torch.equal(a, c)
        del a, c
    fns = {}
    for k, m in masks.items():
        fns[f"fused, {k}"] = lambda m=m: ops.boxlift_apply_paste_u8(P, coef, tabs, U, m, canvas, l, t, bw, bh)
        fns[f"apply + paste, {k}"] = lambda m=m: ops.clusters_paste_u8(ops.lift_apply_u8(Pc, coef, tabs, U, out=Q), m, canvas, l, t)
    fns["ce_lift_apply_u8 on the crop alone"] = lambda: ops.lift_apply_u8(Pc, coef, tabs, U, out=Q)
    ts = alternate(fns, max(reps, 10), device_ms)
    med = {k: statistics.median(v) for k, v in ts.items()}
    for k in fns:
        print(f"{name} F={F:2d} {k:45s} {fmt(ts[k], 1e3)} us", flush=True)
    for k in masks:
        lines.append(f"| {name}: {bw}x{bh}, mask over {share:.3f} of it, mean g {float(coef[..., 6].mean()):.3f} | {F} | {k} | {fmt(ts['fused, ' + k], 1e3)} | "
                     f"{fmt(ts['apply + paste, ' + k], 1e3)} | {med['fused, ' + k] / med['apply + paste, ' + k]:.2f} | {same} |")
    lines.append(f"| | {F} | (`ce_lift_apply_u8` on the crop alone) | | {fmt(ts['ce_lift_apply_u8 on the crop alone'], 1e3)} | | |")
    return med, share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes and the output stage only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_focus_lift.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("focus_lift_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    cfg = lift.LiftConfig(radius=a.radius)
    im, mask = photo_and_mask()
    bg, cp = photo_and_composite()
    value = {"background": bg, "composite": cp}
    lines = ["# Detail lift inside focus boxes: what lifting a crop before the paste costs", "",
             f"`tools/focus_lift_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps} --radius {a.radius}` on {torch.cuda.get_device_name(0)}, torch "
             f"{torch.__version__}, commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, the edit at {W}x{H}, radius {cfg.radius}, eps {cfg.eps:g}, gate {cfg.gate}, max_gain {cfg.max_gain:g}.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions.", ""]

    # ---- the plans: one box from the elliptic mask, two crops from the strokes ------------------------------------------------------
    plans = focus.setup(im, mask, H, W, 0.25, "pil", dev)
    focus.inputs(plans, H, W, dev, keep_L=True)
    entry = sketch.masks(sketch.SketchConfig(GROW, FEATHER, max_crops=2), [bg], [cp], dev)[0]
    crops = clusters.plan(entry, 2, W, H, 0.25)
    assert crops.reason == "crops" and len(crops.plans) == 2, crops.reason
    focus.inputs(crops.plans, H, W, dev, keep_L=True)
    crop_of = [(0, 0), (0, 1)]
    lines += ["The boxes: " + "; ".join(f"{n} {p.box} = {p.box[2] - p.box[0]}x{p.box[3] - p.box[1]}, scale {p.report['scale']:.3f}, the mask over "
                                        f"{p.report['mask_fraction_of_box']:.3f} of it" for n, p in (("ellipse", plans[0]), ("crop 0", crops.plans[0]), ("crop 1", crops.plans[1]))) + ".", ""]

    # ---- the fused pass against the composition ------------------------------------------------------------------------------------
    lines += ["## The fused pass against the composition it replaces", "",
              "Device time per call (events on the stream around 10 calls back to back, divided).  The composition is `ce_lift_apply_u8` on the contiguous",
              "crop followed by `ce_clusters_paste_u8` of the lifted box into the same canvas; `equal` says that both left the same canvas bytes.  E is",
              "`lift_bench.py`'s drifting tone curve with one rectangle of noise, the cells are its fit.", "",
              "| box | frames | mask | fused, us | apply + paste, us | fused / composition | equal |", "|---|---|---|---|---|---|---|"]
    for F in (2, 29):
        for name, p in (("ellipse", plans[0]), ("crop 1", crops.plans[1])):
            fused_against_composition(name, p, F, cfg, g, a.reps, lines)

    # ---- the output stage behind the decode ------------------------------------------------------------------------------------------
    lines += ["", "## The output stage behind the decode", "",
              "`ce_video_to_u8` -> per frame the Lanczos upsample to the box -> (lift: fit, smooth, gate, the fused pass; plain: the paste) -> one",
              "device-to-host copy -> `Image.fromarray` per frame, ending with PIL frames of the photo's size.", "",
              "| boxes | frames | focused paste-back, ms | focused + lift, ms | difference, ms |", "|---|---|---|---|---|"]
    for F in (2, 29):
        for name, ps, co in (("ellipse", plans, None), ("two crops", crops.plans, crop_of)):
            video = (torch.rand((len(ps), 3, F, H, W), generator=g, device=dev) * 2.2 - 1.1).to(torch.bfloat16)
            image_of = lambda b_: 0
            forms = {"plain": (lambda: focus.paste(video, ps, image_of, "pil", True)) if co is None else (lambda: clusters.paste(video, ps, co, "pil", True)),
                     "lift": (lambda: focus.paste(video, ps, image_of, "pil", True, lift=cfg)) if co is None else (lambda: clusters.paste(video, ps, co, "pil", True, lift=cfg))}
            ts = alternate(forms, max(3, a.reps // 2), wall)
            m = {k: statistics.median(v) for k, v in ts.items()}
            print(f"output stage {name} {F} frames: plain {fmt(ts['plain'])} ms, lifted {fmt(ts['lift'])} ms", flush=True)
            lines.append(f"| {name} | {F} | {fmt(ts['plain'])} | {fmt(ts['lift'])} | {m['lift'] - m['plain']:+.1f} |")
            del video, forms
    del plans, crops, entry

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
            boxes, lifted = form
            pipe.disable_detail_lift().disable_region_focus().clear_edit_region().disable_sketch_region()
            if lifted:
                pipe.enable_detail_lift(radius=a.radius, focus=True)
            if boxes == "ellipse":
                pipe.enable_region_focus(0.25).set_edit_region(mask)
                frames = pipe(image=im, latents=lat0.clone(), **kw).frames
            else:
                pipe.enable_sketch_region(grow=GROW, feather=FEATHER, max_crops=2)
                frames = pipe(image=value, latents=lat0.clone(), **kw).frames
            reports[form] = pipe.lift_report
            return frames

        names = {("ellipse", False): "focused region edit, the elliptic mask", ("ellipse", True): "... + lift inside the box",
                 ("crops", False): "sketch edit, two crops", ("crops", True): "... + lift inside the boxes"}
        for form in names:  # warm-up: packs the engine, captures the graphs
            edit(form), edit(form)
        ts = alternate({form: (lambda form=form: edit(form)) for form in names}, max(2, a.reps // 2), wall)
        lines += ["", f"## A whole {a.steps}-step `__call__`, PIL in, PIL out, 5 frames", "",
                  "The synthetic VAE decodes noise, so the fitted gate is nearly 1 everywhere (fallback_fraction "
                  + ", ".join(f"{r['fallback_fraction']:.3f}" for f_ in names if f_[1] for r in reports[f_]) + "): every byte of U is read.", "",
                  "| edit | ms |", "|---|---|"]
        for form, name in names.items():
            print(f"__call__ {name:50s} {fmt(ts[form])} ms", flush=True)
            lines.append(f"| {name} | {fmt(ts[form])} |")
        pipe.disable_detail_lift().disable_region_focus().clear_edit_region().disable_sketch_region()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
