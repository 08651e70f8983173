"""What an automatic edit region (chronoedit_amd/auto_region.py, csrc/ce_region_auto.hip; `ChronoEditPipeline.enable_auto_region`) costs and
saves at the bench shape: 1280x720, 5 frames (2 latent frames, 7 200 tokens per sample), guidance 5, hipGraph replay on, the 14B
architecture with seeded random weights.

    passes     device time of the four passes (and of ce_region_blend_f32 next to them), and the detection as a whole - four launches and
               the one device-to-host read - on the host clock
    steps      the graph-replayed loop with the detector off and with it on (detecting behind a middle step and declining, so that every
               step stays the plain one): per-step device time, alternating edits of one run
    __call__   a whole 8-step edit, PIL in, PIL out: the plain edit against the auto edit (detect_step 1) dense, and sparse with
               refresh_every 2 and 4.  Random source latents have no region, so - as in tests/test_auto_region_gpu.py - z_src is x0 behind
               step 1 of the plain edit, + 2.0 on a centred rectangle of 1/4 of the last latent frame: exactly that rectangle is detected.

One process; mean and spread (sample standard deviation).  Writes the tables as markdown.

    timeout 900 python tools/region_auto_bench.py [--reps 6] [--layers 40] [--no-edit] [--out profiles/notes_region_auto.md]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd import auto_region as ar  # noqa: E402
from chronoedit_amd import ops, region  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline, denoise  # noqa: E402

H, W, FRAMES, G = 720, 1280, 5, 5.0
INNER = 50


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(INNER):
        fn()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / INNER


def ms(ts):
    return statistics.mean(ts), statistics.stdev(ts)


def alternate(fns, reps, timer, warm=1):
    for _ in range(warm):
        for fn in fns.values():
            timer(fn)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timer(fn))
    return ts


def quarter_rect(h, w):
    """Rows and columns of a centred rectangle of 1/4 of an h x w plane, on even cells."""
    hh, ww = h // 2 // 2 * 2, w // 2 // 2 * 2
    y0, x0 = (h - hh) // 2 // 2 * 2, (w - ww) // 2 // 2 * 2
    return slice(y0, y0 + hh), slice(x0, x0 + ww)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--loop-steps", type=int, default=12)
    ap.add_argument("--no-edit", action="store_true", help="passes and steps only: no VAE, no pipeline")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "notes_region_auto.md"))
    a = ap.parse_args()
    import bench  # build_model: the 14B architecture with seeded random weights
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    T, h, w = 2, H // 8, W // 8
    N = T * (h // 2) * (w // 2)
    lines = ["# Automatic edit regions: what the detection costs and what the edit behind it saves", "",
             f"`tools/region_auto_bench.py --reps {a.reps} --layers {a.layers}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  "
             f"{W}x{H}, {FRAMES} frames (2 latent frames, {N} tokens per sample), guidance {G:g}, graph replay on, seeded random weights.  One process; mean +- sample",
             "standard deviation over the repetitions.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------------
    x0 = torch.randn((1, 16, T, h, w), generator=g, device=dev)
    z = x0.clone()
    rect = quarter_rect(h, w)
    z[:, :, -1, rect[0], rect[1]] += 2.0
    cfg = ar.AutoRegionConfig(1)
    d = ops.auto_region_change(x0, z)
    thr, dmax = ops.auto_region_otsu(d)
    wts = ops.auto_region_ramp(d, thr, cfg.dilate, cfg.feather)
    mask = ops.auto_region_mask_u8(wts)
    eps, sig, xb = torch.randn_like(x0), torch.full((1,), 0.5, device=dev), x0.clone()
    fns = {"ce_auto_region_change_f32": (lambda: ops.auto_region_change(x0, z, out=d), 8 * 16 * h * w + 4 * h * w),
           "ce_auto_region_otsu_f32": (lambda: ops.auto_region_otsu(d, 0.0, thr, dmax), 8 * h * w),
           "ce_auto_region_ramp_f32": (lambda: ops.auto_region_ramp(d, thr, cfg.dilate, cfg.feather, out=wts), 8 * h * w),
           "ce_auto_region_ramp_f32 (dilate 3, feather 5)": (lambda: ops.auto_region_ramp(d, thr, 3, 5, out=wts), 8 * h * w),
           "ce_auto_region_mask_u8": (lambda: ops.auto_region_mask_u8(wts, out=mask), 4 * h * w + 64 * h * w),
           "ce_region_blend_f32 (for scale)": (lambda: ops.region_blend_(xb, z, eps, wts, sig), 16 * x0.numel() + 4 * h * w)}
    ts = alternate({k: v[0] for k, v in fns.items()}, max(a.reps, 10), device_ms)
    lines += ["## The four passes", "",
              f"Device time per launch (events around {INNER} launches back to back, divided), the {h} x {w} map of 720p, 16 channels, one sample.",
              "", "| pass | bytes moved | us per launch | GB/s |", "|---|---|---|---|"]
    for k, (_, nbytes) in fns.items():
        m_, s_ = ms(ts[k])
        print(f"{k}: {m_ * 1e3:.1f} +- {s_ * 1e3:.1f} us", flush=True)
        lines.append(f"| `{k}` | {nbytes / 1e6:.2f} MB | {m_ * 1e3:.1f} +- {s_ * 1e3:.1f} | {nbytes / (m_ * 1e-3) / 1e9:.0f} |")
    det = [wall(lambda: ar.detect(x0, z, cfg)) for _ in range(max(a.reps, 10) + 2)][2:]
    frac = ar.decide(ar.detect(x0, z, cfg)[2], cfg, 1)
    print(f"detect as a whole: {ms(det)[0] * 1e3:.0f} +- {ms(det)[1] * 1e3:.0f} us; decision {frac}", flush=True)
    lines += ["", f"The detection as a whole - the change map's allocation, four launches, the one read of w / thr / dmax, host clock, device idle before: "
              f"{ms(det)[0] * 1e3:.0f} +- {ms(det)[1] * 1e3:.0f} us.  The decision on this map: {frac[1]}, active fraction {frac[2]:.3f} with the sparse margin 1."]

    # ---- the graph-replayed loop -----------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    model = bench.build_model(a.layers, dev)
    pos = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
    neg = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
    img_emb = torch.randn((1, 257, 1280), generator=g, device=dev).to(torch.bfloat16)
    cond = torch.randn((1, 20, T, h, w), generator=g, device=dev).to(torch.bfloat16)
    lat0 = torch.randn((1, 16, T, h, w), generator=g, device=dev)
    zr = torch.randn((1, 16, T, h, w), generator=g, device=dev)  # random source latents: everything "changed", declined by max_area
    n, kd, warm = a.loop_steps, a.loop_steps // 2, set()

    def run_loop(auto):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        marks[0].record()
        denoise(model, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pos, neg, img_emb, n, G, use_graph=True, graph_warm=warm,
                on_step_end=lambda i, t, lat: marks[i + 1].record(), auto_region=ar.AutoRegion(ar.AutoRegionConfig(kd), zr) if auto else None)
        torch.cuda.synchronize()
        if auto:
            assert model.auto_region_report["reason"] == "max_area", model.auto_region_report
        return [marks[i].elapsed_time(marks[i + 1]) for i in range(n)]

    run_loop(False), run_loop(True)
    per = {"off": [], "on": [], "off_k": [], "on_k": []}
    for _ in range(a.reps):
        for name, auto in (("off", False), ("on", True)):
            t = run_loop(auto)
            per[name].append(statistics.median(t[2:kd] + t[kd + 1:]))  # (steps 0-1 hold the warm check and the capture)
            per[name + "_k"].append(t[kd])
    lines += ["", "## The graph-replayed loop", "",
              f"`denoise(use_graph=True)` over {n} steps, {a.layers} layers, edits with the detector off and on alternating in one run; on = detecting behind step {kd}",
              "and declining (random source latents: everything changed), so every step is the plain step and only the detection is added.  Device time",
              "per step between `on_step_end` marks; `other steps` is the median over the steps of an edit except 0, 1 and the detection step.  With the",
              "detector off the loop is the parent commit's, launch for launch.", "",
              "| detector | other steps ms | the detection step ms |", "|---|---|---|"]
    for name in ("off", "on"):
        (m1, s1), (m2, s2) = ms(per[name]), ms(per[name + "_k"])
        print(f"loop, detector {name}: other steps {m1:.2f} +- {s1:.2f} ms, step {kd} {m2:.2f} +- {s2:.2f} ms", flush=True)
        lines.append(f"| {name} | {m1:.2f} +- {s1:.2f} | {m2:.2f} +- {s2:.2f} |")
    del lat0, zr, cond

    # ---- the whole edit --------------------------------------------------------------------------------------------------------------------
    if not a.no_edit:
        from PIL import Image
        from transformers import CLIPImageProcessor

        from chronoedit_amd.clip_vision import CLIPVisionModel
        from chronoedit_amd.vae import AutoencoderKLWan
        vae = AutoencoderKLWan.random_init(dev, seed=4321)
        vae.use_graph = True
        pipe = ChronoEditPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0),
                                  image_encoder=CLIPVisionModel(device=dev), image_processor=CLIPImageProcessor())
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([xx * 255.0 / W, yy * 255.0 / H, (xx + yy) * 255.0 / (W + H)], axis=2)
        im = Image.fromarray(np.clip(base + np.random.default_rng(0).normal(0, 20, base.shape), 0, 255).astype(np.uint8))
        lat_e = torch.randn((1, 16, T, h, w), generator=g, device=dev)
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=FRAMES, num_inference_steps=a.steps, guidance_scale=G)
        seen = {}

        def grab(p, i, t, kws):
            if i == 1:
                seen["x0"] = p.scheduler.model_outputs[-1].clone()
            return {}

        pipe(image=im, latents=lat_e.clone(), output_type="latent", callback_on_step_end=grab, **kw)
        z_e = seen["x0"].clone()
        z_e[:, :, -1, rect[0], rect[1]] += 2.0
        real = region.static_source_latents
        # the VAE encode still runs (its cost belongs to the edit); what it returns is replaced by the source latents that have a region
        region.static_source_latents = lambda vae_, image, nf: (real(vae_, image, nf), z_e)[1]

        def edit(mode, output_type="pil"):
            pipe.disable_auto_region(), pipe.disable_sparse_region()
            if mode != "plain":
                pipe.enable_auto_region(1)
                if mode != "dense":
                    pipe.enable_sparse_region(int(mode))
            return pipe(image=im, latents=lat_e.clone(), output_type=output_type, **kw).frames

        info = {}
        for mode in ("dense", "2", "4"):
            edit(mode, "latent")
            rep, srep = pipe.auto_region_report, model.sparse_report
            assert rep["accepted"], rep
            info[mode] = (rep["active_fraction"], "c" * a.steps if srep is None else "".join(k[0] for k in srep["plan"]), None if srep is None else srep["active"])
        fns = {m_: (lambda mm: lambda: edit(mm))(m_) for m_ in ("plain", "dense", "2", "4")}
        ts = alternate(fns, max(3, a.reps // 2), wall)
        mp, sp = ms(ts["plain"])
        lines += ["", f"## A whole {a.steps}-step `__call__`, PIL in, PIL out", "",
                  "`plain` is the edit with the detector off (the parent commit's `__call__`, launch for launch).  The auto edits detect behind step 1 (defaults:",
                  "Otsu, dilate 1, feather 1) the 1/4 rectangle the source latents were given, pay one more VAE encode, the detection, the blend per step and",
                  "the paste-back, and with `enable_sparse_region` run the steps behind the first refresh on the active rows only.", "",
                  "| edit | plan | active patch fraction | active rows | ms | against plain |", "|---|---|---|---|---|---|",
                  f"| plain | {'c' * a.steps} | | | {mp:.1f} +- {sp:.1f} | |"]
        print(f"__call__ plain {mp:.1f} +- {sp:.1f} ms", flush=True)
        for mode, label in (("dense", "auto, dense"), ("2", "auto, refresh_every=2"), ("4", "auto, refresh_every=4")):
            mk, sk = ms(ts[mode])
            fr, plan, rows = info[mode]
            print(f"__call__ {label} ({plan}) {mk:.1f} +- {sk:.1f} ms  x{mk / mp:.3f}", flush=True)
            lines.append(f"| {label} | {plan} | {fr:.3f} | {'' if rows is None else rows} | {mk:.1f} +- {sk:.1f} | x {mk / mp:.3f} |")
        lines += ["", "Plan letters: c = compute, r = refresh, s = sparse."]
        region.static_source_latents = real
        pipe.disable_auto_region(), pipe.disable_sparse_region()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
