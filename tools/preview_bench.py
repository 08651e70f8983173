"""What live previews (chronoedit_amd/preview.py, csrc/ce_preview.hip; `ChronoEditPipeline.enable_preview`) cost at the bench shape:
1280x720, 5 frames (2 latent frames, 7 200 tokens per sample), guidance 5, hipGraph replay on, the 14B architecture with seeded random
weights.

    kernel     device time of ce_preview_rgb_u8 per scale, with and without the region composite
    steps      the graph-replayed loop with previews off and on (scale 2 and 8, every=1, lag=1): per-step device time between
               `on_step_end` marks and the wall time of the whole loop, alternating edits of one run, against the spread of the off leg
    delivery   host time of one delivery (event wait on a finished copy, the PIL image, the callback) per scale
    fit        ce_preview_gram_f64 on one 720p image, and the whole `fit_preview_factors` call on the synthetic VAE

One process; mean and spread (sample standard deviation).  Writes the tables as markdown.

    timeout 900 python tools/preview_bench.py [--reps 6] [--layers 40] [--steps 50] [--no-fit] [--out profiles/notes_preview.md]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd import ops  # noqa: E402
from chronoedit_amd import preview as pv  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline, denoise  # noqa: E402

H, W, FRAMES, G = 720, 1280, 5, 5.0
INNER = 50


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--no-fit", action="store_true", help="no VAE: kernel, steps and delivery only")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "notes_preview.md"))
    a = ap.parse_args()
    import bench  # build_model: the 14B architecture with seeded random weights
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    T, h, w = 2, H // 8, W // 8
    factors = torch.randn(17, 3, generator=torch.Generator().manual_seed(1)) * 0.2
    lines = ["# Live previews: what they cost", "",
             f"`tools/preview_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  "
             f"{W}x{H}, {FRAMES} frames (2 latent frames), guidance {G:g}, graph replay on, seeded random weights, random fixed factors.  One process; "
             "mean +- sample standard deviation over the repetitions.", ""]

    # ---- the kernel ------------------------------------------------------------------------------------------------------------------------
    x0 = torch.randn((1, 16, T, h, w), generator=g, device=dev)
    z = torch.randn((1, 16, T, h, w), generator=g, device=dev)
    wt = torch.rand((h, w), generator=g, device=dev)
    fd = factors.to(dev)
    lines += ["## ce_preview_rgb_u8", "", f"Device time per launch (events around {INNER} launches back to back, divided), the {h} x {w} cells of 720p, one sample.", "",
              "| scale | picture | composite | bytes moved | us per launch |", "|---|---|---|---|---|"]
    for scale in pv.SCALES:
        out = torch.empty((1, h * scale, w * scale, 3), dtype=torch.uint8, device=dev)
        for comp in (False, True):
            fn = (lambda: ops.preview_rgb_u8(x0, fd, scale, -1, wt, z, out=out)) if comp else (lambda: ops.preview_rgb_u8(x0, fd, scale, -1, out=out))
            fn()
            ts = [device_ms(fn) for _ in range(max(a.reps, 5))]
            nbytes = (2 if comp else 1) * 64 * h * w + out.numel()
            print(f"ce_preview_rgb_u8 scale {scale} composite {comp}: {ms(ts)[0] * 1e3:.1f} +- {ms(ts)[1] * 1e3:.1f} us", flush=True)
            lines.append(f"| {scale} | {w * scale} x {h * scale} | {'yes' if comp else 'no'} | {nbytes / 1e6:.2f} MB | {ms(ts)[0] * 1e3:.1f} +- {ms(ts)[1] * 1e3:.1f} |")

    # ---- delivery on the host ---------------------------------------------------------------------------------------------------------------
    lines += ["", "## One delivery on the host", "",
              "`PreviewDelivery.submit` (the launch, the copy into the pinned buffer, the event) and, after a device synchronise - so that the event has fired "
              "and nothing is waited for -, `deliver` (the event query, one copy out of the pinned buffer, the PIL image, an empty callback): host clock.", "",
              "| scale | submit us | deliver us |", "|---|---|---|"]
    for scale in pv.SCALES:
        d = pv.PreviewDelivery(pv.PreviewConfig(lambda p: None, scale=scale, factors=factors, lag=1), dev, [0] * 64)
        sub, dl = [], []
        for i in range(max(a.reps, 5) + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.submit(i, i, x0)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            d.deliver(i)
            t3 = time.perf_counter()
            sub.append((t1 - t0) * 1e6), dl.append((t3 - t2) * 1e6)
        print(f"delivery scale {scale}: submit {ms(sub[2:])[0]:.0f} us, deliver {ms(dl[2:])[0]:.0f} us", flush=True)
        lines.append(f"| {scale} | {ms(sub[2:])[0]:.0f} +- {ms(sub[2:])[1]:.0f} | {ms(dl[2:])[0]:.0f} +- {ms(dl[2:])[1]:.0f} |")

    # ---- the graph-replayed loop -----------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    model = bench.build_model(a.layers, dev)
    pos = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
    neg = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
    img_emb = torch.randn((1, 257, 1280), generator=g, device=dev).to(torch.bfloat16)
    cond = torch.randn((1, 20, T, h, w), generator=g, device=dev).to(torch.bfloat16)
    lat0 = torch.randn((1, 16, T, h, w), generator=g, device=dev)
    n, warm = a.steps, set()
    seen = []

    def run_loop(scale):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        cfg = None if scale is None else pv.PreviewConfig(lambda p: seen.append(p["step"]), every=1, scale=scale, lag=1, factors=factors)
        del seen[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        marks[0].record()
        denoise(model, FlowUniPCMultistepScheduler(flow_shift=5.0), lat0.clone(), cond, pos, neg, img_emb, n, G, use_graph=True, graph_warm=warm,
                on_step_end=lambda i, t, lat: marks[i + 1].record(), preview=cfg)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert scale is None or seen == list(range(n)), seen
        t = [marks[i].elapsed_time(marks[i + 1]) for i in range(n)]
        return statistics.median(t[2:]), wall  # (steps 0-1 hold the warm check and the capture)

    legs = {"off": None, "scale 2": 2, "scale 8": 8}
    for s in legs.values():
        run_loop(s)
    per = {k: [] for k in legs}
    walls = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, s in legs.items():
            step, wall = run_loop(s)
            per[k].append(step), walls[k].append(wall)
    m0, s0 = ms(per["off"])
    lines += ["", "## The graph-replayed loop", "",
              f"`denoise(use_graph=True)` over {n} steps, {a.layers} layers, previews off and on (every=1, lag=1, an `on_preview` that only notes the step), the legs "
              "alternating in one run.  `step` is the median device time between `on_step_end` marks over the steps of an edit except 0 and 1; `loop` is the host",
              "clock around the whole `denoise` call, deliveries and the final flush included.  With previews off the loop is the parent commit's, launch for launch.", "",
              "| previews | step ms | against off | loop ms | against off |", "|---|---|---|---|---|"]
    for k in legs:
        (m1, s1), (m2, s2) = ms(per[k]), ms(walls[k])
        print(f"loop, previews {k}: step {m1:.3f} +- {s1:.3f} ms, loop {m2:.1f} +- {s2:.1f} ms", flush=True)
        lines.append(f"| {k} | {m1:.3f} +- {s1:.3f} | {(m1 - m0) * 1e3:+.0f} us | {m2:.1f} +- {s2:.1f} | {m2 - ms(walls['off'])[0]:+.1f} ms |")
    lines += ["", f"The run-to-run spread of the off leg's step is {s0 * 1e3:.0f} us (sample standard deviation over {a.reps} edits)."]
    del lat0, cond

    # ---- the fit -----------------------------------------------------------------------------------------------------------------------------
    if not a.no_fit:
        from PIL import Image

        from chronoedit_amd.vae import AutoencoderKLWan
        vae = AutoencoderKLWan.random_init(dev, seed=4321)
        pipe = ChronoEditPipeline(vae=vae)
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([xx * 255.0 / W, yy * 255.0 / H, (xx + yy) * 255.0 / (W + H)], axis=2)
        im = Image.fromarray(np.clip(base + np.random.default_rng(0).normal(0, 20, base.shape), 0, 255).astype(np.uint8))
        zf, yf = pipe.preview_fit_tensors([im], H, W)
        out = torch.empty((20, 20), dtype=torch.float64, device=dev)
        scratch = torch.empty(ops.PREVIEW_GRAM_SCRATCH, dtype=torch.uint8, device=dev)
        fn = lambda: ops.preview_gram(zf, yf, 0, out=out, scratch=scratch)
        fn()
        tg = [device_ms(fn) for _ in range(max(a.reps, 5))]
        tf = []
        for _ in range(max(3, a.reps // 2) + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.fit_preview_factors([im], H, W)
            torch.cuda.synchronize()
            tf.append((time.perf_counter() - t0) * 1e3)
        rep = pipe.preview_fit_report
        print(f"ce_preview_gram_f64: {ms(tg)[0] * 1e3:.1f} +- {ms(tg)[1] * 1e3:.1f} us; fit_preview_factors {ms(tf[1:])[0]:.1f} +- {ms(tf[1:])[1]:.1f} ms; report {rep}", flush=True)
        lines += ["", "## The fit", "",
                  f"One {W}x{H} image on the synthetic VAE (seeded random weights).  `ce_preview_gram_f64` ({yf.dtype} pixels, {zf.numel() * 4 / 1e6:.2f} MB of latents and "
                  f"{yf.numel() * yf.element_size() / 1e6:.2f} MB of pixels in, two launches): {ms(tg)[0] * 1e3:.1f} +- {ms(tg)[1] * 1e3:.1f} us per call.  The whole "
                  f"`fit_preview_factors` call - pre-processing, encode, decode, the Gram matrix, its read, the solve -: {ms(tf[1:])[0]:.1f} +- {ms(tf[1:])[1]:.1f} ms "
                  "(the first call, which also warms the VAE, left out).", "",
                  f"The report of this fit: rms {[round(v, 4) for v in rep['rms']]}, r2 {[round(v, 4) for v in rep['r2']]}.  These are figures of a VAE with RANDOM weights: "
                  "they say nothing about how good the preview looks on the real checkpoint.  `pipe.preview_fit_report` after a fit on the loaded checkpoint is how a user finds out."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
