"""What a region-limited edit (chronoedit_amd/region.py, csrc/ce_region.hip; `ChronoEditPipeline.set_edit_region`) costs at the bench shape:
1280x720, 5 frames (2 latent frames), guidance 5, hipGraph replay on, the 14B architecture with seeded random weights.

    passes     ce_region_weights_u8, ce_region_blend_f32, ce_region_composite next to ce_video_to_u8 and ce_cfg_unipc_step: device time per
               launch (events on the stream around a group of launches) and the bandwidth that makes of the bytes each pass must move
    step       one graph-replayed denoising step with and without a region (without: the parent commit's step, launch for launch)
    encode     the extra VAE encode of the static source video, next to the whole prepare_latents
    __call__   a whole 8-step edit, PIL in, PIL out, with and without a region

One process; region on / off alternate repetition by repetition; mean and spread (sample standard deviation).  Writes the table as markdown.

    timeout 900 python tools/region_bench.py [--reps 10] [--layers 40] [--no-edit] [--out profiles/notes_region.md]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chronoedit_amd import ops, region  # noqa: E402
from chronoedit_amd.pipeline import ChronoEditPipeline, GraphedDenoiser, prepare_latents  # noqa: E402

H, W, FRAMES, G = 720, 1280, 5, 5.0


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


INNER = 20  # launches between the two events of one pass timing: a single launch of a few microseconds would measure the clock


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


def alternate(fns, reps, timer):
    """{name: [ms]}: one warm-up call each, then the callables in turn, repetition by repetition."""
    for fn in fns.values():
        timer(fn)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(timer(fn))
    return ts


def soft_mask():
    """An ellipse to edit, feathered over 64 pixels, on a kept background: 0, 255 and greys."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.sqrt(((xx - W * 0.55) / (W * 0.25)) ** 2 + ((yy - H * 0.5) / (H * 0.3)) ** 2)
    return np.clip((1.15 - d) / 0.3, 0, 1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--no-edit", action="store_true", help="the passes only: no model is built")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "notes_region.md"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev).manual_seed(42)
    mask_u8 = region.normalize_mask(soft_mask(), H, W).to(dev)
    lines = ["# Region-limited edits: what the region costs", "",
             f"`tools/region_bench.py --reps {a.reps} --layers {a.layers}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  {W}x{H}, {FRAMES} frames "
             f"(2 latent frames), guidance {G:g}, graph replay on, seeded random weights.  One process, region on / off alternating; mean +- sample",
             "standard deviation over the repetitions.", ""]

    # ---- the passes ------------------------------------------------------------------------------------------------------------------
    T, h, w = 2, H // 8, W // 8
    x, z, e = (torch.randn((1, 16, T, h, w), generator=g, device=dev) for _ in range(3))
    x_last, m0, m1 = (torch.randn((1, 16, T, h, w), generator=g, device=dev) for _ in range(3))
    vc, vu = (torch.randn((1, 16, T, h, w), generator=g, device=dev).to(torch.bfloat16) for _ in range(2))
    coef = torch.tensor([G, 0.9, 1.0, 0.5, 0.2, 0.1, 0.2, 0.8, 0.1, 0.1], device=dev)
    wts = region.latent_weights(mask_u8)
    sig = torch.full((1,), 0.37, device=dev)
    video = (torch.rand((1, 3, FRAMES, H, W), generator=g, device=dev) * 2.2 - 1.1).to(torch.bfloat16)
    video32 = video.float()
    src = (torch.rand((1, 3, H, W), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    out32, out8 = torch.empty_like(video32), torch.empty((1, FRAMES, H, W, 3), dtype=torch.uint8, device=dev)
    n, nv = x.numel(), video.numel()
    passes = {  # name -> (callable, bytes the pass must move)
        "ce_region_weights_u8": (lambda: ops.region_weights_u8(mask_u8, wts), mask_u8.numel() + 4 * wts.numel()),
        "ce_region_blend_f32": (lambda: ops.region_blend_(x, z, e, wts, sig), 16 * n + 4 * wts.numel()),
        "ce_cfg_unipc_step": (lambda: ops.cfg_unipc_step(vc, vu, x, x_last, m0, m1, coef, round_sigma_v=False), 36 * n),
        "ce_region_composite (bf16 video)": (lambda: ops.region_composite(video, src, mask_u8, out32), 6 * nv + 2 * src.numel() + mask_u8.numel()),
        "ce_region_composite (fp32 video)": (lambda: ops.region_composite(video32, src, mask_u8, out32), 8 * nv + 2 * src.numel() + mask_u8.numel()),
        "ce_video_to_u8 (bf16 video)": (lambda: ops.video_to_u8(video, out8), 3 * nv),
        "ce_video_to_u8 (fp32 video, the composite's output)": (lambda: ops.video_to_u8(out32, out8), 5 * nv),
    }
    ts = alternate({k: v[0] for k, v in passes.items()}, max(a.reps, 20), device_ms)
    lines += ["## The passes", "",
              f"Device time per launch (events on the stream around {INNER} launches back to back, divided; every sample is one such group), and the bandwidth",
              "that makes of the bytes the pass has to move.  Every working set here (1 to 138 MB) fits the 256 MB last-level cache and is touched again by the",
              "next launch, so these are cache-assisted rates, comparable between the passes and not with the HBM peak; the three small passes sit at the",
              "floor one launch takes in a back-to-back train (8 to 10 us), whatever they move.", "",
              "| pass | bytes | us | GB/s |", "|---|---|---|---|"]
    for k, (_, nbytes) in passes.items():
        mean, sd = ms(ts[k])
        print(f"{k:55s} {nbytes / 1e6:8.2f} MB  {mean * 1e3:9.1f} +- {sd * 1e3:7.1f} us  {nbytes / mean / 1e6:8.1f} GB/s", flush=True)
        lines.append(f"| `{k}` | {nbytes / 1e6:.2f} MB | {mean * 1e3:.1f} +- {sd * 1e3:.1f} | {nbytes / mean / 1e6:.0f} |")
    del video32, out32, out8, video

    if not a.no_edit:
        import bench  # build_model: the 14B architecture with seeded random weights
        from PIL import Image
        from transformers import CLIPImageProcessor

        from chronoedit_amd.clip_vision import CLIPVisionModel
        from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
        from chronoedit_amd.vae import AutoencoderKLWan
        torch.manual_seed(0)
        model = bench.build_model(a.layers, dev)
        vae = AutoencoderKLWan.random_init(dev, seed=4321)
        pos = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        neg = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
        img_emb = torch.randn((1, 257, 1280), generator=g, device=dev).to(torch.bfloat16)
        cond = torch.randn((1, 20, T, h, w), generator=g, device=dev).to(torch.bfloat16)

        # ---- the graph-replayed step -------------------------------------------------------------------------------------------------
        def stepper(with_region):
            sch = FlowUniPCMultistepScheduler(flow_shift=5.0)
            sch.set_timesteps(50, device=dev)
            lat = torch.randn((1, 16, T, h, w), generator=g, device=dev)
            st = region.RegionState.begin(region.RegionConfig(w=wts, z_src=z), lat, sch) if with_region else None
            sch._step_index = 0
            gd = GraphedDenoiser(model, sch, lat, cond, pos, neg, img_emb, G, keep_warmup_step=False, region=st)  # every step() is a replay
            count = [0]

            def step():
                gd.step(count[0] % 40)
                count[0] += 1
            return step

        steps = {"plain": stepper(False), "region": stepper(True)}
        ts = alternate(steps, a.reps, wall)
        (mp, sp), (mr, sr) = ms(ts["plain"]), ms(ts["region"])
        print(f"graphed step: plain {mp:.2f} +- {sp:.2f} ms, region {mr:.2f} +- {sr:.2f} ms", flush=True)
        verdict = (f"The region step is slower than the plain step by {mr - mp:.2f} ms ({(mr - mp) / mp * 100:.2f} %), more than twice the plain step's spread."
                   if mr - mp > 2 * sp else f"The difference ({mr - mp:+.2f} ms) lies inside twice the plain step's spread ({2 * sp:.2f} ms): not resolved.")
        lines += ["", "## The graph-replayed step", "",
                  f"One `GraphedDenoiser.step()` (a replay, device synchronised), {a.layers} layers.  Without a region the step is the parent commit's launch for",
                  "launch (the region code is not entered), so `plain` is the parent's step time measured in this run.", "",
                  "| step | ms |", "|---|---|", f"| plain | {mp:.2f} +- {sp:.2f} |", f"| region | {mr:.2f} +- {sr:.2f} |", "", verdict]
        del steps

        # ---- the extra VAE encode ----------------------------------------------------------------------------------------------------
        vae.use_graph = True
        img = src
        enc = {"prepare_latents (the condition encode)": lambda: prepare_latents(vae, img, FRAMES, latents=x),
               "static_source_latents (the extra encode)": lambda: region.static_source_latents(vae, img, FRAMES)}
        for fn in enc.values():  # the second call of a shape captures the VAE's graph, the third replays it
            fn(), fn()
        ts = alternate(enc, a.reps, wall)
        lines += ["", "## The extra VAE encode", "", "Both replay the VAE's captured encode graph (the same shape).", "", "| stage | ms |", "|---|---|"]
        for k in enc:
            mean, sd = ms(ts[k])
            print(f"{k:45s} {mean:9.2f} +- {sd:6.2f} ms", flush=True)
            lines.append(f"| {k} | {mean:.2f} +- {sd:.2f} |")

        # ---- the whole edit ----------------------------------------------------------------------------------------------------------
        proc = CLIPImageProcessor()
        pipe = ChronoEditPipeline(vae=vae, transformer=model, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0),
                                  image_encoder=CLIPVisionModel(device=dev), image_processor=proc)
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([xx * 255.0 / W, yy * 255.0 / H, (xx + yy) * 255.0 / (W + H)], axis=2)
        im = Image.fromarray(np.clip(base + np.random.default_rng(0).normal(0, 20, base.shape), 0, 255).astype(np.uint8))
        lat0 = torch.randn((1, 16, T, h, w), generator=g, device=dev)
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=FRAMES, num_inference_steps=a.steps, guidance_scale=G,
                  output_type="pil")
        mask_img = Image.fromarray(mask_u8.cpu().numpy())

        def edit(with_region):
            pipe.set_edit_region(mask_img) if with_region else pipe.clear_edit_region()
            return pipe(image=im, latents=lat0.clone(), **kw).frames

        edit(False), edit(True)  # warm-up: packs the engine, captures the graphs of both forms
        frames = edit(True)
        keep = mask_u8.cpu().numpy() == 0
        exact = all(np.array_equal(np.asarray(f)[keep], np.asarray(im)[keep]) for f in frames[0])
        print(f"source bytes kept where the mask is 0, in every frame: {exact}", flush=True)
        ts = alternate({"plain": lambda: edit(False), "region": lambda: edit(True)}, max(3, a.reps // 2), wall)
        pipe.clear_edit_region()
        (mp, sp), (mr, sr) = ms(ts["plain"]), ms(ts["region"])
        print(f"__call__ {a.steps} steps: plain {mp:.1f} +- {sp:.1f} ms, region {mr:.1f} +- {sr:.1f} ms", flush=True)
        lines += ["", f"## A whole {a.steps}-step `__call__`, PIL in, PIL out", "",
                  f"The region adds the mask's normalisation and upload, the weights pass, one VAE encode, {a.steps} blends and the paste-back.  Source bytes kept",
                  f"exactly where the mask is 0, in every returned frame: **{exact}**.", "",
                  "| edit | ms |", "|---|---|", f"| plain | {mp:.1f} +- {sp:.1f} |", f"| region | {mr:.1f} +- {sr:.1f} |", "",
                  f"Difference {mr - mp:+.1f} ms ({(mr - mp) / mp * 100:+.2f} %); twice the plain edit's spread is {2 * sp:.1f} ms."]
    lines += ["", "## What these numbers do not say", "",
              "The weights are random: nothing here judges how well the model fills a masked region.  What the feature guarantees is arithmetic -",
              "the returned frames carry the resized source's bytes exactly where the mask is 0, and where the 8x8 box mean of the mask is 1 the blend",
              "leaves the sample bit-unchanged (an all-255 mask is the plain loop's trajectory) - and is pinned by tests/test_region_gpu.py and",
              "tests/test_exact_region_gpu.py.  Quality on the real checkpoint is unmeasured."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
