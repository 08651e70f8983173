"""What dropping speckle costs (chronoedit_amd/components.py, csrc/ce_components.hip; `enable_sketch_region(min_stroke=)`,
`enable_auto_region(min_area=)`): the bench photo of tools/sketch_bench.py - 4032x3024, strokes over about 1/16 of it -, the edit at
1280x720, hipGraph replay on, the 14B architecture with seeded random weights.

    passes      ce_components_roots_i32 / _sums_i32 / _keep_u8 on the grown plane of the photo, and the whole filter, next to the unfiltered
                mask build (`sketch.mask`) and the filtered one measured in the same run; bytes moved and the rate
    worst       the same passes on a full plane, a serpentine and density-0.4 noise of the photo's size - for the record
    host        components.reference on the grown plane, and sketch.reference with and without min_stroke
    grid        the filter on a 90 x 160 change map (the automatic region's grid at 1280x720), next to ce_auto_region_ramp_f32
    __call__    an 8-step sketch edit with min_stroke off / on, and the speck example: one stray pixel pair in the far corner, with the
                filter (a focused crop) and without it ("fit")

One process; the forms alternate repetition by repetition; median and spread (min .. max).  Writes the table as markdown.

    timeout 1100 python tools/components_bench.py [--reps 5] [--layers 40] [--steps 8] [--no-edit] [--commit HASH] [--out profiles/notes_components.md]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]

import components_shapes as S  # noqa: E402
from sketch_bench import H, SH, SW, W, alternate, commit, device_ms, fmt, photo_and_composite, wall  # noqa: E402

from chronoedit_amd import auto_region as ar, components, image_io, ops, sketch  # noqa: E402

GROW, FEATHER = 32, 16


def passes(plane: torch.Tensor, weight, reps: int):
    """{pass: [ms]} for roots / sums / keep / the whole filter on one plane."""
    Hp, Wp = plane.shape
    lab = ops.components_roots_i32(plane)
    sm = ops.components_sums_i32(lab, weight)
    out, cnt = ops.components_keep_u8(plane, lab, sm, 4)
    scratch = torch.empty(components.scratch_bytes(Hp, Wp), dtype=torch.uint8, device=plane.device)
    fns = {"roots": lambda: ops.components_roots_i32(plane, lab), "sums": lambda: ops.components_sums_i32(lab, weight, sm),
           "keep": lambda: ops.components_keep_u8(plane, lab, sm, 4, out=out, counters=cnt),
           "filter": lambda: components.filter(plane, 4, weight, scratch, out)}
    return alternate(fns, reps, device_ms), cnt.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--commit", default=None, help="the commit the tree was made from, where the tree itself is no git checkout")
    ap.add_argument("--no-edit", action="store_true", help="no model is built: the passes and the host forms only")
    ap.add_argument("--only-edit", action="store_true", help="the whole calls only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "notes_components.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs the GPU: nothing here is measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    reps = max(a.reps, 10)
    im, cp = photo_and_composite()
    bg_u8, cp_u8 = image_io.upload_rgb(im, dev), image_io.upload_rgb(cp, dev)
    ch, grown, _ = sketch.stages(bg_u8, cp_u8, GROW, FEATHER, 0)
    plane = SH * SW
    lines = ["# Connected components: the tables of `tools/components_bench.py`", "",
             f"`tools/components_bench.py --reps {a.reps} --layers {a.layers} --steps {a.steps}` on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
             f"commit {a.commit or commit()} plus this change.",
             f"A {SW}x{SH} photo, strokes over {int((ch > 0).sum()) / plane:.3f} of it, (grow, feather) = ({GROW}, {FEATHER}), the edit at {W}x{H}.",
             "One process, the forms alternating repetition by repetition; median (min .. max) over the repetitions; device time per launch from events",
             "around 10 calls back to back.", ""]

    def pass_tables(lines):
        # ---- the passes on the photo -------------------------------------------------------------------------------------------------------
        # roots: plane read, labels written, (border: a sliver), compress: labels read; sums: memset, labels + weight read; keep: labels twice, plane, out
        moved = {"roots": (1 + 4 + 4) * plane, "sums": (4 + 4 + 1) * plane, "keep": (4 + 4 + 1 + 1) * plane}
        moved["filter"] = sum(moved.values())
        ts, cnt = passes(grown, ch, reps)
        build = alternate({"unfiltered": lambda: sketch.mask(bg_u8, cp_u8, GROW, FEATHER, 0), "filtered": lambda: sketch.mask(bg_u8, cp_u8, GROW, FEATHER, 0, 4)}, reps, device_ms)
        same = bool(torch.equal(sketch.mask(bg_u8, cp_u8, GROW, FEATHER, 0, 4).cpu(), sketch.reference(im, cp, GROW, FEATHER, 0, 4)))
        lines += ["## The passes on the bench photo's grown plane (weight = the changed plane)", "",
                  "`MB` is what a pass has to move when nothing is cached (int32 labels and sums: 4 bytes a pixel), `GB/s` that over the median.", "",
                  "| pass | us | MB | GB/s |", "|---|---|---|---|"]
        for k in ("roots", "sums", "keep", "filter"):
            print(f"photo {k:8s} {fmt(ts[k], 1e3)} us", flush=True)
            lines.append(f"| `{k}` | {fmt(ts[k], 1e3)} | {moved[k] / 1e6:.0f} | {moved[k] / statistics.median(ts[k]) / 1e6:.0f} |")
        lines += ["", f"Counters: {cnt} (clusters kept, dropped, changed pixels dropped, the heaviest cluster).", "",
                  "| mask build (`sketch.mask`) | us |", "|---|---|",
                  f"| min_stroke = 0 (five launches) | {fmt(build['unfiltered'], 1e3)} |", f"| min_stroke = 4 | {fmt(build['filtered'], 1e3)} |", "",
                  f"The filtered device mask equals `sketch.reference(..., min_stroke=4)`: **{same}**.", ""]
        print(f"build unfiltered {fmt(build['unfiltered'], 1e3)} us, filtered {fmt(build['filtered'], 1e3)} us, same bytes {same}", flush=True)

        # ---- worst cases ---------------------------------------------------------------------------------------------------------------------
        lines += ["## Worst cases, for the record", "", "| plane | roots, us | sums | keep | filter | same labels as the host |", "|---|---|---|---|---|---|"]
        for name, p in (("full", S.full(SH, SW)), ("serpentine", S.serpentine(SH, SW)), ("noise 0.4", S.noise(SH, SW, 0.4, 1))):
            d = torch.from_numpy(p).to(dev)
            ts, _ = passes(d, None, reps)
            ok = bool(torch.equal(components.roots(d).cpu(), components.roots(torch.from_numpy(p))))
            print(f"{name:12s} " + ", ".join(f"{k} {fmt(ts[k], 1e3)} us" for k in ts) + f"; same {ok}", flush=True)
            lines.append(f"| {name} | " + " | ".join(fmt(ts[k], 1e3) for k in ("roots", "sums", "keep", "filter")) + f" | {ok} |")
            del d

        # ---- the host forms ------------------------------------------------------------------------------------------------------------------
        g_cpu, c_cpu = grown.cpu(), ch.cpu()
        host = {"components.reference (grown, weight = changed)": lambda: components.reference(g_cpu, 4, c_cpu),
                "sketch.reference, min_stroke = 0": lambda: sketch.reference(im, cp, GROW, FEATHER, 0),
                "sketch.reference, min_stroke = 4": lambda: sketch.reference(im, cp, GROW, FEATHER, 0, 4)}
        lines += ["", "## The host forms on the same photo", "", "| form | ms |", "|---|---|"]
        for k, fn in host.items():
            t = [wall(fn) for _ in range(3)]
            print(f"host {k:55s} {fmt(t)} ms", flush=True)
            lines.append(f"| `{k}` | {fmt(t)} |")

        # ---- the automatic region's grid -----------------------------------------------------------------------------------------------------
        gen = torch.Generator().manual_seed(3)
        d = torch.rand(H // 8, W // 8, generator=gen).to(dev)
        thr = torch.tensor([0.7], device=dev)
        w = torch.empty_like(d)
        ts = alternate({"kept_map (seeds, filter, d')": lambda: ar.kept_map(d, thr, 4), "ce_auto_region_ramp_f32": lambda: ops.auto_region_ramp(d, thr, 1, 1, out=w)}, reps, device_ms)
        lines += ["", f"## The automatic region's grid ({H // 8} x {W // 8} cells, 30 % seeds)", "", "| pass | us |", "|---|---|"]
        for k in ts:
            print(f"grid {k:40s} {fmt(ts[k], 1e3)} us", flush=True)
            lines.append(f"| `{k}` | {fmt(ts[k], 1e3)} |")

    if not a.only_edit:
        pass_tables(lines)

    # ---- the whole edit --------------------------------------------------------------------------------------------------------------------
    if not a.no_edit:
        import bench  # build_model: the 14B architecture with seeded random weights
        from transformers import CLIPImageProcessor

        from chronoedit_amd.clip_vision import CLIPVisionModel
        from chronoedit_amd.pipeline import ChronoEditPipeline
        from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
        from chronoedit_amd.vae import AutoencoderKLWan
        del bg_u8, cp_u8, ch, grown
        gd = torch.Generator(device=dev).manual_seed(42)
        torch.manual_seed(0)
        model = bench.build_model(a.layers, dev)
        pipe = ChronoEditPipeline(vae=AutoencoderKLWan.random_init(dev, seed=4321), transformer=model, scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0),
                                  image_encoder=CLIPVisionModel(device=dev), image_processor=CLIPImageProcessor())
        pos = torch.randn((1, 512, 4096), generator=gd, device=dev).to(torch.bfloat16)
        neg = torch.randn((1, 512, 4096), generator=gd, device=dev).to(torch.bfloat16)
        lat0 = torch.randn((1, 16, 2, H // 8, W // 8), generator=gd, device=dev)
        speck = np.array(cp)
        speck[SH - 3, 2:4] ^= 128  # two pixels in the far corner
        from PIL import Image
        values = {"sketch": {"background": im, "composite": cp}, "speck": {"background": im, "composite": Image.fromarray(speck)}}
        reports = {}
        kw = dict(prompt_embeds=pos, negative_prompt_embeds=neg, height=H, width=W, num_frames=5, num_inference_steps=a.steps, guidance_scale=5.0, output_type="pil")

        def sketch_edit(value, min_stroke, sparse):
            pipe.enable_sketch_region(grow=GROW, feather=FEATHER, min_stroke=min_stroke)
            if sparse:
                pipe.enable_sparse_region(refresh_every=2)
            try:
                out = pipe(image=values[value], latents=lat0.clone(), **kw).frames
                reports[(value, min_stroke, sparse)] = (pipe.sketch_report[0], pipe.transformer.sparse_report if sparse else None)
            finally:
                pipe.disable_sketch_region().disable_sparse_region()
            return out

        def auto_edit(min_area):
            pipe.enable_auto_region(detect_step=1, max_area=1.0, min_area=min_area)
            try:
                out = pipe(image=im, latents=lat0.clone(), **kw).frames
                reports[("auto", min_area)] = pipe.auto_region_report
            finally:
                pipe.disable_auto_region()
            return out

        def run(forms, fn):
            for f in forms.values():  # warm-up: packs the engine, captures the graphs of every form
                fn(*f), fn(*f)
            return alternate({k: (lambda f=f: fn(*f)) for k, f in forms.items()}, max(3, a.reps // 2 + 1), wall)

        forms = {"the bench sketch, min_stroke = 0": ("sketch", 0, False), "the bench sketch, min_stroke = 4": ("sketch", 4, False)}
        ts = run(forms, sketch_edit)
        lines += ["", f"## A whole {a.steps}-step sketch `__call__` (guidance 5, PIL in, PIL out, 5 frames)", "",
                  "| call | ms | reason | box | clusters kept / dropped |", "|---|---|---|---|---|"]
        for k, f in forms.items():
            rep = reports[f][0]
            print(f"__call__ {k:45s} {fmt(ts[k])} ms {rep['reason']} {rep['box']}", flush=True)
            lines.append(f"| {k} | {fmt(ts[k])} | {rep['reason']} | {rep['box']} | {rep.get('clusters', '-')} / {rep.get('dropped_clusters', '-')} |")
        d = statistics.median(ts["the bench sketch, min_stroke = 4"]) - statistics.median(ts["the bench sketch, min_stroke = 0"])
        lines += ["", f"On minus off: {d:.1f} ms (medians)."]

        forms = {"a far 2-pixel speck, min_stroke = 0": ("speck", 0, True), "a far 2-pixel speck, min_stroke = 4": ("speck", 4, True)}
        ts = run(forms, sketch_edit)
        lines += ["", "## The speck example: the same sketch plus two changed pixels in the far corner (sparse steps, refresh_every = 2)", "",
                  "| call | ms | reason | box | scale | active tokens / tokens |", "|---|---|---|---|---|---|"]
        for k, f in forms.items():
            rep, sp = reports[f]
            act = f"{sp['active']} / {sp['tokens']}" if sp else "-"
            print(f"__call__ {k:45s} {fmt(ts[k])} ms {rep['reason']} {rep['box']} active {act}", flush=True)
            lines.append(f"| {k} | {fmt(ts[k])} | {rep['reason']} | {rep['box']} | {rep['scale']:.3f} | {act} |")

        forms = {"auto region, min_area = 0": (0,), "auto region, min_area = 4": (4,)}
        ts = run(forms, auto_edit)
        lines += ["", "## The automatic region's `__call__` on the photo (detect_step = 1, Otsu, max_area = 1; random weights: the change map is noise)", "",
                  "| call | ms | accepted | active fraction | components kept / dropped |", "|---|---|---|---|---|"]
        for k, f in forms.items():
            rep = reports[("auto",) + f]
            print(f"__call__ {k:45s} {fmt(ts[k])} ms accepted {rep['accepted']} {rep['active_fraction']:.3f}", flush=True)
            lines.append(f"| {k} | {fmt(ts[k])} | {rep['accepted']} | {rep['active_fraction']:.3f} | {rep.get('components', '-')} / {rep.get('dropped_components', '-')} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
