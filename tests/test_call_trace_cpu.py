"""What `ChronoEditPipeline.__call__` and `edit_tensors` do around the denoising loop, traced on the CPU with stubs: which images the VAE and
CLIP are shown, what `denoise` is handed per sample, what is composited and pasted, which guardrails and callbacks run and in which order,
and that the user's switches are what the user set after every call - a refused one and one whose loop raises included.  No GPU and no
built library: the host image paths run, `denoise` and `region.composite` are recorders.  The expected traces are written out below."""
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import auto_region, region
from chronoedit_amd.pipeline import ChronoEditPipeline, WanPipelineOutput

W, H, FRAMES, STEPS = 96, 64, 5, 3  # the edit: 96x64, 5 frames (2 latent frames), 3 steps
SW, SH = 203, 150  # the photo: no multiple of the edit, in either direction


def photo(w=SW, h=SH, k=0):
    y, x = np.mgrid[0:h, 0:w]
    return Image.fromarray(np.stack([(x * 3 + y + k) % 256, (x + y * 2 + 2 * k) % 256, (x * y + k) % 256], axis=-1).astype(np.uint8))


def drawn(im, box):  # the photo with a red rectangle on it: an editor's composite
    a = np.array(im)
    l, t, r, b = box
    a[t:b, l:r] = (255, 0, 0)
    return Image.fromarray(a)


def rect_mask(h, w, box):
    m = np.zeros((h, w), np.uint8)
    l, t, r, b = box
    m[t:b, l:r] = 255
    return m


PHOTO, PHOTO2 = photo(), photo(150, 203, 40)
SRC_MASK, SRC_MASK2 = rect_mask(SH, SW, (110, 20, 170, 60)), rect_mask(203, 150, (30, 90, 80, 150))  # at the photos' sizes: region focus
EDIT_MASK, EDIT_MASK2 = rect_mask(H, W, (16, 8, 56, 40)), rect_mask(H, W, (40, 24, 88, 56))  # at the edit's size: plain region edits
EDITOR = {"background": PHOTO, "composite": drawn(PHOTO, (120, 30, 160, 50)), "layers": []}
EDITOR2 = {"background": PHOTO2, "composite": drawn(PHOTO2, (40, 100, 80, 130))}
EDITOR_EMPTY = {"background": PHOTO, "composite": PHOTO.copy()}
DETECTED = torch.from_numpy(rect_mask(H, W, (48, 16, 80, 40)))  # what the stub detector finds, at the edit's size


def crc(a) -> str:
    return f"{zlib.crc32(np.ascontiguousarray(a).tobytes()):08x}"


def show(v):
    """A report entry or a returned value as a short literal."""
    if isinstance(v, Image.Image):
        return f"{v.mode}{v.size[0]}x{v.size[1]}:{crc(np.asarray(v))}"
    if isinstance(v, torch.Tensor):
        return f"T{list(v.shape)}"
    if isinstance(v, float):
        return round(v, 3)
    if isinstance(v, dict):
        return {k: show(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(show(x) for x in v)
    return v


def frames(out) -> str:
    f = out.frames if isinstance(out, WanPipelineOutput) else out
    if isinstance(f, list):
        return "pil " + " | ".join(f"{len(s)}x{s[0].size[0]}x{s[0].size[1]}:{crc(np.stack([np.asarray(i) for i in s]))}" for s in f)
    if isinstance(f, np.ndarray):
        return f"np {list(f.shape)}:{crc(f)}"
    if f.dim() == 5 and f.shape[1] == 16:  # "latent": the loop's output as it is (drawn noise + 1: no bytes to pin)
        return f"latents {list(f.shape)} {f.dtype}"
    return f"pt {list(f.shape)} {f.dtype}:{crc(f.float().numpy())}"


class Rig:
    """A pipeline of stubs on the CPU and the trace they write."""

    def __init__(self, monkeypatch):
        self.trace, self.detect, self.boom = [], None, False
        rig = self

        class VAE:
            temperal_downsample = [False, True, True]
            config = SimpleNamespace(z_dim=16, latents_mean=[0.0] * 16, latents_std=[1.0] * 16)
            use_graph = None

            def encode(self, video):  # every latent of a sample carries the mean of its first frame: which image it was
                rig.trace.append(f"encode {list(video.shape)}")
                B, _, F, h, w = video.shape
                lat = video[:, :, 0].float().mean((1, 2, 3)).view(B, 1, 1, 1, 1).expand(B, 16, (F - 1) // 4 + 1, h // 8, w // 8)
                return SimpleNamespace(latent_dist=SimpleNamespace(mode=lambda: lat.to(torch.bfloat16)))

            def decode(self, latents, return_dict=False):  # a fixed picture of bytes
                rig.trace.append(f"decode {list(latents.shape)}")
                B, _, T, h, w = latents.shape
                b, c, f, y, x = torch.meshgrid(*(torch.arange(n) for n in (B, 3, (T - 1) * 4 + 1, h * 8, w * 8)), indexing="ij")
                return (((x * 3 + y * 5 + c * 50 + f * 20 + b * 70) % 256).float() / 127.5 - 1.0,)

        class Transformer:
            dtype, device = torch.bfloat16, torch.device("cpu")
            _auto_region = auto_region_report = auto_region_measurement = guidance_measurement = None

            def enable_auto_region(self, *a):
                self._auto_region = auto_region.AutoRegionConfig(*a)

            def disable_auto_region(self):
                self._auto_region = None

            def calibrate_teacache(self, runners, degree=4):
                return [r() for r in runners]

        def processor(images, return_tensors="pt"):
            imgs = images if isinstance(images, list) else [images]
            rig.trace.append("clip " + " ".join(f"{i.size[0]}x{i.size[1]}" for i in imgs))
            return {"pixel_values": torch.zeros(len(imgs), 3, 4, 4)}

        def encoder(pixel_values, output_hidden_states=True):
            return SimpleNamespace(hidden_states=[None, torch.zeros(pixel_values.shape[0], 2, 8), None])

        def t5(prompt, num_videos_per_prompt=1, max_sequence_length=512, device=None, dtype=None):
            rig.trace.append(f"t5 {prompt}")
            return torch.zeros(len(prompt) * num_videos_per_prompt, 4, 8)

        def denoise(transformer, scheduler, latents, condition, prompt_embeds, negative_prompt_embeds, image_embeds, num_inference_steps,
                    guidance_scale, enable_temporal_reasoning=False, num_temporal_reasoning_steps=0, use_graph=False, on_step_end=None,
                    interrupted=None, graph_warm=None, region=None, auto_region=None, start_step=0, start_eps=None, preview=None, **measure):
            tag = []
            if preview is not None:
                preview.on_preview({"step": -1})
                tag = [f"preview={rig.previews.pop()}"]
            rig.trace.append(" ".join(
                [f"denoise {list(latents.shape)} image={float(condition[0, 4, 0, 0, 0]):.2f}",
                 "region=" + ("-" if region is None else f"{float(region.w.sum()):.2f}/{float(region.z_src.float().mean()):.2f}"),
                 "auto=" + ("-" if auto_region is None else "measure" if auto_region.measure else "detect"), f"start={start_step}",
                 f"eps={start_eps is not None}", f"cb={on_step_end is not None}", f"graph={use_graph}/{rig.pipe.vae.use_graph}"] + tag + [f"{k}={v}" for k, v in sorted(measure.items())]))
            if rig.boom:
                raise RuntimeError("boom")
            if auto_region is not None and auto_region.measure:
                transformer.auto_region_measurement = {"steps": []}
            if "guidance_measure" in measure:
                transformer.guidance_measurement = {"rel_l2": []}
            scheduler.sigmas = torch.linspace(1.0, 0.0, num_inference_steps + 1)
            for i in range(start_step, num_inference_steps):
                scheduler.model_outputs = [None, latents.float() * 0.5]
                d, a = rig.detect, auto_region
                if d is not None and a is not None and not a.measure and i == d["k"]:  # the detector's part
                    a.report = {"step": i, "accepted": d["accept"], "reason": "ok" if d["accept"] else "area"}
                    if d["accept"] and a.on_accept is not None and a.on_accept(d["mask"]):
                        a.mask_u8, a.exited = d["mask"], True
                    elif d["accept"]:
                        a.mask_u8 = d["mask"]
                if on_step_end is not None:
                    on_step_end(i, 1000 - i, latents)
                if auto_region is not None and auto_region.exited:
                    break
            return latents.float() + 1

        def composite(video, src, mask_u8):
            rig.trace.append(f"composite {list(video.shape)} image={float(src.float().mean()):.2f} mask={int(mask_u8.sum())}")
            return video.float()

        for name, mod in list(sys.modules.items()):
            if name.startswith("chronoedit_amd") and mod is not None and hasattr(mod, "denoise"):
                monkeypatch.setattr(mod, "denoise", denoise)
        monkeypatch.setattr(region, "composite", composite)
        self.previews = []
        self.pipe = ChronoEditPipeline(image_encoder=encoder, image_processor=processor, transformer=Transformer(), vae=VAE(),
                                       scheduler=SimpleNamespace(trajectory_dtype=torch.float32, model_outputs=[None, None], sigmas=None))
        self.pipe._get_t5_prompt_embeds = t5

    def switches(self):
        p = self.pipe
        return (p._edit_region, p._region_focus, p._auto_focus, p._sketch_region, p._detail_lift, p._preview, p._auto_region_measure,
                p._guidance_measure, p.transformer._auto_region, p.device_image_io, p.use_graph, getattr(p, "_focus_pass", None))

    def embeds(self, n=1):
        return dict(prompt_embeds=torch.zeros(n, 4, 8), negative_prompt_embeds=torch.zeros(n, 4, 8))

    def call(self, image, reports=(), **kw):
        """One `__call__`; its trace, then the frames (or the refusal) and the named reports.  The switches must be the user's afterwards."""
        self.trace.clear()
        if "prompt" not in kw and "prompt_embeds" not in kw:
            kw.update(self.embeds(len(image) if isinstance(image, list) else 1))
        kw = dict(dict(height=H, width=W, num_frames=FRAMES, num_inference_steps=STEPS, output_type="pil"), **kw)
        before = self.switches()
        try:
            out = self.pipe(image=image, **kw)
            assert self.pipe._interrupt is False and self.pipe._current_timestep is None
            self.trace.append("-> " + frames(out))
        except Exception as e:  # (the guardrails raise a bare Exception, as the reference's do)
            assert not isinstance(e, AssertionError)
            self.trace.append(f"-> {type(e).__name__}: {str(e)[:80]}")
        after = self.switches()
        assert len(before) == len(after) and all(a is b or a == b for a, b in zip(before, after)) and after[-1] is None
        for r in reports:
            self.trace.append(f"{r} = {show(getattr(self.pipe, r))!r}")
        return list(self.trace)

    def check(self, key, image, reports=(), **kw):
        assert self.call(image, reports, **kw) == EXPECTED[key]


@pytest.fixture
def rig(monkeypatch):
    return Rig(monkeypatch)


def test_the_plain_call(rig):
    rig.check("the_plain_call/0", PHOTO, ("focus_report", "lift_report", "auto_region_report", "sketch_report"))
    rig.check("the_plain_call/1", PHOTO, output_type="np")
    rig.check("the_plain_call/2", PHOTO, output_type="pt")
    rig.check("the_plain_call/3", PHOTO, output_type="latent")
    assert rig.pipe._num_timesteps == STEPS and rig.pipe._guidance_scale == 5.0
    rig.check("the_plain_call/4", PHOTO, output_type="jpeg")
    rig.pipe.use_graph = False
    rig.check("the_plain_call/5", PHOTO)
    assert isinstance(rig.pipe(image=PHOTO, height=H, width=W, num_frames=FRAMES, num_inference_steps=STEPS, return_dict=False, **rig.embeds()), tuple)


def test_an_explicit_region(rig):
    rig.pipe.set_edit_region(EDIT_MASK)
    rig.check("an_explicit_region/1", PHOTO, ("focus_report",))
    rig.pipe.set_edit_region(EDIT_MASK, composite=False)
    rig.check("an_explicit_region/2", PHOTO)
    rig.pipe.set_edit_region([EDIT_MASK, EDIT_MASK2])
    rig.check("an_explicit_region/3", PHOTO)


def test_region_focus(rig):
    rig.pipe.set_edit_region(Image.fromarray(SRC_MASK)).enable_region_focus(0.25)
    rig.check("region_focus/1", PHOTO, ("focus_report", "lift_report"))
    rig.pipe.set_edit_region(SRC_MASK, composite=False)
    rig.check("region_focus/2", PHOTO)
    rig.pipe.set_edit_region([SRC_MASK, SRC_MASK2])
    rig.check("region_focus/3", [PHOTO, PHOTO2], ("focus_report",))
    rig.check("region_focus/4", [PHOTO, PHOTO2], output_type="np")
    rig.check("region_focus/5", np.zeros((H, W, 3), np.float32))
    rig.check("region_focus/6", PHOTO, output_type="latent")


def test_sketch_edits(rig):
    rig.check("sketch_edits/1", EDITOR)  # the switch is off: refused
    rig.pipe.enable_sketch_region(grow=4, feather=2, context=0.25)
    rig.check("sketch_edits/2", EDITOR, ("sketch_report", "focus_report"))
    rig.check("sketch_edits/3", EDITOR_EMPTY, ("sketch_report", "focus_report"))
    rig.check("sketch_edits/4", [EDITOR, EDITOR2], ("sketch_report",))
    rig.check("sketch_edits/5", [EDITOR, EDITOR2], output_type="pt")
    rig.check("sketch_edits/6", PHOTO, ("sketch_report",))  # no editor value: the call it is without the switch
    rig.pipe.set_edit_region(EDIT_MASK)  # an explicit mask wins: the value stands for its composite
    rig.check("sketch_edits/7", EDITOR, ("sketch_report", "focus_report"))
    rig.pipe.clear_edit_region().enable_sketch_region(grow=4, feather=2, composite=False)
    rig.check("sketch_edits/8", EDITOR)


def test_auto_region(rig):
    rig.pipe.enable_auto_region(1)
    rig.detect = {"k": 1, "accept": True, "mask": DETECTED}
    rig.check("auto_region/1", PHOTO, ("auto_region_report",))
    rig.detect = {"k": 1, "accept": False, "mask": DETECTED}
    rig.check("auto_region/2", PHOTO, ("auto_region_report",))
    rig.pipe.set_edit_region(EDIT_MASK)  # an explicit mask wins
    rig.check("auto_region/3", PHOTO, ("auto_region_report",))


def test_auto_focus(rig):
    rig.pipe.enable_auto_region(1).enable_auto_focus(0.25)
    rig.detect = {"k": 1, "accept": True, "mask": DETECTED}
    reports = ("focus_report", "auto_region_report", "lift_report")
    rig.check("auto_focus/1", PHOTO, reports)  # cold
    rig.pipe.enable_auto_focus(0.25, warm_start=True)
    rig.check("auto_focus/2", PHOTO, reports)  # warm
    rig.detect = {"k": 2, "accept": True, "mask": DETECTED}
    rig.check("auto_focus/3", PHOTO, ("focus_report",))  # warm, but the detection follows the last step: cold
    rig.detect = {"k": 1, "accept": False, "mask": DETECTED}
    rig.check("auto_focus/4", PHOTO, reports)  # declined
    rig.detect = {"k": 1, "accept": True, "mask": torch.full((H, W), 255, dtype=torch.uint8)}
    rig.check("auto_focus/5", PHOTO, reports)  # "whole"
    rig.detect = {"k": 1, "accept": True, "mask": DETECTED}
    rig.check("auto_focus/6", PHOTO, output_type="latent")
    rig.check("auto_focus/7", np.zeros((H, W, 3), np.float32))
    rig.check("auto_focus/8", [PHOTO, PHOTO2])
    rig.check("auto_focus/9", PHOTO, num_videos_per_prompt=2)
    rig.check("auto_focus/10", PHOTO, enable_temporal_reasoning=True)
    rig.check("auto_focus/11", PHOTO, offload_model=True)
    rig.pipe.set_edit_region(EDIT_MASK)  # an explicit mask wins
    rig.check("auto_focus/12", PHOTO, ("focus_report",))


def test_an_auto_focused_call_with_everything_watching(rig):
    """Strings for prompts, `image_embeds` left to CLIP, both guardrails, a step callback and previews: the scout's steps 0..k, then the
    focused pass's; one text-guardrail call; the prompts encoded once; CLIP on the photo, then on the crop."""
    pipe = rig.pipe
    pipe.text_guardrail_runner = lambda prompt: rig.trace.append(f"text guardrail {prompt}") or True
    pipe.video_guardrail_runner = lambda video: rig.trace.append(f"video guardrail {list(video.shape)}") or video
    pipe.enable_preview(lambda d: rig.previews.append(f"{d['sample']}/{d['pass']}"), factors=torch.zeros(17, 3))
    cb = lambda p, i, t, kw: rig.trace.append(f"callback {i} {t} {sorted(kw)}")
    watched = dict(prompt="make it snow", callback_on_step_end=cb, callback_on_step_end_tensor_inputs=["latents", "prompt_embeds"])
    rig.check("an_auto_focused_call_with_everything_watching/1", PHOTO, **watched)  # the plain call
    pipe.enable_sketch_region(grow=4, feather=2)
    rig.check("an_auto_focused_call_with_everything_watching/2", EDITOR, **watched)
    pipe.enable_auto_region(1).enable_auto_focus(0.25, warm_start=True)
    rig.detect = {"k": 1, "accept": True, "mask": DETECTED}
    rig.check("an_auto_focused_call_with_everything_watching/3", PHOTO, **watched)
    rig.check("an_auto_focused_call_with_everything_watching/4", PHOTO, image_embeds=torch.zeros(1, 2, 8), negative_prompt="blurry", **watched)  # the user's embeds: no CLIP at all
    pipe.video_guardrail_runner = lambda video: None
    rig.check("an_auto_focused_call_with_everything_watching/5", PHOTO, **watched)


def test_detail_lift(rig):
    rig.pipe.enable_detail_lift(radius=2)
    rig.check("detail_lift/1", PHOTO, ("lift_report",))
    rig.check("detail_lift/2", photo(W, H), ("lift_report",))  # already of the edit's size: "same"
    rig.check("detail_lift/3", [PHOTO, PHOTO2], ("lift_report",))
    rig.check("detail_lift/4", [PHOTO, PHOTO2], output_type="np")
    rig.check("detail_lift/5", PHOTO, ("lift_report",), output_type="np")
    rig.check("detail_lift/6", PHOTO, ("lift_report",), output_type="latent")
    rig.check("detail_lift/7", np.zeros((H, W, 3), np.float32))
    rig.pipe.set_edit_region(EDIT_MASK)  # behind the edit-size composite
    rig.check("detail_lift/8", PHOTO, ("lift_report",))
    rig.pipe.set_edit_region(SRC_MASK).enable_region_focus()
    rig.check("detail_lift/9", PHOTO, ("lift_report",))  # focus returns what focus returns


def test_two_images_two_samples_each(rig):
    """Which image and which mask each sample gets."""
    two = dict(prompt=["a", "b"], num_videos_per_prompt=2)
    rig.check("two_images_two_samples_each/1", [PHOTO, PHOTO2], **two)
    rig.pipe.set_edit_region([EDIT_MASK, EDIT_MASK2])
    rig.check("two_images_two_samples_each/2", [PHOTO, PHOTO2], **two)
    rig.pipe.clear_edit_region().enable_auto_region(1)
    rig.detect = {"k": 1, "accept": True, "mask": DETECTED}
    rig.check("two_images_two_samples_each/3", [PHOTO, PHOTO2], ("auto_region_report",), **two)
    rig.pipe.disable_auto_region().set_edit_region([SRC_MASK, SRC_MASK2]).enable_region_focus()
    rig.check("two_images_two_samples_each/4", [PHOTO, PHOTO2], **two)


def test_a_loop_that_raises_leaves_the_switches(rig):
    rig.boom = True
    rig.pipe.enable_sketch_region(grow=4, feather=2)
    rig.check("a_loop_that_raises_leaves_the_switches/1", EDITOR)
    rig.pipe.disable_sketch_region().enable_auto_region(1).enable_auto_focus()
    rig.check("a_loop_that_raises_leaves_the_switches/2", PHOTO)
    rig.boom, rig.detect = False, {"k": 1, "accept": True, "mask": DETECTED}
    raising = lambda p, i, t, kw: (_ for _ in ()).throw(RuntimeError("boom")) if i == 2 else None  # raises in the focused pass
    rig.check("a_loop_that_raises_leaves_the_switches/3", PHOTO, callback_on_step_end=raising)


def test_edit_tensors(rig):
    pipe, image = rig.pipe, torch.zeros(1, 3, H, W)
    run = lambda **kw: (rig.trace.clear(), rig.trace.append("-> " + frames(pipe.edit_tensors(image, torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), torch.zeros(1, 2, 8), FRAMES, STEPS, **kw))),
                        list(rig.trace))[-1]
    assert run() == EXPECTED["edit_tensors/1"]
    assert run(output_type="latent") == EXPECTED["edit_tensors/2"]
    assert run(region_mask=torch.from_numpy(EDIT_MASK)) == EXPECTED["edit_tensors/3"]
    assert run(region_mask=torch.from_numpy(EDIT_MASK), composite=False) == EXPECTED["edit_tensors/4"]
    pipe.set_edit_region(EDIT_MASK2)  # not looked at here
    pipe.enable_auto_region(1)
    rig.detect = {"k": 1, "accept": True, "mask": DETECTED}
    assert run() == EXPECTED["edit_tensors/5"] and pipe.auto_region_report == {"step": 1, "accepted": True, "reason": "ok"}
    assert run(composite=False) == EXPECTED["edit_tensors/6"]
    assert run(region_mask=torch.from_numpy(EDIT_MASK)) == EXPECTED["edit_tensors/7"] and pipe.auto_region_report is None
    rig.detect = {"k": 1, "accept": False, "mask": DETECTED}
    assert run() == EXPECTED["edit_tensors/8"]


def test_the_measuring_methods_pick_their_entry(rig):
    """An edit dict that carries the three embeds and nothing `edit_tensors` does not take runs through `edit_tensors` (no step callback),
    anything else through `__call__`."""
    pipe = rig.pipe
    tensors = dict(image=torch.zeros(1, 3, H, W), prompt_embeds=torch.zeros(1, 4, 8), negative_prompt_embeds=torch.zeros(1, 4, 8),
                   image_embeds=torch.zeros(1, 2, 8), num_frames=FRAMES)
    called = dict(image=PHOTO, height=H, width=W, num_frames=FRAMES, **rig.embeds())
    pipe.set_edit_region(EDIT_MASK).enable_auto_region(1)
    measures = {"calibrate_teacache": lambda e: pipe.calibrate_teacache(e, STEPS),
                "measure_auto_region": lambda e: pipe.measure_auto_region(e, STEPS, max_area=0.4),
                "measure_guidance_reuse": lambda e: pipe.measure_guidance_reuse(e, STEPS, max_age=2)}
    for name, measure in measures.items():
        rig.trace.clear()
        before = rig.switches()
        out = measure([tensors, called, dict(tensors, height=H, width=W)])  # (the third names what `edit_tensors` does not take)
        assert all(a is b or a == b for a, b in zip(before, rig.switches()))
        assert len(out) == 3 and rig.trace == EXPECTED[name]
    assert pipe.auto_region_report is None and pipe.transformer._auto_region is not None


# What the stubs saw, call by call: `test name/call number` -> the trace.
EXPECTED = {'a_loop_that_raises_leaves_the_switches/1': ['clip 96x64',
                                              'encode [1, 3, 5, 64, 96]',
                                              'encode [1, 3, 5, 64, 96]',
                                              'denoise [1, 16, 2, 8, 12] image=-0.03 region=26.00/-0.03 auto=- start=0 eps=False cb=True '
                                              'graph=True/True',
                                              '-> RuntimeError: boom'],
 'a_loop_that_raises_leaves_the_switches/2': ['clip 203x150',
                                              'encode [1, 3, 5, 64, 96]',
                                              'encode [1, 3, 5, 64, 96]',
                                              'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                                              '-> RuntimeError: boom'],
 'a_loop_that_raises_leaves_the_switches/3': ['clip 203x150',
                                              'encode [1, 3, 5, 64, 96]',
                                              'encode [1, 3, 5, 64, 96]',
                                              'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                                              'clip 143x95',
                                              'encode [1, 3, 5, 64, 96]',
                                              'encode [1, 3, 5, 64, 96]',
                                              'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=0 eps=False cb=True '
                                              'graph=True/True',
                                              '-> RuntimeError: boom'],
 'an_auto_focused_call_with_everything_watching/1': ['text guardrail make it snow',
                                                     "t5 ['make it snow']",
                                                     "t5 ['']",
                                                     'clip 203x150',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True '
                                                     'graph=True/True preview=0/None',
                                                     "callback 0 1000 ['latents', 'prompt_embeds']",
                                                     "callback 1 999 ['latents', 'prompt_embeds']",
                                                     "callback 2 998 ['latents', 'prompt_embeds']",
                                                     'decode [1, 16, 2, 8, 12]',
                                                     'video guardrail [1, 3, 5, 64, 96]',
                                                     '-> pil 5x96x64:d1f717c9'],
 'an_auto_focused_call_with_everything_watching/2': ['text guardrail make it snow',
                                                     "t5 ['make it snow']",
                                                     "t5 ['']",
                                                     'clip 96x64',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.03 region=26.00/-0.03 auto=- start=0 eps=False cb=True '
                                                     'graph=True/True preview=0/None',
                                                     "callback 0 1000 ['latents', 'prompt_embeds']",
                                                     "callback 1 999 ['latents', 'prompt_embeds']",
                                                     "callback 2 998 ['latents', 'prompt_embeds']",
                                                     'decode [1, 16, 2, 8, 12]',
                                                     'video guardrail [1, 3, 5, 64, 96]',
                                                     '-> pil 5x203x150:08face1d'],
 'an_auto_focused_call_with_everything_watching/3': ['text guardrail make it snow',
                                                     "t5 ['make it snow']",
                                                     "t5 ['']",
                                                     'clip 203x150',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True '
                                                     'graph=True/True preview=0/scout',
                                                     "callback 0 1000 ['latents', 'prompt_embeds']",
                                                     "callback 1 999 ['latents', 'prompt_embeds']",
                                                     'clip 143x95',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=2 eps=True cb=True '
                                                     'graph=True/True preview=0/focus',
                                                     "callback 2 998 ['latents', 'prompt_embeds']",
                                                     'decode [1, 16, 2, 8, 12]',
                                                     'video guardrail [1, 3, 5, 64, 96]',
                                                     '-> pil 5x203x150:932cfa2a'],
 'an_auto_focused_call_with_everything_watching/4': ['text guardrail make it snow',
                                                     "t5 ['make it snow']",
                                                     "t5 ['blurry']",
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True '
                                                     'graph=True/True preview=0/scout',
                                                     "callback 0 1000 ['latents', 'prompt_embeds']",
                                                     "callback 1 999 ['latents', 'prompt_embeds']",
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=2 eps=True cb=True '
                                                     'graph=True/True preview=0/focus',
                                                     "callback 2 998 ['latents', 'prompt_embeds']",
                                                     'decode [1, 16, 2, 8, 12]',
                                                     'video guardrail [1, 3, 5, 64, 96]',
                                                     '-> pil 5x203x150:932cfa2a'],
 'an_auto_focused_call_with_everything_watching/5': ['text guardrail make it snow',
                                                     "t5 ['make it snow']",
                                                     "t5 ['']",
                                                     'clip 203x150',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True '
                                                     'graph=True/True preview=0/scout',
                                                     "callback 0 1000 ['latents', 'prompt_embeds']",
                                                     "callback 1 999 ['latents', 'prompt_embeds']",
                                                     'clip 143x95',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'encode [1, 3, 5, 64, 96]',
                                                     'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=2 eps=True cb=True '
                                                     'graph=True/True preview=0/focus',
                                                     "callback 2 998 ['latents', 'prompt_embeds']",
                                                     'decode [1, 16, 2, 8, 12]',
                                                     '-> Exception: Guardrail blocked video2world generation.'],
 'an_explicit_region/1': ['clip 203x150',
                          'encode [1, 3, 5, 64, 96]',
                          'encode [1, 3, 5, 64, 96]',
                          'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                          'decode [1, 16, 2, 8, 12]',
                          'composite [1, 3, 5, 64, 96] image=-0.01 mask=326400',
                          '-> pil 5x96x64:d1f717c9',
                          'focus_report = None'],
 'an_explicit_region/2': ['clip 203x150',
                          'encode [1, 3, 5, 64, 96]',
                          'encode [1, 3, 5, 64, 96]',
                          'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                          'decode [1, 16, 2, 8, 12]',
                          '-> pil 5x96x64:d1f717c9'],
 'an_explicit_region/3': ['clip 203x150',
                          'encode [1, 3, 5, 64, 96]',
                          '-> ValueError: the edit region holds 2 masks, but the call has 1 image(s): pass one mask, or on'],
 'auto_focus/1': ['clip 203x150',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                  'clip 143x95',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=0 eps=False cb=True graph=True/True',
                  'decode [1, 16, 2, 8, 12]',
                  '-> pil 5x203x150:932cfa2a',
                  "focus_report = [{'box': (60, 18, 203, 113), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.49, "
                  "'mask_fraction_of_box': 0.304, 'mask': 'L203x150:236d7cf1', 'detect': {'step': 1, 'accepted': True, 'reason': 'ok'}, "
                  "'start_step': 0}]",
                  "auto_region_report = {'step': 1, 'accepted': True, 'reason': 'ok'}",
                  'lift_report = None'],
 'auto_focus/2': ['clip 203x150',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                  'clip 143x95',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=2 eps=True cb=True graph=True/True',
                  'decode [1, 16, 2, 8, 12]',
                  '-> pil 5x203x150:932cfa2a',
                  "focus_report = [{'box': (60, 18, 203, 113), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.49, "
                  "'mask_fraction_of_box': 0.304, 'mask': 'L203x150:236d7cf1', 'detect': {'step': 1, 'accepted': True, 'reason': 'ok'}, "
                  "'start_step': 2}]",
                  "auto_region_report = {'step': 1, 'accepted': True, 'reason': 'ok'}",
                  'lift_report = None'],
 'auto_focus/3': ['clip 203x150',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                  'clip 143x95',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=0 eps=False cb=True graph=True/True',
                  'decode [1, 16, 2, 8, 12]',
                  '-> pil 5x203x150:932cfa2a',
                  "focus_report = [{'box': (60, 18, 203, 113), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.49, "
                  "'mask_fraction_of_box': 0.304, 'mask': 'L203x150:236d7cf1', 'detect': {'step': 2, 'accepted': True, 'reason': 'ok'}, "
                  "'start_step': 0}]"],
 'auto_focus/4': ['clip 203x150',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                  'decode [1, 16, 2, 8, 12]',
                  '-> pil 5x96x64:d1f717c9',
                  "focus_report = [{'reason': 'declined', 'detect': {'step': 1, 'accepted': False, 'reason': 'area'}}]",
                  "auto_region_report = {'step': 1, 'accepted': False, 'reason': 'area'}",
                  'lift_report = None'],
 'auto_focus/5': ['clip 203x150',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                  'decode [1, 16, 2, 8, 12]',
                  'composite [1, 3, 5, 64, 96] image=-0.01 mask=1566720',
                  '-> pil 5x96x64:d1f717c9',
                  "focus_report = [{'box': (0, 0, 203, 150), 'reason': 'whole', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 2.115, "
                  "'mask_fraction_of_box': 1.0, 'box_reason': 'fit', 'detect': {'step': 1, 'accepted': True, 'reason': 'ok'}}]",
                  "auto_region_report = {'step': 1, 'accepted': True, 'reason': 'ok'}",
                  'lift_report = None'],
 'auto_focus/6': ['clip 203x150',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                  'clip 143x95',
                  'encode [1, 3, 5, 64, 96]',
                  'encode [1, 3, 5, 64, 96]',
                  'denoise [1, 16, 2, 8, 12] image=-0.04 region=26.92/-0.04 auto=- start=2 eps=True cb=True graph=True/True',
                  '-> latents [1, 16, 2, 8, 12] torch.float32'],
 'auto_focus/7': ["-> ValueError: `image` has to be of type `torch.Tensor` or `PIL.Image.Image` but is <class 'num"],
 'auto_focus/8': ['-> NotImplementedError: auto focus edits one photo per call: a list of images or prompts, or num_videos_'],
 'auto_focus/9': ['-> NotImplementedError: auto focus edits one photo per call: a list of images or prompts, or num_videos_'],
 'auto_focus/10': ['-> NotImplementedError: auto focus with temporal reasoning is not implemented (the scout would run the r'],
 'auto_focus/11': ['-> NotImplementedError: auto focus with offload_model is not implemented (the encoders leave the device '],
 'auto_focus/12': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=326400',
                   '-> pil 5x96x64:d1f717c9',
                   'focus_report = None'],
 'auto_region/1': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=195840',
                   '-> pil 5x96x64:d1f717c9',
                   "auto_region_report = {'step': 1, 'accepted': True, 'reason': 'ok'}"],
 'auto_region/2': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   '-> pil 5x96x64:d1f717c9',
                   "auto_region_report = {'step': 1, 'accepted': False, 'reason': 'area'}"],
 'auto_region/3': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=326400',
                   '-> pil 5x96x64:d1f717c9',
                   'auto_region_report = None'],
 'detail_lift/1': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   '-> pil 5x203x150:fa0c03b9',
                   "lift_report = [{'size': (203, 150), 'edit_size': (96, 64), 'applied': True, 'reason': 'ok', 'fallback_fraction': 0.56}]"],
 'detail_lift/2': ['clip 96x64',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.09 region=- auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   '-> pil 5x96x64:d1f717c9',
                   "lift_report = [{'size': (96, 64), 'edit_size': (96, 64), 'applied': False, 'reason': 'same', 'fallback_fraction': None}]"],
 'detail_lift/3': ['clip 203x150 150x203',
                   'encode [2, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                   'denoise [1, 16, 2, 8, 12] image=0.02 region=- auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [2, 16, 2, 8, 12]',
                   '-> pil 5x203x150:fa0c03b9 | 5x150x203:47fb9c43',
                   "lift_report = [{'size': (203, 150), 'edit_size': (96, 64), 'applied': True, 'reason': 'ok', 'fallback_fraction': 0.56}, {'size': "
                   "(150, 203), 'edit_size': (96, 64), 'applied': True, 'reason': 'ok', 'fallback_fraction': 0.566}]"],
 'detail_lift/4': ["-> ValueError: detail lift returns frames of the images' sizes [(203, 150), (150, 203)]: output"],
 'detail_lift/5': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   '-> np [1, 5, 150, 203, 3]:662250be',
                   "lift_report = [{'size': (203, 150), 'edit_size': (96, 64), 'applied': True, 'reason': 'ok', 'fallback_fraction': 0.56}]"],
 'detail_lift/6': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                   '-> latents [1, 16, 2, 8, 12] torch.float32',
                   'lift_report = None'],
 'detail_lift/7': ["-> ValueError: `image` has to be of type `torch.Tensor` or `PIL.Image.Image` but is <class 'num"],
 'detail_lift/8': ['clip 203x150',
                   'encode [1, 3, 5, 64, 96]',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=326400',
                   '-> pil 5x203x150:fa0c03b9',
                   "lift_report = [{'size': (203, 150), 'edit_size': (96, 64), 'applied': True, 'reason': 'ok', 'fallback_fraction': 0.56}]"],
 'detail_lift/9': ['clip 105x70',
                   'encode [1, 3, 5, 64, 96]',
                   'encode [1, 3, 5, 64, 96]',
                   'denoise [1, 16, 2, 8, 12] image=0.04 region=31.35/0.04 auto=- start=0 eps=False cb=True graph=True/True',
                   'decode [1, 16, 2, 8, 12]',
                   '-> pil 5x203x150:c5d0d170',
                   "lift_report = [{'size': (203, 150), 'edit_size': (96, 64), 'applied': False, 'reason': 'focus', 'fallback_fraction': None}]"],
 'edit_tensors/1': ['encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=- start=0 eps=False cb=False graph=True/None',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pt [1, 3, 5, 64, 96] torch.float32:e78ffcc4'],
 'edit_tensors/2': ['encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=- start=0 eps=False cb=False graph=True/None',
                    '-> latents [1, 16, 2, 8, 12] torch.float32'],
 'edit_tensors/3': ['encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=20.00/0.00 auto=- start=0 eps=False cb=False graph=True/None',
                    'decode [1, 16, 2, 8, 12]',
                    'composite [1, 3, 5, 64, 96] image=0.00 mask=326400',
                    '-> pt [1, 3, 5, 64, 96] torch.float32:e78ffcc4'],
 'edit_tensors/4': ['encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=20.00/0.00 auto=- start=0 eps=False cb=False graph=True/None',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pt [1, 3, 5, 64, 96] torch.float32:e78ffcc4'],
 'edit_tensors/5': ['encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=detect start=0 eps=False cb=False graph=True/None',
                    'decode [1, 16, 2, 8, 12]',
                    'composite [1, 3, 5, 64, 96] image=0.00 mask=195840',
                    '-> pt [1, 3, 5, 64, 96] torch.float32:e78ffcc4'],
 'edit_tensors/6': ['encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=detect start=0 eps=False cb=False graph=True/None',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pt [1, 3, 5, 64, 96] torch.float32:e78ffcc4'],
 'edit_tensors/7': ['encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=20.00/0.00 auto=- start=0 eps=False cb=False graph=True/None',
                    'decode [1, 16, 2, 8, 12]',
                    'composite [1, 3, 5, 64, 96] image=0.00 mask=326400',
                    '-> pt [1, 3, 5, 64, 96] torch.float32:e78ffcc4'],
 'edit_tensors/8': ['encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=detect start=0 eps=False cb=False graph=True/None',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pt [1, 3, 5, 64, 96] torch.float32:e78ffcc4'],
 'region_focus/1': ['clip 105x70',
                    'encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.04 region=31.35/0.04 auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pil 5x203x150:c5d0d170',
                    "focus_report = [{'box': (88, 5, 193, 75), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.094, "
                    "'mask_fraction_of_box': 0.327}]",
                    'lift_report = None'],
 'region_focus/2': ['clip 105x70',
                    'encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.04 region=31.35/0.04 auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pil 5x203x150:2099bb28'],
 'region_focus/3': ['clip 105x70 135x90',
                    'encode [2, 3, 5, 64, 96]',
                    'encode [2, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=0.04 region=31.35/0.04 auto=- start=0 eps=False cb=True graph=True/True',
                    'denoise [1, 16, 2, 8, 12] image=0.01 region=23.69/0.01 auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [2, 16, 2, 8, 12]',
                    '-> pil 5x203x150:c5d0d170 | 5x150x203:34eb57e6',
                    "focus_report = [{'box': (88, 5, 193, 75), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.094, "
                    "'mask_fraction_of_box': 0.327}, {'box': (0, 75, 135, 165), 'reason': 'ok', 'source_size': (150, 203), 'edit_size': (96, 64), "
                    "'scale': 1.406, 'mask_fraction_of_box': 0.247}]"],
 'region_focus/4': ["-> ValueError: region focus returns frames of the sources' sizes [(203, 150), (150, 203)]: outp"],
 'region_focus/5': ["-> ValueError: `image` has to be of type `torch.Tensor` or `PIL.Image.Image` but is <class 'num"],
 'region_focus/6': ['-> ValueError: the edit region holds 2 masks, but the call has 1 image(s): pass one mask, or on'],
 'sketch_edits/1': ['-> ValueError: `image` is an image editor\'s value (a dict with "background" and "composite"): s'],
 'sketch_edits/2': ['clip 96x64',
                    'encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=-0.03 region=26.00/-0.03 auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pil 5x203x150:08face1d',
                    "sketch_report = [{'box': (92, 8, 188, 72), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.0, "
                    "'mask_fraction_of_box': 0.328, 'mask': 'L203x150:816c80bb', 'grow_px': 4, 'feather_px': 2, 'threshold': 0, 'changed_pixels': "
                    '800}]',
                    "focus_report = [{'box': (92, 8, 188, 72), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.0, "
                    "'mask_fraction_of_box': 0.328}]"],
 'sketch_edits/3': ['clip 203x150',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pil 5x96x64:d1f717c9',
                    "sketch_report = [{'box': (0, 0, 203, 150), 'reason': 'empty', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 2.115, "
                    "'mask_fraction_of_box': 0.0, 'mask': 'L203x150:8e41ed70', 'grow_px': 4, 'feather_px': 2, 'threshold': 0, 'changed_pixels': 0}]",
                    'focus_report = None'],
 'sketch_edits/4': ['clip 96x64 111x74',
                    'encode [2, 3, 5, 64, 96]',
                    'encode [2, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=-0.03 region=26.00/-0.03 auto=- start=0 eps=False cb=True graph=True/True',
                    'denoise [1, 16, 2, 8, 12] image=-0.02 region=25.53/-0.02 auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [2, 16, 2, 8, 12]',
                    '-> pil 5x203x150:08face1d | 5x150x203:3282f01e',
                    "sketch_report = [{'box': (92, 8, 188, 72), 'reason': 'ok', 'source_size': (203, 150), 'edit_size': (96, 64), 'scale': 1.0, "
                    "'mask_fraction_of_box': 0.328, 'mask': 'L203x150:816c80bb', 'grow_px': 4, 'feather_px': 2, 'threshold': 0, 'changed_pixels': "
                    "800}, {'box': (5, 78, 116, 152), 'reason': 'ok', 'source_size': (150, 203), 'edit_size': (96, 64), 'scale': 1.156, "
                    "'mask_fraction_of_box': 0.314, 'mask': 'L150x203:3637402d', 'grow_px': 4, 'feather_px': 2, 'threshold': 0, 'changed_pixels': "
                    '1200}]'],
 'sketch_edits/5': ["-> ValueError: a sketch edit returns frames of the photos' sizes [(203, 150), (150, 203)]: outp"],
 'sketch_edits/6': ['clip 203x150',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pil 5x96x64:d1f717c9',
                    'sketch_report = None'],
 'sketch_edits/7': ['clip 203x150',
                    'encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=-0.03 region=20.00/-0.03 auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [1, 16, 2, 8, 12]',
                    'composite [1, 3, 5, 64, 96] image=-0.03 mask=326400',
                    '-> pil 5x96x64:d1f717c9',
                    'sketch_report = None',
                    'focus_report = None'],
 'sketch_edits/8': ['clip 96x64',
                    'encode [1, 3, 5, 64, 96]',
                    'encode [1, 3, 5, 64, 96]',
                    'denoise [1, 16, 2, 8, 12] image=-0.03 region=26.00/-0.03 auto=- start=0 eps=False cb=True graph=True/True',
                    'decode [1, 16, 2, 8, 12]',
                    '-> pil 5x203x150:685b8957'],
 'calibrate_teacache': ['encode [1, 3, 5, 64, 96]',
                        'encode [1, 3, 5, 64, 96]',
                        'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=detect start=0 eps=False cb=False graph=True/None',
                        'clip 203x150',
                        'encode [1, 3, 5, 64, 96]',
                        'encode [1, 3, 5, 64, 96]',
                        'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                        'encode [1, 3, 5, 64, 96]',
                        'encode [1, 3, 5, 64, 96]',
                        'denoise [1, 16, 2, 8, 12] image=-1.00 region=20.00/-1.00 auto=- start=0 eps=False cb=True graph=True/True'],
 'measure_auto_region': ['encode [1, 3, 5, 64, 96]',
                         'encode [1, 3, 5, 64, 96]',
                         'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=measure start=0 eps=False cb=False graph=True/True',
                         'clip 203x150',
                         'encode [1, 3, 5, 64, 96]',
                         'encode [1, 3, 5, 64, 96]',
                         'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=measure start=0 eps=False cb=True graph=True/True',
                         'encode [1, 3, 5, 64, 96]',
                         'encode [1, 3, 5, 64, 96]',
                         'denoise [1, 16, 2, 8, 12] image=-1.00 region=- auto=measure start=0 eps=False cb=True graph=True/True'],
 'measure_guidance_reuse': ['encode [1, 3, 5, 64, 96]',
                            'encode [1, 3, 5, 64, 96]',
                            'denoise [1, 16, 2, 8, 12] image=0.00 region=- auto=detect start=0 eps=False cb=False graph=True/True guidance_measure=2 '
                            'keep_deltas=False',
                            'clip 203x150',
                            'encode [1, 3, 5, 64, 96]',
                            'encode [1, 3, 5, 64, 96]',
                            'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True '
                            'guidance_measure=2 keep_deltas=False',
                            'encode [1, 3, 5, 64, 96]',
                            'encode [1, 3, 5, 64, 96]',
                            'denoise [1, 16, 2, 8, 12] image=-1.00 region=20.00/-1.00 auto=- start=0 eps=False cb=True graph=True/True '
                            'guidance_measure=2 keep_deltas=False'],
 'the_plain_call/0': ['clip 203x150',
                      'encode [1, 3, 5, 64, 96]',
                      'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                      'decode [1, 16, 2, 8, 12]',
                      '-> pil 5x96x64:d1f717c9',
                      'focus_report = None',
                      'lift_report = None',
                      'auto_region_report = None',
                      'sketch_report = None'],
 'the_plain_call/1': ['clip 203x150',
                      'encode [1, 3, 5, 64, 96]',
                      'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                      'decode [1, 16, 2, 8, 12]',
                      '-> np [1, 5, 64, 96, 3]:402bed7b'],
 'the_plain_call/2': ['clip 203x150',
                      'encode [1, 3, 5, 64, 96]',
                      'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                      'decode [1, 16, 2, 8, 12]',
                      '-> pt [1, 5, 3, 64, 96] torch.float32:cbc927ef'],
 'the_plain_call/3': ['clip 203x150',
                      'encode [1, 3, 5, 64, 96]',
                      'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                      '-> latents [1, 16, 2, 8, 12] torch.float32'],
 'the_plain_call/4': ['clip 203x150',
                      'encode [1, 3, 5, 64, 96]',
                      'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                      'decode [1, 16, 2, 8, 12]',
                      "-> ValueError: jpeg does not exist. Please choose one of ['np', 'pt', 'pil']"],
 'the_plain_call/5': ['clip 203x150',
                      'encode [1, 3, 5, 64, 96]',
                      'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=False/False',
                      'decode [1, 16, 2, 8, 12]',
                      '-> pil 5x96x64:d1f717c9'],
 'two_images_two_samples_each/1': ["t5 ['a', 'b']",
                                   "t5 ['', '']",
                                   'clip 203x150 150x203',
                                   'encode [2, 3, 5, 64, 96]',
                                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.02 region=- auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.02 region=- auto=- start=0 eps=False cb=True graph=True/True',
                                   'decode [4, 16, 2, 8, 12]',
                                   '-> pil 5x96x64:d1f717c9 | 5x96x64:cc2d51d4 | 5x96x64:f167ad05 | 5x96x64:2cb1da71'],
 'two_images_two_samples_each/2': ["t5 ['a', 'b']",
                                   "t5 ['', '']",
                                   'clip 203x150 150x203',
                                   'encode [2, 3, 5, 64, 96]',
                                   'encode [2, 3, 5, 64, 96]',
                                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.02 region=20.00/-0.01 auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=24.00/0.02 auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.02 region=24.00/0.02 auto=- start=0 eps=False cb=True graph=True/True',
                                   'decode [4, 16, 2, 8, 12]',
                                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=326400',
                                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=326400',
                                   'composite [1, 3, 5, 64, 96] image=0.02 mask=391680',
                                   'composite [1, 3, 5, 64, 96] image=0.02 mask=391680',
                                   '-> pil 5x96x64:d1f717c9 | 5x96x64:cc2d51d4 | 5x96x64:f167ad05 | 5x96x64:2cb1da71'],
 'two_images_two_samples_each/3': ["t5 ['a', 'b']",
                                   "t5 ['', '']",
                                   'clip 203x150 150x203',
                                   'encode [2, 3, 5, 64, 96]',
                                   'encode [2, 3, 5, 64, 96]',
                                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.02 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=-0.01 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.02 region=- auto=detect start=0 eps=False cb=True graph=True/True',
                                   'decode [4, 16, 2, 8, 12]',
                                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=195840',
                                   'composite [1, 3, 5, 64, 96] image=-0.01 mask=195840',
                                   'composite [1, 3, 5, 64, 96] image=0.02 mask=195840',
                                   'composite [1, 3, 5, 64, 96] image=0.02 mask=195840',
                                   '-> pil 5x96x64:d1f717c9 | 5x96x64:cc2d51d4 | 5x96x64:f167ad05 | 5x96x64:2cb1da71',
                                   "auto_region_report = [{'step': 1, 'accepted': True, 'reason': 'ok'}, {'step': 1, 'accepted': True, 'reason': "
                                   "'ok'}, {'step': 1, 'accepted': True, 'reason': 'ok'}, {'step': 1, 'accepted': True, 'reason': 'ok'}]"],
 'two_images_two_samples_each/4': ["t5 ['a', 'b']",
                                   "t5 ['', '']",
                                   'clip 105x70 135x90',
                                   'encode [2, 3, 5, 64, 96]',
                                   'encode [2, 3, 5, 64, 96]',
                                   'denoise [1, 16, 2, 8, 12] image=0.04 region=31.35/0.04 auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.01 region=31.35/0.04 auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.04 region=23.69/0.01 auto=- start=0 eps=False cb=True graph=True/True',
                                   'denoise [1, 16, 2, 8, 12] image=0.01 region=23.69/0.01 auto=- start=0 eps=False cb=True graph=True/True',
                                   'decode [4, 16, 2, 8, 12]',
                                   '-> pil 5x203x150:c5d0d170 | 5x203x150:583dfa9d | 5x150x203:9a3c6476 | 5x150x203:9f69183f']}
