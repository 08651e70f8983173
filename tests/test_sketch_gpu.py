"""Sketch edits through `ChronoEditPipeline.__call__`: an image editor's {"background", "composite"} -> the mask built on the device at the
photo's size -> the focused region edit of the composite's crop, pasted into the background.  Bit for bit what a second implementation from
public pieces gives: `set_edit_region(sketch.reference(...) as a PIL mask)` + `enable_region_focus(context)` + `__call__(image=composite)`,
and PIL's own paste into the background."""
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import focus, sketch, sparse_region

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H = 96, 64
BF = torch.bfloat16
GROW, FEATHER = 3, 4


@pytest.fixture(scope="module")
def pipe():
    from transformers import CLIPImageProcessor

    from chronoedit_amd.clip_vision import CLIPVisionModel
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    from chronoedit_amd.vae import AutoencoderKLWan
    from oracle import dit_oracle as D
    from oracle import vae_oracle as V
    dcfg = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320, added_kv_proj_dim=256)
    dp = D.make_synthetic_params(dcfg, dtype=BF)
    vp = V.make_synthetic_params(V.VAEConfig(dim=32, z_dim=16))
    m = ChronoEditTransformer3DModel(num_attention_heads=2, in_channels=36, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320,
                                     added_kv_proj_dim=256, device=DEV)
    m.load_synthetic_({k: v.cuda() for k, v in dp.items()})
    vae = AutoencoderKLWan({k: v.cuda() for k, v in vp.items()}, dim=32, z_dim=16)
    torch.manual_seed(0)
    ie = CLIPVisionModel(hidden_size=320, intermediate_size=640, num_hidden_layers=3, num_attention_heads=4, image_size=56, patch_size=14, device=DEV)
    proc = CLIPImageProcessor(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})
    return ChronoEditPipeline(image_encoder=ie, image_processor=proc, transformer=m, vae=vae,
                              scheduler=FlowUniPCMultistepScheduler(flow_shift=5.0, sigma_grid="diffusers"))


def photo(size=(203, 150), seed=9):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (size[1], size[0], 3), dtype=np.uint8))


def draw(image, strokes, faint=0, seed=1):
    """The editor's composite: `strokes` = (left, top, right, bottom) rectangles of the photo overwritten (every byte moved by 128); faint:
    every other byte moved by 1..faint as well - what a lossy editor does to pixels nobody drew on."""
    bg = np.array(image)
    cp = bg.copy()
    if faint:
        step = np.random.default_rng(seed).integers(1, faint + 1, bg.shape)
        cp = np.where(bg >= 128, bg - step, bg + step).astype(np.uint8)
    for l, t, r, b in strokes:
        cp[t:b, l:r] = bg[t:b, l:r] ^ 128
    return Image.fromarray(cp)


IMAGE = photo()
STROKES = [(150, 12, 190, 20), (160, 20, 168, 50), (176, 30, 185, 44)]  # near the top right corner: the box is shifted into the image
VALUE = {"background": IMAGE, "composite": draw(IMAGE, STROKES), "layers": ["ignored"]}
SMALL = {"background": IMAGE, "composite": draw(IMAGE, [(30, 106, 40, 112)])}  # with context 1: a few tokens of the crop


def inputs(n=1, frames=5, steps=2, seed=5, guidance_scale=5.0):
    g = torch.Generator().manual_seed(seed)
    T = (frames - 1) // 4 + 1
    return dict(prompt_embeds=torch.randn(n, 40, 128, generator=g).to(BF).cuda(), negative_prompt_embeds=torch.randn(n, 40, 128, generator=g).to(BF).cuda(),
                height=H, width=W, num_frames=frames, num_inference_steps=steps, guidance_scale=guidance_scale,
                latents=torch.randn(n, 16, T, H // 8, W // 8, generator=g).to(BF).float())


def call(pipe, image, kw, output_type="pil", **more):
    return pipe(image=image, **dict(kw, latents=kw["latents"].clone(), output_type=output_type), **more).frames


def arrays(frames):
    return [np.stack([np.asarray(f) for f in sample]) for sample in frames]


def sketched(pipe, value, kw, output_type="pil", **switch):
    """The sketch call -> (frames, sketch_report, focus_report)."""
    pipe.enable_sketch_region(**dict(dict(grow=GROW, feather=FEATHER), **switch))
    try:
        out = call(pipe, value, kw, output_type)
        return out, pipe.sketch_report, pipe.focus_report
    finally:
        pipe.disable_sketch_region()


def reference_masks(value, threshold=0, grow=GROW, feather=FEATHER):
    values = value if isinstance(value, list) else [value]
    return [Image.fromarray(sketch.reference(v["background"], v["composite"], grow, feather, threshold).numpy(), mode="L") for v in values]


def explicit(pipe, value, masks, kw, context=0.25, composite=True):
    """The second implementation: the explicit-mask focused call on the composite(s) -> (frames as arrays, focus_report)."""
    images = [v["composite"] for v in value] if isinstance(value, list) else value["composite"]
    pipe.enable_region_focus(context).set_edit_region(masks if isinstance(value, list) else masks[0], composite=composite)
    try:
        return arrays(call(pipe, images, kw)), pipe.focus_report
    finally:
        pipe.disable_region_focus().clear_edit_region()


def assert_mask_is_not_trivial(report):
    """0, 255 and intermediate greys inside the box: otherwise the equalities below say nothing about the blend."""
    l, t, r, b = report["box"]
    inside = np.array(report["mask"])[t:b, l:r]
    assert (inside == 0).any() and (inside == 255).any() and ((inside > 0) & (inside < 255)).any()


def assert_sketch_equals_explicit(pipe, value, kw, context=0.25):
    got, report, freport = sketched(pipe, value, kw, context=context)
    masks = reference_masks(value)
    for rep, m in zip(report, masks):
        assert rep["mask"].mode == "L" and np.array_equal(np.array(rep["mask"]), np.array(m))  # the device's mask is the reference's
        assert_mask_is_not_trivial(rep)
    want, wreport = explicit(pipe, value, masks, kw, context)
    got = arrays(got)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    keys = ("box", "reason", "source_size", "edit_size", "scale", "mask_fraction_of_box")
    assert [{k: r[k] for k in keys} for r in report] == freport == wreport  # the plan an explicit mask gets, from one read of ten integers
    return got, report


@pytest.mark.parametrize("guidance_scale", [5.0, 1.0])
@pytest.mark.parametrize("use_graph", [True, False])
def test_sketch_call_equals_the_explicit_mask_call(pipe, use_graph, guidance_scale):
    kw = inputs(guidance_scale=guidance_scale)
    pipe.use_graph = use_graph
    try:
        got, report = assert_sketch_equals_explicit(pipe, VALUE, kw)
    finally:
        pipe.use_graph = True
    rep = report[0]
    assert (rep["grow_px"], rep["feather_px"], rep["threshold"]) == (GROW, FEATHER, 0)
    assert rep["changed_pixels"] == 40 * 8 + 8 * 30 + 9 * 14 and rep["source_size"] == IMAGE.size and rep["reason"] == "ok"
    l, t, r, b = rep["box"]
    assert r == IMAGE.size[0] and t == 0 and (r - l, b - t) == (138, 92)  # centred on the mask the box would leave the image: shifted into it
    frames, mask = got[0], np.array(rep["mask"])
    assert frames.shape == (5, IMAGE.size[1], IMAGE.size[0], 3)  # the PHOTO's size
    bg, cp = np.array(IMAGE), np.array(VALUE["composite"])
    assert np.array_equal(bg[mask < 255], cp[mask < 255]) and not np.array_equal(bg, cp)
    for f in range(5):
        assert np.array_equal(frames[f][mask == 0], bg[mask == 0]), f
    assert not np.array_equal(frames[-1][mask == 255], cp[mask == 255])  # the strokes are gone: the model's pixels


def test_sketch_sparse_edit(pipe):
    kw = inputs()
    pipe.enable_sparse_region(refresh_every=2)
    try:
        got, report = assert_sketch_equals_explicit(pipe, SMALL, kw, context=1.0)
        rep = pipe.transformer.sparse_report  # (of the second implementation's call; the sketch call is compared bit for bit)
        assert rep["plan"] == ["refresh", "sparse"] and sparse_region.PAD <= rep["active"] < rep["tokens"] == 48, rep
        sketched(pipe, SMALL, kw, context=1.0)
        assert pipe.transformer.sparse_report == rep
    finally:
        pipe.disable_sparse_region()
    assert report[0]["reason"] == "ok"


def test_two_values_of_two_photo_sizes(pipe):
    other = photo((150, 180), seed=11)
    values = [VALUE, {"background": other, "composite": draw(other, [(12, 130, 50, 140), (20, 140, 28, 168)])}]
    kw = inputs(n=2)
    got, report = assert_sketch_equals_explicit(pipe, values, kw)
    assert report[0]["box"] != report[1]["box"] and [r["source_size"] for r in report] == [IMAGE.size, other.size]
    assert got[0].shape[1:3] == (150, 203) and got[1].shape[1:3] == (180, 150)
    pipe.enable_sketch_region(grow=GROW, feather=FEATHER)
    try:
        with pytest.raises(ValueError, match="one size"):
            call(pipe, values, kw, "np")
    finally:
        pipe.disable_sketch_region()


def test_a_lossy_composite_pastes_into_the_background(pipe):
    """threshold 5, and a composite that differs by 1..5 from the photo everywhere: the frames carry the BACKGROUND's bytes wherever the
    mask is 0, and are PIL's paste of the box's content - the explicit-mask call on the composite, whole box replaced - into the background."""
    kw = inputs()
    value = {"background": IMAGE, "composite": draw(IMAGE, STROKES, faint=5)}
    bg, cp = np.array(IMAGE), np.array(value["composite"])
    assert (bg != cp).all() and np.abs(bg.astype(int) - cp.astype(int))[100:].max() <= 5  # (far from the strokes too)
    got, report, _ = sketched(pipe, value, kw, threshold=5)
    rep = report[0]
    masks = reference_masks(value, threshold=5)
    assert np.array_equal(np.array(rep["mask"]), np.array(masks[0])) and np.array_equal(np.array(masks[0]), np.array(reference_masks(VALUE)[0]))
    assert rep["threshold"] == 5 and rep["changed_pixels"] == 40 * 8 + 8 * 30 + 9 * 14
    assert_mask_is_not_trivial(rep)
    frames, mask = arrays(got)[0], np.array(rep["mask"])
    for f in range(5):
        assert np.array_equal(frames[f][mask == 0], bg[mask == 0]), f
    content, wreport = explicit(pipe, value, masks, kw, composite=False)
    box = wreport[0]["box"]
    assert box == rep["box"]
    for f in range(5):
        want = IMAGE.copy()
        want.paste(Image.fromarray(content[0][f]).crop(box), box[:2], masks[0].crop(box))
        assert np.array_equal(frames[f], np.asarray(want)), f


def test_the_host_path_gives_the_same_frames(pipe):
    kw = inputs()
    on_device, report, _ = sketched(pipe, VALUE, kw)
    pipe.enable_device_image_io(False)
    try:
        on_host, host_report, _ = sketched(pipe, VALUE, kw)
    finally:
        pipe.enable_device_image_io(True)
    assert np.array_equal(arrays(on_host)[0], arrays(on_device)[0])
    assert np.array_equal(np.array(host_report[0]["mask"]), np.array(report[0]["mask"]))
    assert {k: v for k, v in host_report[0].items() if k != "mask"} == {k: v for k, v in report[0].items() if k != "mask"}


def test_no_strokes_is_the_plain_call_on_the_composite(pipe):
    kw = inputs()
    plain, plain_lat = arrays(call(pipe, IMAGE, kw))[0], call(pipe, IMAGE, kw, "latent")
    value = {"background": IMAGE, "composite": IMAGE.copy()}
    got, report, freport = sketched(pipe, value, kw)
    assert freport is None and report[0]["reason"] == "empty" and report[0]["changed_pixels"] == 0 and report[0]["box"] == (0, 0, 203, 150)
    assert not np.array(report[0]["mask"]).any() and report[0]["mask"].size == IMAGE.size
    frames = arrays(got)[0]
    assert frames.shape == (5, H, W, 3) and np.array_equal(frames, plain)
    assert torch.equal(sketched(pipe, value, kw, "latent")[0], plain_lat)
    # a lossy composite under a threshold that covers its error: still no strokes
    faint = {"background": IMAGE, "composite": draw(IMAGE, [], faint=5)}
    got, report, _ = sketched(pipe, faint, kw, threshold=5)
    assert report[0]["reason"] == "empty" and np.array_equal(arrays(got)[0], arrays(call(pipe, faint["composite"], kw))[0])


def test_a_plain_image_under_the_switch_is_the_plain_call(pipe):
    kw = inputs()
    plain = arrays(call(pipe, VALUE["composite"], kw))[0]
    got, report, freport = sketched(pipe, VALUE["composite"], kw)
    assert report is None and freport is None and np.array_equal(arrays(got)[0], plain)


def test_the_switch_off_refuses_an_editor_value(pipe):
    kw = inputs()
    with pytest.raises(ValueError, match="enable_sketch_region"):
        call(pipe, VALUE, kw)
    sketched(pipe, VALUE, kw)
    assert pipe.sketch_report is not None
    with pytest.raises(ValueError, match="enable_sketch_region"):  # disable_sketch_region() restores the refusal
        call(pipe, VALUE, kw)
    call(pipe, IMAGE, kw)
    assert pipe.sketch_report is None


def test_an_explicit_mask_wins(pipe):
    kw = inputs()
    m = np.zeros((150, 203), np.uint8)
    m[90:130, 20:70] = 255
    mask = Image.fromarray(m)
    want, wreport = explicit(pipe, VALUE, [mask], kw)
    pipe.enable_region_focus().set_edit_region(mask)
    try:
        got, report, freport = sketched(pipe, VALUE, kw)
    finally:
        pipe.disable_region_focus().clear_edit_region()
    assert report is None and freport == wreport and np.array_equal(arrays(got)[0], want[0])


def test_sketch_mask_is_the_reports_mask(pipe):
    kw = inputs()
    _, report, _ = sketched(pipe, VALUE, kw, grow=0.02, feather=0.01)
    assert (report[0]["grow_px"], report[0]["feather_px"]) == (5, 3)  # ceil(0.02 * 203), ceil(0.01 * 203)
    pipe.enable_sketch_region(grow=0.02, feather=0.01)
    try:
        shown = pipe.sketch_mask(IMAGE, VALUE["composite"])
    finally:
        pipe.disable_sketch_region()
    assert shown.mode == "L" and shown.size == IMAGE.size and np.array_equal(np.array(shown), np.array(report[0]["mask"]))
    assert np.array_equal(np.array(shown), sketch.reference(IMAGE, VALUE["composite"], 5, 3).numpy())
    assert focus.mask_bbox(torch.from_numpy(np.array(shown))) is not None


class HostReads:
    """Counts what comes back from the device: every `.cpu()`, `.tolist()`, `.item()`, `.numpy()` and `.to(<cpu>)` of a CUDA tensor, as the
    number of elements it moves, in the order of the calls."""

    def __init__(self, monkeypatch):
        self.log, self.depth = [], 0
        for name in ("cpu", "tolist", "item", "numpy", "to"):
            monkeypatch.setattr(torch.Tensor, name, self.wrap(name, getattr(torch.Tensor, name)))

    def wrap(self, name, inner):
        def counted(t, *a, **k):
            to_host = name != "to" or any(str(v) == "cpu" or (isinstance(v, torch.device) and v.type == "cpu") for v in list(a) + list(k.values()))
            record = t.is_cuda and to_host and self.depth == 0
            if record:
                self.log.append(t.numel())
            self.depth += 1
            try:
                return inner(t, *a, **k)
            finally:
                self.depth -= 1
        return counted


def test_one_read_of_ten_integers_per_image_before_the_edit(pipe, monkeypatch):
    """In front of the first step the sketch call reads ten integers per image from the device and nothing else that the explicit-mask call
    does not read too; the report's copy of the photo-size mask is made behind the edit."""
    other = photo((150, 180), seed=11)
    values = [VALUE, {"background": other, "composite": draw(other, [(12, 130, 50, 140), (20, 140, 28, 168)])}]
    kw = inputs(n=2)
    masks = reference_masks(values)
    reads = HostReads(monkeypatch)
    before = {}

    def first_step(name):
        def cb(p, i, t, kwargs):
            before.setdefault(name, list(reads.log))
            return {}
        return cb

    pipe.enable_sketch_region(grow=GROW, feather=FEATHER)
    try:
        del reads.log[:]
        entries = sketch.masks(pipe._sketch_region, [v["background"] for v in values], [v["composite"] for v in values], torch.device(DEV))
        assert reads.log == [10, 10] and all(e["mask_u8"] is None and e["mask_dev"].is_cuda for e in entries)
        del reads.log[:]
        call(pipe, values, kw, callback_on_step_end=first_step("sketch"))
        sketch_all = list(reads.log)
        report = pipe.sketch_report
    finally:
        pipe.disable_sketch_region()
    pipe.enable_region_focus().set_edit_region(masks)
    try:
        del reads.log[:]
        call(pipe, [v["composite"] for v in values], kw, callback_on_step_end=first_step("explicit"))
    finally:
        pipe.disable_region_focus().clear_edit_region()
    extra = list(before["sketch"])
    for n in before["explicit"]:
        extra.remove(n)  # (whatever the focused call itself reads in front of the first step, the sketch call reads too)
    assert extra == [10, 10], (before["sketch"], before["explicit"])
    sizes = [203 * 150, 150 * 180]
    assert all(n not in before["sketch"] for n in sizes) and all(sketch_all.count(n) == 1 for n in sizes)  # the masks come back once, behind the edit
    for rep, m in zip(report, masks):
        assert np.array_equal(np.array(rep["mask"]), np.array(m))
