"""Device image pre- / post-processing (csrc/ce_image.hip, chronoedit_amd/image_io.py) against the host path it replaces - PIL's resize,
pipeline.preprocess_image, the CLIPImageProcessor, pipeline.postprocess_video - bit for bit."""
import numpy as np
import pytest
import torch
from PIL import Image

from chronoedit_amd import image_io

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (W, H) -> (W2, H2): both passes, one pass, none; enlarging and reducing; row bytes that are and are not a multiple of 4; 41-tap rows
SHAPES = [((37, 23), (16, 16)), ((64, 48), (80, 96)), ((301, 200), (128, 80)), ((129, 77), (129, 40)), ((77, 129), (40, 129)),
          ((50, 50), (224, 224)), ((640, 360), (398, 224)), ((1, 9), (5, 3)), ((1000, 40), (150, 40)), ((1280, 720), (1280, 720))]
FILTERS = {image_io.LANCZOS: Image.LANCZOS, image_io.BICUBIC: Image.BICUBIC}


def random_rgb(size, seed=0):
    w, h = size
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("filter", list(FILTERS))
@pytest.mark.parametrize("src_size,dst_size", SHAPES)
def test_resize_u8_equals_pil(src_size, dst_size, filter):
    src = random_rgb(src_size, seed=sum(src_size) + sum(dst_size))
    want = np.asarray(Image.fromarray(src).resize(dst_size, FILTERS[filter]))
    dev = torch.from_numpy(src).to(DEV)
    got = image_io.resize_u8(dev, dst_size, filter)
    if src_size == dst_size:
        assert got is dev  # no launch at all
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)


def test_preprocess_pil_equals_preprocess_image():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    H, W = 64, 96
    rgb = Image.fromarray(random_rgb((90, 70), 1))
    same = Image.fromarray(random_rgb((W, H), 2))  # already at the target size: the lookup alone
    grey = Image.fromarray(random_rgb((53, 41), 3)[..., 0])
    rgba = Image.fromarray(np.concatenate([random_rgb((120, 75), 4), random_rgb((120, 75), 5)[..., :1]], axis=2))
    for image in (rgb, same, grey, rgba, [rgb, Image.fromarray(random_rgb((200, 131), 6))]):
        want = ChronoEditPipeline.preprocess_image(image, H, W).to(device=DEV, dtype=torch.bfloat16)
        got = image_io.preprocess_pil(image, H, W, DEV)
        assert got.dtype == torch.bfloat16 and got.shape == want.shape and got.is_contiguous()
        assert torch.equal(bits(got), bits(want))
    # a width that is no multiple of 4: the element-wise stores of the lookup
    want = ChronoEditPipeline.preprocess_image(rgb, 23, 37).to(device=DEV, dtype=torch.bfloat16)
    assert torch.equal(bits(image_io.preprocess_pil(rgb, 23, 37, DEV)), bits(want))


def clip_processors():
    from transformers import CLIPImageProcessor
    return {224: CLIPImageProcessor(), 56: CLIPImageProcessor(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 56})}


@pytest.mark.parametrize("edge,size", [(224, (1280, 720)), (56, (1280, 720)), (224, (300, 500)), (56, (300, 500)), (56, (224, 224))])
def test_clip_pixel_values_equal_the_processor(edge, size):
    proc = clip_processors()[edge]
    img = Image.fromarray(random_rgb(size, seed=edge + size[0]))
    want = proc(images=img, return_tensors="pt")["pixel_values"]
    got = image_io.clip_pixel_values(proc, img, DEV)
    assert got is not None and got.dtype == torch.float32 and got.shape == want.shape == (1, 3, edge, edge)
    assert torch.equal(bits(got), bits(want))


def test_clip_pixel_values_batch_of_two_sizes():
    proc = clip_processors()[56]
    imgs = [Image.fromarray(random_rgb((90, 70), 7)), Image.fromarray(random_rgb((61, 133), 8)).convert("L")]
    want = proc(images=imgs, return_tensors="pt")["pixel_values"]
    got = image_io.clip_pixel_values(proc, imgs, DEV)
    assert torch.equal(bits(got), bits(want))


def host_frames(video):
    from chronoedit_amd.pipeline import ChronoEditPipeline
    return ChronoEditPipeline.postprocess_video(video.cpu(), "pil")


def frames_array(frames):
    return np.stack([np.stack([np.asarray(f) for f in sample]) for sample in frames])


def test_frames_to_pil_on_every_bf16_bit_pattern():
    """[1, 3, 2, 96, 128] holds 73 728 bf16 elements: all 65 536 bit patterns, then a seeded shuffle of them again.  The 254 NaN patterns
    are left out of the comparison (the host casts a NaN to uint8, which numpy leaves undefined; the kernel writes 0); the infinities stay in."""
    n = 3 * 2 * 96 * 128
    pat = torch.arange(65536, dtype=torch.int32)
    pat = torch.cat([pat, pat[torch.randperm(65536, generator=torch.Generator().manual_seed(0))[:n - 65536]]])
    video = pat.to(torch.int16).view(torch.bfloat16).reshape(1, 3, 2, 96, 128)
    nan = torch.isnan(video.float())
    assert int(nan.flatten()[:65536].sum()) == 254 and bool(torch.isinf(video.float()).any())
    want = frames_array(host_frames(video))
    frames = image_io.frames_to_pil(video.to(DEV))
    assert len(frames) == 1 and len(frames[0]) == 2 and frames[0][0].size == (128, 96) and frames[0][0].mode == "RGB"
    got = frames_array(frames)
    keep = ~nan.permute(0, 2, 3, 4, 1).numpy()  # [B, F, H, W, 3]
    assert got.shape == want.shape == keep.shape
    assert np.array_equal(got[keep], want[keep])
    assert (got[~keep] == 0).all()


@pytest.mark.parametrize("shape,dtype", [((2, 3, 1, 3, 50), torch.bfloat16), ((1, 3, 3, 5, 17), torch.bfloat16), ((1, 3, 1, 7, 33), torch.float32),
                                         ((2, 3, 2, 4, 8), torch.float32)])
def test_frames_to_pil_tail_shapes(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    video = (torch.randn(shape, generator=g) * 0.8).to(dtype)
    video.view(-1)[::7] = torch.round(video.view(-1)[::7].float() * 255) / 255  # values near the rounding ties of * 255
    want = frames_array(host_frames(video))
    got = frames_array(image_io.frames_to_pil(video.to(DEV)))
    assert got.shape == want.shape and np.array_equal(got, want)


def tiny_pipeline():
    from transformers import CLIPImageProcessor

    from chronoedit_amd.clip_vision import CLIPVisionModel
    from chronoedit_amd.pipeline import ChronoEditPipeline
    from chronoedit_amd.scheduler import FlowUniPCMultistepScheduler
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    from chronoedit_amd.vae import AutoencoderKLWan
    from oracle import dit_oracle as D
    from oracle import vae_oracle as V
    dcfg = D.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=320, added_kv_proj_dim=256)
    dp = D.make_synthetic_params(dcfg, dtype=torch.bfloat16)
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


def test_pipeline_call_is_the_same_with_the_switch_on_and_off(monkeypatch):
    pipe = tiny_pipeline()
    assert pipe.device_image_io is True
    g = torch.Generator().manual_seed(5)
    H, W = 64, 96
    image = Image.fromarray(random_rgb((90, 70), 9))
    kw = dict(image=image, prompt_embeds=torch.randn(1, 40, 128, generator=g).to(torch.bfloat16).cuda(),
              negative_prompt_embeds=torch.randn(1, 40, 128, generator=g).to(torch.bfloat16).cuda(), height=H, width=W, num_frames=5,
              num_inference_steps=2, guidance_scale=5.0, latents=torch.randn(1, 16, 2, H // 8, W // 8, generator=g))
    calls = []
    for name in ("preprocess_pil", "clip_pixel_values", "frames_to_pil"):
        fn = getattr(image_io, name)
        monkeypatch.setattr(image_io, name, lambda *a, _fn=fn, _name=name, **k: (calls.append(_name), _fn(*a, **k))[1])
    out = {}
    for flag in (True, False):
        pipe.enable_device_image_io(flag)
        del calls[:]
        frames = pipe(**dict(kw, latents=kw["latents"].clone(), output_type="pil")).frames
        lat = pipe(**dict(kw, latents=kw["latents"].clone(), output_type="latent")).frames
        assert sorted(calls) == (["clip_pixel_values"] * 2 + ["frames_to_pil"] + ["preprocess_pil"] * 2 if flag else [])
        assert len(frames) == 1 and len(frames[0]) == 5 and frames[0][0].size == (W, H)
        out[flag] = (frames_array(frames), lat)
    assert np.array_equal(out[True][0], out[False][0])
    assert out[True][1].dtype == out[False][1].dtype and torch.equal(bits(out[True][1]), bits(out[False][1]))
