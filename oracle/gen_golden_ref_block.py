"""The reference's own ChronoEditTransformerBlock and ChronoEditRotaryPosEmbed (transformer_chronoedit.py, executed from the build output
oracle/_ref/transformer_ref.bin) on one tiny seeded case.  Writes tests/golden/ref_block_tiny.pt: the recorded result that
tests/test_oracle_golden.py checks oracle/dit_oracle.block_forward against on every box, also where that build output is absent.
Needs oracle/_ref (built where the reference exists).  Run from the repository root: python -m oracle.gen_golden_ref_block"""
import os

import torch

from oracle import build_ref
from oracle import dit_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ref_block_tiny.pt")


def block_case():
    """Config, block-0 parameters, inputs and (latent frames, patch rows, patch columns) of the case - seeded."""
    cfg = O.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=1, text_dim=96, image_dim=64, added_kv_proj_dim=256)
    p = {k: v for k, v in O.make_synthetic_params(cfg, seed=3).items() if k.startswith("blocks.0.")}
    g = torch.Generator().manual_seed(2)
    T, hp, wp = 2, 6, 8
    x = torch.randn(1, T * hp * wp, cfg.inner_dim, generator=g)
    enc = torch.randn(1, 257 + 40, cfg.inner_dim, generator=g)
    temb6 = torch.randn(1, 6, cfg.inner_dim, generator=g) * 0.1
    return cfg, p, x, enc, temb6, (T, hp, wp)


def reference_block(mod, cfg, p, x, enc, temb6, grid):
    """(rotary table, block output) of the reference's classes in module `mod` (build_ref.load_transformer())."""
    T, hp, wp = grid
    blk = mod.ChronoEditTransformerBlock(cfg.inner_dim, cfg.ffn_dim, cfg.num_attention_heads, cfg.qk_norm, cfg.cross_attn_norm, cfg.eps,
                                         cfg.added_kv_proj_dim).eval()
    blk.load_state_dict({k[len("blocks.0."):]: v for k, v in p.items()}, strict=True, assign=True)
    rope = mod.ChronoEditRotaryPosEmbed(cfg.attention_head_dim, tuple(cfg.patch_size), cfg.rope_max_seq_len, temporal_skip_len=cfg.rope_temporal_skip_len)
    rot = rope(torch.empty(1, 1, T, 2 * hp, 2 * wp))
    with torch.no_grad():
        out = blk(x, enc, temb6, rot)
    return rot, out


def main():
    mod = build_ref.load_transformer()
    assert mod is not None, "oracle/_ref/transformer_ref.bin not built"
    cfg, p, x, enc, temb6, grid = block_case()
    rot, out = reference_block(mod, cfg, p, x, enc, temb6, grid)
    torch.save({"rot": rot, "out": out, "what": "reference ChronoEditTransformerBlock + ChronoEditRotaryPosEmbed, fp32 CPU, "
                                                  "oracle/gen_golden_ref_block.block_case()"}, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
