"""Where a text context's padding is found (pipeline.text_real_lengths / text_compaction_plan / compact_text_context) and the new entry
point's place in the header and the signature table.  No GPU."""
import math

import torch

from chronoedit_amd import hiplib, pipeline


def _text(ns, Tt=512, C=16, pad=0.0, dtype=torch.bfloat16, seed=1):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(len(ns), Tt, C, generator=g).to(dtype)
    for b, n in enumerate(ns):
        t[b, n:] = pad
    return t


def test_lengths_with_zero_padding_and_with_any_constant_row():
    for dtype in (torch.bfloat16, torch.float32):
        assert pipeline.text_real_lengths(_text([64, 37, 0, 511], dtype=dtype)).tolist() == [64, 37, 0, 511]
    t = _text([64, 200])
    row = torch.randn(16).to(torch.bfloat16)  # non-zero identical trailing rows
    t[0, 64:], t[1, 200:] = row, row
    assert pipeline.text_real_lengths(t).tolist() == [64, 200]


def test_a_full_prompt_and_a_look_alike_row_are_not_shortened():
    t = _text([512, 300])
    assert pipeline.text_real_lengths(t).tolist() == [511, 300]  # (no padding: a trailing run of one row, which the plan keeps whole)
    assert pipeline.text_compaction_plan([511, 300], 512) is None
    # the last real row resembles the padding: one bf16 ulp off zero in one channel, and a negative zero - neither is padding
    t[1, 299] = 0
    t[1, 299, 3] = torch.finfo(torch.bfloat16).smallest_normal
    t[1, 298] = 0
    t[1, 298, 0] = -0.0
    assert pipeline.text_real_lengths(t).tolist() == [511, 300]
    t[1, 299, 3] = 0  # now it IS a padding row; the negative zero in front of it still is not
    assert pipeline.text_real_lengths(t).tolist() == [511, 299]


def test_plan_counts_weights_and_the_tile_rule():
    Lc, valid, w = pipeline.text_compaction_plan([64, 37], 512)
    assert (Lc, valid) == (72, [65, 38]) and w == [math.log2(448), math.log2(475)]
    assert pipeline.text_compaction_plan([0, 0], 512) == (8, [1, 1], [9.0, 9.0])
    assert pipeline.text_compaction_plan([447, 3], 512)[0] == 448      # 7 tiles instead of 8
    assert pipeline.text_compaction_plan([448, 3], 512) is None        # 449 keys: 8 tiles, nothing saved
    assert pipeline.text_compaction_plan([512, 3], 512) is None
    Lc, valid, w = pipeline.text_compaction_plan([10, 191], 192 + 64)  # another full length: 3 tiles instead of 4
    assert valid == [11, 192] and Lc == 192 and w[0] == math.log2(246) and w[1] == math.log2(65)


def test_compact_text_context_hangs_the_rows_on_the_tensor_and_follows_its_version():
    t = _text([64, 37])
    assert pipeline.compact_text_context(t) is t
    c = t._ce_compact
    assert c.real == [64, 37] and c.Lc == 72 and c.shape == (2, 512, 16) and c.version == t._version
    assert torch.equal(c.text, t[:, :72]) and c.text.is_contiguous()
    assert c.valid.dtype == torch.int32 and c.valid.tolist() == [65, 38] and c.w.dtype == torch.float32
    assert pipeline.compact_text_context(t)._ce_compact is c  # examined once
    t[0, 100] = 1.0  # an in-place change: examined again
    assert pipeline.compact_text_context(t)._ce_compact is not c and t._ce_compact.real == [101, 37]
    full = _text([512, 512])
    assert pipeline.compact_text_context(full)._ce_compact.text is None
    text2, image2 = pipeline.make_cfg_inputs(_text([64]), _text([37], seed=2), None)
    assert text2._ce_compact.real == [64, 37] and image2 is None


def test_weighted_entry_is_declared_everywhere():
    name = "ce_attention_2seg_vt_weighted_bf16"
    assert name in hiplib.header_symbols() and name in hiplib.SIGNATURES
    assert len(hiplib.SIGNATURES[name]) == len(hiplib.SIGNATURES["ce_attention_2seg_vt_strided_bf16"]) + 2
