"""TeaCache step skipping, host side (chronoedit_amd/teacache.py): the compute / skip rule of the reference's `TeaCache.check`
(wan_video_new_chronoedit.py:1211-1231) restated as a pure function of the per-step ratios, the host bf16 rounding the ratios go
through, and the three new entry points in the header, the signature table and the built library.  No GPU."""
import math

import numpy as np
import torch

from chronoedit_amd import hiplib
from chronoedit_amd.teacache import TeaCacheConfig, bf16_round, plan_from_ratios, ratios_from_sums, report

C, S = True, False
TEA_SYMBOLS = ("ce_tea_rel_l1_bf16", "ce_tea_store_bf16", "ce_tea_apply_bf16")


def test_plan_accumulates_until_the_threshold_and_the_ends_compute():
    ratios = [0.3] * 6  # (not looked at by a constant polynomial)
    assert plan_from_ratios(ratios, 6, 2.5, (1.0,)) == [C, S, S, C, S, C]
    assert plan_from_ratios(ratios, 6, 2.5, (1.0,), forced={2}) == [C, S, C, S, S, C]
    assert plan_from_ratios(ratios, 6, 0.5, (1.0,)) == [C] * 6  # every step reaches the threshold at once


def test_plan_of_one_and_two_step_schedules_is_all_compute():
    assert plan_from_ratios([0.0], 1, 1e9, (1.0, 0.0)) == [C]
    assert plan_from_ratios([0.0, 0.0], 2, 1e9, (1.0, 0.0)) == [C, C]


def test_plan_with_a_polynomial_that_goes_negative_skips_until_the_last_step():
    ratios = [0.0] + [0.1] * 7
    assert plan_from_ratios(ratios, 8, 0.05, (-1.0, 0.0)) == [C] + [S] * 6 + [C]


def test_plan_uses_the_ratio_of_every_step_and_the_polynomial_highest_power_first():
    # poly(r) = 2 r^2 + 1: steps 1..4 add 1.02, 1.08, 1.5, 3.0 -> the accumulator passes 2.05 at step 2 (2.10) and again at step 4 (1.5 + 3.0)
    ratios = [9.0, 0.1, 0.2, 0.5, 1.0, 0.1]
    assert plan_from_ratios(ratios, 6, 2.05, (2.0, 0.0, 1.0)) == [C, S, C, S, C, C]
    want = np.poly1d([2.0, 0.0, 1.0])
    acc = float(want(0.1)) + float(want(0.2))
    assert acc >= 2.05 > float(want(0.1))
    # a skipped step's ratio is not carried over: step 3 starts from zero after the computed step 2
    assert plan_from_ratios(ratios, 6, 1.6, (2.0, 0.0, 1.0)) == [C, S, C, S, C, C]
    assert plan_from_ratios(ratios, 6, 1.4, (2.0, 0.0, 1.0))[3] is True  # 1.5 alone reaches 1.4


def test_plan_computes_on_a_nan_or_infinite_ratio():
    for bad in (math.nan, math.inf):
        assert plan_from_ratios([0.0, 0.01, bad, 0.01, 0.0], 5, 0.5, (1.0, 0.0)) == [C, S, C, S, C]


def test_report_counts():
    r = report([C, S, S, C], [0.0, 0.1, 0.2, 0.3])
    assert r == {"plan": [True, False, False, True], "computed": 2, "skipped": 2, "ratios": [0.0, 0.1, 0.2, 0.3]}
    assert TeaCacheConfig(0.1).coefficients == (1.0, 0.0)  # the identity rescale is the default


def test_host_bf16_rounding_matches_torch():
    g = torch.Generator().manual_seed(5)
    vals = (torch.randn(300, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-130, 128, (300,), generator=g).double())).tolist()
    # exact values, rounding ties (to even, both ways), the largest finite value and what rounds up to inf, subnormals, signed zeros
    vals += [0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895313892515355e38, 3.4e38, -3.4e38, 1e39, 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134,
             1.0 / 3.0, math.inf, -math.inf]
    for v in vals:
        want = torch.tensor(v, dtype=torch.float64).float().bfloat16()
        got = bf16_round(v)
        assert got == float(want) and math.copysign(1.0, got) == math.copysign(1.0, float(want)), (v, got, float(want))
    assert math.isnan(bf16_round(math.nan))


def test_ratios_follow_the_bf16_arithmetic_of_the_reference():
    g = torch.Generator().manual_seed(6)
    n = 1536
    rows = torch.randn(5, n, generator=g).bfloat16()
    sums = torch.zeros(5, 2, dtype=torch.float32)
    want = [0.0]
    for i in range(1, 5):
        a, b = rows[i], rows[i - 1]
        sums[i, 0] = (a - b).abs().float().sum()
        sums[i, 1] = b.abs().float().sum()
        m1 = (sums[i, 0] / n).bfloat16()
        m0 = (sums[i, 1] / n).bfloat16()
        want.append(float(m1 / m0))  # a bf16 quotient
    assert ratios_from_sums(sums.numpy(), n) == want


def test_entry_points_are_declared_typed_and_exported():
    path = hiplib.build()
    assert "ce_tea.hip" in hiplib.SOURCES
    for s in TEA_SYMBOLS:
        assert s in hiplib.header_symbols(), s
        assert s in hiplib.SIGNATURES, s
        assert s in hiplib.exported_symbols(path), s
        assert s in hiplib.exported_symbols(hiplib.DIAG_LIB_PATH), s
