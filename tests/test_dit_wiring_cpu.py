"""The constructions of tests/wiring_util.py, checked on the fp32 and the bf16-eager oracle alone (no GPU): conditions the wiring tests of
the engine (tests/test_dit_wiring_gpu.py) rest on.  For every listed wire, in every case:
  * it moves the fp32 oracle's output by at least SIZE_FLOOR (0.05) of its norm - no wire is a whisper;
  * the bf16-eager oracle reproduces that change to within EAGER_CAP (0.15) - the engine's cap, 3 x this + 0.02, stays below 0.47, and a
    dead (err = 1) or crossed (err ~ 1.4) wire cannot pass;
and per case the bf16-eager oracle's whole output is within 2e-2 of the fp32 oracle's at the loud parameters.
These are conditions on the recipe, not measurements: a wire that misses one gets a larger factor in wiring_util (FACTOR, VOXEL_GAIN, the
small-signal scales), never a lower floor.  Measured over every case and text: smallest size 0.056 and largest eager error 0.122, both at
`in:latent_voxel_last`, T = 8 (one token of 768: its size saturates near 0.06 however loud the voxel); the next wires are the key biases
(size 0.06 - 0.1 at 8 x rms).  Base eager-vs-fp32 1.1e-2 - 1.2e-2 (T = 2), 1.4e-2 (T = 8).
The cases with 128 text rows and the second prompt are what the text-compaction and the two-sample modes of the GPU tests run; their
eager figures enter those tests' caps, so they are held to the same conditions."""
import dataclasses

import pytest
import torch

import wiring_util as W

CASE_TEXTS = [(c, False) for c in W.ALL_CASES] + [(c, True) for c in W.CASES]
WIRE_PARAMS = [pytest.param(c, tb, w.name, id=f"{c}{'-textb' if tb else ''}-{w.name}") for c, tb in CASE_TEXTS for w in W.wires_of(c)]
WIRE_PARAMS += [pytest.param(c, True, w.name, id=f"{c}-textb-{w.name}") for c in W.CASES for w in W.sample1_wires()]


def test_parameter_wires_cover_the_parameter_tree():
    names = {w.name for w in W.WIRES}
    assert set(W.O.param_shapes(W.CFG)) <= names
    assert len(W.O.param_shapes(W.CFG)) == 87
    for i in range(W.CFG.num_layers):
        assert {f"blocks.{i}.scale_shift_table[{r}]" for r in range(6)} <= names
    assert {"scale_shift_table[0]", "scale_shift_table[1]"} <= names


def test_loud_params_keep_the_fp32_islands():
    p = W.loud_params(W.CFG, 21)
    for k, v in p.items():
        assert v.dtype == (torch.float32 if W.O.keep_fp32(k) else W.BF), k
    assert torch.equal(p["proj_out.weight"], W.loud_params(W.CFG, 21)["proj_out.weight"])


@pytest.mark.parametrize("case,text_b", CASE_TEXTS)
def test_base_eager_oracle_within_bound_at_loud_parameters(case, text_b):
    ref32, ref_bf = W.reference(case, "loud", None, text_b)
    e = W.rel_l2(ref_bf, ref32)
    print(f"{case} text_b={text_b}: bf16-eager vs fp32 at the loud parameters {e:.3e}")
    assert torch.isfinite(ref32).all() and e <= W.BASE_EAGER_CAP


@pytest.mark.parametrize("case,text_b,wire", WIRE_PARAMS)
def test_wire_is_loud_and_the_eager_oracle_reproduces_it(case, text_b, wire):
    size, err = W.wire_figures(case, W.WIRE_BY_NAME[wire], text_b)
    print(f"{case} {wire}: size {size:.3f}  eager err {err:.3f}")
    assert size >= W.SIZE_FLOOR
    assert err <= W.EAGER_CAP


def test_dead_and_crossed_wires_score_one_and_more():
    """delta_err itself: an ignored wire is err = 1; another wire's change in its place is more (sqrt 2 at equal size)."""
    case = "T2"
    a, b = W.WIRE_BY_NAME["blocks.0.attn1.to_k.bias"], W.WIRE_BY_NAME["blocks.0.attn2.to_k.bias"]
    base = W.reference(case)[0]
    ra, rb = W.reference(case, "loud", a.name)[0], W.reference(case, "loud", b.name)[0]
    assert W.delta_err(base, base, base, ra)[1] == pytest.approx(1.0)
    assert W.delta_err(base, rb, base, ra)[1] > 1.05
    assert W.delta_err(base, ra, base, ra)[1] == 0.0


@pytest.mark.parametrize("case", list(W.CASES))
def test_small_signal_wires_hear_a_tenfold_eps(case):
    """The point of the small_* bases: a forward with cfg.eps = 1e-5 instead of 1e-6 (fp32 arithmetic otherwise) misses the cap of every
    wire that targets a cfg.eps norm, while at the loud base the same mistake is far inside it."""
    wrong = lambda st: (st[0], st[1], dataclasses.replace(st[2], eps=1e-5))
    for w in W.wires_of(case):
        if not w.name.startswith("eps:") or "image_embedder" in w.name:
            continue
        got_b = W.oracle(*wrong(W.state(case, w.base)), torch.float32)
        got_p = W.oracle(*wrong(W.state(case, w.base, w.name)), torch.float32)
        _, err = W.delta_err(got_b, got_p, W.reference(case, w.base)[0], W.reference(case, w.base, w.name)[0])
        cap = 3 * W.wire_figures(case, w)[1] + 0.02
        print(f"{case} {w.name}: err with a tenfold eps {err:.3f}  cap {cap:.3f}")
        assert err > cap + 0.1
    loud = W.WIRE_BY_NAME["blocks.0.attn1.to_q.weight"]
    got_b, got_p = W.oracle(*wrong(W.state(case)), torch.float32), W.oracle(*wrong(W.state(case, "loud", loud.name)), torch.float32)
    assert W.delta_err(got_b, got_p, W.reference(case)[0], W.reference(case, "loud", loud.name)[0])[1] < 0.02
