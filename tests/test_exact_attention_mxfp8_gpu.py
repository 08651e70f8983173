"""The MXFP8 attention family element by element: ce_attention_mxfp8, ce_attention_mxfp8_quant and ce_attention_mxfp8_add (both bodies,
attn_fwd_mxfp8_kernel and attn_fwd_mxfp8_sp_kernel, and the persistent item loop) against answers that are known exactly.  Every comparison is
`assert_exact(..., ulps=0)`.

The operands are BYTES the test writes itself (tests/exact_util.py, "MXFP8 attention"): e4m3 elements and E8M0 block scales of integer-valued
q, k and V with at most four significant bits, so nothing is quantised on the way in and the producers (pinned bit for bit in
tests/test_fp8_gpu.py) stay out of the comparison.  Every score is an integer in the exp2 domain, every P a power of two or exactly 0, l is
exact under both offset schedules and the output row is V[winner] (needle rows) or the mean of V over 2, 4 or 8 tied keys, the last valid key
among them (tie rows: they pin l).  Block scales differ per row, block and head; balance dimensions in two MX blocks cancel only under the
right scale bytes; every sample's keys stand in a row order of their own; whatever must not be read wins if it is read.  The constructions,
the contract oracle's agreement with the closed form under both schedules, and the list of wrong indices each case can see (X.MX_MISTAKES)
are proved on the CPU in tests/test_exact_constructions.py - no oracle runs here.

Operands stand in roomy buffers with row strides larger than D (q8 + 16, k8 + 32, out + 16, out8 + 48, add + 32); the gap columns of every
output hold a sentinel that must survive.

Bodies: the plain loop (variant 0; the plain entry point only - the other two always run the pipelined kernel), the default, and the
persistent loop forced to 8 workgroups so that every shape walks several items per workgroup; one case runs on the product defaults with
2 * 16 * 17 = 544 items for the 512 default workgroups.

Routes (diagnostic build's counter, waves x key tiles on the raise route), observed on an MI355X: 691 for q300-k130-h16-b3 (454 waves hold a
row that must raise), 429 for the mixed wave groups of q300-k257-h5-b3 (148), 19 for the far first tile of q300-k130-h2-b1 (19: 18 waves
with needle rows raise once, at tile 1, and one of the two tie-only last waves has a row without a tied key in tile 0), 0 for q256-k130-h16-b1 with every winner
in tile 0.  test_mxfp8_needles_take_the_raise_route_and_tile0_winners_never_do asserts the lower bounds and the zero.

First run on an MI355X: all 133 comparisons bit exact, for every body, entry point and shape - no kernel bug found.  The pipelined kernel
differs from the contract oracle only where it cannot show: P = exp2(S) / 2^offset underflows in exp2(S) for a tile hundreds of octaves
below the offset-to-be, where the oracle's exp2(S - offset) gives 8; such a tile is multiplied by 2^-64 or less at the raise that must follow.
Run time: 134 tests, 5.3 s for the file including the imports; the two slowest, 0.6 s each, are the first launches of a library.

What is NOT pinned here: the roundings of P on non-integer scores, exp2 at the last ulp and the fp32 order of the row sum on smooth data
(the norm tests of tests/test_fp8_gpu.py and the worst-block test of tests/test_exact_attention_gpu.py cover those), the second work order's
derivation under a deliberately wrong index (the needle data would see one; X.MX_MISTAKES names none there).

Mutants: each one-line change applied to a scratch copy of ce_attn_fp8.hip (reads stay inside the operands), the product library rebuilt
from it, the 61 default-body tests of this file and the 14 older MXFP8 attention tests (tests/test_fp8_gpu.py, tests/test_exact_attention_gpu.py)
run against it:

    mutant (pipelined kernel)                              new tests failing   older tests failing
    tail mask removed (clamped last key counted)                  51                 10
    tail mask at Nkv - 1                                          51                 10
    sq dword of head + 1                                          56                 11
    sv byte of the other 32-key half                              61                 12
    K rows of sample b + 1                                        41                  5
    K row stride H * 128 in place of ldk8                         56                  0   (not caught before)
    remainder block's sample = l2 / H                             21                  1
"""
import pytest
import torch

import exact_util as X
from exact_util import BF, assert_exact
from test_mxfp8_gemm_gpu import _contract

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
SENTINEL8 = 0xA5
NAMES = list(X.MX_CASES)
GAP_O, GAP_O8, GAP_ADD = 16, 48, 32


@pytest.fixture(params=["plain-loop", "default", "persistent-8"])
def mx_body(request):
    from chronoedit_amd import ops
    old_v = ops.set_attention_mxfp8_variant(0 if request.param == "plain-loop" else 1)
    old_p = ops.set_attention_mxfp8_persistent(8 if request.param == "persistent-8" else 512)
    yield request.param
    ops.set_attention_mxfp8_variant(old_v)
    ops.set_attention_mxfp8_persistent(old_p)


@pytest.fixture(params=["default", "persistent-8"])
def sp_body(request):
    from chronoedit_amd import ops
    old_p = ops.set_attention_mxfp8_persistent(8 if request.param == "persistent-8" else 512)
    yield request.param
    ops.set_attention_mxfp8_persistent(old_p)


_on_device = {}


def _operands(name):
    """(case, the six operand views of its launch on the GPU): the first B n rows and D columns of the roomy buffers, the first B sample blocks."""
    c = X.mx_named_case(name)
    if name not in _on_device:
        _on_device[name] = tuple(t.cuda() for t in (c.q8, c.sq, c.k8, c.sk, c.v8t, c.sv))
    q8, sq, k8, sk, v8t, sv = _on_device[name]
    mq, mk = c.B * c.n_q, c.B * c.n_kv
    return c, (q8[:mq, :c.D], sq[:mq], k8[:mk, :c.D], sk[:mk], v8t[:c.B], sv[:c.B])


def _bf16_out(c, gap):
    buf = torch.full((c.B * c.n_q, c.D + gap), SENTINEL, dtype=BF, device="cuda")
    return buf, buf[:, :c.D]


def _gap_untouched(buf, D, sentinel, what):
    assert bool((buf[:, D:] == sentinel).all()), f"{what}: the gap columns behind the rows were written"


def _check_mx(c, out8, scale8, want_bf16, what):
    from chronoedit_amd import ops
    want_s, want_q = _contract(want_bf16)
    assert_exact(out8[:, :c.D].cpu(), want_q, what + ": e4m3 bytes")
    assert_exact(ops.mx_scales_to_rows(scale8, c.B * c.n_q, c.D).cpu(), want_s, what + ": E8M0 scale bytes")
    _gap_untouched(out8, c.D, SENTINEL8, what)


@pytest.mark.parametrize("name", NAMES)
def test_attention_mxfp8_needles_and_ties(name, mx_body):
    from chronoedit_amd import ops
    c, opnd = _operands(name)
    buf, out = _bf16_out(c, GAP_O)
    ops.attention_mxfp8(*opnd, c.H, out=out, batch=c.B)
    assert_exact(out.cpu(), c.want, f"attention_mxfp8 {name} [{mx_body}]")
    _gap_untouched(buf, c.D, SENTINEL, name)


@pytest.mark.parametrize("name", NAMES)
def test_attention_mxfp8_quant_needles_and_ties(name, sp_body):
    from chronoedit_amd import ops
    c, opnd = _operands(name)
    out8 = torch.full((c.B * c.n_q, c.D + GAP_O8), SENTINEL8, dtype=torch.uint8, device="cuda")
    scale8 = torch.zeros(ops.mx_scale_bytes(c.B * c.n_q, c.D), dtype=torch.uint8, device="cuda")
    ops.attention_mxfp8(*opnd, c.H, batch=c.B, out8=out8[:, :c.D], scale8=scale8)
    _check_mx(c, out8, scale8, c.want, f"attention_mxfp8_quant {name} [{sp_body}]")


@pytest.mark.parametrize("form", ["out-of-place", "in-place", "mx-output"])
@pytest.mark.parametrize("name", NAMES)
def test_attention_mxfp8_add_needles_and_ties(name, form, sp_body):
    from chronoedit_amd import ops
    c, opnd = _operands(name)
    abuf, add = _bf16_out(c, GAP_ADD)
    add.copy_(c.add.cuda())
    what = f"attention_mxfp8_add {form} {name} [{sp_body}]"
    if form == "out-of-place":
        buf, out = _bf16_out(c, GAP_O)
        ops.attention_mxfp8(*opnd, c.H, out=out, batch=c.B, add=add)
        assert_exact(out.cpu(), c.want_add, what)
        _gap_untouched(buf, c.D, SENTINEL, what)
        assert_exact(add.cpu(), c.add, what + ": the add rows themselves")
    elif form == "in-place":
        got = ops.attention_mxfp8(*opnd, c.H, out=add, batch=c.B, add=add)
        assert got is add
        assert_exact(add.cpu(), c.want_add, what)
    else:
        out8 = torch.full((c.B * c.n_q, c.D + GAP_O8), SENTINEL8, dtype=torch.uint8, device="cuda")
        scale8 = torch.zeros(ops.mx_scale_bytes(c.B * c.n_q, c.D), dtype=torch.uint8, device="cuda")
        ops.attention_mxfp8(*opnd, c.H, batch=c.B, out8=out8[:, :c.D], scale8=scale8, add=add)
        _check_mx(c, out8, scale8, c.want_add, what)
        assert_exact(add.cpu(), c.add, what + ": the add rows themselves")
    _gap_untouched(abuf, c.D, SENTINEL, what + " (add)")


def test_attention_mxfp8_more_items_than_default_workgroups():
    """Product defaults, no knob touched: 2 query blocks x 16 heads x 17 samples = 544 work items for the persistent form's 512 workgroups, so
    workgroups 0..31 walk a second item (the remainder blocks of the last samples) and derive sample, head and block again."""
    from chronoedit_amd import ops
    name = "q257-k70-h16-b17"
    c, opnd = _operands(name)
    default = ops._KNOB_DEFAULTS["ce_set_attention_mxfp8_persistent"]
    assert ops.set_attention_mxfp8_persistent(-1) == default == 512 and ops.set_attention_mxfp8_variant(-1) == 1  # (-1: refused, reads the value)
    assert len(X.mx_work_items(c.n_q, c.H, c.B)) == (c.n_q + 255) // 256 * c.H * c.B > default
    buf, out = _bf16_out(c, GAP_O)
    ops.attention_mxfp8(*opnd, c.H, out=out, batch=c.B)
    assert_exact(out.cpu(), c.want, name + " on the product defaults")
    _gap_untouched(buf, c.D, SENTINEL, name)


def _waves_that_must_raise(c):
    """(sample, head, 32-row wave) groups with a row that has no key scoring 0 in tile 0 - its offset after tile 0 is <= -64 - 3, so the key
    that scores 0 later is 2^67 there, past e4m3: the wave raises once at least.  (A wave whose rows all hold a 0 in tile 0 never does.)"""
    late = torch.zeros(c.B, c.H, c.n_q, dtype=torch.bool)
    late[:, :, :c.n_needle] = (c.win >= 64).permute(0, 2, 1)
    for b in range(c.B):
        for h in range(c.H):
            for i in range(c.n_tie):
                late[b, h, c.n_needle + i] = int(c.tie_sets[b][h][i % 3].min()) >= 64
    pad = (-c.n_q) % 32
    return int(torch.nn.functional.pad(late, (0, pad)).view(c.B, c.H, -1, 32).any(-1).sum())


def test_mxfp8_needles_take_the_raise_route_and_tile0_winners_never_do():
    """The diagnostic build counts waves x key tiles on the raise route of the default kernel (an element of P past the e4m3 range: the offset
    of the wave's 32 rows is raised, O and l rescaled, the tile redone).  Needle rows whose winner sits past tile 0 must take it; with every
    winner in tile 0 (three key tiles, no tie rows) nobody does.  Mixed wave groups: rows that never raise share their wave with rows that do."""
    from chronoedit_amd import ops
    forced = ops._force_diag
    ops.force_diagnostics(True)
    try:
        seen = {}
        for name in ("q300-k130-h16-b3", "q300-k257-h5-b3-mixed", "q300-k130-h2-b1-far", "q256-k130-h16-b1-tile0"):
            c, opnd = _operands(name)
            ops.attention_exact_route_hits(reset=True)
            out = ops.attention_mxfp8(*opnd, c.H, batch=c.B)
            torch.cuda.synchronize()
            seen[name] = ops.attention_exact_route_hits(reset=True)[1]
            assert_exact(out.cpu(), c.want, name + " (diagnostic build)")
        print("MXFP8 raise-route hits (waves x tiles):", seen)
        assert seen.pop("q256-k130-h16-b1-tile0") == 0, seen
        least = {n: _waves_that_must_raise(X.mx_named_case(n)) for n in seen}
        assert all(seen[n] >= least[n] > 0 for n in seen), (seen, least)
    finally:
        ops.force_diagnostics(forced)
