"""ce_cfg_unipc_step element by element, exactly, on all five outputs (x, x_last, m0, m1, x0_out).

coef is an input of the kernel, so the test hands it dyadic coefficients (exact_util.UNIPC_COEF) with integer bf16 velocities in [-8, 8] and
a state in multiples of 1/4 in [-16, 16]: the CFG combine bf16(u + bf16(g * bf16(c - u))), x0 = x - sigma v, the corrector and the predictor
are then all exact in fp32, in any association and with or without FMA contraction, and under bf16_state more than a quarter of the new
latents need a real rounding.  The expected values come from the fp64 evaluation of the contract (exact_util.unipc_exact, which asserts that
every fp32 value is exact); the comparison is bit for bit.  The contract of the history: x_last <- the corrected sample (the old x when the
corrector is off), m1 <- the OLD m0, m0 <- the new x0."""
import pytest
import torch

import exact_util as X
from exact_util import assert_exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -24576.0
NAMES = ("x", "x_last", "m0", "m1", "x0_out")
GRID_CAP = 2048 * 256  # the launcher caps the grid at 2048 blocks of 256: any n above takes the grid-stride loop


def _ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from chronoedit_amd import ops
    return ops


def _step(ops, state, vc, vu, coef, flags, with_x0):
    """One kernel step on device copies of `state` = (x, x_last, m0, m1) that carry 8 sentinel elements past n; returns the five outputs."""
    n = vc.numel()
    bufs = []
    for t in state:
        b = torch.full((n + 8,), SENTINEL)
        b[:n] = t
        bufs.append(b.to(DEV))
    x0o = torch.full((n + 8,), SENTINEL, device=DEV)
    ops.cfg_unipc_step(vc.to(DEV), None if vu is None else vu.to(DEV), *[b[:n] for b in bufs], torch.tensor(coef, device=DEV),
                       x0_out=x0o[:n] if with_x0 else None, round_sigma_v=bool(flags & 1), bf16_state=bool(flags & 2))
    for b in bufs + [x0o]:
        assert bool((b[n:] == SENTINEL).all()), "cfg_unipc_step wrote past n"
    if not with_x0:
        assert bool((x0o == SENTINEL).all())
    return [b[:n].cpu() for b in bufs] + [x0o[:n].cpu() if with_x0 else None]


def _check(got, want, what):
    for name, g_, w_ in zip(NAMES, got, want):
        if g_ is not None:
            assert_exact(g_, w_, f"{what}: {name}")


@pytest.mark.parametrize("n", [1, 255, 257, GRID_CAP + 257])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_cfg_unipc_two_steps_exact(n, flags):
    """Two steps in a row with fresh velocities: the second one reads the history the first one wrote (m1 = the first step's old m0 is
    distinct from its new m0 in nearly every element).  n = 2048 * 256 + 257 makes the grid-stride loop take a second trip."""
    ops = _ops()
    g = torch.Generator().manual_seed(6000 + flags)
    vc, vu, *state = X.unipc_state(n, g)
    want, rounded = X.unipc_exact(vc, vu, *state, flags=flags)
    if flags & 2 and n > 255:
        assert rounded >= 0.25, rounded
    got = _step(ops, state, vc, vu, X.UNIPC_COEF, flags, True)
    _check(got, want, f"step 1 n={n} flags={flags}")
    assert torch.equal(want[3], state[2]) and (n < 255 or not torch.equal(want[3], want[2]))
    vc2, vu2 = X.unipc_state(n, g)[:2]
    want2, _ = X.unipc_exact(vc2, vu2, *want[:4], flags=flags)
    got2 = _step(ops, got[:4], vc2, vu2, X.UNIPC_COEF, flags, True)
    _check(got2, want2, f"step 2 n={n} flags={flags}")
    assert torch.equal(want2[3], want[2])  # m1 after step 2 = m0 after step 1


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "cond-only"])
@pytest.mark.parametrize("corrector", [1, 0])
@pytest.mark.parametrize("with_x0", [True, False], ids=["x0_out", "no-x0_out"])
def test_cfg_unipc_exact_in_every_mode(flags, cfg, corrector, with_x0):
    ops = _ops()
    n = 1000
    g = torch.Generator().manual_seed(6100 + flags + 2 * corrector)
    vc, vu, *state = X.unipc_state(n, g)
    vu = vu if cfg else None
    coef = list(X.UNIPC_COEF)
    coef[2] = float(corrector)
    want, _ = X.unipc_exact(vc, vu, *state, coef=coef, flags=flags)
    got = _step(ops, state, vc, vu, coef, flags, with_x0)
    _check(got, want, f"cfg={cfg} corrector={corrector} flags={flags}")
    if not corrector:
        assert_exact(got[1], X.round_bf16_f64(state[0].double()).float() if flags & 2 else state[0], "x_last = the old x without the corrector")


def test_cfg_unipc_rejects_an_empty_update():
    ops = _ops()
    x = torch.full((8,), SENTINEL, device=DEV)
    v = torch.zeros(8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ops.HipKernelError):
        ops.cfg_unipc_step(v[:0], None, x[:0], x[:0], x[:0], x[:0], torch.tensor(X.UNIPC_COEF, device=DEV))
    assert bool((x == SENTINEL).all())
