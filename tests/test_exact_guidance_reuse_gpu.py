"""ce_cfg_unipc_step_delta element by element, exactly (the style of test_exact_sched_gpu.py; chronoedit_amd/guidance.py has the contract).

Store mode: the five outputs against ops.cfg_unipc_step on copies of the same state, and delta against (vc - vu) in CPU bf16 arithmetic.
Reuse mode: on exact_util.unipc_state inputs (integer velocities: c - d and c - (c - d) are exact) against X.unipc_exact(vc, vc - d, ...);
on random bf16 inputs the guided velocity the kernel used, recovered from x0_out, against the contract restated on CPU bf16 tensors.
Measure mode: exactly summable integer directions against the integer sums; random directions against float64 sums.
Every buffer, the delta buffer included, carries 8 sentinel elements behind its n."""
import math

import pytest
import torch

import exact_util as X
from exact_util import assert_exact

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
SENTINEL = -24576.0  # exact in bf16 and in fp32
NAMES = ("x", "x_last", "m0", "m1", "x0_out")
GRID_CAP = 2048 * 256  # the launcher caps the grid at 2048 blocks of 256: any n above takes the grid-stride loop
SIZES = [1, 255, 257, GRID_CAP + 257]


def _ops():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from chronoedit_amd import ops
    return ops


def _padded(t, n, dtype=torch.float32):
    b = torch.full((n + 8,), SENTINEL, dtype=dtype)
    b[:n] = t
    return b.to(DEV)


def _step(ops, state, vc, vu, coef, flags, with_x0, delta=None, plain=False):
    """One kernel step on device copies of `state` that carry 8 sentinel elements past n.  delta: the bf16 direction a reuse step reads (vu
    None) - a store step gets a sentinel-filled buffer.  plain: ops.cfg_unipc_step instead.  Returns (the five outputs, delta after)."""
    n = vc.numel()
    bufs = [_padded(t, n) for t in state]
    x0o = torch.full((n + 8,), SENTINEL, device=DEV)
    dbuf = _padded(delta if delta is not None else torch.full((n,), SENTINEL), n, BF)
    kw = dict(x0_out=x0o[:n] if with_x0 else None, round_sigma_v=bool(flags & 1), bf16_state=bool(flags & 2))
    args = (vc.to(DEV), None if vu is None else vu.to(DEV), *[b[:n] for b in bufs], torch.tensor(coef, device=DEV))
    if plain:
        ops.cfg_unipc_step(*args, **kw)
    else:
        ops.cfg_unipc_step_delta(*args, dbuf[:n], **kw)
    for b in bufs + [x0o, dbuf]:
        assert bool((b[n:] == SENTINEL).all()), "the step wrote past n"
    if not with_x0:
        assert bool((x0o == SENTINEL).all())
    return [b[:n].cpu() for b in bufs] + [x0o[:n].cpu() if with_x0 else None], dbuf[:n].cpu()


def _check(got, want, what):
    for name, g_, w_ in zip(NAMES, got, want):
        if g_ is not None:
            assert_exact(g_, w_, f"{what}: {name}")


def _random_bf16(n, gen, spread=6):
    return (torch.randn(n, generator=gen) * torch.exp2(torch.randint(-spread, spread + 1, (n,), generator=gen).float())).to(BF)


# ---- store mode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_store_mode_is_the_plain_step_plus_the_direction(n, flags):
    ops = _ops()
    g = torch.Generator().manual_seed(7000 + flags)
    vc, vu, *state = X.unipc_state(n, g)
    plain, _ = _step(ops, state, vc, vu, X.UNIPC_COEF, flags, True, plain=True)
    want, _ = X.unipc_exact(vc, vu, *state, flags=flags)
    _check(plain, want, "the plain step")
    got, delta = _step(ops, state, vc, vu, X.UNIPC_COEF, flags, True)
    for name, a, b in zip(NAMES, got, plain):
        assert_exact(a, b, f"store n={n} flags={flags}: {name} against cfg_unipc_step")
    assert_exact(delta, vc - vu, "delta = bf16(vc - vu)")  # (CPU bf16 tensor arithmetic: one rounding)
    # random bf16 velocities (real roundings in the combine): still the plain step's bits, still bf16(c - u)
    vc, vu = _random_bf16(n, g), _random_bf16(n, g)
    state = [torch.randn(n, generator=g) for _ in range(4)]
    plain, _ = _step(ops, state, vc, vu, X.UNIPC_COEF, flags, True, plain=True)
    got, delta = _step(ops, state, vc, vu, X.UNIPC_COEF, flags, True)
    for name, a, b in zip(NAMES, got, plain):
        assert_exact(a, b, f"store (random) n={n} flags={flags}: {name} against cfg_unipc_step")
    assert_exact(delta, vc - vu, "delta = bf16(vc - vu), random velocities")
    if n > 255:
        assert not torch.equal((vc - vu).float(), vc.float() - vu.float())  # (the direction really needs its rounding)


# ---- reuse mode --------------------------------------------------------------------------------------------------------------------
def _direction(n, gen):
    """Integer bf16 directions in [-8, 8]: with integer vc in [-8, 8], vc - d is an exact bf16 integer and vc - (vc - d) == d."""
    return torch.randint(-8, 9, (n,), generator=gen).to(BF)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_reuse_mode_two_steps_exact(n, flags):
    ops = _ops()
    g = torch.Generator().manual_seed(7100 + flags)
    vc, _, *state = X.unipc_state(n, g)
    d = _direction(n, g)
    want, _ = X.unipc_exact(vc, vc - d, *state, flags=flags)
    got, d_after = _step(ops, state, vc, None, X.UNIPC_COEF, flags, True, delta=d)
    _check(got, want, f"reuse step 1 n={n} flags={flags}")
    assert_exact(d_after, d, "a reuse step only reads delta")
    vc2 = X.unipc_state(n, g)[0]
    want2, _ = X.unipc_exact(vc2, vc2 - d, *want[:4], flags=flags)
    got2, d_after = _step(ops, got[:4], vc2, None, X.UNIPC_COEF, flags, True, delta=d)
    _check(got2, want2, f"reuse step 2 n={n} flags={flags}")
    assert_exact(d_after, d, "a reuse step only reads delta")
    assert torch.equal(want2[3], want[2])  # m1 after step 2 = m0 after step 1
    if n > 255:  # the direction matters: without it the result differs
        assert not torch.equal(want[0], X.unipc_exact(vc, None, *state, flags=flags)[0][0])


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("corrector", [1, 0])
@pytest.mark.parametrize("with_x0", [True, False], ids=["x0_out", "no-x0_out"])
def test_reuse_mode_exact_in_every_mode(flags, corrector, with_x0):
    ops = _ops()
    n = 1000
    g = torch.Generator().manual_seed(7200 + flags + 2 * corrector)
    vc, _, *state = X.unipc_state(n, g)
    d = _direction(n, g)
    coef = list(X.UNIPC_COEF)
    coef[2] = float(corrector)
    want, _ = X.unipc_exact(vc, vc - d, *state, coef=coef, flags=flags)
    got, d_after = _step(ops, state, vc, None, coef, flags, with_x0, delta=d)
    _check(got, want, f"reuse corrector={corrector} flags={flags}")
    assert_exact(d_after, d, "a reuse step only reads delta")


@pytest.mark.parametrize("n", SIZES)
def test_reuse_mode_velocity_on_random_bf16_inputs(n):
    """flag 0, sigma = 0.5, x = 0: x0_out = -0.5 v exactly, so v = -2 x0_out is the guided velocity the kernel used.  The contract on CPU
    bf16 tensors, one op per rounding: u' = c - d, v = u' + g * d."""
    ops = _ops()
    g = torch.Generator().manual_seed(7300)
    vc, d = _random_bf16(n, g), _random_bf16(n, g, spread=3)
    zeros = [torch.zeros(n) for _ in range(4)]
    coef = list(X.UNIPC_COEF)  # g = 4 (a power of two would hide the rounding of g * d: use 5)
    coef[0] = 5.0
    gs = torch.tensor(5.0, dtype=BF)
    got, d_after = _step(ops, zeros, vc, None, coef, 0, True, delta=d)
    u = vc - d
    want = u + gs * d
    assert want.dtype == BF and u.dtype == BF
    assert_exact((-2.0 * got[4]).to(BF), want, f"guided velocity n={n}")
    assert torch.equal((-2.0 * got[4]).to(BF).float(), -2.0 * got[4])  # (the recovered velocity is a bf16 value)
    assert_exact(d_after, d, "a reuse step only reads delta")
    if n > 255:
        assert not torch.equal((gs * d).float(), 5.0 * d.float())  # (g * d really needs its rounding)


# ---- measure mode ------------------------------------------------------------------------------------------------------------------
def _measured_steps(ops, dirs, A, n, rows=None):
    """Feed the directions one after the other through measuring store steps (vc = d, vu = 0 give direction d exactly when d is bf16);
    returns (table fp32 [len(dirs), A + 1] on the CPU, ring [A, n] on the CPU)."""
    ring = torch.full((A * n + 8,), SENTINEL, dtype=BF, device=DEV)
    ring[: A * n] = 0
    table = torch.full((len(dirs) + 1, A + 1), SENTINEL, device=DEV)
    zero_v = torch.zeros(n, dtype=BF, device=DEV)
    coef = torch.tensor(X.UNIPC_COEF, device=DEV)
    for i, d in enumerate(dirs):
        state = [torch.zeros(n, device=DEV) for _ in range(4)]
        ops.cfg_unipc_step_delta(d.to(DEV), zero_v, *state, coef, ring[: A * n].view(A, n), slot=i % A, table=table[: len(dirs)], row=i)
    assert bool((ring[A * n:] == SENTINEL).all()) and bool((table[len(dirs):] == SENTINEL).all()), "the measuring step wrote past its buffers"
    return table[: len(dirs)].cpu(), ring[: A * n].view(A, n).cpu()


@pytest.mark.parametrize("n", SIZES)
def test_measure_mode_sums_are_exact_on_integer_directions(n):
    """A = 3, the ring filled by three earlier stores, directions in [-2, 2]: every term is an integer <= 16 and every partial sum an
    integer below 2^24 - the fp32 accumulators hold the integer answer whatever the order."""
    ops = _ops()
    A = 3
    g = torch.Generator().manual_seed(7400)
    dirs = [torch.randint(-2, 3, (n,), generator=g).to(BF) for _ in range(5)]
    table, ring = _measured_steps(ops, dirs, A, n)
    for i in (3, 4):  # (steps whose ring is full)
        want = [float(((dirs[i].double() - dirs[i - a].double()) ** 2).sum()) for a in (1, 2, 3)] + [float((dirs[i].double() ** 2).sum())]
        assert table[i].tolist() == want, (i, table[i].tolist(), want)
    for i in (2, 3, 4):
        assert_exact(ring[i % A], dirs[i], f"slot {i % A} holds direction {i}")


@pytest.mark.parametrize("n", [257, GRID_CAP + 257])
def test_measure_mode_random_sums_within_the_fp32_bound_and_repeatable(n):
    """Non-negative fp32 terms summed in two stages over at most 2^21 terms: about 30 * 2^-24 = 2e-6 relative; the bound is 1e-5."""
    ops = _ops()
    from chronoedit_amd.guidance import rel_l2_from_sums
    A = 3
    g = torch.Generator().manual_seed(7500)
    dirs = [_random_bf16(n, g, spread=2) for _ in range(5)]
    table, _ = _measured_steps(ops, dirs, A, n)
    again, _ = _measured_steps(ops, dirs, A, n)
    assert torch.equal(table.view(torch.int32), again.view(torch.int32)), "two runs, different bits"
    for i in (3, 4):
        want = [float(((dirs[i].double() - dirs[i - a].double()) ** 2).sum()) for a in (1, 2, 3)] + [float((dirs[i].double() ** 2).sum())]
        for k, w in enumerate(want):
            e = abs(float(table[i, k]) - w) / w
            print(f"measure n={n} step {i} sum {k}: relative error {e:.2e} (bound 1e-5)")
            assert e <= 1e-5, (i, k, e)
    # ages older than the ring's history are NaN on the host side
    hist = [min(i, A) for i in range(5)]
    rel = rel_l2_from_sums(table.numpy(), A, hist)
    for i in range(5):
        for a in range(A):
            assert math.isnan(rel[i][a]) == (a >= hist[i]), (i, a, rel[i])
    want = math.sqrt(float(((dirs[4].double() - dirs[2].double()) ** 2).sum()) / float((dirs[4].double() ** 2).sum()))
    assert abs(rel[4][1] - want) <= 1e-5 * want


def test_delta_entry_rejects_bad_arguments():
    ops = _ops()
    n = 16
    x = [torch.full((n,), SENTINEL, device=DEV) for _ in range(4)]
    v = torch.zeros(n, dtype=BF, device=DEV)
    coef = torch.tensor(X.UNIPC_COEF, device=DEV)
    with pytest.raises(ValueError):
        ops.cfg_unipc_step_delta(v, v, *x, coef, torch.zeros(n - 1, dtype=BF, device=DEV))
    with pytest.raises(ValueError):  # a ring of 5
        ops.cfg_unipc_step_delta(v, v, *x, coef, torch.zeros(5, n, dtype=BF, device=DEV), slot=0, table=torch.zeros(1, 6, device=DEV))
    with pytest.raises(ValueError):  # measuring without the unconditional sample
        ops.cfg_unipc_step_delta(v, None, *x, coef, torch.zeros(2, n, dtype=BF, device=DEV), slot=0, table=torch.zeros(1, 3, device=DEV))
    lib = ops.lib()
    d = torch.zeros(n, dtype=BF, device=DEV)
    p = ops._ptr
    assert lib.ce_cfg_unipc_step_delta(p(v), p(v), p(x[0]), p(x[1]), p(x[2]), p(x[3]), p(None), p(coef), p(None), n, 0, 0, 0, p(None), 0, p(None), 0,
                                       ops._stream()) == -1  # no delta
    assert lib.ce_cfg_unipc_step_delta(p(v), p(v), p(x[0]), p(x[1]), p(x[2]), p(x[3]), p(None), p(coef), p(d), n, 0, 2, 2, p(x[0]), 40960, p(x[1]), 0,
                                       ops._stream()) == -1  # slot outside the ring
    assert lib.ce_cfg_unipc_step_delta(p(v), p(v), p(x[0]), p(x[1]), p(x[2]), p(x[3]), p(None), p(coef), p(d), n, 0, 2, 0, p(x[0]), 16, p(x[1]), 0,
                                       ops._stream()) == -1  # scratch too small
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in x)  # nothing was written
