"""Inputs whose right answer is known per element, and the element-wise comparison the exact tests share.

GEMM / conv operands: small integers times a power of two per row (`int_rows`).  Every product is exact in fp32 and every partial sum of
one output element is an integer multiple of that element's unit 2^(e_a + e_w), below 2^20 units: the fp32 accumulator holds the exact
value whatever the summation order, tile shape or split-K slab count, and the expected output is the exact value rounded once to bf16.

Attention needles (`needle_q`, `needle_k`): every query row has one winning key per head, chosen by the test, that leads every other key by
>= 22 nats after the 1/sqrt(128) scale; the output row is then V[winner] (to within one bf16 ulp in general; exactly for V rows
away from zero).  Keys a kernel must not read
(rows past the valid length, padding, the neighbouring samples) win outright if they are read at all.

An ordinary module (not a conftest): the test files import it by name."""
import math

import torch

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------------------------
# element-wise comparison
# ------------------------------------------------------------------------------------------------------------------------------------
def _ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 / fp32 bit patterns as integers that are monotonic in the value (adjacent representable values differ by 1)."""
    if t.dtype == BF:
        bits = t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
        sign = 0x8000
    else:
        assert t.dtype == torch.float32, t.dtype
        bits = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        sign = 0x80000000
    return torch.where(bits >= sign, sign - bits, bits)  # -0 and +0 both map to 0


def mismatches(got: torch.Tensor, want: torch.Tensor, ulps: int = 0) -> torch.Tensor:
    """Bool mask of the elements where got and want differ (bit for bit, or by more than `ulps` units in the last place)."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    g, w = got.detach(), want.detach()
    if w.device != g.device:
        w = w.to(g.device)
    nan = torch.isnan(g.float()) | torch.isnan(w.float())
    if ulps == 0:
        bad = ~((g == w) | (torch.isnan(g.float()) & torch.isnan(w.float())))
        return bad
    return nan | ((_ordered(g) - _ordered(w)).abs() > ulps)


def assert_exact(got: torch.Tensor, want: torch.Tensor, what: str = "", ulps: int = 0, show: int = 6) -> None:
    """Fail unless every element of got equals want (or lies within `ulps` bf16 / fp32 ulps of it).  The message names the number of
    mismatching elements and the first few as (index, got, want) - no norm."""
    bad = mismatches(got, want, ulps)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()[:show].cpu()
    g, w = got.detach().float().cpu(), want.detach().float().cpu()
    rows = [f"{tuple(int(i) for i in ix)}: got {g[tuple(ix)].item()!r} want {w[tuple(ix)].item()!r}" for ix in idx]
    tol = "exactly" if ulps == 0 else f"within {ulps} ulp"
    raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ ({tol}); first: " + "; ".join(rows))


# ------------------------------------------------------------------------------------------------------------------------------------
# exactly computable GEMM / conv data
# ------------------------------------------------------------------------------------------------------------------------------------
def int_rows(rows: int, cols: int, gen: torch.Generator, lo: int = -4, hi: int = 4, emin: int = -2, emax: int = 2,
             device=None) -> torch.Tensor:
    """bf16 [rows, cols]: integers in [lo, hi] times 2^e, one e in [emin, emax] per row."""
    device = device or gen.device
    v = torch.randint(lo, hi + 1, (rows, cols), generator=gen, device=device, dtype=torch.int32).float()
    e = torch.randint(emin, emax + 1, (rows, 1), generator=gen, device=device, dtype=torch.int32).float()
    return (v * torch.exp2(e)).to(BF)


def int_vector(n: int, gen: torch.Generator, lo: int = -64, hi: int = 64, e: int = -2, device=None) -> torch.Tensor:
    """fp32 [n]: integers in [lo, hi] times 2^e (bias values that keep acc + bias exact in fp32)."""
    device = device or gen.device
    return torch.randint(lo, hi + 1, (n,), generator=gen, device=device, dtype=torch.int32).float() * 2.0 ** e


def exact_f64(x: torch.Tensor) -> torch.Tensor:
    """x (fp64) as fp32, asserting that the conversion is exact: the one rounding that follows (to bf16) is then the only one."""
    f = x.float()
    assert torch.equal(f.double(), x), "reference value not exact in fp32: the data recipe left its range"
    return f


def linear_f64(a: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """a @ w^T (+ bias) in fp64 - exact for `int_rows` data (on the device of the operands)."""
    r = a.double() @ w.double().t()
    if bias is not None:
        r = r + bias.double()
    return r


def bf16_rne(x64: torch.Tensor) -> torch.Tensor:
    """The exact fp64 value rounded ONCE to bf16 (round to nearest even)."""
    return exact_f64(x64).to(BF)


def gate_res_ref(lin_bf16: torch.Tensor, gate, res: torch.Tensor) -> torch.Tensor:
    """bf16(res.float() + lin * gate) with both fp32 roundings (a multiply, then an add: two eager CPU ops, never contracted)."""
    lin, r = lin_bf16.float().cpu(), res.float().cpu()
    t = lin if gate is None else torch.mul(lin, gate.cpu())
    return torch.add(r, t).to(BF)


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """bf16 ulp of |x| (fp32), for reporting."""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 7)


def mx_operand(rows: int, K: int, gen: torch.Generator) -> torch.Tensor:
    """bf16 [rows, K]: integers in [-15, 15] times 2^e per 32-element block, e in {e_row - 1, e_row}, e_row in [-2, 2]; an all-zero row,
    all-zero blocks, a block whose amax is negative, and blocks at |int| = 15 (amax mantissa 1.875 > 1.75: the scale's +1 branch)."""
    v = torch.randint(-15, 16, (rows, K), generator=gen).float()
    er = torch.randint(-2, 3, (rows, 1), generator=gen).float()
    eb = er - torch.randint(0, 2, (rows, K // 32), generator=gen).float()
    v[min(2, rows - 1)] = 0
    v[0, 32:64] = 0
    v[rows - 1, -32:] = 0
    v[min(1, rows - 1), 64:96] = -v[min(1, rows - 1), 64:96].abs()
    v[min(1, rows - 1), 64] = -15
    v[min(3, rows - 1), 0:32:2] = 15
    return (v * torch.exp2(eb).repeat_interleave(32, dim=1)).to(BF)


# ------------------------------------------------------------------------------------------------------------------------------------
# attention needles
# ------------------------------------------------------------------------------------------------------------------------------------
NEEDLE_C = 512.0       # score = -C * sum_p (a_p - d_p)^2 + const(row): the runner-up trails by C / sqrt(128) = 45 nats
NEEDLE_DIGITS = 5      # base-8 digits of the key index: up to 32768 keys per sample
NEEDLE_BIG = 2.0 ** 18  # weight of the winner-if-read dimensions: beats the largest in-sample lead, 512 * 5 * 49, exactly in fp32
LEAK_DIM = 100         # dims 100, 101, 102: neighbour bonus (key of sample s carries +1 on dim 100 + s % 3)
INVALID_DIM = 103      # keys that must never be read carry +1 here; every query carries NEEDLE_BIG
MIN_MARGIN_NATS = 22.0


def key_digits(j: torch.Tensor) -> torch.Tensor:
    """[n] key indices -> [n, 5] base-8 digits (least significant first)."""
    return torch.stack([(j >> (3 * p)) & 7 for p in range(NEEDLE_DIGITS)], -1).double()


def needle_k(n_keys: int, heads: int, sample: int = 0, invalid=None) -> torch.Tensor:
    """K rows [n_keys, heads*128] (fp64, exact in bf16) of one sample: key j has (d_p, d_p^2) on dims (2p, 2p+1) of every head,
    +1 on the neighbour-bonus dim 100 + sample % 3, and +1 on dim 103 where `invalid` (bool [n_keys]) is set."""
    d = key_digits(torch.arange(n_keys))
    kh = torch.zeros(n_keys, 128, dtype=torch.float64)
    kh[:, 0:2 * NEEDLE_DIGITS:2] = d
    kh[:, 1:2 * NEEDLE_DIGITS:2] = d * d
    kh[:, LEAK_DIM + sample % 3] = 1.0
    if invalid is not None:
        kh[invalid, INVALID_DIM] = 1.0
    return kh.repeat(1, heads)


def needle_q(winners: torch.Tensor, sample: int = 0, batch: int = 1) -> torch.Tensor:
    """Q rows [n_q, heads*128] (fp64, exact in bf16) for winners [n_q, heads] (key index per query row and head): (2C a_p, -C) on
    dims (2p, 2p+1), so that score(i, j) = -C sum_p (a_p - d_p)^2 + const(i), 0 below the maximum only at j = winner; +NEEDLE_BIG on
    dim 103 (a key flagged invalid wins outright if it is read) and, when batch > 1, on the bonus dims of the other two residues
    (sample +- 1) % 3 (a key of a neighbouring sample wins outright if it is read; the sample's own bonus dim meets 0)."""
    nq, heads = winners.shape
    a = key_digits(winners.reshape(-1)).view(nq, heads, NEEDLE_DIGITS)
    qh = torch.zeros(nq, heads, 128, dtype=torch.float64)
    qh[:, :, 0:2 * NEEDLE_DIGITS:2] = 2.0 * NEEDLE_C * a
    qh[:, :, 1:2 * NEEDLE_DIGITS:2] = -NEEDLE_C
    if batch > 1:
        for nb in {(sample + 1) % 3, (sample - 1) % 3} - {sample % 3}:
            qh[:, :, LEAK_DIM + nb] = NEEDLE_BIG
    qh[:, :, INVALID_DIM] = NEEDLE_BIG
    return qh.reshape(nq, heads * 128)


def needle_scores(q: torch.Tensor, k: torch.Tensor, heads: int) -> torch.Tensor:
    """fp64 scores [heads, n_q, n_k] * 1/sqrt(128)."""
    qh = q.double().view(q.shape[0], heads, 128).transpose(0, 1)
    kh = k.double().view(k.shape[0], heads, 128).transpose(0, 1)
    return qh @ kh.transpose(1, 2) / math.sqrt(128.0)


def winners_for(n_q: int, n_keys: int, heads: int, gen: torch.Generator, must=()) -> torch.Tensor:
    """[n_q, heads] winning key per query row and head: a different random permutation per head (head mix-ups show), with the keys in
    `must` (edge keys, every key of the ragged last tile, ...) placed on the LAST query rows of every head (the partial query block)
    and on the first ones."""
    w = torch.empty(n_q, heads, dtype=torch.int64)
    must = [int(m) for m in must if 0 <= int(m) < n_keys]
    for h in range(heads):
        col = torch.randint(0, n_keys, (n_q,), generator=gen)
        perm = torch.randperm(n_keys, generator=gen)
        col[: min(n_q, n_keys)] = perm[: min(n_q, n_keys)]
        if must:
            m = torch.tensor(must, dtype=torch.int64)
            m = m[torch.randperm(len(m), generator=gen)]  # another order per head
            k = min(len(m), n_q)
            col[n_q - k:] = m[:k]
            k2 = min(len(m), max(n_q - k, 0))
            col[:k2] = m.flip(0)[:k2]
        w[:, h] = col
    return w


def edge_keys(n_keys: int):
    """Keys the tests always make winners: 0, n-1, 63, 64, 127, 128 and every key of the ragged last 64-key tile."""
    last = (n_keys - 1) // 64 * 64
    return sorted({0, n_keys - 1, 63, 64, 127, 128} | set(range(last, n_keys)))


def poison_v(n: int, D: int, gen: torch.Generator, scale: float = 1.0) -> torch.Tensor:
    """Ordinary V rows [n, D] (bf16): distinct per key and column, so that a wrong winner or a permuted column shows."""
    return (torch.randn(n, D, generator=gen) * scale).to(BF)


POISON = 3.0e4  # value behind every key that must never be read (finite, exact in bf16)


def needle_margins(q: torch.Tensor, k: torch.Tensor, heads: int, winners: torch.Tensor, forbidden=None):
    """(lead, forbidden_lead): per query row and head, the winner's scaled score minus the best other ALLOWED key's, and the best
    FORBIDDEN key's scaled score minus the winner's (+inf / -inf where there is none).  Both must be >= MIN_MARGIN_NATS."""
    allowed = torch.ones(k.shape[0], dtype=torch.bool) if forbidden is None else ~forbidden
    leads, fls = [], []
    for r0 in range(0, q.shape[0], 1024):  # (row chunks: the fp64 score block of 7200 x 14400 keys would not fit comfortably)
        s = needle_scores(q[r0:r0 + 1024], k, heads)                 # [H, rows, nk]
        wi = winners[r0:r0 + 1024].t().unsqueeze(-1)                 # [H, rows, 1]
        sw = s.gather(-1, wi)
        other = s.masked_fill(~allowed, -math.inf).scatter(-1, wi, -math.inf)
        leads.append((sw - other.amax(-1, keepdim=True)).squeeze(-1))
        fls.append((s.masked_fill(allowed, -math.inf).amax(-1, keepdim=True) - sw).squeeze(-1))
    lead, fl = torch.cat(leads, 1), torch.cat(fls, 1)
    if forbidden is None or not forbidden.any():
        fl = torch.full_like(lead, math.inf)
    return lead, fl
