"""Inputs whose right answer is known per element, and the element-wise comparison the exact tests share.

GEMM / conv operands: small integers times a power of two per row (`int_rows`).  Every product is exact in fp32 and every partial sum of
one output element is an integer multiple of that element's unit 2^(e_a + e_w), below 2^20 units: the fp32 accumulator holds the exact
value whatever the summation order, tile shape or split-K slab count, and the expected output is the exact value rounded once to bf16.

Attention needles (`needle_q`, `needle_k`): every query row has one winning key per head, chosen by the test, that leads every other key by
>= 22 nats after the 1/sqrt(128) scale; the output row is then V[winner] (to within one bf16 ulp in general; exactly for V rows
away from zero).  Keys a kernel must not read
(rows past the valid length, padding, the neighbouring samples) win outright if they are read at all.

Self-attention sums (`sums_case`, `SUM_CASES`, `sum_named_case`, `attention_sums_f64`, `SUM_MISTAKES`, `online_softmax_f32`, `sum_margins`,
`sum_split_count`): tie rows (a set of keys scores exactly 0, the row is the mean of the set's V rows) and stair rows (keys j octaves below
the top, one nonzero V entry per column, the row is +-r / 8) in the same 32-row groups as needle rows, silent all-zero keys behind the
valid ones - they pin the row sum, the accumulation over tiles, the rescale and attention_1head's split merge.

MXFP8 attention (`mx_case`, `mxfp8_attention_f64`, `MX_MISTAKES`): the same idea on operands handed over as e4m3 bytes with E8M0 block
scales - integer scores in the exp2 domain, every P a power of two or 0, needle rows and tie rows, scales that a wrong scale byte betrays.

The fp8 mode's operand producers and GEMM tails (`row_fp8_ref`, `mx_contract`, `ln_mx_case`, `rms_mx_case`, `sat_gemm_case`, `bend_gemm_case`,
`fp8_tail_plan`, `FP8_MISTAKES`): the per-row quantiser restated operation by operation, MX producers on rows that are known exactly, GEMM
operands whose GELU input is exact and saturated (the FFN-up form's bytes need no transcendental), and the split-K plan restated.

The VAE's implicit-GEMM conv, RMS_norm (+ SiLU) and the conv with the norm in its epilogue (`conv_frames_f64`, `CONV_CASES`, `conv_case`,
`CONV_MISTAKES`, `rms_case`, `rms_restate_f32`, `fused_case`, `RMS_MISTAKES`): the header's conv formula restated on the stored frames, border
included, one case per configuration the engine sends, and rows of +-2^k whose norm is known bit for bit.

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


def needle_k(n_keys: int, heads: int, sample=0, invalid=None, labels=None) -> torch.Tensor:
    """K rows [n_keys, heads*128] (fp64, exact in bf16) of one sample: key j has (d_p, d_p^2) on dims (2p, 2p+1) of every head,
    +1 on the neighbour-bonus dim 100 + sample % 3, and +1 on dim 103 where `invalid` (bool [n_keys]) is set.  `labels` (int64 [n_keys]):
    row j carries the digits of labels[j] in place of j (another row order per sample: a neighbour's rows read instead of the sample's own
    pick another row); sample=None: no neighbour bonus (an operand that every sample of a launch reads)."""
    d = key_digits(torch.arange(n_keys) if labels is None else labels)
    kh = torch.zeros(n_keys, 128, dtype=torch.float64)
    kh[:, 0:2 * NEEDLE_DIGITS:2] = d
    kh[:, 1:2 * NEEDLE_DIGITS:2] = d * d
    if sample is not None:
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


def needle_margins(q: torch.Tensor, k: torch.Tensor, heads: int, winners: torch.Tensor, forbidden=None, bias=None):
    """(lead, forbidden_lead): per query row and head, the winner's scaled score minus the best other ALLOWED key's, and the best
    FORBIDDEN key's scaled score minus the winner's (+inf / -inf where there is none).  Both must be >= MIN_MARGIN_NATS.  `bias` (fp64
    [n_k], nats): added to every row's scores - a key's softmax weight counted in."""
    allowed = torch.ones(k.shape[0], dtype=torch.bool) if forbidden is None else ~forbidden
    leads, fls = [], []
    for r0 in range(0, q.shape[0], 1024):  # (row chunks: the fp64 score block of 7200 x 14400 keys would not fit comfortably)
        s = needle_scores(q[r0:r0 + 1024], k, heads)                 # [H, rows, nk]
        if bias is not None:
            s = s + bias
        wi = winners[r0:r0 + 1024].t().unsqueeze(-1)                 # [H, rows, 1]
        sw = s.gather(-1, wi)
        other = s.masked_fill(~allowed, -math.inf).scatter(-1, wi, -math.inf)
        leads.append((sw - other.amax(-1, keepdim=True)).squeeze(-1))
        fls.append((s.masked_fill(allowed, -math.inf).amax(-1, keepdim=True) - sw).squeeze(-1))
    lead, fl = torch.cat(leads, 1), torch.cat(fls, 1)
    if forbidden is None or not forbidden.any():
        fl = torch.full_like(lead, math.inf)
    return lead, fl


# ------------------------------------------------------------------------------------------------------------------------------------
# cross-attention: two key segments on one query row, operands shared between the samples, segment 1 cut per sample and its last
# readable key weighted (ce_attention_2seg_vt_bf16 / _strided_bf16 / _weighted_bf16 / _quant_bf16)
#
# Needle rows: as above, per segment.  Every sample's keys sit in another row order (`needle_k(labels=)`): the neighbour's rows read in
# place of the sample's own pick another row.  A weight of a few octaves on a key cannot overturn a 65-octave lead: a needle row pins
# masking, the per-sample cut, strides and positions, never the weight.
# Flat rows pin the weight: the query is zero on segment 1's digit dims, every readable key of segment 1 scores exactly 0, the last one
# counts m = 2^w times, and valid - 1 + m = 2^k: the softmax is 1 / 2^k per plain key and m / 2^k for the last, exactly.  V1 is sparse - column
# c is zero except at ONE key i(c), where it holds +-r 2^(k-3), r in 1..7 - so the segment's output in column c is +-r mult / 8 (mult = m for
# the weighted key, else 1): three significant bits, and one fp32 ulp of relative error in exp2, the row sum or 1 / l cannot move the
# rounding to bf16.  Segment 2 of a flat row is a needle with an integer V2 row, scaled so that the final bf16 add is exact.
# ------------------------------------------------------------------------------------------------------------------------------------
SEG2_DIM0 = 12  # segment 2's digits sit on dims 12..21 of the one query row and its invalid flag on INVALID_DIM + 1
LOG2E = 1.4426950408889634


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def vt_stride(n: int) -> int:
    """The engine's V^T column stride between samples: the key count rounded up to 8 (16-byte rows), no multiple of the 64-key tile."""
    return (n + 7) // 8 * 8


def seg2_keys(k: torch.Tensor, heads: int) -> torch.Tensor:
    """Needle keys moved to segment 2's dims: digits 0..9 -> 12..21, the invalid flag -> INVALID_DIM + 1, the neighbour bonus stays."""
    kh = k.reshape(-1, heads, 128)
    out = torch.zeros_like(kh)
    out[:, :, SEG2_DIM0:SEG2_DIM0 + 2 * NEEDLE_DIGITS] = kh[:, :, 0:2 * NEEDLE_DIGITS]
    out[:, :, LEAK_DIM:LEAK_DIM + 3] = kh[:, :, LEAK_DIM:LEAK_DIM + 3]
    out[:, :, INVALID_DIM + 1] = kh[:, :, INVALID_DIM]
    return out.reshape(-1, heads * 128)


def two_segment_q(q1: torch.Tensor, q2: torch.Tensor, heads: int) -> torch.Tensor:
    """One query row for both segments: q1 (segment 1's needle query, with the neighbour-bonus dims) plus q2's digits on dims 12..21 and the
    invalid weight on INVALID_DIM + 1 as well."""
    q = q1.clone().reshape(-1, heads, 128)
    q[:, :, SEG2_DIM0:SEG2_DIM0 + 2 * NEEDLE_DIGITS] = q2.reshape(-1, heads, 128)[:, :, 0:2 * NEEDLE_DIGITS]
    q[:, :, INVALID_DIM + 1] = q[:, :, INVALID_DIM]
    return q.reshape(-1, heads * 128)


def needle_v(n: int, D: int, gen: torch.Generator, positive: bool = False) -> torch.Tensor:
    """V rows with |v| in [1, 2): no value near zero (a 1e-20 weight times a neighbour must stay below half an ulp)."""
    mag = 1.0 + torch.rand(n, D, generator=gen)
    sign = torch.where(torch.rand(n, D, generator=gen) < 0.5, -1.0, 1.0)
    return (mag if positive else mag * sign).to(BF)


def needle_segment(n_q: int, n_rows: int, valid, heads: int, batch: int, gen: torch.Generator, share_q: bool = False, share_k: bool = False):
    """One key segment of `batch` samples: (qs, ks, wins).  ks: fp64 [n_rows, heads*128] per sample (one if share_k), rows >= valid[s] flagged
    invalid, rows < valid[s] in a random order of their own (label l sits in row order[l]; the rows `edge_keys(valid)`, valid - 1 and valid - 2
    carry the lowest labels).  qs: needle queries [n_q, heads*128] per sample (one if share_q; then the labels stay below min(valid) and the
    query carries no neighbour bonus); the lowest labels are forced onto the first and last rows.  wins: int64 [batch, n_q, heads], the winning
    ROW of sample b's keys."""
    assert len(valid) == batch and (not share_k or len(set(valid)) == 1) and max(valid) <= n_rows and min(valid) >= 1
    orders, ks = [], []
    for s in range(1 if share_k else batch):
        v = int(valid[s])
        first = [r for r in dict.fromkeys([v - 1, v - 2, 0] + edge_keys(v)) if 0 <= r < v]
        rest = torch.tensor(sorted(set(range(v)) - set(first)), dtype=torch.int64)
        order = torch.cat([torch.tensor(first, dtype=torch.int64), rest[torch.randperm(len(rest), generator=gen)]])
        label = torch.arange(n_rows)
        label[order] = torch.arange(v)
        orders.append(order)
        ks.append(needle_k(n_rows, heads, sample=None if share_k else s, invalid=torch.arange(n_rows) >= v, labels=label))
    labs = [winners_for(n_q, min(valid) if share_q else int(valid[b]), heads, gen, must=range(72)) for b in range(1 if share_q else batch)]
    qs = [needle_q(lab, sample=b, batch=1 if share_q else batch) for b, lab in enumerate(labs)]
    wins = torch.stack([orders[0 if share_k else b][labs[0 if share_q else b]] for b in range(batch)])
    return qs, ks, wins


def flat_wcols(D: int) -> torch.Tensor:
    """bool [D]: the columns whose one nonzero V1 entry sits at the weighted key (a quarter of them, another phase in every head)."""
    c = torch.arange(D)
    return (c + c // 128) % 4 == 0


def flat_v1(n_rows: int, valid: int, m: int, D: int, gen: torch.Generator):
    """(v1 fp64 [n_rows, D], out1 fp64 [D], key int64 [D]) for valid - 1 plain keys and the last one counted m times, valid - 1 + m = 2^k:
    column c is zero except at key[c] (valid - 1 on `flat_wcols`; elsewhere cycling through edge_keys(valid) and valid - 2; -1: an all-zero
    column, when the weighted key is the only one), where it holds +-r 2^(k-3); rows >= valid hold POISON.  out1: the segment's exact output
    of a flat row, +-r mult / 8."""
    k = int(math.log2(valid - 1 + m))
    assert 2 ** k == valid - 1 + m and m & (m - 1) == 0 and k >= 3
    wcol = flat_wcols(D)
    others = sorted(x for x in (set(edge_keys(valid)) | {valid - 2}) if 0 <= x < valid - 1)
    key = torch.full((D,), -1, dtype=torch.int64)
    key[wcol] = valid - 1
    if others:
        idx = (~wcol).nonzero()[:, 0]
        key[idx] = torch.tensor(others)[(torch.arange(len(idx)) + int(torch.randint(0, len(others), (1,), generator=gen))) % len(others)]
    r = torch.randint(1, 8, (D,), generator=gen).double() * (torch.randint(0, 2, (D,), generator=gen).double() * 2 - 1)
    v1 = torch.zeros(n_rows, D, dtype=torch.float64)
    has = key >= 0
    v1[key[has], has.nonzero()[:, 0]] = r[has] * 2.0 ** (k - 3)
    v1[valid:] = POISON
    out1 = torch.where(has, r * torch.where(wcol, float(m), 1.0) / 8, torch.zeros(()).double())
    return v1, out1, key


def flat_v2(n_rows: int, m: int, D: int, gen: torch.Generator) -> torch.Tensor:
    """fp64 [n_rows, D]: integers 1..15, times m on `flat_wcols`: added to +-r mult / 8 the sum keeps at most seven significant bits."""
    n = torch.randint(1, 16, (n_rows, D), generator=gen).double()
    return n * torch.where(flat_wcols(D), float(m), 1.0)


def _gather_rows(v: torch.Tensor, win: torch.Tensor, heads: int) -> torch.Tensor:
    """out[i, h*128:(h+1)*128] = v[win[i, h], h*128:(h+1)*128]."""
    out = torch.empty(win.shape[0], heads * 128, dtype=v.dtype)
    for h in range(heads):
        out[:, h * 128:(h + 1) * 128] = v[win[:, h], h * 128:(h + 1) * 128]
    return out


def _pack_k(ks, extra: int, heads: int, seg2: bool) -> torch.Tensor:
    tail = needle_k(extra, heads, sample=None, invalid=torch.ones(extra, dtype=torch.bool))
    k = torch.cat(list(ks) + [tail])
    return (seg2_keys(k, heads) if seg2 else k).to(BF)


def _pack_vt(vs, n: int, cols: int, extra_cols: int) -> torch.Tensor:
    """V^T [D, (samples - 1) cols + 64 ceil(n / 64) + extra_cols]: sample s at columns [s cols, s cols + n), POISON everywhere else."""
    vt = torch.full((vs[0].shape[1], (len(vs) - 1) * cols + pad64(n) + extra_cols), POISON, dtype=BF)
    for s, v in enumerate(vs):
        vt[:, s * cols:s * cols + n] = v.to(BF).t()
    return vt


class CrossCase:
    """The operands of one launch (CPU, bf16) and its expected output."""


def cross_case(n_q: int, len1: int, len2: int, heads: int, batch: int, seed: int, share_q: bool = False, share1: bool = False,
               share2: bool = False, valid=None, w=None, m=None, n_flat: int = 0, extra: int = 64, extra_cols: int = 0, extra_q: int = 0):
    """Needle (and flat) operands of one two-segment launch.  valid (per sample): segment 1 is cut there, rows valid[b] .. len1 - 1 win if read
    and their V is POISON; w (per sample): the log2-weight of key valid[b] - 1, or m (per sample, powers of two with valid - 1 + m = 2^k):
    w = log2 m, V1 / V2 the flat recipe's, and the last n_flat query rows of every sample flat.  Buffers: q [(1 | B) n_q + extra_q, D];
    k [(1 | B) len + extra, D] (the extra rows win if read); v^T at the column stride `vt_stride(len)`, POISON behind each sample's keys and in
    `extra_cols` more columns; want [B n_q, D] = bf16(bf16(V1[winner 1]) + bf16(V2[winner 2])), flat rows bf16(+-r mult / 8 + V2[winner 2])."""
    g = torch.Generator().manual_seed(seed)
    c = CrossCase()
    D = heads * 128
    c.n_q, c.len1, c.len2, c.H, c.B, c.n_flat = n_q, len1, len2, heads, batch, n_flat
    c.share_q, c.share1, c.share2 = share_q, share1, share2
    c.valid = [int(v) for v in valid] if valid is not None else None
    assert not (share1 and valid is not None) and (m is None or valid is not None) and (n_flat == 0 or m is not None)
    if m is not None:
        assert not share2 or len(set(m)) == 1  # (one V2 for all samples cannot follow a scale per sample)
        w = [math.log2(x) for x in m]
    c.w = [float(x) for x in w] if w is not None else None
    v1 = c.valid if c.valid is not None else [len1] * batch
    q1s, k1s, c.win1 = needle_segment(n_q, len1, v1, heads, batch, g, share_q, share1)
    q2s, k2s, c.win2 = needle_segment(n_q, len2, [len2] * batch, heads, batch, g, share_q, share2)
    qs = []
    for q1, q2 in zip(q1s, q2s):
        q = two_segment_q(q1, q2, heads).view(n_q, heads, 128)
        q[n_q - n_flat:, :, 0:2 * NEEDLE_DIGITS] = 0  # flat rows: nothing on segment 1's digit dims
        qs.append(q.view(n_q, D))
    q = torch.cat(qs)
    behind = q.roll(q.shape[0] // 2 + 1, 0)  # (other queries behind the last sample's: every row another one)
    c.q = torch.cat([q] + [behind] * ((extra_q + q.shape[0] - 1) // q.shape[0]))[:q.shape[0] + extra_q].to(BF)
    v1s, v2s, out1 = [], [], []
    for s in range(1 if share1 else batch):
        if m is None:
            v = needle_v(len1, D, g, positive=True).double()
            v[v1[s]:] = POISON
        else:
            v, o, _ = flat_v1(len1, v1[s], int(m[s]), D, g)
            out1.append(o)
        v1s.append(v)
    for s in range(1 if share2 else batch):
        v2s.append(needle_v(len2, D, g, positive=True).double() if m is None else flat_v2(len2, int(m[s]), D, g))
    c.c1, c.c2 = vt_stride(len1), vt_stride(len2)
    c.k1, c.k2 = _pack_k(k1s, extra, heads, False), _pack_k(k2s, extra, heads, True)
    c.v1t, c.v2t = _pack_vt(v1s, len1, c.c1, extra_cols), _pack_vt(v2s, len2, c.c2, extra_cols)
    want = torch.empty(batch, n_q, D, dtype=BF)
    c.flat_exact = True
    for b in range(batch):
        o1 = _gather_rows(v1s[0 if share1 else b], c.win1[b], heads)
        o2 = _gather_rows(v2s[0 if share2 else b], c.win2[b], heads)
        if n_flat:
            o1[n_q - n_flat:] = out1[b]
        want[b] = (o1.to(BF).float() + o2.to(BF).float()).to(BF)
        c.flat_exact = c.flat_exact and torch.equal(want[b, n_q - n_flat:].double(), (o1 + o2)[n_q - n_flat:])
    c.want = want.view(batch * n_q, D)
    return c


def cross_margins(c: CrossCase):
    """(lead, forbidden lead, flat forbidden lead), the minimum over both segments, all samples, needle rows and heads, in nats, the weight
    counted in; flat rows: every readable key of segment 1 scores exactly 0 (asserted) and the third figure is the worst forbidden key's lead
    over the weighted key.  Forbidden: every row of the buffer but the sample's own readable ones - except the readable rows of the samples
    that the neighbour bonus cannot tell from this one (under a shared query all others, else the samples b +- 3, b +- 6, ...): they carry
    the same labels, and there the row order and V, not the score, tell the samples apart."""
    lead_min, forb_min, flat_min = math.inf, math.inf, math.inf
    nn = c.n_q - c.n_flat
    for seg in (1, 2):
        k, ln, shared = (c.k1, c.len1, c.share1) if seg == 1 else (c.k2, c.len2, c.share2)
        win = c.win1 if seg == 1 else c.win2
        for b in range(c.B):
            base = 0 if shared else b * ln
            nv = c.valid[b] if (seg == 1 and c.valid is not None) else ln
            keep = torch.ones(k.shape[0], dtype=torch.bool)
            if not shared:
                for o in range(c.B):
                    if o != b and (c.share_q or (o - b) % 3 == 0):
                        keep[o * ln:o * ln + (c.valid[o] if (seg == 1 and c.valid is not None) else ln)] = False
            sel = keep.nonzero()[:, 0]
            pos = torch.full((k.shape[0],), -1, dtype=torch.int64)
            pos[sel] = torch.arange(len(sel))
            forb = torch.ones(k.shape[0], dtype=torch.bool)
            forb[base:base + nv] = False
            bias = torch.zeros(k.shape[0], dtype=torch.float64)
            if seg == 1 and c.w is not None:
                bias[base + nv - 1] = c.w[b] * math.log(2.0)
            qb = c.q[(0 if c.share_q else b) * c.n_q:][:c.n_q]
            if nn:
                lead, fl = needle_margins(qb[:nn], k[sel], c.H, pos[win[b][:nn] + base], forb[sel], bias[sel])
                lead_min, forb_min = min(lead_min, lead.min().item()), min(forb_min, fl.min().item())
            if c.n_flat:
                s = needle_scores(qb[nn:], k[sel], c.H)
                if seg == 1:
                    assert not s[:, :, ~forb[sel]].any(), "flat rows: a readable key of segment 1 does not score exactly 0"
                    if forb[sel].any():
                        flat_min = min(flat_min, (s[:, :, forb[sel]].amin() - bias.max()).item())
                else:
                    lead, fl = needle_margins(qb[nn:], k[sel], c.H, pos[win[b][nn:] + base], forb[sel])
                    lead_min, forb_min = min(lead_min, lead.min().item()), min(forb_min, fl.min().item())
    return lead_min, forb_min, flat_min


# ten (valid, m) pairs with valid <= 200, all different: the launches with more items than workgroups take one per sample
MANY_PAIRS = [(193, 64), (1, 64), (64, 1), (65, 64), (127, 2), (9, 8), (97, 32), (17, 16), (121, 8), (33, 32)]


def n_flat_rows(n_q: int) -> int:
    """Flat rows at the end of a sample: from the middle of the partial last query block on (it then holds needle rows and flat rows)."""
    return n_q - (n_q // 256 * 256 + (n_q % 256) // 2)


def roomy_cross_case(n_q: int, len1: int, len2: int, heads: int, batch: int, seed: int, **kw):
    """`cross_case` in roomy buffers - what the GPU tests launch: a wrong sample stride (a stride where an operand is shared, 64 ceil(len / 64)
    for a V^T column stride) still lands in rows and columns the test owns (winner-if-read keys, POISON, other queries) and gives a wrong
    answer, not a stray read."""
    shared_k = kw.get("share1") or kw.get("share2")
    return cross_case(n_q, len1, len2, heads, batch, seed, extra=64 + ((batch - 1) * max(len1, len2) if shared_k else 0),
                      extra_cols=(batch - 1) * pad64(max(len1, len2)), extra_q=(batch - 1) * n_q if kw.get("share_q") else 0, **kw)


def far_first_tile(n_q: int, n_k: int, heads: int, gen: torch.Generator):
    """(q, k, v, rows): needle operands (bf16) of ONE sample whose first 64-key tile lies far below every row's winner: rows 0..63 carry the
    labels 4032 + i (digits (i % 8, i // 8, 7, 7, 0)), rows 64.. the labels 0, 1, ..., and the winners are labels whose two digits are <= 5 -
    every tile-0 key trails the winner by >= 48 digit units, thousands of octaves, so the first tile's row maximum is far below -128 in the
    log2 domain and exp2(-maximum) overflows.  An online softmax that rescales by that factor at the first tile (where there is nothing to
    rescale) turns 0 * inf into a NaN row.  rows: int64 [n_q, heads], the winning key row."""
    assert n_k >= 64 + 46
    labels = torch.cat([4032 + torch.arange(64), torch.arange(n_k - 64)])
    ok = torch.tensor([l for l in range(min(n_k - 64, 64)) if l % 8 <= 5 and l // 8 <= 5])
    lab = ok[torch.randint(0, len(ok), (n_q, heads), generator=gen)]
    q = needle_q(lab).to(BF)
    k = needle_k(n_k, heads, labels=labels).to(BF)
    return q, k, needle_v(n_k, heads * 128, gen), lab + 64


CROSS_MISTAKES = ("weight ignored", "weight on key valid-2", "valid[0] for all samples", "w[0] for all samples", "tail mask at valid+1",
                  "tail mask at len1", "neighbour's K1 rows", "shared operand at stride len", "V^T column stride 64 ceil(len/64)")


def cross_attention_f64(c: CrossCase, mistake=None) -> torch.Tensor:
    """The two-segment attention of the entry points' contract on the PACKED buffers of `c`, plain fp64 (softmax in the log2 domain: an integer
    weight is an exact factor), with the kernel's three roundings at the end: bf16(bf16(o1) + bf16(o2)).  `mistake` (one of CROSS_MISTAKES):
    the same with one deliberately wrong index."""
    assert mistake is None or mistake in CROSS_MISTAKES
    H, B, nq, D = c.H, c.B, c.n_q, c.H * 128
    valid = list(c.valid) if c.valid is not None else [c.len1] * B
    w = list(c.w) if c.w is not None else [0.0] * B
    q_rows, k1_rows, k2_rows = (0 if c.share_q else nq), (0 if c.share1 else c.len1), (0 if c.share2 else c.len2)
    c1, c2 = (0 if c.share1 else c.c1), (0 if c.share2 else c.c2)
    wpos = [v - 1 for v in valid]
    k1_of = list(range(B))
    if mistake == "weight ignored":
        w = [0.0] * B
    elif mistake == "weight on key valid-2":
        wpos = [v - 2 for v in valid]
    elif mistake == "valid[0] for all samples":
        valid = [valid[0]] * B
        wpos = [v - 1 for v in valid]
    elif mistake == "w[0] for all samples":
        w = [w[0]] * B
    elif mistake == "tail mask at valid+1":
        valid = [v + 1 for v in valid]
    elif mistake == "tail mask at len1":
        valid = [c.len1] * B
    elif mistake == "neighbour's K1 rows":
        k1_of = [(b + 1) % B for b in range(B)]
    elif mistake == "shared operand at stride len":
        q_rows, k1_rows, k2_rows, c1, c2 = nq, c.len1, c.len2, c.c1, c.c2
    elif mistake == "V^T column stride 64 ceil(len/64)":
        c1, c2 = (0 if c.share1 else pad64(c.len1)), (0 if c.share2 else pad64(c.len2))

    def seg(qh, k, vt, n, wp, wt):
        kh = k.double().view(n, H, 128).transpose(0, 1)
        s = qh @ kh.transpose(1, 2) * (LOG2E / math.sqrt(128.0))
        if wt != 0.0 and 0 <= wp < n:
            s[:, :, wp] += wt
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        p = p / p.sum(-1, keepdim=True)
        o = p @ vt.double().view(H, 128, n).transpose(1, 2)
        return o.transpose(0, 1).reshape(-1, D)

    out = torch.empty(B * nq, D, dtype=BF)
    for b in range(B):
        qh = c.q[b * q_rows:b * q_rows + nq].double().view(nq, H, 128).transpose(0, 1)
        n1 = valid[b]
        o1 = seg(qh, c.k1[k1_of[b] * k1_rows:][:n1], c.v1t[:, b * c1:b * c1 + n1], n1, wpos[b], w[b])
        o2 = seg(qh, c.k2[b * k2_rows:][:c.len2], c.v2t[:, b * c2:b * c2 + c.len2], c.len2, -1, 0.0)
        out[b * nq:(b + 1) * nq] = (o1.float().to(BF).float() + o2.float().to(BF).float()).to(BF)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# self-attention sums (ce_attention_bf16 / _batched / _vt / _vt_blocked / _1head): tie rows and stair rows in one launch with needle rows
#
# A needle row pins addressing; it says nothing about the row sum l, the accumulation of P.V over keys and tiles, or a rescale by a factor
# that is neither 1 nor 0.  Two more row kinds do, interleaved with the needle rows inside every 32-row wave group (`sum_row_kinds`; rows
# 64..127 hold no needle row, so some waves never leave the speculative route on a needle's account).  Their queries are zero on the digit
# dims and keep the neighbour bonus and NEEDLE_BIG on the invalid dim.
# Tie rows: the keys of a tie set carry 0 on the set's dim (SUM_TIE_DIM + 0..3: sets of 2, 4, 8 and 32 or 64 keys), every other key 1, the
# query -SUM_TIE_T: the set scores exactly 0 under any scale, every loser trails by >= TIE_GAP nats (its exp2 is 0 in fp32), V on the set is
# small integers times one power of two with one sign per column, and the row is the set's mean - exactly.  The large set holds key 0, the
# last valid key and a key in every key tile (64 keys; 32 for attention_1head: both sides of every key-split boundary).
# Stair rows: the stair keys carry their level j on SUM_STEP_DIM and SUM_STEP_DIM + 1 (every other key SUM_OFF_LEVEL), the query -u: a key
# at level j lies j octaves below the top.  Family "r" - the kernels that round Q * scale * log2(e) to bf16 before the first product
# (attn_fwd_sp_kernel, attn_fwd_w4_kernel, ce_attn16.hip: `ops.attention` under waves 0 / 64, every attention_vt / attention_vt_blocked
# selector): one component, 7.84375, whose rounded product is exactly 1.0 - integer scores, every P a power of two.  Family "f" - the
# kernels that scale the fp32 score (the register-staged attn_fwd_kernel: `ops.attention` under waves 8 / 4, two-segment form included;
# attn_1head_kernel): a coarse and a fine component whose sum times scale * log2(e) is within 2^-16 of 1.  sum 2^-j over the stair is a
# power of two; V is sparse as in `flat_v1` - column c is nonzero at ONE stair key, +-r 2^level l / 8 - and the row is +-r / 8: every
# column shows one key's weight, a wrong l or rescale shows in all of them.  Layouts of the levels over the 64-key tiles (`_stair_plan`):
# falling (the offset never moves), rising by one octave per tile over five tiles (P runs above 1 in the speculative bodies, nothing
# re-bases), jump (two keys ten octaves down, then 31 top keys in one tile: a lane's partial row sum passes 2^10 and the lazy bodies' +8).
# Silent keys: in the `silent` cases the rows behind a sample's last valid key (past L, the blocked layout's padding tokens, past Nk) are
# all-zero K rows over zero V: read by mistake they join every tie set and the stair's top, and change l and nothing else.  In the other
# cases those rows win outright over POISON.
# ------------------------------------------------------------------------------------------------------------------------------------
SUM_TIE_DIM = 30        # dims 30..33: the tie sets of 2, 4, 8 and 32 / 64 keys
SUM_TIE_T = 4096.0      # a tie row's losers trail by T * scale: 362 nats at head_dim 128, 209 at 384
SUM_STEP_DIM = 40       # dims 40, 41: the level of a stair key
SUM_OFF_LEVEL = 512.0   # ... and what every other key carries there: 512 octaves down
SUM_STEP = {("r", 128): (7.84375, 0.0), ("f", 128): (7.84375, -0.00168609619140625), ("f", 384): (13.5625, 0.0203857421875)}
SUM_PATTERN = (0, 5, 1, 5, 0, 2, 5, 0, 5, 3, 0, 5, 4, 0, 5, 5)  # 0 needle, 1..4 tie row of set 0..3, 5 stair
# which family a selector of ce_set_attention_waves runs (the header comment above)
SUM_FAMILY = {("attention", 0): "r", ("attention", 64): "r", ("attention", 8): "f", ("attention", 4): "f", ("attention_vt", 0): "r",
              ("attention_vt", 128): "r", ("attention_vt", 129): "r", ("attention_vt", 16): "r", ("attention_vt_blocked", 0): "r",
              ("attention_vt_blocked", 128): "r", ("attention_vt_blocked", 129): "r", ("attention_1head", 0): "f"}


def sum_scale_log2e(C: int) -> float:
    """The launchers' fp32 constant softmax_scale * 1.4426950408889634f at scale C^-1/2."""
    return float(torch.tensor(C ** -0.5, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def sum_row_kinds(n_q: int, pure: bool = False) -> torch.Tensor:
    """int64 [n_q]: SUM_PATTERN repeated; rows 64..127 (all rows when `pure`) take a stair row in place of every needle row."""
    i = torch.arange(n_q)
    kind = torch.tensor(SUM_PATTERN)[i % len(SUM_PATTERN)]
    no_needle = torch.ones(n_q, dtype=torch.bool) if pure else (i >= 64) & (i < 128)
    return torch.where(no_needle & (kind == 0), torch.tensor(5), kind)


def _stair_plan(layout: str, nt: int):
    """([(64-key tile, level, keys)], sum of 2^-level over them) of a stair over nt key tiles."""
    if layout == "falling":
        top = 4 if nt >= 4 else 2
        return [(0, 0, top)] + [(l * (nt - 1) // top, l, 2 ** l) for l in range(1, top + 1)], 2 * top
    if layout == "rising":
        assert nt >= 5
        return [(4 - l, l, 2 ** l if l else 4) for l in range(4, -1, -1)], 8
    assert layout == "jump" and nt >= 3, (layout, nt)
    J = max(2, 2 * nt // 3)
    return [(0, 10, 1), (1, 10, 1), (J, 0, 31)] + [(min(J + 1 + (l - 1) // 3, nt - 1), l, 1) for l in range(1, 10)], 32


class SumsCase:
    """The packed operands of one launch (CPU, bf16), its row kinds, tie sets and stairs, and its expected output."""


def sums_case(n_q: int, n_k: int, heads: int, batch: int, seed: int, layout=("falling",), silent: bool = False, C: int = 128, stride=None,
              extra: int = 64, tile: int = 64, nsplit: int = 1, families=("r", "f"), pure: bool = False) -> SumsCase:
    """Needle, tie and stair rows of `batch` stacked samples.  Packed buffers: q[family] [batch n_q, D]; k, v [batch stride + extra, D] with
    sample b's n_k valid keys from row b stride on (stride > n_k: the blocked layout's padding tokens, un-blocked) - the rows behind them
    and the `extra` rows at the end are silent (zero K, zero V) or win if read (V = POISON); want [batch n_q, D].  layout: one per head,
    cycling.  tile: the kernel's key tile (where the large tie set needs members), nsplit: the key split the launcher is expected to choose."""
    assert (C == 128 or heads == 1) and all((f, C) in SUM_STEP for f in families)
    gs, gt, gw, gv = (torch.Generator().manual_seed(seed * 4 + i) for i in range(4))  # tie sets, stairs, winners, V: one stream each
    c = SumsCase()
    H, B, D = heads, batch, heads * C
    stride = n_k if stride is None else stride
    nt, ntl = (n_k + 63) // 64, (n_k + tile - 1) // tile
    big = 32 if ntl <= 32 else 64
    assert ntl <= big and stride >= n_k
    c.n_q, c.n_k, c.H, c.B, c.C, c.stride, c.extra, c.silent, c.tile, c.nsplit = n_q, n_k, H, B, C, stride, extra, silent, tile, nsplit
    c.families, c.sizes, c.kind = tuple(families), (2, 4, 8, big), sum_row_kinds(n_q, pure)
    c.layouts = [layout[h % len(layout)] for h in range(H)]
    rows = B * stride + extra
    k = torch.zeros(rows, H, C, dtype=torch.float64)
    v = torch.zeros(rows, H, C, dtype=torch.float64)
    q = {f: torch.zeros(B * n_q, H, C, dtype=torch.float64) for f in families}
    want = torch.zeros(B * n_q, H, C, dtype=torch.float64)
    c.sets, c.stair, c.win = [], [], torch.zeros(B, n_q, H, dtype=torch.int64)
    needle, stair_rows = c.kind == 0, c.kind == 5
    for b in range(B):
        nb = stride + (extra if b == B - 1 else 0)
        base = b * stride
        behind = torch.arange(nb) >= n_k
        k[base:base + nb, :, :128] = needle_k(nb, H, sample=b, invalid=None if silent else behind).view(nb, H, 128)
        c.sets.append([])
        c.stair.append([])
        for h in range(H):
            kh, vh = k[base:base + nb, h], v[base:base + nb, h]
            # ---- tie sets: the large one first (key 0, the last valid key, one key per key tile), then random free keys
            large = [0, n_k - 1]
            for t in range(ntl):
                lo, hi = t * tile, min((t + 1) * tile, n_k)
                if not any(lo <= x < hi for x in large):
                    large.append(lo + int(torch.randint(0, hi - lo, (1,), generator=gs)))
            free = [x for x in torch.randperm(n_k, generator=gs).tolist() if x not in set(large)]
            large += free[:big - len(large)]
            free = [x for x in free if x not in set(large)]
            sets = []
            for s in (2, 4, 8):
                sets.append(torch.tensor(sorted(free[:s])))
                free = free[s:]
            sets.append(torch.tensor(sorted(large)))
            c.sets[b].append(sets)
            # ---- the stair: `count` free keys of each planned tile at the planned level
            plan, units = _stair_plan(c.layouts[h], nt)
            skeys, slev = [], []
            for (t, lev, count) in plan:
                cand = [x for x in free if 64 * t <= x < 64 * (t + 1)]
                assert len(cand) >= count, "stair recipe: a key tile has too few free keys"
                pick = [cand[i] for i in torch.randperm(len(cand), generator=gt)[:count].tolist()]
                free = [x for x in free if x not in set(pick)]
                skeys += pick
                slev += [lev] * count
            skeys, slev = torch.tensor(skeys), torch.tensor(slev, dtype=torch.float64)
            assert float(torch.exp2(-slev).sum()) == units
            c.stair[b].append((skeys, slev, units))
            # ---- K: tie dims, step dims; V: ordinary rows, the sets' integers, the stair's one entry per column
            kh[:, SUM_TIE_DIM:SUM_TIE_DIM + 4] = 1.0
            for s, members in enumerate(sets):
                kh[members, SUM_TIE_DIM + s] = 0.0
            kh[:, SUM_STEP_DIM:SUM_STEP_DIM + 2] = SUM_OFF_LEVEL
            kh[skeys, SUM_STEP_DIM] = slev
            kh[skeys, SUM_STEP_DIM + 1] = slev
            vh[:] = needle_v(nb, C, gv).double()
            means = []
            for s, members in enumerate(sets):
                ints = torch.randint(1, (3 if len(members) == 64 else 7) + 1, (len(members), C), generator=gv).double()
                sign = torch.randint(0, 2, (C,), generator=gv).double() * 2 - 1
                vh[members] = ints * sign * 2.0 ** int(torch.randint(-2, 3, (1,), generator=gv))
                means.append(vh[members].mean(0))
            col = torch.arange(C)
            at = (col + int(torch.randint(0, len(skeys), (1,), generator=gv))) % len(skeys)  # column c's stair key: all of them, cycling
            r = torch.randint(1, 8, (C,), generator=gv).double() * (torch.randint(0, 2, (C,), generator=gv).double() * 2 - 1)
            vh[skeys] = 0.0
            vh[skeys[at], col] = r * torch.exp2(slev[at]) * units / 8
            if silent:
                kh[behind] = 0.0
            vh[behind] = 0.0 if silent else float(torch.tensor(POISON).to(BF))  # (as the buffers of the needle tests hold it)
            # ---- winners of the needle rows: any key outside the stair (its V rows hold zeros)
            avail = torch.tensor(sorted(set(range(n_k)) - set(skeys.tolist())))
            c.win[b, :, h] = avail[winners_for(n_q, len(avail), 1, gw, must=(0, len(avail) - 1))[:, 0]]
            wr = want[b * n_q:(b + 1) * n_q, h]
            wr[needle] = vh[c.win[b, needle, h]]
            for s in range(4):
                wr[c.kind == 1 + s] = means[s]
            wr[stair_rows] = r / 8
        qn = needle_q(c.win[b], sample=b, batch=B).view(n_q, H, 128)
        qn[~needle, :, 0:2 * NEEDLE_DIGITS] = 0.0
        for s in range(4):
            qn[c.kind == 1 + s, :, SUM_TIE_DIM + s] = -SUM_TIE_T
        for f in families:
            qf = qn.clone()
            qf[stair_rows, :, SUM_STEP_DIM] = -SUM_STEP[(f, C)][0]
            qf[stair_rows, :, SUM_STEP_DIM + 1] = -SUM_STEP[(f, C)][1]
            q[f][b * n_q:(b + 1) * n_q, :, :128] = qf
    for t in [k, v, want] + list(q.values()):
        assert torch.equal(t.to(BF).double(), t), "sums recipe: a value is not exact in bf16"
    c.q = {f: t.view(B * n_q, D).to(BF) for f, t in q.items()}
    c.k, c.v, c.want = k.view(rows, D).to(BF), v.view(rows, D).to(BF), want.view(B * n_q, D).to(BF)
    return c


SUM_MISTAKES = ("a tied key dropped", "the last valid key dropped", "one silent key counted", "a tile's keys counted twice",
                "rescale applied to O but not to l", "rescale applied one tile late", "split merge without the non-maximal splits' l",
                "split merge with the splits' weights exchanged")


def _sum_scores(c: SumsCase, family: str, b: int, h: int, n: int, f32: bool = False) -> torch.Tensor:
    """Scores [n_q, n] in the exp2 domain of sample b, head h against the first n packed key rows of the sample, with the family's
    rounding of the operands: "r" rounds fl32(q * scale * log2 e) to bf16 first, "f" scales the score.  fp64, or the kernels' fp32."""
    sl2 = sum_scale_log2e(c.C)
    qh = c.q[family][b * c.n_q:(b + 1) * c.n_q, h * c.C:(h + 1) * c.C]
    kh = c.k[b * c.stride:b * c.stride + n, h * c.C:(h + 1) * c.C]
    dt = torch.float32 if f32 else torch.float64
    if family == "r":
        return (qh.float() * sl2).to(BF).to(dt) @ kh.to(dt).t()
    return (qh.to(dt) @ kh.to(dt).t()) * torch.tensor(sl2, dtype=dt)


def attention_sums_f64(c: SumsCase, mistake=None, family=None) -> torch.Tensor:
    """softmax(q k^T scale) v per sample and head on the PACKED buffers of `c`, plain fp64 (the exp2 domain, the family's operand rounding),
    rounded to bf16 at the end (through fp32; no expected value lies near a rounding boundary of either).  `mistake` (one of SUM_MISTAKES): the same with one deliberate error; the two rescale mistakes walk the 64-key
    tiles with a running maximum, the two merge mistakes the `c.nsplit` key splits of 32-key tiles (no change where nsplit == 1)."""
    assert mistake is None or mistake in SUM_MISTAKES
    family = family or c.families[0]
    out = torch.empty(c.B * c.n_q, c.H * c.C, dtype=BF)
    for b in range(c.B):
        for h in range(c.H):
            n = c.n_k + (1 if mistake == "one silent key counted" else 0)
            s = _sum_scores(c, family, b, h, n)
            vh = c.v[b * c.stride:b * c.stride + n, h * c.C:(h + 1) * c.C].double()
            wgt = torch.ones(n, dtype=torch.float64)
            if mistake == "a tied key dropped":
                for members in c.sets[b][h]:
                    wgt[members[1]] = 0.0
            elif mistake == "the last valid key dropped":
                wgt[c.n_k - 1] = 0.0
            elif mistake == "a tile's keys counted twice":
                t = 1 if c.n_k > 64 else 0
                wgt[64 * t:64 * (t + 1)] = 2.0
            if mistake in ("rescale applied to O but not to l", "rescale applied one tile late"):
                m = s[:, :64].amax(1)
                l = torch.zeros_like(m)
                o = torch.zeros(c.n_q, c.C, dtype=torch.float64)
                a_prev = torch.ones_like(m)
                for t0 in range(0, n, 64):
                    st = s[:, t0:t0 + 64]
                    m_new = torch.maximum(m, st.amax(1))
                    alpha = torch.exp2(m - m_new)
                    m = m_new
                    p = torch.exp2(st - m[:, None])
                    a = a_prev if mistake == "rescale applied one tile late" else alpha
                    a_prev = alpha
                    o = o * a[:, None] + p @ vh[t0:t0 + 64]
                    l = (l if mistake == "rescale applied to O but not to l" else l * a) + p.sum(1)
                res = o / l[:, None]
            elif mistake in ("split merge without the non-maximal splits' l", "split merge with the splits' weights exchanged") and c.nsplit > 1:
                per = ((n + 31) // 32 + c.nsplit - 1) // c.nsplit * 32
                ms, ls, os_ = [], [], []
                for t0 in range(0, n, per):
                    st = s[:, t0:t0 + per]
                    ms.append(st.amax(1))
                    p = torch.exp2(st - ms[-1][:, None])
                    ls.append(p.sum(1))
                    os_.append(p @ vh[t0:t0 + per])
                ms, ls, os_ = torch.stack(ms), torch.stack(ls), torch.stack(os_)
                w = torch.exp2(ms - ms.amax(0))
                if mistake == "split merge with the splits' weights exchanged":
                    w = w.flip(0)
                    lw = ls * w
                else:  # only the first split that holds the maximum brings its l
                    first = torch.zeros_like(w).scatter_(0, ms.argmax(0, keepdim=True), 1.0)
                    lw = ls * w * first
                res = (os_ * w[:, :, None]).sum(0) / lw.sum(0)[:, None]
            else:
                p = torch.exp2(s - s[:, wgt > 0].amax(1, keepdim=True)) * wgt
                res = (p @ vh) / p.sum(1, keepdim=True)
            out[b * c.n_q:(b + 1) * c.n_q, h * c.C:(h + 1) * c.C] = res.float().to(BF)
    return out


def online_softmax_f32(c: SumsCase, family: str, schedule: str) -> torch.Tensor:
    """An fp32 model of the kernels' online softmax over 64-key tiles: the offset of a row is tile 0's maximum and moves to a later tile's
    maximum whenever that is larger (schedule "max") or only when it is more than 8 octaves larger ("lazy": P runs up to 2^8); P = exp2(score -
    offset) in fp32, summed un-rounded into l, rounded to bf16 for P.V; O and l rescaled by exp2(old - new offset); O * (1 / l) rounded to bf16."""
    assert schedule in ("max", "lazy")
    out = torch.empty(c.B * c.n_q, c.H * c.C, dtype=BF)
    for b in range(c.B):
        for h in range(c.H):
            s = _sum_scores(c, family, b, h, c.n_k, f32=True)
            vh = c.v[b * c.stride:b * c.stride + c.n_k, h * c.C:(h + 1) * c.C].float()
            m = s[:, :64].amax(1)
            l = torch.zeros_like(m)
            o = torch.zeros(c.n_q, c.C)
            for t0 in range(0, c.n_k, 64):
                st = s[:, t0:t0 + 64]
                mt = st.amax(1)
                m_new = torch.where(mt > (m if schedule == "max" else m + 8.0), mt, m)
                alpha = torch.exp2(m - m_new)
                m = m_new
                p = torch.exp2(st - m[:, None])
                l = l * alpha + p.sum(1)
                o = o * alpha[:, None] + p.to(BF).float() @ vh[t0:t0 + 64]
            out[b * c.n_q:(b + 1) * c.n_q, h * c.C:(h + 1) * c.C] = (o * (1.0 / l)[:, None]).to(BF)
    return out


def sum_margins(c: SumsCase, family: str):
    """(needle lead, needle forbidden lead, tie gap) in nats, the minimum over samples, heads and rows; asserts that every member of a tie
    row's set scores exactly 0.  Forbidden: every packed row but the sample's own valid keys - in a silent case only the other samples' keys
    (a silent row carries no flag: it is told by the sums, not by a needle)."""
    lead_min, forb_min, gap_min = math.inf, math.inf, math.inf
    rows = c.k.shape[0]
    ln2 = math.log(2.0)
    for b in range(c.B):
        forb = torch.ones(rows, dtype=torch.bool)
        forb[b * c.stride:b * c.stride + c.n_k] = False
        flagged = forb & (c.k.double().view(rows, c.H, c.C)[:, 0, :128].abs().sum(1) > 0)  # (silent rows are all-zero)
        for h in range(c.H):
            qh = c.q[family][b * c.n_q:(b + 1) * c.n_q, h * c.C:(h + 1) * c.C].double()
            s = (qh @ c.k[:, h * c.C:(h + 1) * c.C].double().t()) * c.C ** -0.5   # nats, every packed row
            nd = c.kind == 0
            sw = s[nd].gather(1, (c.win[b, nd, h] + b * c.stride)[:, None])
            own = s[nd].masked_fill(forb[None, :], -math.inf).scatter(1, (c.win[b, nd, h] + b * c.stride)[:, None], -math.inf)
            if nd.any():
                lead_min = min(lead_min, float((sw - own.amax(1, keepdim=True)).min()))
            if nd.any() and flagged.any():
                forb_min = min(forb_min, float((s[nd][:, flagged].amin(1, keepdim=True) - sw).min()))
            valid = s[:, b * c.stride:b * c.stride + c.n_k]
            for i, members in enumerate(c.sets[b][h]):
                tr = valid[c.kind == 1 + i]
                assert not tr[:, members].any(), "tie rows: a member of the set does not score exactly 0"
                lose = torch.ones(c.n_k, dtype=torch.bool)
                lose[members] = False
                gap_min = min(gap_min, float(-tr[:, lose].amax()))
                if flagged.any():
                    forb_min = min(forb_min, float(s[c.kind == 1 + i][:, flagged].amin()))
            if flagged.any():
                forb_min = min(forb_min, float(s[c.kind == 5][:, flagged].amin()))
    return lead_min, forb_min, gap_min


def sum_split_count(n_q: int, n_k: int, C: int, cus: int, ws_floats: int) -> int:
    """ce_attention_1head_bf16's key-split rule, restated: as many splits (<= 4, >= 16 32-key tiles each) as fill the chip."""
    blocks, ntiles = (n_q + 127) // 128, (n_k + 31) // 32
    if blocks * 4 < cus * 3:
        for sp in (4, 3, 2):
            if blocks * sp <= cus + cus // 8 and ntiles >= 16 * sp and sp * n_q * (C + 2) <= ws_floats:
                return sp
    return 1


# every launch of tests/test_exact_attention_sums_gpu.py.  Row-major and V^T forms share the first group (696 = 8 x 87: the 16 x 16 x 32
# body's column stride); 700 keys for the row-major forms alone; stride > n_k: the blocked layout (N valid of W x n tokens, queries on all).
SUM_CASES = {
    "mid-a": dict(n_q=300, n_k=696, heads=2, batch=2, layout=("falling", "rising"), silent=True),
    "mid-b": dict(n_q=300, n_k=696, heads=2, batch=2, layout=("jump", "falling"), silent=False),
    "rows-700": dict(n_q=300, n_k=700, heads=2, batch=2, layout=("rising", "jump"), silent=True),
    "one-tile": dict(n_q=70, n_k=64, heads=2, batch=3, layout=("falling",), silent=True),
    "long": dict(n_q=100, n_k=2104, heads=2, batch=1, layout=("jump", "rising"), silent=False),
    "blk-300": dict(n_q=384, n_k=300, heads=2, batch=2, layout=("jump", "rising"), silent=True, stride=384, extra=0),
    "blk-500": dict(n_q=512, n_k=500, heads=2, batch=2, layout=("falling", "jump"), silent=False, stride=512, extra=0),
    "vae-1000-128": dict(n_q=1000, n_k=1000, heads=1, batch=1, layout=("jump",), silent=True, C=128, tile=32, nsplit=2, families=("f",)),
    "vae-1000-384": dict(n_q=1000, n_k=1000, heads=1, batch=1, layout=("rising",), silent=False, C=384, tile=32, nsplit=2, families=("f",)),
    "vae-2040-128": dict(n_q=2040, n_k=2040, heads=1, batch=1, layout=("falling",), silent=False, C=128, tile=32, nsplit=4, families=("f",)),
    "vae-2040-384": dict(n_q=2040, n_k=2040, heads=1, batch=1, layout=("jump",), silent=True, C=384, tile=32, nsplit=4, families=("f",)),
    # the route counters: no needle rows, one layout for every head, the same tie sets in both (one seed: the sets have a stream of their own)
    "route-rising": dict(n_q=300, n_k=696, heads=2, batch=2, layout=("rising",), silent=True, pure=True, families=("r",), seed=77),
    "route-jump": dict(n_q=300, n_k=696, heads=2, batch=2, layout=("jump",), silent=True, pure=True, families=("r",), seed=77),
}
_sum_cases = {}


def sum_named_case(name: str) -> SumsCase:
    """The case of that name, built once and shared (nobody writes to it)."""
    if name not in _sum_cases:
        _sum_cases[name] = sums_case(**dict({"seed": sorted(SUM_CASES).index(name) + 1}, **SUM_CASES[name]))
    return _sum_cases[name]


# ------------------------------------------------------------------------------------------------------------------------------------
# row kernels (LayerNorm / RMSNorm / RoPE), the scheduler step and the softmaxes: exactly computable data and their fp64 answers
#
# `unit_rows`: rows whose sum is 0 and whose sum of squares is exactly D, scaled by a power of two and shifted by a multiple of 1/4.  With
# eps = 0 the fp32 statistics of a norm kernel are exact in any summation order (mean = mu, var = s^2, rstd = 1 / s) and the normalised values
# are the integers 0, +-1, +-2 again; what follows (an affine, a weight, a rotation by a DYADIC table) is exact in fp32 and the one rounding
# to bf16 is the only one.  Every vector the kernels index (a, b, w, cos/sin, bias) differs in every column and row: a wrong index shows.
# ------------------------------------------------------------------------------------------------------------------------------------
def dyadic(shape, gen: torch.Generator, lo: int, hi: int, e: int) -> torch.Tensor:
    """fp32 tensor of integers in [lo, hi] times 2^e."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, dtype=torch.int32).float() * 2.0 ** e


def unit_rows(M: int, D: int, gen: torch.Generator, centred: bool = False):
    """(x, v): x bf16 [M, D] = mu + s * v, v fp64 [M, D] with n2 entries of +-2 (balanced), 3 * n2 zeros and +-1 (balanced) elsewhere, permuted,
    n2 random per row; s = 2^e per row, e in [-2, 2]; mu a per-row multiple of 1/4 in [-8, 8] (0 when `centred`: the RMS kernels).
    sum(v) = 0 and sum(v^2) = D exactly; x is exact in bf16 (a multiple of 1/4 below 32)."""
    assert D % 8 == 0
    v = torch.empty(M, D, dtype=torch.float64)
    for m in range(M):
        n2 = 2 * int(torch.randint(0, D // 16 + 1, (1,), generator=gen))
        ones = D - 4 * n2
        row = torch.cat([torch.full((n2 // 2,), 2.0), torch.full((n2 // 2,), -2.0), torch.zeros(3 * n2), torch.ones(ones // 2),
                         -torch.ones(ones // 2)]).double()
        v[m] = row[torch.randperm(D, generator=gen)]
    assert torch.equal(v.sum(1), torch.zeros(M, dtype=torch.float64)) and torch.equal((v * v).sum(1), torch.full((M,), float(D), dtype=torch.float64))
    s = torch.exp2(torch.randint(-2, 3, (M, 1), generator=gen).double())
    mu = torch.zeros(M, 1, dtype=torch.float64) if centred else torch.randint(-32, 33, (M, 1), generator=gen).double() / 4
    x64 = mu + s * v
    x = x64.to(BF)
    assert torch.equal(x.double(), x64)
    return x, v


def affine_vectors(rows: int, D: int, gen: torch.Generator):
    """(a, b) fp32 [rows, D]: a in units of 2^-8 up to 4 (fine enough that v * a + b needs a real bf16 rounding), b in units of 2^-10 up to 1/4."""
    return dyadic((rows, D), gen, -1024, 1024, -8), dyadic((rows, D), gen, -256, 256, -10)


def sample_of(M: int, ab_rows: int) -> torch.Tensor:
    """The (a, b) row that row m of a stacked batch uses."""
    return torch.arange(M) // ab_rows if ab_rows > 0 else torch.zeros(M, dtype=torch.int64)


def ln_affine_exact(v: torch.Tensor, a: torch.Tensor, b: torch.Tensor, ab_rows: int = 0, sample=None) -> torch.Tensor:
    """fp64 v * a[sample(m)] + b[sample(m)] for `unit_rows` data at eps = 0 (a, b [rows, D]); `sample` overrides the row -> sample map."""
    idx = sample_of(v.shape[0], ab_rows) if sample is None else sample
    return v * a.double()[idx] + b.double()[idx]


def ln_affine_f64(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, eps: float, ab_rows: int = 0) -> torch.Tensor:
    """The LayerNorm-affine formula in fp64 on any data (biased variance), before the one rounding to bf16."""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    idx = sample_of(x.shape[0], ab_rows)
    return (xd - mean) / torch.sqrt(var + eps) * a.double()[idx] + b.double()[idx]


def round_bf16_f64(x64: torch.Tensor) -> torch.Tensor:
    """An exact-in-fp32 fp64 value rounded to bf16, back in fp64 (an intermediate rounding point of a kernel)."""
    return bf16_rne(x64).double()


def rope_table(R: int, head_dim: int, gen: torch.Generator) -> torch.Tensor:
    """fp32 [R, head_dim / 2, 2]: (cos, sin) entries that are no rotation - random multiples of 1/8 in [-1, 1], different for every (row, pair) -
    with true quarter turns ((0, 1), (-1, 0), (0, -1), (1, 0)) on every fifth pair."""
    cs = dyadic((R, head_dim // 2, 2), gen, -8, 8, -3)
    turns = torch.tensor([[0.0, 1.0], [-1.0, 0.0], [0.0, -1.0], [1.0, 0.0]])
    n = cs[:, ::5].shape[1]
    cs[:, ::5] = turns[torch.randint(0, 4, (R, n), generator=gen)]
    return cs


def rms_rope_exact(v: torch.Tensor, w: torch.Tensor, cs=None, head_dim: int = 0, table_row=None, pair_shift: int = 0) -> torch.Tensor:
    """bf16 result of RMSNorm * w (+ RoPE) for centred `unit_rows` data at eps = 0: bf16(bf16(v) * w), then the rotation of every (even, odd)
    pair by (cos, sin) = cs[m % R][pair within the head], rounded once.  `table_row` (int64 [M]) overrides m % R and `pair_shift` moves every
    pair's table entry to a neighbour's: the deliberately wrong references of the sensitivity checks."""
    M, D = v.shape
    t = round_bf16_f64(round_bf16_f64(v) * w.double())
    if cs is None:
        return t.to(BF)
    R, half = cs.shape[0], head_dim // 2
    rows = torch.arange(M) % R if table_row is None else table_row
    pair = (torch.arange(D // 2) % half + pair_shift) % half
    c = cs.double()[rows][:, pair]  # [M, D/2, 2]
    v0, v1 = t[:, 0::2], t[:, 1::2]
    out = torch.empty_like(t)
    out[:, 0::2] = v0 * c[..., 0] - v1 * c[..., 1]
    out[:, 1::2] = v0 * c[..., 1] + v1 * c[..., 0]
    return bf16_rne(out)


def rms_weights(D: int, gen: torch.Generator) -> torch.Tensor:
    """fp32 [D] RMSNorm weights in units of 2^-8 up to 4, never 0: the product with 0, +-1, +-2 needs a real bf16 rounding."""
    w = dyadic((D,), gen, 1, 1024, -8)
    return w * (torch.randint(0, 2, (D,), generator=gen).float() * 2 - 1)


# ---- the fused CFG + UniPC step ----------------------------------------------------------------------------------------------------
UNIPC_COEF = (4.0, 0.5, 1.0, 0.5, -0.25, 2.0, 1.5, 0.75, -1.5, 0.5)


def unipc_state(n: int, gen: torch.Generator):
    """(v_cond, v_uncond, x, x_last, m0, m1): bf16 integer velocities in [-8, 8], fp32 state in multiples of 1/4 in [-16, 16]."""
    vc, vu = (torch.randint(-8, 9, (n,), generator=gen).to(BF) for _ in range(2))
    return (vc, vu) + tuple(dyadic((n,), gen, -64, 64, -2) for _ in range(4))


def unipc_exact(vc, vu, x, xl, m0, m1, coef=UNIPC_COEF, flags: int = 0, m1_from_new: bool = False):
    """One ce_cfg_unipc_step in fp64 with the kernel's documented rounding points; returns fp32 (x, x_last, m0, m1, x0).  Every fp32 value
    the kernel forms is checked to be exact (`exact_f64`) - the recipe's premise.  `m1_from_new`: the deliberately wrong history shift."""
    r = (lambda t: round_bf16_f64(t))
    g, sigma, use_corr = coef[0], coef[1], coef[2] != 0
    a0, a1, a2, a3, p0, p1, p2 = coef[3:10]
    v = vc.double()
    if vu is not None:
        u = vu.double()
        v = r(u + r(g * r(v - u)))
    sv = sigma * v
    x0 = x.double() - (r(sv) if flags & 1 else exact_f64(sv).double())
    x0 = r(x0) if flags & 2 else exact_f64(x0).double()
    xc = x.double()
    if use_corr:
        xc = a0 * xl.double() + a1 * m0.double() + a2 * m1.double() + a3 * x0
    xc = r(xc) if flags & 2 else exact_f64(xc).double()
    xn = p0 * xc + p1 * x0 + p2 * m0.double()
    xn_r = r(xn) if flags & 2 else exact_f64(xn).double()
    rounded = (xn_r != xn).double().mean().item()
    out = (xn_r.float(), xc.float(), x0.float(), (x0 if m1_from_new else m0.double()).float(), x0.float())
    return out, rounded


# ---- softmax with exact ties ---------------------------------------------------------------------------------------------------------
TIE_GAP = 200  # exp(-200) = 1.4e-87 is 0 in fp32 (the smallest denormal is 1.4e-45), for libm's expf and for the hardware exp2 alike


def tie_targets(rows: int, n: int, valid, gen: torch.Generator) -> torch.Tensor:
    """int64 [rows, n] score targets: per row 2^k keys (k random in 1..3, as many as fit) tie at 0 - one of them the LAST valid key, so that
    a mask one key too tight changes the count - every other valid key sits at -TIE_GAP - (0..63), and every key at or past the row's valid
    length (`valid`: int per row) carries +64: it wins outright if it is read."""
    t = torch.empty(rows, n, dtype=torch.int64)
    for r in range(rows):
        nv = int(valid[r])
        t[r] = -TIE_GAP - torch.randint(0, 64, (n,), generator=gen)
        if nv > 0:
            k = 1 << int(torch.randint(1, 4, (1,), generator=gen))  # (two keys at least: a single winner would survive any bias error)
            while k > nv:
                k >>= 1
            tied = torch.randperm(nv - 1, generator=gen)[:k - 1]
            t[r, tied] = 0
            t[r, nv - 1] = 0
        t[r, nv:] = 64
    return t


def tie_probs(total: torch.Tensor, valid, check: bool = True) -> torch.Tensor:
    """fp64 [rows, n] softmax of `total` (fp64 scores with every bias added) over each row's first valid[r] keys where the maximum is shared by
    some keys and every other valid key trails by >= TIE_GAP: 1 / count on the tied keys, 0 elsewhere (all zeros for a row with no valid key).
    check=False skips the premise (a deliberately wrong reference need not keep it; its near-ties then count as losers, which changes the
    answer all the same)."""
    rows, n = total.shape
    mask = torch.arange(n)[None, :] < torch.as_tensor(valid).view(-1, 1)
    neg = torch.full_like(total, -math.inf)
    mx = torch.where(mask, total, neg).amax(1, keepdim=True)
    tied = mask & (total == mx)
    cnt = tied.sum(1, keepdim=True)
    if check:
        rest = torch.where(mask & ~tied, total, neg).amax(1, keepdim=True)
        assert bool((((mx - rest) >= TIE_GAP) | (cnt == 0)).all()), "tie recipe: a losing key is closer than TIE_GAP"
        assert bool(((cnt & (cnt - 1)) == 0).all()), "tie recipe: the tie count is no power of two"
    return tied.double() / cnt.clamp(min=1).double()


def t5_bias(heads: int, Lq: int, Lk: int, gen: torch.Generator):
    """(table fp32 [Lq + Lk - 1, heads], lut int32 [Lq + Lk - 1]): every offset k - q has a bucket of its own (lut is a permutation) and the
    integer entry of (bucket, head) is p * heads + h + p * h * nb * heads for a permutation p of the buckets, centred: distinct per
    (bucket, head), and the DIFFERENCE between two heads' entries is distinct per bucket - the wrong head, or the wrong offset, moves two tied
    keys by different amounts (at least 1) and so breaks their tie.  All below 2^23: scores = target - bias are exact in fp32."""
    nb = Lq + Lk - 1
    p = torch.randperm(nb, generator=gen).view(nb, 1)
    h = torch.arange(heads).view(1, heads)
    table = p * heads + h + p * h * nb * heads
    assert int(table.max()) < 2 ** 23
    return (table - int(table.max()) // 2).float(), torch.randperm(nb, generator=gen).to(torch.int32)


def t5_bias_rows(table: torch.Tensor, lut: torch.Tensor, batch: int, heads: int, Lq: int, Lk: int, head=None) -> torch.Tensor:
    """fp64 [batch * heads * Lq, Lk]: bias[(b, h, q)][k] = table[lut[k - q + Lq - 1]][h]; `head` overrides h for every row (the wrong reference)."""
    q = torch.arange(Lq).view(1, 1, Lq, 1)
    k = torch.arange(Lk).view(1, 1, 1, Lk)
    h = torch.arange(heads).view(1, heads, 1, 1) if head is None else torch.full((1, heads, 1, 1), head)
    bk = lut.long()[k - q + Lq - 1].expand(batch, heads, Lq, Lk)
    return table.double()[bk, h.expand(batch, heads, Lq, Lk)].reshape(batch * heads * Lq, Lk)


def softmax_f64(total: torch.Tensor, valid) -> torch.Tensor:
    """Ordinary fp64 softmax over each row's first valid[r] keys (zeros past them)."""
    mask = torch.arange(total.shape[1])[None, :] < torch.as_tensor(valid).view(-1, 1)
    return torch.softmax(total.masked_fill(~mask, -math.inf), dim=1).masked_fill(~mask, 0.0)


def unequal_share(got: torch.Tensor, want: torch.Tensor) -> float:
    """Share of elements that differ at all (the companion figure of every within-1-ulp comparison)."""
    return mismatches(got, want, 0).double().mean().item()


def gemv_bias(N: int, gen: torch.Generator) -> torch.Tensor:
    """fp32 [N] bias: distinct multiples of 8 (bias[0] for every row shows, also after a rounding to bf16 of a result below 2048)."""
    return (torch.randperm(N, generator=gen) - N // 2).float() * 8


# ------------------------------------------------------------------------------------------------------------------------------------
# MXFP8 attention (ce_attention_mxfp8 / _quant / _add): operands handed over as BYTES - e4m3 elements with E8M0 block scales - that the
# test writes itself, so every value is exact in MXFP8 and the producers (pinned elsewhere) stay out of the comparison.
#
# Per head (128 channels = four 32-channel MX blocks), all values integers of at most 4 significant bits times a power of two:
#   dims 3p .. 3p+2, p < 7   K = (d_p, d_p^2, 1), Q = (2 C a_p, -C, -C a_p^2): score = -C sum_p (a_p - d_p)^2, base-4 digits, C = 64 - the winner
#                            scores exactly 0 and every other key <= -64 in the exp2 domain (the kernel applies no further factor): 44 nats,
#                            and exp2(-64 + 3) rounds to 0 in e4m3, so every P is a power of two or 0 and l is exact under both schedules
#   dims 21, 22, 23          tie flags: K = 0 on the 2 / 4 / 8 keys of the head's tie set (the last valid key among them), else 1; a tie row's
#                            query is -128 on one of them and 0 on the digits: the set scores 0, everyone else -128
#   dims (30, 40), (72, 110) balance pairs in blocks (0, 1) and (2, 3): Q = (+G, -G), K = (u, u), u in 1..14 per key - they cancel exactly
#                            under the right block scales and leave G u (2^a - 2^b) under a scale byte taken from elsewhere: the key with
#                            the largest (or smallest) u then wins.  A needle alone survives any positive reweighting of a block.
#   dims 100..102, 103       neighbour-sample bonus and invalid flag as in `needle_k` / `needle_q`, weight 2^13 > 64 * 7 * 9
# Every block is stored under a scale chosen at random among those that hold it exactly (the canonical 2^(floor(log2 amax) - 8) times 1, 2, 4).
# ------------------------------------------------------------------------------------------------------------------------------------
MX_C = 64.0
MX_DIGITS = 7            # base-4 digits: up to 16384 keys per sample
MX_TIE_DIM = 21          # dims 21, 22, 23: tie sets of 2, 4, 8 keys
MX_TIE_C = 128.0
MX_BAL = ((30, 40), (72, 110))
MX_G = 2.0 ** 13
MX_BIG = 2.0 ** 13       # beats the largest in-sample lead, 64 * 7 * 9 = 4032, by 4160 octaves
MX_OCTAVES = MIN_MARGIN_NATS * LOG2E  # the margin in the exp2 domain
E4M3_LUT = torch.arange(256, dtype=torch.int16).to(torch.uint8).view(torch.float8_e4m3fn).double()
MX_KEY_OF_POS = torch.tensor([32 * ((p % 32) >> 4) + (p % 32 & 3) + 8 * (((p % 32) & 15) >> 2) + 4 * (p // 32) for p in range(64)])
MX_POS_OF_KEY = torch.argsort(MX_KEY_OF_POS)  # position inside a 64-key tile of V^T that holds key k (test_mxfp8_v_transpose_matches_contract)
MX_GAP_BYTE = 0x7E       # e4m3 448: what the gap columns and the spare V^T blocks hold


def mx_key_digits(j: torch.Tensor) -> torch.Tensor:
    """[n] labels -> [n, 7] base-4 digits (least significant first)."""
    return torch.stack([(j >> (2 * p)) & 3 for p in range(MX_DIGITS)], -1).double()


def mx_pack(x: torch.Tensor, gen: torch.Generator, vary: bool = True):
    """fp64 [..., 32 n] -> (e4m3 bytes of the same shape, E8M0 bytes [..., n]): every 32-element block under the scale 2^(floor(log2 amax) - 8 + s),
    s random in 0..2 (0 when not `vary`); an all-zero block gets the contract's 2^-126.  Asserts that the bytes hold x exactly."""
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = xb.abs().amax(-1)
    e = torch.floor(torch.log2(amax.clamp(min=2.0 ** -100))) - 8.0
    if vary:
        e = e + torch.randint(0, 3, e.shape, generator=gen).double()
    e = torch.where(amax > 0, e, torch.full_like(e, -126.0))
    el = (xb / torch.exp2(e)[..., None]).float().to(torch.float8_e4m3fn)
    assert torch.equal(el.double() * torch.exp2(e)[..., None], xb), "mx_pack: a block is not exact in MXFP8 under its scale"
    return el.view(torch.uint8).reshape(x.shape), (e + 127.0).to(torch.uint8)


def mx_unpack(b8: torch.Tensor, s8: torch.Tensor) -> torch.Tensor:
    """bytes [..., 32 n] and scale bytes [..., n] -> fp64 values."""
    return E4M3_LUT[b8.long()] * torch.exp2(s8.double() - 127.0).repeat_interleave(32, dim=-1)


class MxCase:
    """The operands of one ce_attention_mxfp8* launch (CPU) and its expected outputs."""


def _mx_tie_sizes(n_kv: int):
    return [min(1 << k, 1 << (n_kv.bit_length() - 1)) for k in (1, 2, 3)]


def mx_case(n_q: int, n_kv: int, heads: int, batch: int, seed: int, mode: str = "perm", n_tie=None, gap_q: int = 16, gap_k: int = 32) -> MxCase:
    """Needle and tie operands of one launch, as bytes in roomy buffers.
    mode "perm":  every sample's keys carry their labels in a random order of its own (a neighbour's rows read in place of the sample's own pick
                  another row); winners from `winners_for` with `edge_keys` on the first and last needle rows
         "tile0": the same with every winner among keys 0..63 (no offset raise after the first tile; use with n_tie = 0)
         "mixed": even rows win in tile 0, odd rows at a key >= 64: in every 32-row wave group some rows raise the offset late, the others never
         "far":   the MX form of `far_first_tile`: rows 0..63 carry labels with four digits at 3, the winners' are 0 there: all of tile 0 lies
                  >= 64 * 4 * 9 = 2304 octaves below every winner
    The last n_tie rows of every sample (default 12, a quarter of the rows of a short sample; they share the partial last query block with needle
    rows) are tie rows: 2^k keys (k = 1 + i % 3, as many as fit) of a set per (sample, head) score 0, the last valid key among them, all others
    -128; the expected row is the mean of V over the set, exact in fp32.
    V = +-n 2^e, n in 8..14, e in -1..2 per (channel, 32-key block): exact in MXFP8, never near zero, another scale in most neighbouring blocks;
    the keys of a tie set share one sign per column, so that no mean cancels: a mean of exactly 0 would expose the 2^-128 weights of the losers.
    Buffers: q8 [B n_q + 256 B, D + gap_q] (the spare rows hold other queries), k8 [B n_kv + 64 B + 64, D + gap_k] (the spare rows win if read),
    their scale rows alike; v8t / sv with one spare sample block behind the last; gap columns and spare V^T blocks hold 448.  Fields: q, k
    (fp64, de-quantised, [rows, D]), v (fp64 [B, n_kv, D]), win (int64 [B, n_needle, H]: winning ROW), tie_sets[b][h][k - 1], want /
    add / want_add (bf16 [B n_q, D])."""
    g = torch.Generator().manual_seed(seed)
    c = MxCase()
    H, B, D = heads, batch, heads * 128
    if n_tie is None:
        n_tie = 12 if n_q >= 36 else n_q // 4
    nn = n_q - n_tie
    c.n_q, c.n_kv, c.H, c.B, c.D, c.mode, c.n_tie, c.n_needle = n_q, n_kv, H, B, D, mode, n_tie, nn
    c.npad = pad64(n_kv)
    c.ldq8, c.ldk8 = D + gap_q, D + gap_k
    nt = c.npad // 64
    extra_q, extra_k = 256 * B, 64 * B + 64
    sizes = _mx_tie_sizes(n_kv)

    qv = torch.zeros(B, n_q, H, 128, dtype=torch.float64)
    kv = torch.zeros(B * n_kv + extra_k, H, 128, dtype=torch.float64)
    c.win = torch.empty(B, nn, H, dtype=torch.int64)
    c.labels, c.tie_sets = [], []
    for b in range(B):
        if mode == "far":
            assert 128 <= n_kv <= 64 + 255 * 64
            labels = torch.cat([255 * 64 + torch.arange(64), torch.arange(n_kv - 64)])
            win = 64 + torch.randint(0, 64, (nn, H), generator=g)
        else:
            labels = torch.randperm(n_kv, generator=g)
            if mode == "tile0":
                win = winners_for(nn, min(n_kv, 64), H, g, must=(0, 63))
            else:
                win = winners_for(nn, n_kv, H, g, must=edge_keys(n_kv))
                if mode == "mixed":
                    assert n_kv > 64
                    even = (torch.arange(nn) % 2 == 0)[:, None]
                    win = torch.where(even, win % 64, 64 + win % (n_kv - 64))
        c.labels.append(labels)
        c.win[b] = win
        kb = kv[b * n_kv:(b + 1) * n_kv]
        dg = mx_key_digits(labels)                                     # [n_kv, 7]
        kb[:, :, 0:3 * MX_DIGITS:3] = dg[:, None, :]
        kb[:, :, 1:3 * MX_DIGITS:3] = (dg * dg)[:, None, :]
        kb[:, :, 2:3 * MX_DIGITS:3] = 1.0
        kb[:, :, LEAK_DIM + b % 3] = 1.0
        for (d0, d1) in MX_BAL:
            u = torch.randint(1, 15, (n_kv, H), generator=g).double()
            kb[:, :, d0] = u
            kb[:, :, d1] = u
        sets = []
        for h in range(H):
            per_k = []
            for ki, m in enumerate(sizes):
                t = torch.cat([torch.randperm(n_kv - 1, generator=g)[:m - 1], torch.tensor([n_kv - 1])])
                kb[:, h, MX_TIE_DIM + ki] = 1.0
                kb[t, h, MX_TIE_DIM + ki] = 0.0
                per_k.append(t)
            sets.append(per_k)
        c.tie_sets.append(sets)
        a = mx_key_digits(labels[win.reshape(-1)]).view(nn, H, MX_DIGITS)
        qb = qv[b]
        qb[:nn, :, 0:3 * MX_DIGITS:3] = 2.0 * MX_C * a
        qb[:nn, :, 1:3 * MX_DIGITS:3] = -MX_C
        qb[:nn, :, 2:3 * MX_DIGITS:3] = -MX_C * a * a
        for i in range(n_tie):
            qb[nn + i, :, MX_TIE_DIM + i % 3] = -MX_TIE_C
        for (d0, d1) in MX_BAL:
            qb[:, :, d0] = MX_G
            qb[:, :, d1] = -MX_G
        if B > 1:
            for nb in {(b + 1) % 3, (b - 1) % 3} - {b % 3}:
                qb[:, :, LEAK_DIM + nb] = MX_BIG
        qb[:, :, INVALID_DIM] = MX_BIG
    tail = kv[B * n_kv:]                                               # rows nobody may read: flagged, otherwise ordinary keys
    dg = mx_key_digits(torch.arange(extra_k))
    tail[:, :, 0:3 * MX_DIGITS:3] = dg[:, None, :]
    tail[:, :, 1:3 * MX_DIGITS:3] = (dg * dg)[:, None, :]
    tail[:, :, 2:3 * MX_DIGITS:3] = 1.0
    for (d0, d1) in MX_BAL:
        tail[:, :, d0] = 1.0
        tail[:, :, d1] = 1.0
    tail[:, :, INVALID_DIM] = 1.0
    qall = qv.view(B * n_q, D)
    behind = qall.roll(B * n_q // 2 + 1, 0)
    qall = torch.cat([qall] + [behind] * ((extra_q + B * n_q - 1) // (B * n_q)))[:B * n_q + extra_q]
    c.q, c.k = qall, kv.view(-1, D)
    qb8, c.sq = mx_pack(c.q, g)
    kb8, c.sk = mx_pack(c.k, g)
    c.q8 = torch.full((c.q.shape[0], c.ldq8), MX_GAP_BYTE, dtype=torch.uint8)
    c.q8[:, :D] = qb8
    c.k8 = torch.full((c.k.shape[0], c.ldk8), MX_GAP_BYTE, dtype=torch.uint8)
    c.k8[:, :D] = kb8

    nblk = c.npad // 32
    sign = torch.randint(0, 2, (B, n_kv, D), generator=g).double() * 2 - 1
    colsign = torch.randint(0, 2, (D,), generator=g).double() * 2 - 1
    for b in range(B):                                                 # one sign per column on the keys of a tie set: no mean cancels to (near) zero
        for h in range(H):
            for t in c.tie_sets[b][h]:
                sign[b, t, h * 128:(h + 1) * 128] = colsign[h * 128:(h + 1) * 128]
    n = torch.randint(8, 15, (B, n_kv, D), generator=g).double() * sign
    e = torch.randint(-1, 3, (B, nblk, D), generator=g).double()
    c.v = n * torch.exp2(e).repeat_interleave(32, dim=1)[:, :n_kv]
    vt = torch.zeros(B, H, 128, c.npad, dtype=torch.float64)           # key order, zero padding
    vt[..., :n_kv] = c.v.view(B, n_kv, H, 128).permute(0, 2, 3, 1)
    vb8, vs8 = mx_pack(vt, g)                                          # [B, H, 128, npad], [B, H, 128, npad / 32]
    pos = torch.arange(c.npad)
    key_at = pos // 64 * 64 + MX_KEY_OF_POS[pos % 64]
    c.v8t = torch.full((B + 1, H, 128, c.npad), MX_GAP_BYTE, dtype=torch.uint8)
    c.v8t[:B] = vb8[..., key_at]
    c.sv = torch.full((B + 1, H, nt, 128, 2), 130, dtype=torch.uint8)
    c.sv[:B] = vs8.view(B, H, 128, nt, 2).permute(0, 1, 3, 2, 4)

    want = torch.empty(B, n_q, D, dtype=torch.float64)
    for b in range(B):
        want[b, :nn] = _gather_rows(c.v[b], c.win[b], H)
        for i in range(n_tie):
            for h in range(H):
                t = c.tie_sets[b][h][i % 3]
                want[b, nn + i, h * 128:(h + 1) * 128] = c.v[b][t, h * 128:(h + 1) * 128].sum(0) / len(t)
    c.want = bf16_rne(want.view(B * n_q, D))
    mag = 100.0 + torch.randint(0, 56, (B * n_q, D), generator=g).double() / 2
    c.add = (mag * (torch.randint(0, 2, (B * n_q, D), generator=g).double() * 2 - 1)).to(BF)
    c.want_add = (c.want.float() + c.add.float()).to(BF)
    return c


def mx_margins(c: MxCase):
    """(lead, forbidden lead, tie gap) in octaves (the exp2 domain of the kernel), from the de-quantised buffers: needle rows - the winner's
    score (asserted to be exactly 0) minus the best other key's of the sample, and the worst forbidden row's score minus the winner's; tie rows
    - the set scores exactly 0 (asserted), and the gap to the best other key of the sample.  Forbidden: every other row of the K buffer, except
    the samples b +- 3, +- 6 ... that the bonus dims cannot tell from b (their row order and V differ)."""
    lead, forb, gap = math.inf, math.inf, math.inf
    kh = c.k.view(-1, c.H, 128).transpose(0, 1)
    for b in range(c.B):
        qh = c.q[b * c.n_q:(b + 1) * c.n_q].view(c.n_q, c.H, 128).transpose(0, 1)
        s = qh @ kh.transpose(1, 2)                                     # [H, n_q, rows]
        own = s[:, :, b * c.n_kv:(b + 1) * c.n_kv]
        keep = torch.ones(s.shape[-1], dtype=torch.bool)
        for o in range(c.B):
            if o == b or (o - b) % 3 == 0:
                keep[o * c.n_kv:(o + 1) * c.n_kv] = False
        if keep.any():
            forb = min(forb, s[:, :, keep].amin().item())
        wi = c.win[b].t().unsqueeze(-1)
        sw = own[:, :c.n_needle].gather(-1, wi)
        assert not sw.any(), "a winner's score is not exactly 0"
        if c.n_kv > 1 and c.n_needle:
            lead = min(lead, -own[:, :c.n_needle].scatter(-1, wi, -math.inf).amax().item())
        for i in range(c.n_tie):
            for h in range(c.H):
                t = c.tie_sets[b][h][i % 3]
                row = own[h, c.n_needle + i].clone()
                assert not row[t].any(), "a tie key does not score exactly 0"
                row[t] = -math.inf
                if len(t) < c.n_kv:
                    gap = min(gap, -row.max().item())
    return lead, forb, gap


MX_MISTAKES = ("neighbour sample's K rows", "neighbour sample's V^T", "neighbour head's sq dword", "neighbour head's sk dword",
               "sv of the other 32-key half", "sv of the neighbouring tile", "key order inside a tile unpermuted", "no tail mask",
               "tail mask at Nkv-1", "Nkv rounded up to npad", "row stride D", "head and query block swapped", "remainder block of the wrong sample",
               "neighbour sample's add rows")
_MX_ORDER_MISTAKES = ("head and query block swapped", "remainder block of the wrong sample", "neighbour sample's add rows")


def mx_mistake_applies(mistake: str, n_q: int, n_kv: int, heads: int, batch: int, mode: str = "perm", gap_q: int = 16, gap_k: int = 32) -> bool:
    """Whether a launch of this shape can tell `mistake` from the right index at all (one key: the softmax is 1 whatever the score; mode "tile0":
    no row wins or ties at the last key, so only a key past it that is READ shows)."""
    nqb_full, hx = n_q // 256, heads // 8
    last = mode != "tile0"
    return {"neighbour sample's K rows": batch > 1, "neighbour sample's V^T": batch > 1, "neighbour sample's add rows": batch > 1,
            "neighbour head's sq dword": heads > 1 and n_kv > 1, "neighbour head's sk dword": heads > 1 and n_kv > 1, "sv of the other 32-key half": True,
            "sv of the neighbouring tile": n_kv > 64, "key order inside a tile unpermuted": n_kv > 4, "no tail mask": n_kv % 64 != 0 and last,
            "tail mask at Nkv-1": n_kv > 1 and last, "Nkv rounded up to npad": n_kv % 64 != 0, "row stride D": (gap_q > 0 or gap_k > 0) and n_kv > 1,
            "head and query block swapped": heads % 8 == 0 and nqb_full >= 1 and nqb_full != hx,
            "remainder block of the wrong sample": heads % 8 == 0 and batch > 1 and n_q % 256 != 0}[mistake]


def mx_work_items(n_q: int, heads: int, batch: int, mistake=None):
    """(sample, head, query block) of every work item in the order of the persistent kernel: with H % 8 == 0 item -> (xcd, local), every xcd takes
    its heads' full 256-row blocks first, sample by sample, and the remainder blocks last; otherwise sample-major, head, block.
    "head and query block swapped": quotient and remainder of the full-block index used for one another; "remainder block of the wrong sample":
    the remainder index divided by H in place of H / 8."""
    nqb, nqb_full = (n_q + 255) // 256, n_q // 256
    out = []
    for item in range(nqb * heads * batch):
        if heads % 8 == 0:
            xcd, local, hx = item & 7, item >> 3, heads >> 3
            full = batch * hx * nqb_full
            if local < full:
                bz, r = local // (hx * nqb_full), local % (hx * nqb_full)
                hq, qb = r // nqb_full, r % nqb_full
                if mistake == "head and query block swapped":
                    hq, qb = qb, hq
                head = xcd + 8 * hq
            else:
                l2 = local - full
                bz = l2 // heads if mistake == "remainder block of the wrong sample" else l2 // hx
                head, qb = xcd + 8 * (l2 % hx), nqb_full
        else:
            bz, r = item // (nqb * heads), item % (nqb * heads)
            head, qb = r // nqb, r % nqb
        out.append((bz, head, qb))
    return out


def _mx_head_f64(c: MxCase, bz: int, head: int, m) -> torch.Tensor:
    """fp64 [n_q, 128]: the attention of one (sample, head) from the flat byte buffers, every address written out as the kernel derives it."""
    H, B, nq, nkv, npad, D = c.H, c.B, c.n_q, c.n_kv, c.npad, c.D
    D32, nt = D // 32, npad // 64
    ldq, ldk = (D, D) if m == "row stride D" else (c.ldq8, c.ldk8)
    d = torch.arange(128)
    rq = (bz * nq + torch.arange(nq))[:, None]
    hq = (head + 1) % H if m == "neighbour head's sq dword" else head
    q = E4M3_LUT[c.q8.reshape(-1)[rq * ldq + head * 128 + d].long()] * torch.exp2(c.sq.reshape(-1)[rq * D32 + hq * 4 + d // 32].double() - 127.0)
    bk = (bz + 1) % B if m == "neighbour sample's K rows" else bz
    if m == "no tail mask":           # the ragged tile's clamped rows counted: the last key once more for every padding position
        j = torch.arange(npad)
        rk = bk * nkv + j.clamp(max=nkv - 1)
    elif m == "Nkv rounded up to npad":
        j = torch.arange(npad)
        rk = bk * nkv + j
    else:
        j = torch.arange(nkv - 1 if m == "tail mask at Nkv-1" else nkv)
        rk = bk * nkv + j
    rk = rk[:, None]
    hk = (head + 1) % H if m == "neighbour head's sk dword" else head
    k = E4M3_LUT[c.k8.reshape(-1)[rk * ldk + head * 128 + d].long()] * torch.exp2(c.sk.reshape(-1)[rk * D32 + hk * 4 + d // 32].double() - 127.0)
    bv = (bz + 1) % B if m == "neighbour sample's V^T" else bz
    t, kk = j // 64, j % 64
    pos = kk if m == "key order inside a tile unpermuted" else MX_POS_OF_KEY[kk]
    beta = 1 - kk // 32 if m == "sv of the other 32-key half" else kk // 32
    ts = (t + 1) % nt if m == "sv of the neighbouring tile" else t
    v = E4M3_LUT[c.v8t.reshape(-1)[((bv * H + head) * 128 + d[None, :]) * npad + (t * 64 + pos)[:, None]].long()]
    v = v * torch.exp2(c.sv.reshape(-1)[(((bv * H + head) * nt + ts[:, None]) * 128 + d[None, :]) * 2 + beta[:, None]].double() - 127.0)
    s = q @ k.t()
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    return (p @ v) / p.sum(-1, keepdim=True)


def mxfp8_attention_f64(c: MxCase, mistake=None, add: bool = False, cache=None) -> torch.Tensor:
    """The attention of the entry points' contract on the PACKED buffers of `c`, plain fp64 (the scores are already in the exp2 domain), walked
    item by item in the kernel's work order, with the single rounding to bf16 at the end (add: bf16(bf16(o) + add row) after it).  Rows that no
    item writes stay NaN.  `mistake` (one of MX_MISTAKES): the same with one deliberately wrong index.  cache: a dict shared between calls on
    one case (the per-head results of the unmistaken loads serve every work-order mistake)."""
    assert mistake is None or mistake in MX_MISTAKES
    load_m = None if mistake in _MX_ORDER_MISTAKES else mistake
    cache = {} if cache is None else cache
    out = torch.full((c.B, c.n_q, c.D), math.nan, dtype=torch.float64)
    for bz, head, qb in mx_work_items(c.n_q, c.H, c.B, mistake):
        if not (0 <= bz < c.B and 0 <= head < c.H and qb * 256 < c.n_q):
            continue  # (a kernel with this mistake reads and writes past its operands here; the rows it should have written stay NaN)
        key = (load_m, bz, head)
        if key not in cache:
            cache[key] = _mx_head_f64(c, bz, head, load_m)
        out[bz, qb * 256:(qb + 1) * 256, head * 128:(head + 1) * 128] = cache[key][qb * 256:(qb + 1) * 256]
    o = out.view(c.B * c.n_q, c.D).float().to(BF)
    if add:
        a = c.add.view(c.B, c.n_q, c.D).roll(-1, 0).reshape(c.B * c.n_q, c.D) if mistake == "neighbour sample's add rows" else c.add
        o = (o.float() + a.float()).to(BF)
    return o


# The launches of tests/test_exact_attention_mxfp8_gpu.py, proven on the CPU in tests/test_exact_constructions.py: (n_q, n_kv, H, B, mode, n_tie).
# n_q: no full 256-row block, exactly one, one or two plus a remainder; n_kv: 1, 2, 3, 5 and 11 tiles, ragged and full, one key; H: both work
# orders, one and two heads per xcd; the last one has more work items than the persistent form has workgroups by default (2 * 16 * 17 = 544).
MX_CASES = {
    "q31-k1-h2-b1": (31, 1, 2, 1, "perm", None),
    "q31-k31-h3-b3": (31, 31, 3, 3, "perm", None),
    "q256-k64-h5-b2": (256, 64, 5, 2, "perm", None),
    "q300-k65-h8-b2": (300, 65, 8, 2, "perm", None),
    "q300-k130-h16-b3": (300, 130, 16, 3, "perm", None),
    "q556-k257-h8-b2": (556, 257, 8, 2, "perm", None),
    "q556-k700-h2-b1": (556, 700, 2, 1, "perm", None),
    "q300-k700-h3-b3": (300, 700, 3, 3, "perm", None),
    "q300-k257-h5-b3-mixed": (300, 257, 5, 3, "mixed", None),
    "q300-k130-h2-b1-far": (300, 130, 2, 1, "far", None),
    "q256-k130-h16-b1-tile0": (256, 130, 16, 1, "tile0", 0),
    "q257-k70-h16-b17": (257, 70, 16, 17, "perm", None),
}
_mx_cases = {}


def mx_named_case(name: str) -> MxCase:
    """The case MX_CASES[name], built once per process and never modified."""
    if name not in _mx_cases:
        n_q, n_kv, H, B, mode, n_tie = MX_CASES[name]
        _mx_cases[name] = mx_case(n_q, n_kv, H, B, seed=1000 + len(name) + n_q + n_kv, mode=mode, n_tie=n_tie)
    return _mx_cases[name]


# ------------------------------------------------------------------------------------------------------------------------------------
# The fp8 mode's operand producers and GEMM tails (tests/test_exact_fp8_producers_gpu.py; CPU proofs in tests/test_exact_constructions.py)
#
# Row quantiser with one scale per row (quant_rows_fp8, ln_affine_fp8): `row_fp8_ref` is the kernel's documented arithmetic, one fp32 operation
# per line - bits of the scale and every byte must agree.  Tier A (`fp8_pow2_rows`): rows of e4m3 values times 2^e with amax = 448 2^e, whose
# scale is 2^e exactly and whose bytes dequantise to the input; tier B (`fp8_random_rows`): ordinary rows.
# MX producers (ln_affine_mxfp8, rmsnorm_rope_mxfp8, the FFN-up epilogue): `mx_contract` on a row that is known exactly - `unit_rows` through
# an affine whose 32-column blocks differ by octaves (`mx_affine_vectors`), or a GEMM whose GELU input is exact and lies where the
# activation is x, -0 or 0 (`sat_gemm_case`).  `FP8_MISTAKES`: what each reference must be able to see on the data that is launched.
# ------------------------------------------------------------------------------------------------------------------------------------
F32_INV_448 = torch.ones((), dtype=torch.float32) / 448.0   # the constant 1.0f / 448.0f of the kernels (0x3b124925)
SCALE_SENTINEL = 0xEE   # E8M0 byte no test data produces (2^111): what every scale byte a kernel must not write holds before the call
BYTE_SENTINEL = 0x7F    # e4m3 NaN: what every element byte a kernel must not write holds before the call
FP8_MISTAKES = ("scale byte of the neighbouring block", "W-order scale layout", "affine row of the wrong sample", "bias of column n+4",
                "one slab fewer in the tail sum", "tail raster group 1", "post_scale ignored", "RoPE table row m")


def row_fp8_ref(x: torch.Tensor):
    """(s fp32 [M], e4m3 bytes [M, K]) of a bf16 / fp32 matrix under one scale per row, as ce_quant_rows_fp8 documents it, in fp32:
    s = amax * float32(1 / 448) (1 for a zero row), inv = 1 / s (a correctly rounded division), bytes = RNE_e4m3(x * inv)."""
    xf = x.float()
    amax = xf.abs().amax(1)
    s = torch.where(amax > 0, torch.mul(amax, F32_INV_448), torch.ones_like(amax))
    inv = torch.div(torch.ones_like(s), s)
    return s, torch.mul(xf, inv[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)


def fp8_pow2_rows(M: int, K: int, gen: torch.Generator):
    """Tier A: (x bf16 [M, K], bytes uint8 [M, K], e int [M]): x = e4m3(bytes) * 2^e, e in -6..6 per row, every finite byte value allowed
    (-0 and the subnormals among them) and one element per row at +-448 2^e, so that amax * float32(1 / 448) = 2^e exactly."""
    b = torch.randint(0, 256, (M, K), generator=gen, dtype=torch.int64)
    b[(b & 0x7F) == 0x7F] = 0x38                                    # (no NaN bytes: 1.0 in their place)
    b[:, 0], b[:, 1] = 0x80, 0x01                                    # (-0 and the smallest subnormal in every row)
    top = torch.where(torch.randint(0, 2, (M,), generator=gen) == 1, 0xFE, 0x7E)
    b[torch.arange(M), torch.randint(2, K, (M,), generator=gen)] = top
    e = torch.randint(-6, 7, (M,), generator=gen)
    x64 = E4M3_LUT[b] * torch.exp2(e.double())[:, None]
    x = x64.to(BF)
    assert torch.equal(x.double(), x64)
    return x, b.to(torch.uint8), e


def fp8_random_rows(M: int, K: int, gen: torch.Generator) -> torch.Tensor:
    """Tier B: ordinary rows (normal values, another magnitude per row); row 0 holds its maximum in the last 8-element chunk only, and the
    last row (of two or more) is all zeros."""
    x = torch.randn(M, K, generator=gen) * (0.05 + 3 * torch.rand(M, 1, generator=gen))
    x[0, :K - 8] *= 2.0 ** -5
    x[0, K - 8:] = torch.tensor([3.0, -40.0, 7.0, 0.5, -1.0, 33.0, 2.0, -9.0])
    if M > 1:
        x[M - 1] = 0
    return x.to(BF)


def mx_contract(x: torch.Tensor, saturating: bool = False):
    """(E8M0 bytes [rows, K / 32], e4m3 bytes [rows, K]) of the MX contract for a bf16 / fp32 matrix: scale = 2^(floor(log2 amax) - 8), one step
    up when amax / scale would exceed 448 unless `saturating` (the attention operands keep the floor rule and clip at 448: ce_common.h
    mx_scale_byte / mx_scale_byte_nosat, oracle.dit_oracle.mx_quant), byte 1 (2^-126) for an all-zero block; elements RNE(x / scale) clamped
    to +-448.  The exponent comes from frexp, not from a rounded log2."""
    xf = x.float()
    xb = xf.view(xf.shape[0], -1, 32)
    amax = xb.abs().amax(-1)
    e = torch.frexp(amax)[1].float() - 1.0 - 8.0
    if not saturating:
        e = e + (amax > 448.0 * torch.exp2(e)).float()
    e = torch.where(amax > 0, torch.clamp(e, min=-126.0), torch.full_like(e, -126.0))
    q = torch.clamp(xb / torch.exp2(e)[..., None], -448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).reshape(xf.shape)
    return (e + 127.0).to(torch.uint8), q


def mx_scales_tiled(rows8: torch.Tensor, w_order: bool = False, fill: int = SCALE_SENTINEL) -> torch.Tensor:
    """Scale bytes [R, K / 32] -> the flat tiled buffer of the MX GEMM operands (ce_common.h mx_gemm_scale_offset / mx_gemm_wscale_offset),
    128 ceil(R / 128) rows long; the bytes of the rows past R hold `fill`."""
    R, nb = rows8.shape
    assert nb % 4 == 0
    r, blk = torch.arange(R)[:, None], torch.arange(nb)[None, :]
    inner = (r & 127) if w_order else (r & 15) * 8 + ((r >> 4) & 7)
    off = ((r >> 7) * (nb // 4) + (blk >> 2)) * 512 + (blk & 3) * 128 + inner
    out = torch.full(((R + 127) // 128 * (nb // 4) * 512,), fill, dtype=torch.uint8)
    out[off.reshape(-1)] = rows8.reshape(-1)
    return out


def neighbour_block(rows8: torch.Tensor) -> torch.Tensor:
    """Every scale byte replaced by the one of the next 32-column block of its row (the last by the first)."""
    return rows8.roll(-1, 1)


def scale_diversity(rows8: torch.Tensor) -> float:
    """Share of (row, block) pairs whose scale byte differs from the next block's."""
    return (rows8 != neighbour_block(rows8)).double().mean().item()


def mx_affine_vectors(rows: int, D: int, gen: torch.Generator):
    """`affine_vectors` with a and b of every 32-column block scaled by 2^e, e in -6..6 per (sample, block), and about one block in eight
    at a = b = 0: neighbouring blocks of the output differ by octaves, and zero blocks (scale byte 1, zero bytes) occur."""
    a, b = affine_vectors(rows, D, gen)
    f = torch.exp2(torch.randint(-6, 7, (rows, D // 32), generator=gen).float())
    keep = (torch.randint(0, 8, (rows, D // 32), generator=gen) != 0).repeat_interleave(32, dim=1)
    f = f.repeat_interleave(32, dim=1)
    return torch.where(keep, a * f, torch.zeros(())), torch.where(keep, b * f, torch.zeros(()))  # (+0 in the zero blocks)


class Case:
    """The operands of one launch (CPU) and what it must return."""


_fp8_cases = {}


def _cached(key, build):
    if key not in _fp8_cases:
        _fp8_cases[key] = build()
    return _fp8_cases[key]


LN_FP8_DS = (5120, 520)
LN_MX_DS = (5120, 640)


def ln_fp8_case(D: int, mistake=None) -> Case:
    """ln_affine_fp8: 11 rows, one (a, b) per 3 rows (a sample boundary inside every block of four rows), ab_stride = D + 4.  want_s / want_q:
    `row_fp8_ref` of the exactly known bf16 row."""
    assert mistake in (None, "affine row of the wrong sample")
    if mistake is None and ("ln_fp8", D) in _fp8_cases:
        return _fp8_cases[("ln_fp8", D)]
    g = torch.Generator().manual_seed(4100 + D)
    c = Case()
    c.M, c.D, c.ab_rows, c.S = 11, D, 3, 4
    c.x, c.v = unit_rows(c.M, D, g)
    c.a, c.b = affine_vectors(c.S, D, g)
    sample = None if mistake is None else (torch.arange(c.M) + 1) // c.ab_rows
    c.y = bf16_rne(ln_affine_exact(c.v, c.a, c.b, c.ab_rows, sample=sample))
    c.want_s, c.want_q = row_fp8_ref(c.y)
    if mistake is None:
        _fp8_cases[("ln_fp8", D)] = c
    return c


def ln_mx_case(D: int, mistake=None) -> Case:
    """ln_affine_mxfp8: 130 rows (two 128-row scale blocks, the second holding two rows), one `mx_affine_vectors` pair per 43 rows.  want_rows
    (scale bytes [M, D / 32]), want_q, and want_s: the flat tiled scale buffer with SCALE_SENTINEL in the rows 130 .. 255."""
    assert mistake in (None, "affine row of the wrong sample", "scale byte of the neighbouring block", "W-order scale layout")
    if mistake is None and ("ln_mx", D) in _fp8_cases:
        return _fp8_cases[("ln_mx", D)]
    g = torch.Generator().manual_seed(4200 + D)
    c = Case()
    c.M, c.D, c.ab_rows, c.S = 130, D, 43, 4
    c.x, c.v = unit_rows(c.M, D, g)
    c.a, c.b = mx_affine_vectors(c.S, D, g)
    sample = (torch.arange(c.M) + 1) // c.ab_rows if mistake == "affine row of the wrong sample" else None
    c.y = bf16_rne(ln_affine_exact(c.v, c.a, c.b, c.ab_rows, sample=sample))
    c.want_rows, c.want_q = mx_contract(c.y)
    if mistake == "scale byte of the neighbouring block":
        c.want_rows = neighbour_block(c.want_rows)
    c.want_s = mx_scales_tiled(c.want_rows, w_order=mistake == "W-order scale layout")
    if mistake is None:
        _fp8_cases[("ln_mx", D)] = c
    return c


# (D, head_dim): the full-width form (one cos / sin entry per lane), and a narrow width whose heads do not divide 512 (an entry per chunk) and
# whose last 16 lanes hold no chunk.  (D stays a multiple of 128: the kernel stores four scale bytes as one dword at row * D / 32.)
RMS_MX_SHAPES = ((5120, 128), (384, 96))
RMS_MX_M = 9


def rms_mx_case(D: int, head_dim: int, R, post_scale: float, mistake=None) -> Case:
    """rmsnorm_rope_mxfp8 on 9 rows: R = 9 (a table row per token), 3 (row m uses entry m % 3) or None (no RoPE).  want_rows / want_q: the
    floor-rule contract (the attention operands') of float32(bf16 value) * float32(post_scale)."""
    assert mistake in (None, "post_scale ignored", "RoPE table row m")
    g = torch.Generator().manual_seed(4300 + D + (R or 0))
    c = Case()
    c.M, c.D, c.hd, c.R, c.post_scale = RMS_MX_M, D, head_dim, R, post_scale
    c.x, c.v = unit_rows(c.M, D, g, centred=True)
    c.w = rms_weights(D, g)
    c.cs = rope_table(R, head_dim, g) if R else None
    cs, table_row = c.cs, None
    if mistake == "RoPE table row m" and R:
        cs, table_row = torch.cat([c.cs, rope_table(c.M, head_dim, g)])[:max(c.M, R)], torch.arange(c.M)
    c.t = rms_rope_exact(c.v, c.w, cs, head_dim, table_row=table_row)
    ps = torch.tensor(1.0 if mistake == "post_scale ignored" else post_scale, dtype=torch.float32)
    c.want_rows, c.want_q = mx_contract(torch.mul(c.t.float(), ps), saturating=True)
    return c


# ---- the split-K plan of the fp8 GEMMs, restated (ce_gemm_plan.h ce_split_k, ce_gemm_fp8w4.hip fp8_plan) ------------------------------------
FP8_BM = FP8_BN = 256
FP8_BK = 128
FP8_GROUP = 4


def ce_split_k(tail: int, kt: int, cus: int, slab_bytes: int, ws_bytes: int) -> int:
    if tail <= 0:
        return 1
    for s in range(min(cus // tail, 8), 1, -1):
        if kt % (2 * s) == 0 and tail * s * slab_bytes <= ws_bytes:
            return s
    return 1


def fp8_split_k(tail: int, kt: int, cus: int, ws_bytes: int) -> int:
    split = ce_split_k(tail, kt, cus, FP8_BM * FP8_BN * 4, ws_bytes)
    if split == 1:
        return 1
    saving_us, slabs_us = (1.0 - 1.0 / split) * kt * 1.7, tail * split * 0.128 + 8.0
    return 1 if saving_us < 1.5 * slabs_us else split


def fp8_tail_plan(M: int, N: int, K: int, cus: int, ws_bytes: int):
    """(tiles_m, tiles_n, t_full, tail, split) of a one-wave-per-SIMD fp8 launch: the `tail` tiles of the partially filled last round are cut
    in `split` along K (tail = 0, split = 1: nothing is cut)."""
    tiles_m, tiles_n = -(-M // FP8_BM), -(-N // FP8_BN)
    nwg = tiles_m * tiles_n
    tail = nwg % cus
    split = fp8_split_k(tail, K // FP8_BK, cus, ws_bytes)
    if split == 1:
        tail = 0
    return tiles_m, tiles_n, nwg - tail, tail, split


def fp8_tile_origin(wg: int, tiles_m: int, tiles_n: int, group: int = FP8_GROUP):
    """(m0, n0) of workgroup wg under the grouped raster of gemm_fp8_w4."""
    group_sz = group * tiles_n
    first_m = wg // group_sz * group
    gm = min(tiles_m - first_m, group)
    return (first_m + (wg % group_sz) % gm) * FP8_BM, (wg % group_sz) // gm * FP8_BN


def fp8_tail_launch_f64(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, plan, mistake=None) -> torch.Tensor:
    """fp64 acc + bias [M, N] of a launch, tile by tile as the plan lays it out: a full tile sums all of K; a tail tile is the sum of its `split`
    K slabs, which the reduce kernel places at the origin it recomputes and completes with the bias of its own columns.  Elements that nothing
    writes stay NaN.  `mistake`: "one slab fewer in the tail sum", "tail raster group 1" (the reduce kernel's origin under a raster group of 1)
    or "bias of column n+4" (in the reduce kernel)."""
    assert mistake in (None, "one slab fewer in the tail sum", "tail raster group 1", "bias of column n+4")
    tiles_m, tiles_n, t_full, tail, split = plan
    M, K = a.shape
    N = w.shape[0]
    ad, wd, bd = a.double(), w.double(), bias.double()
    out = torch.full((tiles_m * FP8_BM, tiles_n * FP8_BN), math.nan, dtype=torch.float64)
    ap = torch.zeros(tiles_m * FP8_BM, K, dtype=torch.float64)
    wp = torch.zeros(tiles_n * FP8_BN, K, dtype=torch.float64)
    bp = torch.zeros(tiles_n * FP8_BN, dtype=torch.float64)
    ap[:M], wp[:N], bp[:N] = ad, wd, bd
    for wg in range(tiles_m * tiles_n):
        m0, n0 = fp8_tile_origin(wg, tiles_m, tiles_n)
        md, nd, kk, b = m0, n0, K, bp
        if wg >= t_full:
            if mistake == "one slab fewer in the tail sum":
                kk = K - K // split
            elif mistake == "tail raster group 1":
                md, nd = fp8_tile_origin(wg, tiles_m, tiles_n, group=1)
            elif mistake == "bias of column n+4":
                b = bp.roll(-4)
        out[md:md + FP8_BM, nd:nd + FP8_BN] = ap[m0:m0 + FP8_BM, :kk] @ wp[n0:n0 + FP8_BN, :kk].t() + b[nd:nd + FP8_BN]
    return out[:M, :N]


# ---- GEMM data whose GELU input is exact and lies where the activation is x, -0 or 0 ------------------------------------------------------
SAT_POS, SAT_NEG = 6.0, -12.0   # gelu_tanh in fp32 with the kernel's constants: x at x >= 6 after the bf16 rounding, -0 at x <= -12
# (M, N, K): four tiles, all tail, cut in six, a ragged second row of tiles; one tile, no cut; 256 full tiles and 16 tail tiles cut in five
SAT_SHAPES = ((300, 512, 13824), (129, 256, 256), (4352, 4096, 5120))
SAT_CUT = {(300, 512, 13824): True, (129, 256, 256): False, (4352, 4096, 5120): True}


def sat_gemm_case(M: int, N: int, K: int) -> Case:
    """a bf16 [M, K]: integers 0..7 times 2^e per 32-element block, e in {e_row - 1, e_row}, e_row in -2..2 (an all-zero row, an all-zero block);
    w bf16 [N, K]: integers 0..7 times 2^(oct - 3 - {0, 1} per block), signed by the CLASS of the output column - positive, negative or zero (a
    zero W row); oct in 0..5 per 32 output columns; bias fp32 [N]: class sign times (16..48) 2^oct.  Every partial sum of an output element is an
    integer below 14 * 14 * 13824 < 2^22 units, so fp32 holds acc + bias exactly in any order; positive columns give x >= 16, negative ones
    x <= -16, zero columns 0.  Most 32-column blocks mix the three classes; one in eight, and the second, hold no positive column (all -0 / 0: scale byte 1)."""
    def build():
        g = torch.Generator().manual_seed(4400 + M + N + K)
        c = Case()
        c.M, c.N, c.K = M, N, K
        ia = torch.randint(0, 8, (M, K), generator=g).float()
        er = torch.randint(-2, 3, (M, 1), generator=g).float()
        ea = er - torch.randint(0, 2, (M, K // 32), generator=g).float()
        ia[min(2, M - 1)] = 0
        ia[0, 32:64] = 0
        c.a = (ia * torch.exp2(ea).repeat_interleave(32, dim=1)).to(BF)
        cls = torch.randint(-1, 2, (N,), generator=g)                                # -1 negative, 0 zero, +1 positive
        nopos = torch.randint(0, 8, (N // 32,), generator=g) == 0
        nopos[1] = True
        nopos = nopos.repeat_interleave(32)
        cls = torch.where(nopos & (cls > 0), -cls, cls)
        c.cls = cls
        octv = torch.randint(0, 6, (N // 32,), generator=g).float().repeat_interleave(32)
        iw = torch.randint(0, 8, (N, K), generator=g).float() * cls[:, None].float()
        ew = octv[:, None] - 3.0 - torch.randint(0, 2, (N, K // 32), generator=g).float()
        c.w = (iw * torch.exp2(ew).repeat_interleave(32, dim=1)).to(BF)
        c.bias = cls.float() * torch.randint(16, 49, (N,), generator=g).float() * torch.exp2(octv)
        c.unit = torch.exp2(er.double() - 1.0) * torch.exp2(octv.double() - 4.0)[None, :]   # [M, N]: every term of acc + bias is a multiple
        return c
    return _cached(("sat", M, N, K), build)


def sat_gelu(x: torch.Tensor) -> torch.Tensor:
    """bf16 GELU of inputs in {0} u [6, inf) u (-inf, -12], without a transcendental: x, -0 or 0.  Asserts the premise."""
    xf = x.float()
    assert bool(((xf == 0) | (xf >= SAT_POS) | (xf <= SAT_NEG)).all()), "saturated GELU recipe: an input lies in the activation's bend"
    return torch.where(xf >= SAT_POS, xf, torch.where(xf <= SAT_NEG, torch.full_like(xf, -0.0), torch.zeros_like(xf))).to(BF)


def mixed_block_share(y: torch.Tensor) -> float:
    """Share of 32-column blocks of a `sat_gelu` result that hold a positive value, a -0 and a +0."""
    yb = y.float().view(y.shape[0], -1, 32)
    neg0 = (yb == 0) & torch.signbit(yb)
    pos0 = (yb == 0) & ~torch.signbit(yb)
    return ((yb > 0).any(-1) & neg0.any(-1) & pos0.any(-1)).double().mean().item()


# ---- GEMM data whose GELU input spans the activation's bend ---------------------------------------------------------------------------------
BEND_SHAPES = ((300, 520, 256), (300, 520, 13824))   # no cut; six tiles, all tail, cut in six
BEND_CUT = {(300, 520, 256): False, (300, 520, 13824): True}


def bend_gemm_case(M: int, N: int, K: int) -> Case:
    """Integers in -7..7 (exact in e4m3) under one power-of-two scale per row: ia, iw (fp32 integers), sa = 2^{-1, 0}, sw = 2^{E - 1, E} with E
    chosen so that the largest standard deviation of a sum, 18.7 sqrt(K) 2^E, is about 1.1; bias in units of 1/16 up to 1.  a, w: the bf16 values
    (what the MX quantiser is fed).  Partial sums stay below 49 * 13824 < 2^20 units."""
    def build():
        g = torch.Generator().manual_seed(4500 + M + N + K)
        c = Case()
        c.M, c.N, c.K = M, N, K
        E = -round(math.log2(18.7 * math.sqrt(K)))
        c.ia = torch.randint(-7, 8, (M, K), generator=g).float()
        c.iw = torch.randint(-7, 8, (N, K), generator=g).float()
        c.ia[min(2, M - 1)] = 0
        c.sa = torch.exp2(torch.randint(-1, 1, (M,), generator=g).float())
        c.sw = torch.exp2(E - torch.randint(0, 2, (N,), generator=g).float())
        c.a, c.w = (c.ia * c.sa[:, None]).to(BF), (c.iw * c.sw[:, None]).to(BF)
        c.bias = int_vector(N, g, lo=-16, hi=16, e=-4)
        return c
    return _cached(("bend", M, N, K), build)


# ------------------------------------------------------------------------------------------------------------------------------------
# the VAE's implicit-GEMM conv (ce_conv_igemm_bf16), RMS_norm (+ SiLU) (ce_rms_silu_bf16) and the conv with the norm in its epilogue
# (ce_conv3d_gemm_rms_silu_bf16): tests/test_exact_vae_ops_gpu.py launches them, tests/test_exact_constructions.py proves the recipes.
#
# Conv: `int_rows` activations (one scale) and weights, `int_vector` bias - every sum exact in fp32, the expected output the fp64 value of
# the header's formula rounded once (with a residual: bf16(res + that), an fp32 add of two bf16 values).  Every stored frame is written
# everywhere, BORDER INCLUDED: only the positions the reference network calls padding are zero, and only where the engine's layout makes
# them zero (the whole border under a stride-1 3 x 3, the bottom row and right column under the stride-2 3 x 3 = ZeroPad2d((0, 1, 0, 1)),
# the shared zero frame of the temporal convs) - a read from the wrong side of the border changes the result.
# ------------------------------------------------------------------------------------------------------------------------------------
CONV_MISTAKES = ("in_off ignored", "in_off on rows only", "in_off on columns only", "stride multiplies the tap too", "kh and kw swapped",
                 "frame t+kt instead of t*st+kt", "symmetric pad instead of bottom/right pad", "second slice uses weight rows 0..C",
                 "second slice uses bias rows 0..C", "residual read without border offset")


def _frame_at(frame: torch.Tensor, rows: torch.Tensor, cols: torch.Tensor) -> torch.Tensor:
    """frame [Hs, Ws, C] at the stored positions (rows[i], cols[j]); a position outside the frame reads as zero (only a deliberately wrong
    reference gets there)."""
    Hs, Ws = frame.shape[:2]
    ok = ((rows >= 0) & (rows < Hs))[:, None] & ((cols >= 0) & (cols < Ws))[None, :]
    return frame[rows.clamp(0, Hs - 1)][:, cols.clamp(0, Ws - 1)] * ok[..., None]


def conv_frames_f64(in_frames, w: torch.Tensor, bias, n_out: int, *, KT: int, KH: int, KW: int, st: int, ss: int, H_out: int, W_out: int,
                    in_off: int, cout_slice=None, mistake=None) -> torch.Tensor:
    """The formula of csrc/ce_conv.hip's header, literally, in fp64 - one matmul per (output frame, tap) on shifted views of the frame list:
      out[t][h][w][co] = bias[co] + sum_{kt,kh,kw,ci} W[co][(kt,kh,kw)][ci] * in[t*st+kt][h*ss+kh+in_off][w*ss+kw+in_off][ci]
    in_frames: list of [Hs, Ws, Cin] frames AS STORED (border included; the same frame may appear twice); w [Cout_all, KT*KH*KW, Cin] (the
    pack's layout), bias [Cout_all] or None; cout_slice = (lo, hi): the output channels lo..hi-1 of the pack.  -> fp64 [n_out, H_out, W_out, hi-lo].
    `mistake` (one of CONV_MISTAKES): the same with one deliberately wrong index ("residual ...": nothing changes here - `conv_want`)."""
    assert mistake is None or mistake in CONV_MISTAKES, mistake
    lo, hi = cout_slice if cout_slice is not None else (0, w.shape[0])
    n = hi - lo
    wlo = 0 if mistake == "second slice uses weight rows 0..C" else lo
    blo = 0 if mistake == "second slice uses bias rows 0..C" else lo
    off_h = off_w = in_off
    if mistake == "in_off ignored":
        off_h = off_w = 0
    elif mistake == "in_off on rows only":
        off_w = 0
    elif mistake == "in_off on columns only":
        off_h = 0
    elif mistake == "symmetric pad instead of bottom/right pad":  # one zero row / column in FRONT of the image: every tap one position up and left
        off_h = off_w = in_off - 1
    tap_s, tap_t = (ss, st) if mistake == "stride multiplies the tap too" else (1, 1)
    t_mul = 1 if mistake == "frame t+kt instead of t*st+kt" else st
    swap = mistake == "kh and kw swapped"
    assert not swap or KH == KW
    wd = w.double()[wlo:wlo + n]
    f64 = {}
    h, wv = torch.arange(H_out, device=w.device), torch.arange(W_out, device=w.device)
    out = torch.zeros(n_out, H_out, W_out, n, dtype=torch.float64, device=w.device)
    for t in range(n_out):
        for kt in range(KT):
            fi = t * t_mul + kt * tap_t
            if fi >= len(in_frames):
                continue  # (a wrong reference only)
            f = f64.setdefault(fi, in_frames[fi].double())
            for kh in range(KH):
                for kw in range(KW):
                    x = _frame_at(f, h * ss + kh * tap_s + off_h, wv * ss + kw * tap_s + off_w)
                    tap = (kt * KH + kw) * KW + kh if swap else (kt * KH + kh) * KW + kw
                    out[t] += x @ wd[:, tap].t()
    if bias is not None:
        out += bias.double()[blo:blo + n]
    return out


def _conv_spec(Cin, Cout, k, T, H, W, **kw):
    d = dict(Cin=Cin, Cout=Cout, k=k, T=T, H=H, W=W, st=1, ss=1, in_off=0, pad="none", in_rows=False, out_rows=False, res=False, cstride=None,
             coff=0, cout_all=None, cout_lo=0, in_idx=None, zero_frames=(), out_idx=None, n_out_buf=None, seed_as=None)
    d.update(kw)
    return d


def _conv_table():
    t = {}
    # 1 x 1 (x 1) reading the interior of bordered frames: .shortcut / conv1 / conv2 (one partial M tile; a ragged fourth one)
    t["1x1 off1 M126"] = _conv_spec(96, 192, (1, 1, 1), 2, 9, 7, in_off=1)
    t["1x1 off1 M429"] = _conv_spec(96, 192, (1, 1, 1), 3, 13, 11, in_off=1)
    # .to_qkv: plain-row output, three N tiles; .proj: plain-row input, residual, bordered output
    t["1x1 to rows"] = _conv_spec(128, 384, (1, 1, 1), 2, 9, 11, in_off=1, out_rows=True)
    t["1x1 from rows + res"] = _conv_spec(96, 96, (1, 1, 1), 2, 7, 9, in_rows=True, res=True)
    # .resample.1 down: 3 x 3, stride 2, padding from the bottom and right border only
    for KT in (1, 3):
        t[f"3x3 s2 even KT{KT}"] = _conv_spec(96, 96, (KT, 3, 3), 2, 10, 14, ss=2, in_off=1, pad="br")   # last taps on the border
        t[f"3x3 s2 odd KT{KT}"] = _conv_spec(96, 96, (KT, 3, 3), 2, 11, 9, ss=2, in_off=1, pad="br")     # last taps on the interior
    # .time_conv down: (3, 1, 1), temporal stride 2; the same zero frame twice in front
    t["time down T2"] = _conv_spec(96, 96, (3, 1, 1), 2, 5, 6, st=2, in_off=1, in_idx=[0, 0, 1, 2, 3], zero_frames=(0,))
    t["time down T7"] = _conv_spec(96, 96, (3, 1, 1), 7, 4, 5, st=2, in_off=1, in_idx=list(range(15)))
    # .time_conv up: the two halves of a 2C-channel pack into the even and the odd frames of ONE buffer
    up = dict(in_off=1, in_idx=[0, 0, 1, 2, 3], zero_frames=(0,), cout_all=192, n_out_buf=6, seed_as="time up")
    t["time up lo"] = _conv_spec(96, 96, (3, 1, 1), 3, 5, 7, cout_lo=0, out_idx=[0, 2, 4], **up)
    t["time up hi"] = _conv_spec(96, 96, (3, 1, 1), 3, 5, 7, cout_lo=96, out_idx=[1, 3, 5], **up)
    # Cout <= 32: conv_igemm_kernel<32>; 40: five live chunks of a 128-wide tile; 136: a second N tile with one live chunk
    for Cout in (8, 16, 24, 32, 40, 136):
        for Cin in (32, 384):
            t[f"k1 {Cin}->{Cout}"] = _conv_spec(Cin, Cout, (1, 1, 1), 2, 9, 8, in_off=1)
            t[f"k3 {Cin}->{Cout}"] = _conv_spec(Cin, Cout, (3, 3, 3), 2, 9, 8, pad="all")
    t["k1 32->16 in 32"] = _conv_spec(32, 16, (1, 1, 1), 2, 9, 8, in_off=1, cstride=32)
    t["k3 32->16 in 32"] = _conv_spec(32, 16, (3, 3, 3), 2, 9, 8, pad="all", cstride=32)
    t["coff 8 of 24+16"] = _conv_spec(32, 24, (3, 3, 3), 2, 9, 8, pad="all", cstride=40, coff=8)
    t["coff 8 of 96+16"] = _conv_spec(96, 96, (1, 1, 1), 2, 9, 8, in_off=1, cstride=112, coff=8, res=True)
    t["16 frames"] = _conv_spec(32, 32, (3, 1, 1), 14, 3, 3, in_off=1, in_idx=list(range(16)))
    return t


CONV_CASES = _conv_table()


def conv_case(name: str) -> Case:
    """The operands of one ce_conv_igemm_bf16 launch (CPU): in_stack [frames, Hs, Ws, Cin] as stored and in_idx (the frame list, as indices),
    w [Cout_all, taps, Cin] / b [Cout_all] (the pack; the launch takes rows lo..hi), res (stored like the output) or None, and the output
    buffer's geometry: out_shape [frames, Ho, Wo, out_cstride], out_idx (the frames the launch writes), out_border, out_Wp, out_coff."""
    def build():
        s = CONV_CASES[name]
        g = torch.Generator().manual_seed(7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(s["seed_as"] or name)))
        c = Case()
        c.name, c.Cin, c.Cout, c.st, c.ss, c.in_off = name, s["Cin"], s["Cout"], s["st"], s["ss"], s["in_off"]
        c.KT, c.KH, c.KW = s["k"]
        c.n_out, H, W = s["T"], s["H"], s["W"]
        c.H_out, c.W_out = (H, W) if c.ss == 1 else (H // 2, W // 2)
        c.in_idx = s["in_idx"] if s["in_idx"] is not None else list(range((c.n_out - 1) * c.st + c.KT))
        n_stack = max(c.in_idx) + 1
        Hs, Ws = (H, W) if s["in_rows"] else (H + 2, W + 2)
        c.in_Wp = Ws
        x = int_rows(n_stack * Hs * Ws, c.Cin, g, emin=-1, emax=-1).view(n_stack, Hs, Ws, c.Cin).clone()
        if s["pad"] == "all":
            x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = 0, 0, 0, 0
        elif s["pad"] == "br":
            x[:, -1], x[:, :, -1] = 0, 0
        for z in s["zero_frames"]:
            x[z] = 0
        c.in_stack = x
        c.Cout_all = s["cout_all"] or c.Cout
        c.cout_slice = (s["cout_lo"], s["cout_lo"] + c.Cout)
        taps = c.KT * c.KH * c.KW
        c.w = int_rows(c.Cout_all, taps * c.Cin, g, emin=-2, emax=2).view(c.Cout_all, taps, c.Cin).contiguous()
        c.b = int_vector(c.Cout_all, g)
        c.out_cstride, c.out_coff = s["cstride"] or c.Cout, s["coff"]
        c.out_idx = s["out_idx"] if s["out_idx"] is not None else list(range(c.n_out))
        n_buf = s["n_out_buf"] or c.n_out
        if s["out_rows"]:  # plain rows [H_out * W_out (+ one spare image row), C]
            c.out_border, c.out_Wp, c.out_shape = 0, c.W_out, (n_buf, c.H_out + 1, c.W_out, c.out_cstride)
        else:
            c.out_border, c.out_Wp, c.out_shape = 1, c.W_out + 2, (n_buf, c.H_out + 2, c.W_out + 2, c.out_cstride)
        c.res = None
        if s["res"]:  # written everywhere, border and the channels beside the slice included
            c.res = (torch.randn((c.n_out,) + c.out_shape[1:], generator=g) * 64).to(BF)
        return c
    return _cached(("conv", name), build)


def conv_want(c: Case, mistake=None) -> torch.Tensor:
    """bf16 [n_out, H_out, W_out, Cout]: what the launch must leave in channels out_coff .. out_coff + Cout of the interior of its output frames."""
    y = bf16_rne(conv_frames_f64([c.in_stack[i] for i in c.in_idx], c.w, c.b, c.n_out, KT=c.KT, KH=c.KH, KW=c.KW, st=c.st, ss=c.ss, H_out=c.H_out,
                                 W_out=c.W_out, in_off=c.in_off, cout_slice=c.cout_slice, mistake=mistake))
    if c.res is not None:
        o = 0 if mistake == "residual read without border offset" else c.out_border
        r = c.res[:, o:o + c.H_out, o:o + c.W_out, c.out_coff:c.out_coff + c.Cout]
        y = torch.add(r.float(), y.float()).to(BF)  # (an fp32 add of two bf16 values, rounded once: the kernel's epilogue)
    return y


def conv_mistakes_for(c: Case):
    """The entries of CONV_MISTAKES that name a different computation for this launch."""
    m = []
    if c.in_off:
        m += ["in_off ignored", "in_off on rows only", "in_off on columns only"]
    if (c.ss > 1 and max(c.KH, c.KW) > 1) or (c.st > 1 and c.KT > 1):
        m.append("stride multiplies the tap too")
    if c.KH == c.KW and c.KH > 1:
        m.append("kh and kw swapped")
    if c.st > 1 and c.KT > 1 and c.n_out > 1:
        m.append("frame t+kt instead of t*st+kt")
    if c.ss == 2 and c.in_off == 1 and c.KH == 3:
        m.append("symmetric pad instead of bottom/right pad")
    if c.cout_slice[0] > 0:
        m += ["second slice uses weight rows 0..C", "second slice uses bias rows 0..C"]
    if c.res is not None and c.out_border:
        m.append("residual read without border offset")
    return m


def conv_place(c: Case, buf: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """`buf` (the output buffer as it was before the launch) with `want` where the launch writes: what the WHOLE buffer must hold afterwards."""
    out = buf.clone()
    o = c.out_border
    idx = torch.tensor(c.out_idx, device=buf.device)
    out[idx, o:o + c.H_out, o:o + c.W_out, c.out_coff:c.out_coff + c.Cout] = want.to(buf.device)
    return out


# ---- RMS_norm over channels (+ SiLU) --------------------------------------------------------------------------------------------------------
# Rows of +-2^k, one k per pixel: the sum of squares is n 4^k in any order (n live channels), and for a full row sqrtf(C) / sqrtf(C 4^k) is
# 2^-k exactly (a correctly rounded square root commutes with a factor 4^k): the result is bf16(+-gamma[c]).  Rows with n < C live
# channels and all-zero pixels follow the fp32 restatement of the kernel's three operations (`rms_restate_f32`), evaluated on the CPU.
RMS_CS = (32, 96, 128, 192, 384, 512)   # every (active lanes, chunks per lane) pair of the launcher: (4, 1) (12, 1) (16, 1) (12, 2) (16, 3) (16, 4)
RMS_WS = (1, 17, 70, 129)               # a row that ends inside, at (64 + 6: the PER >= 3 bodies span 32) and one past a workgroup's pixels
RMS_MISTAKES = ("norm of y", "norm before the bf16 rounding", "gamma of the neighbour chunk")
SILU_LOG2E = -1.4426950408889634


def ss_exact_in_any_order(x: torch.Tensor, quantum) -> bool:
    """Is every partial sum of squares over the last axis exact in fp32 whatever the order?  x / quantum are integers and the total of their
    squares stays below 2^24 (quantum: a power of two, a scalar or one per row)."""
    q = x.double() / quantum
    return bool((q == q.round()).all()) and bool(((q * q).sum(-1) < 2 ** 24).all())


def _fl(x64: torch.Tensor) -> torch.Tensor:
    """One rounding to fp32, the value kept in fp64."""
    return x64.float().double()


def rms_restate_f32(x: torch.Tensor, gamma: torch.Tensor, gshift: int = 0, check: bool = True) -> torch.Tensor:
    """The kernel's operations in fp32, one rounding each: scale = fl(fl(sqrt(C)) / max(fl(sqrt(ss)), 1e-12)), pre = fl(fl(x * scale) * gamma)
    -> fp32 [..., C], the value BEFORE the SiLU and the rounding to bf16.  Every operation is carried out in fp64 on fp32 operands and rounded
    once to fp32: for *, / and sqrt that IS the correctly rounded fp32 operation (53 >= 2 * 24 + 2 bits: the second rounding is innocuous),
    whatever the host's vector unit does with fp32.  ss is the exact sum of squares (asserted to be exact in fp32; `ss_exact_in_any_order` is
    the recipes' business).  gshift: gamma[c + gshift] in place of gamma[c]."""
    C = x.shape[-1]
    xd = x.double()
    ss64 = (xd ** 2).sum(-1, keepdim=True)
    ss = exact_f64(ss64).double() if check else _fl(ss64)
    floor = torch.tensor(1e-12, dtype=torch.float32).double()
    scale = _fl(_fl(torch.sqrt(torch.tensor(float(C), dtype=torch.float64))) / torch.clamp(_fl(torch.sqrt(ss)), min=floor))
    return _fl(_fl(xd * scale) * gamma.double().roll(-gshift)).float()


def rms_f64(x: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    """x / max(||x||, 1e-12) * sqrt(C) * gamma in fp64 (F.normalize semantics), before any rounding."""
    xd = x.double()
    nrm = xd.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    return xd / nrm * math.sqrt(x.shape[-1]) * gamma.double()


def silu_f64(pre: torch.Tensor) -> torch.Tensor:
    """bf16 of the fp64 SiLU of an exactly known fp32 pre-activation."""
    p = pre.double()
    return (p / (1.0 + torch.exp(-p))).float().to(BF)


def silu_fast_f32(pre: torch.Tensor) -> torch.Tensor:
    """csrc/ce_common.h's silu_fast with the CPU's fp32 operations in place of v_exp_f32 and v_rcp_f32: x * (1 / (1 + exp2(-log2(e) x)))."""
    one = torch.ones((), dtype=torch.float32)
    return torch.mul(pre, torch.div(one, torch.add(torch.exp2(torch.mul(pre, torch.tensor(SILU_LOG2E, dtype=torch.float32))), one)))


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> int:
    """The largest distance of two bf16 (fp32) tensors in units in the last place."""
    return int((_ordered(a) - _ordered(b.to(a.device))).abs().max())


# Tolerance of the comparisons that hold a SiLU: the largest distance, in bf16 ulps, between the CPU's fp32 evaluation of silu_fast and the fp64
# SiLU on the pre-activations of every SiLU launch of the GPU file (measured by test_exact_constructions.py, which asserts the figure), plus
# one ulp for the two hardware operations (v_exp_f32 and v_rcp_f32, one fp32 ulp each).
SILU_F32_VS_F64_ULPS = 1
SILU_ULPS = SILU_F32_VS_F64_ULPS + 1


def silu_unequal_allowed(pre: torch.Tensor) -> int:
    """How many SiLU results may differ from the fp64 answer at all (each of them within SILU_ULPS).  A result differs when a bf16 rounding
    boundary lies between the true value and the computed one.  Relative error of silu_fast at x: the exponent -log2(e) x carries two fp32
    roundings (the constant, the product) = 2 |x| 2^-24 relative in exp2's value; v_exp_f32 2 2^-24, the add 2^-24, v_rcp_f32 2 2^-24, the
    product 2^-24: (2 |x| + 6) 2^-24 in all.  Rounding boundaries lie more than 2^-8 apart relative to the value, so an element differs with
    probability <= (2 |x| + 6) 2^-16: the expected count lambda is the sum of that, and the allowance lambda + 4 sqrt(lambda) + 1 (four
    standard deviations of a Poisson count, and one element for the small launches)."""
    lam = float((2.0 * pre.double().abs() + 6.0).sum()) * 2.0 ** -16
    return int(lam + 4.0 * math.sqrt(lam) + 1.0)


def rms_case(C: int, T: int, H: int, W: int, diverse: bool = False) -> Case:
    """One ce_rms_silu_bf16 launch: x [T, H+2, W+2, C] bordered input (the border holds other data), gamma, and per pixel a kind: 0 a full
    row of +-2^k (k in -6..6 per pixel), 1 a row with n < C live channels (the others zero), 2 all zeros.  diverse (the SiLU launches): every
    non-zero pixel is of kind 1 with C/4 <= n <= C, so that the pre-activations take many values, |pre| <= 2 max|gamma| = 8."""
    def build():
        g = torch.Generator().manual_seed(8000 + C * 7 + W * 3 + T + H + (1 if diverse else 0))
        c = Case()
        c.C, c.T, c.H, c.W = C, T, H, W
        npix = T * H * W
        k = torch.randint(-6, 7, (npix, 1), generator=g).double()
        v = (torch.randint(0, 2, (npix, C), generator=g).double() * 2 - 1) * torch.exp2(k)
        i = torch.arange(npix)
        kind = torch.where(i % 7 == 5, 2, torch.where(i % 7 == 3, 1, 0))
        if diverse:
            kind = torch.where(kind == 2, 2, 1)
        for p in (kind == 1).nonzero()[:, 0].tolist():
            n = int(torch.randint(max(C // 4, 1), C + 1 if diverse else C, (1,), generator=g))
            v[p, torch.randperm(C, generator=g)[n:]] = 0
        v[kind == 2] = 0
        c.kind = kind.view(T, H, W)
        c.quantum = torch.exp2(k).view(T, H, W)
        c.x = v.to(BF).view(T, H, W, C)
        assert torch.equal(c.x.double().view(npix, C), v)
        c.gamma = rms_weights(C, g)
        c.x_stored = torch.full((T, H + 2, W + 2, C), 96.0, dtype=BF)  # (a border read in place of a pixel: another norm, another value)
        c.x_stored[:, 1:-1, 1:-1] = c.x
        return c
    return _cached(("rms", C, T, H, W, diverse), build)


def rms_ordinary(C: int, T: int, H: int, W: int):
    """(x [T, H, W, C] bf16, gamma fp32 [C]): ordinary random data."""
    g = torch.Generator().manual_seed(8500 + C + W)
    return (torch.randn(T, H, W, C, generator=g) * 2).to(BF), 1.0 + 0.25 * torch.randn(C, generator=g)


def rms_place(buf: torch.Tensor, want: torch.Tensor, border: int) -> torch.Tensor:
    """The whole output buffer after the launch: `want` [T, H, W, C] in the interior of bordered frames [T, H+2, W+2, C] (border 1) or in the
    first T H W rows of a plain row buffer [rows, C] (border 0); everything else as it was."""
    out = buf.clone()
    if border:
        out[:, 1:-1, 1:-1] = want.to(buf.device)
    else:
        out[:want.numel() // want.shape[-1]] = want.reshape(-1, want.shape[-1]).to(buf.device)
    return out


# ---- the stride-1 3 x 3 (x 3) conv onto 96 channels with the next RMS_norm (+ SiLU) in its epilogue -----------------------------------------------
# y = bf16(conv + bias) made exactly known AND norm-friendly: inputs +-2^k (one k per input pixel), every output channel ONE weight +-1 at
# its own tap and input channel, bias 0 - y[p][co] is one input element or 0 (a tap on the border, on a zeroed pixel or on a causal front
# frame).  All 27 taps and every 32-channel chunk of the input are addressed.  The norm of that y: `rms_restate_f32`.
FUSED_CINS = (32, 96, 192)
FUSED_FRAMES = ((1, 3, 5), (2, 5, 7), (2, 40, 64))   # the last one crosses position tiles (510 positions each) and ends in a ragged one


def fused_case(Cin: int, KT: int, T: int, H: int, W: int, kind: str) -> Case:
    """kind "single": k in -3..3 per input pixel, no residual (every pixel's squares are multiples of 2^-6 below 2^6: exact in any order).
    kind "residual": k = 0 and a residual of the SAME sign as y, j 2^-10 with 0 < j < 256 (j 2^-7 with |j| < 128 where y = 0): res + y lies in
    +-[1, 1.25), exact in fp32, and needs a real rounding to bf16's 2^-7 grid - bf16(res + y), y and the unrounded sum are three different
    rows, and all squares are multiples of 2^-14 below 2^2.  kind "ordinary": `int_rows` data on every tap, data in the front frames, a
    dyadic bias.  in_stack [KT-1 + T + 1, H+2, W+2, Cin] (front frames, chunk, zeroed slack frame); w5 [96, Cin, KT, 3, 3]; y bf16 [T, H, W, 96]."""
    def build():
        g = torch.Generator().manual_seed(9000 + Cin * 5 + KT * 3 + T + H + W + len(kind))
        c = Case()
        c.Cin, c.KT, c.T, c.H, c.W, c.kind, Cout = Cin, KT, T, H, W, kind, 96
        n_in = T + KT - 1
        taps = KT * 9
        stack = torch.zeros(n_in + 1, H + 2, W + 2, Cin, dtype=torch.float64)
        if kind == "ordinary":
            stack[:n_in, 1:-1, 1:-1] = int_rows(n_in * H * W, Cin, g, emin=-1, emax=-1).double().view(n_in, H, W, Cin)
            wp = int_rows(Cout, taps * Cin, g, emin=-2, emax=2).view(Cout, taps, Cin)
            c.b = int_vector(Cout, g)
        else:
            k = torch.randint(-3, 4, (T, H, W, 1), generator=g).double() if kind == "single" else torch.zeros(T, H, W, 1, dtype=torch.float64)
            x = (torch.randint(0, 2, (T, H, W, Cin), generator=g).double() * 2 - 1) * torch.exp2(k)
            if H >= 5:
                x[:, 0:3, 1:4] = 0  # a 3 x 3 block of zero pixels in every frame: the output pixel (1, 2) is all zeros
            stack[KT - 1:n_in, 1:-1, 1:-1] = x
            co = torch.arange(Cout)
            c.tap_of, c.ci_of = co % taps, (co * 37 + 5) % Cin
            wp = torch.zeros(Cout, taps, Cin, dtype=torch.float64)
            wp[co, c.tap_of, c.ci_of] = torch.randint(0, 2, (Cout,), generator=g).double() * 2 - 1
            wp = wp.to(BF)
            c.b = torch.zeros(Cout)
        c.in_stack = stack.to(BF)
        c.wp = wp.contiguous()
        c.w5 = wp.view(Cout, KT, 3, 3, Cin).permute(0, 4, 1, 2, 3).contiguous()
        y64 = conv_frames_f64([c.in_stack[i] for i in range(n_in)], c.wp, c.b, T, KT=KT, KH=3, KW=3, st=1, ss=1, H_out=H, W_out=W, in_off=0)
        c.y = bf16_rne(y64)
        c.gamma = rms_weights(Cout, g)
        c.res = None
        if kind == "residual":
            yd = c.y.double()
            near = torch.randint(1, 256, yd.shape, generator=g).double() * 2.0 ** -10 * yd.sign()
            far = torch.randint(-127, 128, yd.shape, generator=g).double() * 2.0 ** -7
            r = torch.where(yd != 0, near, far).to(BF)
            c.res = torch.full((T, H + 2, W + 2, Cout), 3.0, dtype=BF)  # (the border holds data: it must not reach either output)
            c.res[:, 1:-1, 1:-1] = r
            c.sum32 = torch.add(r.float(), c.y.float())
            assert torch.equal(c.sum32.double(), r.double() + yd)
            c.v = c.sum32.to(BF)
        return c
    return _cached(("fused", Cin, KT, T, H, W, kind), build)


def fused_pre(c: Case, mistake=None) -> torch.Tensor:
    """fp32 [T, H, W, 96]: the pre-activation of the normalised output (`rms_restate_f32` of bf16(res + y), or of y without a residual);
    `mistake`: one of RMS_MISTAKES."""
    assert mistake is None or mistake in RMS_MISTAKES
    row = c.v if c.res is not None else c.y
    if mistake == "norm of y":
        row = c.y
    elif mistake == "norm before the bf16 rounding":
        return rms_restate_f32(c.sum32, c.gamma, check=False)
    return rms_restate_f32(row, c.gamma, gshift=4 if mistake == "gamma of the neighbour chunk" else 0)  # (a lane owns 4 consecutive channels)
