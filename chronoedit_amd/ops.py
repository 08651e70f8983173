"""torch-tensor front end of the C ABI (include/chronoedit_hip.h).

Every function checks device/dtype/contiguity, then hands raw device pointers and the current
torch stream to libchronoedit_hip.so.  There is no fallback: a CPU tensor or a missing library
raises.  PyTorch is used here only for device memory and streams.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import hiplib

EPI_BIAS, EPI_BIAS_GELU, EPI_GATE_RES, EPI_BIAS_GELU_ERF = 0, 1, 2, 3
EPI_F32, EPI_MUL, EPI_BIAS_ROW, EPI_BIAS_T = 4, 5, 6, 7

_lib = None      # the library launches go through: the product library unless a diagnostic selector is away from its default
_product = None

# The alternative kernel bodies are selectable only in libchronoedit_hip_diag.so (include/chronoedit_hip_diag.h): while every selector is at
# its default, launches go through the product library; the first non-default value moves them to the diagnostic build, the last reset moves
# them back.  Tools and body-equivalence tests only - the engine, the pipeline and bench.py's timed region never call set_*.
_KNOB_DEFAULTS = {"ce_set_gemm_variant": -1, "ce_set_attention_waves": 0, "ce_set_gemm_fp8_variant": 1,
                  "ce_set_attention_mxfp8_variant": 1, "ce_set_attention_mxfp8_persistent": 512}
_knobs = dict(_KNOB_DEFAULTS)


def lib():
    global _lib, _product
    if _lib is None:
        _lib = _product = hiplib.load()
        import os
        v8 = os.environ.get("CE_GEMM_FP8_VARIANT")  # A/B knobs for whole-step runs (bench.py under another main loop): the diagnostic build
        if v8 is not None:
            _set_knob("ce_set_gemm_fp8_variant", int(v8))
        v = os.environ.get("CE_GEMM_VARIANT")
        if v is not None:
            _set_knob("ce_set_gemm_variant", int(v))
    return _lib


_force_diag = False


def force_diagnostics(on: bool = True) -> None:
    """(tools) send launches through libchronoedit_hip_diag.so even with every selector at its default - e.g. to read the exact-route counters
    of the attention kernels (ce_diag_attention_exact_route_hits) for launches that run the DEFAULT bodies."""
    global _lib, _force_diag
    lib()
    _force_diag = bool(on)
    want = hiplib.load_diagnostics() if (_force_diag or any(_knobs[k] != _KNOB_DEFAULTS[k] for k in _knobs)) else _product
    if want is not _lib:
        _lib = want


def attention_exact_route_hits(reset: bool = True):
    """(diagnostic build) (bf16 kernels, MXFP8 kernel): waves x key tiles that took the exact route of the speculative softmax since the last reset."""
    buf = (ctypes.c_ulonglong * 2)()
    _check(hiplib.load_diagnostics().ce_diag_attention_exact_route_hits(buf, 1 if reset else 0), "ce_diag_attention_exact_route_hits")
    return int(buf[0]), int(buf[1])


def _set_knob(symbol: str, v: int) -> int:
    global _lib
    lib()
    diag = hiplib.load_diagnostics()
    prev = getattr(diag, symbol)(int(v))
    _knobs[symbol] = getattr(diag, symbol)(int(v))  # (setters ignore values they do not know: read back what is in force)
    want = diag if (_force_diag or any(_knobs[k] != _KNOB_DEFAULTS[k] for k in _knobs)) else _product
    if want is not _lib:
        _lib = want
    return prev


class HipKernelError(RuntimeError):
    pass


# ---- optional per-launch timing with HIP events on the launch stream (bench.py roofline leg) ----
_PROF = None  # list of (key, flops_or_bytes, start_event, end_event) while profiling


class profile:
    """with ops.profile() as prof: ...; prof.summary() -> {key: {n, total_ms, avg_ms, work}} (events on the
    current torch stream, which is the stream every launcher enqueues on)."""

    def __enter__(self):
        global _PROF
        _PROF = []
        return self

    def __exit__(self, *exc):
        global _PROF
        self.records, _PROF = _PROF, None
        return False

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for key, work, st, en in self.records:
            d = out.setdefault(key, {"n": 0, "total_ms": 0.0, "work": work})
            d["n"] += 1
            d["total_ms"] += st.elapsed_time(en)
        for d in out.values():
            d["avg_ms"] = d["total_ms"] / d["n"]
        return out


def _prof_begin():
    if _PROF is None:
        return None
    st = torch.cuda.Event(enable_timing=True)
    st.record()
    return st


def _prof_end(st, key, work):
    if st is not None:
        en = torch.cuda.Event(enable_timing=True)
        en.record()
        _PROF.append((key, work, st, en))


def _check(rc: int, name: str):
    if rc != 0:
        kind = {-1: "bad argument", -2: "unsupported shape", -3: "misaligned stride"}.get(rc, f"hipError {rc}")
        raise HipKernelError(f"{name} failed: {kind}")


def _launch(name: str, *args):
    """Call entry point `name` of the library launches go through; a non-zero return raises under that name."""
    _check(getattr(lib(), name)(*args), name)


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise HipKernelError(f"{name}: tensor must live on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _rows(t: torch.Tensor, name: str):
    """2-D view with unit inner stride -> (M, D, ld)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D tensor with contiguous rows, got shape {tuple(t.shape)} stride {t.stride()}")
    return t.shape[0], t.shape[1], t.stride(0)


def ln_affine(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None,
              ab_rows: int = 0, ab_stride: int = 0):
    """out = LN_fp32(x) * a + b  (bf16 in/out, fp32 a/b).  ab_rows > 0: row m uses a/b + (m // ab_rows) * ab_stride."""
    _dev(x, torch.bfloat16, "x"), _dev(a, torch.float32, "a"), _dev(b, torch.float32, "b")
    M, D, ldx = _rows(x, "x")
    if out is None:
        out = torch.empty((M, D), dtype=torch.bfloat16, device=x.device)
    _, _, ldy = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_ln_affine_bf16", _ptr(x), _ptr(out), _ptr(a), _ptr(b), M, D, ldx, ldy, float(eps), int(ab_rows), int(ab_stride),
            _stream())
    _prof_end(st, f"ln_affine_{M}x{D}", 4.0 * M * D)
    return out


def rmsnorm_rope_(x: torch.Tensor, w: torch.Tensor, cos_sin: Optional[torch.Tensor], head_dim: int, eps: float,
                  x2: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None):
    """In place RMSNorm-across-heads (+ RoPE when cos_sin [R, head_dim/2, 2] fp32 is given; row m uses entry m % R).
    (x2, w2): a second tensor of the same geometry (k beside q in the fused qkv buffer) handled by the same launch."""
    _dev(x, torch.bfloat16, "x"), _dev(w, torch.float32, "w")
    M, D, ld = _rows(x, "x")
    rope_rows = 0
    if cos_sin is not None:
        _dev(cos_sin, torch.float32, "cos_sin")
        assert cos_sin.is_contiguous() and cos_sin.shape[1:] == (head_dim // 2, 2) and M % cos_sin.shape[0] == 0, (cos_sin.shape, M)
        rope_rows = cos_sin.shape[0]
    if x2 is not None:
        _dev(x2, torch.bfloat16, "x2"), _dev(w2, torch.float32, "w2")
        assert _rows(x2, "x2") == (M, D, ld)
    st = _prof_begin()
    _launch("ce_rmsnorm_rope_bf16", _ptr(x), _ptr(w), _ptr(x2), _ptr(w2), _ptr(cos_sin), M, D, ld, head_dim, float(eps), rope_rows,
            _stream())
    _prof_end(st, f"rmsnorm_rope_{M}x{D}" + ("x2" if x2 is not None else ""), (8.0 if x2 is not None else 4.0) * M * D)
    return x


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None,
         epilogue: int = EPI_BIAS, gate: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, gate_rows: int = 0,
         res_rows: int = 0):
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T + bias).  gate [N] or, with gate_rows > 0, [M/gate_rows, N] (one per sample).
    res_rows > 0 (EPI_GATE_RES): res is [res_rows, N] and output row m adds residual row m % res_rows - samples stacked along M that share
    one residual (ce_gemm_bf16_res); res must not overlap out then.
    a may be a 3-D [S, M, K/S] tensor (contiguous): the K-segmented operand an all-to-all leaves behind (a_seg_k of ce_gemm_bf16).
    epilogue EPI_BIAS_T: out is [N, M] and receives the TRANSPOSE of a @ w^T + bias[n] (CE_EPI_BIAS_T)."""
    _dev(a, torch.bfloat16, "a"), _dev(w, torch.bfloat16, "w")
    a_seg_k, a_seg_stride = 0, 0
    if a.dim() == 3:
        S, M, Ks = a.shape
        if a.stride(2) != 1 or a.stride(1) < Ks:
            raise ValueError(f"gemm: segmented a needs unit inner stride, got {a.stride()}")
        K, lda, a_seg_k, a_seg_stride = S * Ks, a.stride(1), Ks, a.stride(0)
    else:
        M, K, lda = _rows(a, "a")
    N, K2, ldw = _rows(w, "w")
    if K != K2:
        raise ValueError(f"gemm: K mismatch {K} vs {K2}")
    if bias is not None:
        _dev(bias, torch.float32, "bias")
        assert bias.numel() == (M if epilogue == EPI_BIAS_ROW else N) and bias.is_contiguous()
    oshape = (N, M) if epilogue == EPI_BIAS_T else (M, N)
    if out is None:
        out = torch.empty(oshape, dtype=torch.bfloat16, device=a.device)
    _dev(out, torch.bfloat16, "out")
    Mo, No, ldc = _rows(out, "out")
    assert (Mo, No) == oshape, ((Mo, No), oshape)
    ldres = 0
    if epilogue in (EPI_GATE_RES, EPI_MUL):
        if res is None:
            raise ValueError("EPI_GATE_RES / EPI_MUL need res")
        _dev(res, torch.bfloat16, "res")
        Mr, _, ldres = _rows(res, "res")
        if gate is not None:
            _dev(gate, torch.float32, "gate")
            assert gate.is_contiguous() and gate.numel() == (N if gate_rows <= 0 else (M + gate_rows - 1) // gate_rows * N)
        if res_rows > 0:
            if epilogue != EPI_GATE_RES or Mr < min(res_rows, M):
                raise ValueError(f"gemm: res_rows={res_rows} needs EPI_GATE_RES and a residual of at least that many rows (got {Mr})")
            lo, hi = res.data_ptr(), res.data_ptr() + ((min(res_rows, M) - 1) * ldres + N) * 2
            if lo < out.data_ptr() + ((M - 1) * ldc + N) * 2 and out.data_ptr() < hi:
                raise ValueError("gemm: a residual with a row period must not overlap the output")
    elif res_rows > 0:
        raise ValueError("gemm: res_rows needs EPI_GATE_RES")
    ws, ws_bytes = _gemm_scratch(a.device)
    st = _prof_begin()
    if res_rows > 0:
        _launch("ce_gemm_bf16_res", _ptr(a), _ptr(w), _ptr(out), _ptr(bias), epilogue, _ptr(gate), _ptr(res), M, N, K, lda, ldw, ldc, ldres,
                int(gate_rows), int(res_rows), int(a_seg_k), int(a_seg_stride), 0, 0, ws, ws_bytes, _stream())
        _prof_end(st, f"gemm_{M}x{N}x{K}_epi{epilogue}_res{res_rows}", 2.0 * M * N * K)
        return out
    _launch("ce_gemm_bf16", _ptr(a), _ptr(w), _ptr(out), _ptr(bias), epilogue, _ptr(gate), _ptr(res), M, N, K, lda, ldw, ldc, ldres,
            int(gate_rows), int(a_seg_k), int(a_seg_stride), 0, 0, ws, ws_bytes, _stream())
    _prof_end(st, f"gemm_{M}x{N}x{K}_epi{epilogue}", 2.0 * M * N * K)
    return out


def rope_scatter(x: torch.Tensor, cols, weights, D: int, world: int, cos_sin: Optional[torch.Tensor], head_dim: int, eps: float,
                 out: Optional[torch.Tensor] = None):
    """Ulysses send buffer [world, M, len(cols), D/world] from column blocks `cols` (start columns, each D wide) of x [M, ld]:
    RMSNorm * weights[i] (+ RoPE with cos_sin) where weights[i] is given, plain copy where it is None (ce_rope_scatter_bf16)."""
    _dev(x, torch.bfloat16, "x")
    M, _, ldx = _rows(x, "x")
    nt = len(cols)
    assert 1 <= nt <= 3 and len(weights) == nt
    for w in weights:
        if w is not None:
            _dev(w, torch.float32, "w")
            assert w.is_contiguous() and w.numel() == D
    rope_rows = 0
    if cos_sin is not None:
        _dev(cos_sin, torch.float32, "cos_sin")
        assert cos_sin.is_contiguous() and cos_sin.shape[1:] == (head_dim // 2, 2) and M % cos_sin.shape[0] == 0
        rope_rows = cos_sin.shape[0]
    if out is None:
        out = torch.empty((world, M, nt, D // world), dtype=torch.bfloat16, device=x.device)
    _dev(out, torch.bfloat16, "out")
    assert out.is_contiguous() and out.numel() == M * nt * D
    c = list(cols) + [0] * (3 - nt)
    w = list(weights) + [None] * (3 - nt)
    st = _prof_begin()
    _launch("ce_rope_scatter_bf16", _ptr(x), ldx, _ptr(out), M, D, world, nt, c[0], _ptr(w[0]), c[1], _ptr(w[1]), c[2], _ptr(w[2]),
            _ptr(cos_sin), head_dim, float(eps), rope_rows, _stream())
    _prof_end(st, f"rope_scatter_{M}x{D}x{nt}", 4.0 * M * D * nt)
    return out


_gemm_split = True
GEMM_WS_BYTES = 256 * 384 * 256 * 4  # one fp32 slab of the LARGEST macro tile (384 x 256) per CU: any split-K tail the dispatcher may choose fits (96 MiB; round 6 - with 64 MiB the
# 384-row tile could not cut its tail at M = 7 200 and lost FFN-down by 13 %: profiles/r06_gemm_tile_choice_m7200.txt)


GEMM_WS_STREAMS = 8  # streams per device that get a scratch of their own; further ones evict the least recently used
_gemm_default = {}  # device index -> (the first stream a GEMM ran on, that device's default scratch)
_gemm_own = {}      # (device index, stream) -> the scratch of a further stream, least recently used first (dicts keep insertion order)


def _gemm_scratch(device: torch.device):
    """The split-K scratch (pointer, bytes) a GEMM launched now on the current stream of `device` is given - (None, 0) turns the split off.
    The first stream of a device uses the device's default buffer; every further stream gets a buffer of its own, so concurrent streams
    never share slabs.  A stream that is capturing a graph and has no buffer of its own uses the default (nothing is allocated under capture;
    captures of one device do not overlap in this package)."""
    if not _gemm_split:
        return None, 0
    dev = device.index if device.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(dev).cuda_stream
    first = _gemm_default.get(dev)
    if first is not None and first[0] == stream:
        buf = first[1]
    elif (dev, stream) in _gemm_own:
        buf = _gemm_own[(dev, stream)] = _gemm_own.pop((dev, stream))  # most recently used last
    else:
        with torch.cuda.device(dev):
            capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            if first is None:
                return None, 0
            buf = first[1]
        elif first is None:
            buf = torch.empty(GEMM_WS_BYTES, dtype=torch.uint8, device=dev)
            _gemm_default[dev] = (stream, buf)
        else:
            mine = [k for k in _gemm_own if k[0] == dev]
            if len(mine) >= GEMM_WS_STREAMS:
                # the LEAST RECENTLY USED stream's scratch is DROPPED, not handed on: split-K partials of GEMMs still queued on that stream
                # may be in it, and nothing orders the new stream behind them.  The caching allocator returns the block to the pool of the
                # stream it was allocated on, so whatever reuses it is ordered behind that stream's queued work.
                del _gemm_own[mine[0]]
            buf = _gemm_own[(dev, stream)] = torch.empty(GEMM_WS_BYTES, dtype=torch.uint8, device=dev)
    return buf.data_ptr(), buf.numel()


def set_gemm_split(on: bool) -> bool:
    """Enable/disable the split-K tail of the 256-tile GEMM; returns the previous setting."""
    global _gemm_split
    prev, _gemm_split = _gemm_split, bool(on)
    return prev


def set_gemm_variant(v: int) -> int:
    """-1 auto, 0 force the 128-tile kernel, 1 force the 256-tile LDS-DMA kernel; returns the previous setting."""
    return _set_knob("ce_set_gemm_variant", v)


def set_attention_waves(n: int) -> int:
    """Attention loop body: 0 auto (= 64), 4 / 8 plain kernel with that many waves, 64 software-pipelined (default), 128 / 129 the
    one-wave-per-SIMD body of the V^T form (one workgroup per item / persistent); returns the previous value (include/chronoedit_hip.h)."""
    return _set_knob("ce_set_attention_waves", n)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, out: Optional[torch.Tensor] = None,
              k2: Optional[torch.Tensor] = None, v2: Optional[torch.Tensor] = None, scale: Optional[float] = None,
              batch: int = 1):
    """q [Nq, H*128], k/v [Nkv, H*128] (row strides free) -> out [Nq, H*128]; optional 2nd kv segment.
    batch > 1: every operand holds `batch` samples stacked along its rows (q [batch*Nq, ...], k [batch*Nkv, ...])."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _dev(t, torch.bfloat16, n)
    Nq, Dq, ldq = _rows(q, "q")
    head_dim = Dq // heads
    L1, _, ldk = _rows(k, "k")
    L1v, _, ldv = _rows(v, "v")
    assert L1 == L1v
    if batch < 1 or Nq % batch or L1 % batch or (k2 is not None and k2.shape[0] % batch):
        raise ValueError(f"attention: row counts must be multiples of batch={batch}")
    if out is None:
        out = torch.empty((Nq, Dq), dtype=torch.bfloat16, device=q.device)
    _, _, ldo = _rows(out, "out")
    L2 = ldk2 = ldv2 = 0
    if k2 is not None:
        _dev(k2, torch.bfloat16, "k2"), _dev(v2, torch.bfloat16, "v2")
        L2, _, ldk2 = _rows(k2, "k2")
        _, _, ldv2 = _rows(v2, "v2")
    if scale is None:
        scale = head_dim ** -0.5
    st = _prof_begin()
    nq, l1, l2 = Nq // batch, L1 // batch, L2 // batch
    _launch("ce_attention_batched_bf16", _ptr(q), _ptr(k), _ptr(v), l1, ldk, ldv, _ptr(k2), _ptr(v2), l2, ldk2, ldv2, _ptr(out),
            nq, heads, head_dim, ldq, ldo, float(scale), batch, _stream())
    _prof_end(st, f"attention_{nq}x{l1}+{l2}_h{heads}" + (f"_b{batch}" if batch > 1 else ""),
              4.0 * nq * (l1 + l2) * head_dim * heads * batch)
    return out


def vt_columns(n_keys_total: int) -> int:
    """Row length of the V^T operand for `n_keys_total` keys (all samples side by side): whole 64-key strips, 16-B aligned rows."""
    return (n_keys_total + 63) // 64 * 64 + 64


def v_transpose(v: torch.Tensor, heads: int, out: Optional[torch.Tensor] = None):
    """v [keys of all samples, heads*128] (row stride free) -> V^T [heads*128, vt_columns(keys)] bf16, padding columns zeroed:
    the V operand of `attention_vt`."""
    _dev(v, torch.bfloat16, "v")
    n, D, ldv = _rows(v, "v")
    assert D == heads * 128
    if out is None:
        out = torch.empty((D, vt_columns(n)), dtype=torch.bfloat16, device=v.device)
    _dev(out, torch.bfloat16, "vt")
    assert out.shape[0] == D and out.is_contiguous() and out.shape[1] >= n
    st = _prof_begin()
    _launch("ce_v_transpose_bf16", _ptr(v), ldv, _ptr(out), out.shape[1], n, heads, _stream())
    _prof_end(st, f"v_transpose_{n}x{D}", 4.0 * n * D)
    return out


def attention_vt(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, out: Optional[torch.Tensor] = None,
                 scale: Optional[float] = None, batch: int = 1):
    """Self-attention with V transposed (`v_transpose`): q [batch*Nq, H*128], k [batch*Nkv, H*128], vt [H*128, >= batch*Nkv (+pad)];
    K and V^T tiles both reach LDS by LDS-DMA.  Same arithmetic as `attention` (one KV segment)."""
    for n, t in (("q", q), ("k", k), ("vt", vt)):
        _dev(t, torch.bfloat16, n)
    Nq, Dq, ldq = _rows(q, "q")
    L1, _, ldk = _rows(k, "k")
    assert Dq == heads * 128 and vt.shape[0] == Dq and vt.stride(1) == 1
    if batch < 1 or Nq % batch or L1 % batch:
        raise ValueError(f"attention_vt: row counts must be multiples of batch={batch}")
    if out is None:
        out = torch.empty((Nq, Dq), dtype=torch.bfloat16, device=q.device)
    _, _, ldo = _rows(out, "out")
    if scale is None:
        scale = 128 ** -0.5
    st = _prof_begin()
    nq, l1 = Nq // batch, L1 // batch
    _launch("ce_attention_vt_bf16", _ptr(q), _ptr(k), _ptr(vt), l1, ldk, vt.stride(0), _ptr(out), nq, heads, 128, ldq, ldo, float(scale),
            batch, _stream())
    _prof_end(st, f"attention_{nq}x{l1}+0_h{heads}" + (f"_b{batch}" if batch > 1 else ""), 4.0 * nq * l1 * 128 * heads * batch)
    return out


def attention_2seg_vt(q: torch.Tensor, k1: torch.Tensor, v1t: torch.Tensor, len1: int, k2: torch.Tensor, v2t: torch.Tensor, len2: int,
                      heads: int, out: Optional[torch.Tensor] = None, scale: Optional[float] = None, batch: int = 1,
                      cols1: Optional[int] = None, cols2: Optional[int] = None, out8: Optional[torch.Tensor] = None,
                      scale8: Optional[torch.Tensor] = None):
    """Cross-attention over two key / value segments (a softmax each, outputs added in bf16) with V transposed: k1 [batch*len1, H*128],
    v1t [H*128, >= (batch-1)*c1 + 64*ceil(len1/64)] with sample b's keys at columns [b*c1, b*c1 + len1), c1 = cols1 (default
    v1t.shape[1] // batch; even, >= len1; every column finite); the same for segment 2.  Same arithmetic as `attention(..., k2=, v2=)`; K and V^T tiles by LDS-DMA."""
    for n, t in (("q", q), ("k1", k1), ("v1t", v1t), ("k2", k2), ("v2t", v2t)):
        _dev(t, torch.bfloat16, n)
    Nq, Dq, ldq = _rows(q, "q")
    _, _, ldk1 = _rows(k1, "k1")
    _, _, ldk2 = _rows(k2, "k2")
    assert Dq == heads * 128 and v1t.shape[0] == Dq and v2t.shape[0] == Dq and v1t.stride(1) == 1 and v2t.stride(1) == 1
    assert Nq % batch == 0 and k1.shape[0] == batch * len1 and k2.shape[0] == batch * len2
    if cols1 is None:  # column stride between samples: explicit, or the row length split evenly
        assert v1t.shape[1] % batch == 0
        cols1 = v1t.shape[1] // batch
    if cols2 is None:
        assert v2t.shape[1] % batch == 0
        cols2 = v2t.shape[1] // batch
    if scale is None:
        scale = 128 ** -0.5
    nq = Nq // batch
    if out8 is not None:  # the result as the MX fp8 operand of the out-projection (e4m3 rows + tiled E8M0 block scales): no bf16 output
        _dev(out8, torch.uint8, "out8"), _dev(scale8, torch.uint8, "scale8")
        _, D8, ld8 = _rows(out8, "out8")
        assert out8.shape[0] == Nq and D8 == Dq and scale8.is_contiguous() and scale8.numel() >= mx_scale_bytes(Nq, Dq)
        st = _prof_begin()
        _launch("ce_attention_2seg_vt_quant_bf16", _ptr(q), _ptr(k1), _ptr(v1t), len1, ldk1, v1t.stride(0), int(cols1), _ptr(k2), _ptr(v2t),
                len2, ldk2, v2t.stride(0), int(cols2), _ptr(out8), _ptr(scale8), nq, heads, 128, ldq, ld8,
                float(scale), batch, _stream())
        _prof_end(st, f"attention_{nq}x{len1}+{len2}_h{heads}" + (f"_b{batch}" if batch > 1 else "") + "_mxq",
                  4.0 * nq * (len1 + len2) * 128 * heads * batch)
        return out8
    if out is None:
        out = torch.empty((Nq, Dq), dtype=torch.bfloat16, device=q.device)
    _, _, ldo = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_attention_2seg_vt_bf16", _ptr(q), _ptr(k1), _ptr(v1t), len1, ldk1, v1t.stride(0), int(cols1), _ptr(k2), _ptr(v2t),
            len2, ldk2, v2t.stride(0), int(cols2), _ptr(out), nq, heads, 128, ldq, ldo,
            float(scale), batch, _stream())
    _prof_end(st, f"attention_{nq}x{len1}+{len2}_h{heads}" + (f"_b{batch}" if batch > 1 else ""), 4.0 * nq * (len1 + len2) * 128 * heads * batch)
    return out


def attention_2seg_vt_shared(q: torch.Tensor, k1: torch.Tensor, v1t: torch.Tensor, len1: int, k2: torch.Tensor, v2t: torch.Tensor, len2: int,
                             heads: int, out: torch.Tensor, batch: int, share_q: bool = False, share1: bool = False, share2: bool = False,
                             cols1: Optional[int] = None, cols2: Optional[int] = None, scale: Optional[float] = None):
    """`attention_2seg_vt` for `batch` samples of which some operands are ONE tensor for all samples (ce_attention_2seg_vt_strided_bf16):
    share_q: q is [nq, H*128] (else [batch*nq, ...]); share1 / share2: the segment's k is [len, H*128] and its v^T holds one sample's keys
    from column 0 (else stacked as in `attention_2seg_vt`, column stride cols).  out is [batch*nq, H*128], always per sample.  Bit-equal
    to `attention_2seg_vt` on physically duplicated operands."""
    for n, t in (("q", q), ("k1", k1), ("v1t", v1t), ("k2", k2), ("v2t", v2t), ("out", out)):
        _dev(t, torch.bfloat16, n)
    Nq, Dq, ldq = _rows(q, "q")
    _, _, ldk1 = _rows(k1, "k1")
    _, _, ldk2 = _rows(k2, "k2")
    No, Do, ldo = _rows(out, "out")
    nq = Nq if share_q else Nq // batch
    assert Dq == heads * 128 and Do == Dq and v1t.shape[0] == Dq and v2t.shape[0] == Dq and v1t.stride(1) == 1 and v2t.stride(1) == 1
    assert No == batch * nq and (share_q or Nq == batch * nq), (No, Nq, batch)
    assert k1.shape[0] == (1 if share1 else batch) * len1 and k2.shape[0] == (1 if share2 else batch) * len2
    pad = lambda n: (n + 63) // 64 * 64
    if cols1 is None:
        cols1 = 0 if share1 else v1t.shape[1] // batch
    if cols2 is None:
        cols2 = 0 if share2 else v2t.shape[1] // batch
    assert v1t.shape[1] >= (0 if share1 else (batch - 1) * cols1) + pad(len1) and v2t.shape[1] >= (0 if share2 else (batch - 1) * cols2) + pad(len2)
    if scale is None:
        scale = 128 ** -0.5
    st = _prof_begin()
    _launch("ce_attention_2seg_vt_strided_bf16", _ptr(q), _ptr(k1), _ptr(v1t), len1, ldk1, v1t.stride(0), int(cols1), _ptr(k2), _ptr(v2t),
            len2, ldk2, v2t.stride(0), int(cols2), _ptr(out), nq, heads, 128, ldq, ldo, float(scale), batch,
            0 if share_q else nq, 0 if share1 else len1, 0 if share2 else len2, _stream())
    tag = ("_sq" if share_q else "") + ("_s1" if share1 else "") + ("_s2" if share2 else "")
    _prof_end(st, f"attention_{nq}x{len1}+{len2}_h{heads}" + (f"_b{batch}" if batch > 1 else "") + tag, 4.0 * nq * (len1 + len2) * 128 * heads * batch)
    return out


def attention_2seg_vt_weighted(q: torch.Tensor, k1: torch.Tensor, v1t: torch.Tensor, len1: int, k2: torch.Tensor, v2t: torch.Tensor, len2: int,
                               heads: int, out: torch.Tensor, batch: int, valid1: torch.Tensor, w1: torch.Tensor, share_q: bool = False,
                               share2: bool = False, cols1: Optional[int] = None, cols2: Optional[int] = None, scale: Optional[float] = None):
    """`attention_2seg_vt_shared` with segment 1 cut and weighted per sample (ce_attention_2seg_vt_weighted_bf16): valid1 int32 [batch] on the
    device, 1 <= valid1[b] <= len1 - sample b attends its first valid1[b] keys of segment 1 (the kernel walks ceil(valid1[b] / 64) key tiles of
    it); w1 fp32 [batch] on the device - the log2 of how many times key valid1[b] - 1 counts in the softmax.  len1 is the row count of the
    operand as stored.  Neither array is read on the host.  valid1 = len1, w1 = 0: bit-equal to `attention_2seg_vt_shared`."""
    for n, t in (("q", q), ("k1", k1), ("v1t", v1t), ("k2", k2), ("v2t", v2t), ("out", out)):
        _dev(t, torch.bfloat16, n)
    _dev(valid1, torch.int32, "valid1"), _dev(w1, torch.float32, "w1")
    assert valid1.is_contiguous() and w1.is_contiguous() and valid1.numel() == batch and w1.numel() == batch
    Nq, Dq, ldq = _rows(q, "q")
    _, _, ldk1 = _rows(k1, "k1")
    _, _, ldk2 = _rows(k2, "k2")
    No, Do, ldo = _rows(out, "out")
    nq = Nq if share_q else Nq // batch
    assert Dq == heads * 128 and Do == Dq and v1t.shape[0] == Dq and v2t.shape[0] == Dq and v1t.stride(1) == 1 and v2t.stride(1) == 1
    assert No == batch * nq and (share_q or Nq == batch * nq), (No, Nq, batch)
    assert k1.shape[0] == batch * len1 and k2.shape[0] == (1 if share2 else batch) * len2
    pad = lambda n: (n + 63) // 64 * 64
    if cols1 is None:
        cols1 = v1t.shape[1] // batch
    if cols2 is None:
        cols2 = 0 if share2 else v2t.shape[1] // batch
    assert v1t.shape[1] >= (batch - 1) * cols1 + pad(len1) and v2t.shape[1] >= (0 if share2 else (batch - 1) * cols2) + pad(len2)
    if scale is None:
        scale = 128 ** -0.5
    st = _prof_begin()
    _launch("ce_attention_2seg_vt_weighted_bf16", _ptr(q), _ptr(k1), _ptr(v1t), len1, ldk1, v1t.stride(0), int(cols1), _ptr(k2), _ptr(v2t),
            len2, ldk2, v2t.stride(0), int(cols2), _ptr(out), nq, heads, 128, ldq, ldo, float(scale), batch,
            0 if share_q else nq, len1, 0 if share2 else len2, _ptr(valid1), _ptr(w1), _stream())
    tag = ("_sq" if share_q else "") + ("_s2" if share2 else "") + "_w"
    _prof_end(st, f"attention_{nq}x{len1}+{len2}_h{heads}" + (f"_b{batch}" if batch > 1 else "") + tag, 4.0 * nq * (len1 + len2) * 128 * heads * batch)
    return out


def v_transpose_blocked(v: torch.Tensor, heads: int, batch: int, blk_rows: int, n_keys: int, out: Optional[torch.Tensor] = None):
    """v [W * batch * blk_rows, heads*128] in the all-to-all receive layout ([source rank][sample][local token]) -> V^T
    [heads*128, batch * vt_sample_cols] plain per sample (`attention_vt_blocked`); n_keys = valid tokens per sample."""
    _dev(v, torch.bfloat16, "v")
    rows, D, ldv = _rows(v, "v")
    assert D == heads * 128 and blk_rows % 64 == 0 and rows % (batch * blk_rows) == 0
    cols = (n_keys + 63) // 64 * 64 + 64
    if out is None:
        out = torch.empty((D, batch * cols), dtype=torch.bfloat16, device=v.device)
    assert out.shape == (D, batch * cols) and out.is_contiguous()
    st = _prof_begin()
    _launch("ce_v_transpose_blocked_bf16", _ptr(v), ldv, _ptr(out), out.shape[1], n_keys, heads, batch, blk_rows, batch * blk_rows, cols,
            _stream())
    _prof_end(st, f"v_transpose_{batch * n_keys}x{D}", 4.0 * batch * n_keys * D)
    return out


def attention_vt_blocked(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, batch: int, blk_rows: int, n_keys: int,
                         out: Optional[torch.Tensor] = None, scale: Optional[float] = None):
    """`attention_vt` over the blocked row layout: q / k / out [W * batch * blk_rows, heads*128] with token g of sample b in row
    (g // blk_rows) * batch * blk_rows + b * blk_rows + g % blk_rows; vt from `v_transpose_blocked`; n_keys valid keys per sample."""
    for n, t in (("q", q), ("k", k), ("vt", vt)):
        _dev(t, torch.bfloat16, n)
    rows, Dq, ldq = _rows(q, "q")
    rk, _, ldk = _rows(k, "k")
    assert Dq == heads * 128 and vt.shape[0] == Dq and vt.stride(1) == 1 and rows == rk and rows % (batch * blk_rows) == 0
    nq = rows // batch  # query tokens per sample = W * blk_rows
    cols = vt.shape[1] // batch
    if out is None:
        out = torch.empty((rows, Dq), dtype=torch.bfloat16, device=q.device)
    _, _, ldo = _rows(out, "out")
    if scale is None:
        scale = 128 ** -0.5
    st = _prof_begin()
    _launch("ce_attention_vt_blocked_bf16", _ptr(q), _ptr(k), _ptr(vt), n_keys, ldk, vt.stride(0), _ptr(out), nq, heads, 128, ldq, ldo,
            float(scale), batch, blk_rows, batch * blk_rows, cols, _stream())
    _prof_end(st, f"attention_{nq}x{n_keys}+0_h{heads}" + (f"_b{batch}" if batch > 1 else ""), 4.0 * nq * n_keys * 128 * heads * batch)
    return out


def timestep_sinusoid(t: torch.Tensor, dim: int, out: Optional[torch.Tensor] = None):
    """[cos, sin] table of one timestep: int64 (diffusers path) or float32 (the sibling stacks' float timesteps)."""
    if t.dtype == torch.float32:
        _dev(t, torch.float32, "timestep")
    else:
        _dev(t, torch.int64, "timestep")
    if out is None:
        out = torch.empty((dim,), dtype=torch.float32, device=t.device)
    if t.dtype == torch.float32:
        _launch("ce_timestep_sinusoid_f32", _ptr(t), _ptr(out), dim, _stream())
    else:
        _launch("ce_timestep_sinusoid", _ptr(t), _ptr(out), dim, _stream())
    return out


def gemv(w: torch.Tensor, x: torch.Tensor, bias: Optional[torch.Tensor], flags: int = 0, out: Optional[torch.Tensor] = None):
    """y = post(w @ pre(x) + bias); x/y fp32, w fp32 or bf16 (see include/chronoedit_hip.h for flags)."""
    _dev(x, torch.float32, "x")
    assert w.is_cuda and w.dtype in (torch.float32, torch.bfloat16) and w.is_contiguous()
    N, K = w.shape
    assert x.numel() == K
    if bias is not None:
        _dev(bias, torch.float32, "bias")
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=x.device)
    _launch("ce_gemv", _ptr(w), int(w.dtype == torch.bfloat16), _ptr(x), _ptr(bias), _ptr(out), N, K, flags, _stream())
    return out


def modulation(table: torch.Tensor, v: torch.Tensor, one_mask: int, out: Optional[torch.Tensor] = None):
    """out[L,J,D] = table[L,J,D] + v[J or 1, D]  (+1 on rows in one_mask)."""
    _dev(table, torch.float32, "table"), _dev(v, torch.float32, "v")
    L, J, D = table.shape
    v_rows = v.numel() // D
    assert table.is_contiguous() and v.is_contiguous() and v_rows in (1, J)
    if out is None:
        out = torch.empty_like(table)
    _launch("ce_modulation", _ptr(table), _ptr(v), _ptr(out), L, J, D, v_rows, one_mask, _stream())
    return out


def patchify(x: torch.Tensor, kpad: int, out: Optional[torch.Tensor] = None, row0: int = 0, nrows: Optional[int] = None):
    """x [C,T,H,W] bf16 -> [T*(H/2)*(W/2), kpad]; (row0, nrows): only that range of token rows (zero rows past the last token)."""
    _dev(x, torch.bfloat16, "x")
    assert x.is_contiguous() and x.dim() == 4
    C, T, H, W = x.shape
    n = T * (H // 2) * (W // 2) if nrows is None else int(nrows)
    if out is None:
        out = torch.empty((n, kpad), dtype=torch.bfloat16, device=x.device)
    assert out.is_contiguous() and out.shape == (n, kpad)
    _launch("ce_patchify_rows_bf16", _ptr(x), _ptr(out), C, T, H, W, kpad, int(row0), n, _stream())
    return out


def unpatchify(y: torch.Tensor, cout: int, T: int, H: int, W: int, out: Optional[torch.Tensor] = None):
    _dev(y, torch.bfloat16, "y")
    _, _, ldy = _rows(y, "y")
    if out is None:
        out = torch.empty((cout, T, H, W), dtype=torch.bfloat16, device=y.device)
    _launch("ce_unpatchify_bf16", _ptr(y), _ptr(out), cout, T, H, W, ldy, _stream())
    return out


def cfg_unipc_step(v_cond: torch.Tensor, v_uncond: Optional[torch.Tensor], x: torch.Tensor, x_last: torch.Tensor, m0: torch.Tensor,
                   m1: torch.Tensor, coef: torch.Tensor, x0_out: Optional[torch.Tensor] = None, round_sigma_v: bool = True,
                   bf16_state: bool = False):
    """Fused CFG + flow-UniPC update, in place on (x, x_last, m0, m1).  coef = device float[10].  bf16_state: the stored
    latents / history carry bf16 values like the reference's bf16 tensors (fp32 storage)."""
    _dev(v_cond, torch.bfloat16, "v_cond")
    for n, t in (("x", x), ("x_last", x_last), ("m0", m0), ("m1", m1), ("coef", coef)):
        _dev(t, torch.float32, n)
        assert t.is_contiguous()
    if v_uncond is not None:
        _dev(v_uncond, torch.bfloat16, "v_uncond")
        assert v_uncond.is_contiguous()
    assert v_cond.is_contiguous() and coef.numel() >= 10
    n = x.numel()
    assert v_cond.numel() == n == x_last.numel() == m0.numel() == m1.numel()
    _launch("ce_cfg_unipc_step", _ptr(v_cond), _ptr(v_uncond), _ptr(x), _ptr(x_last), _ptr(m0), _ptr(m1), _ptr(x0_out), _ptr(coef),
            _ptr(None), n, int(round_sigma_v) | (2 if bf16_state else 0), _stream())
    return x


CFG_MAX_AGE = 4  # the largest ring ce_cfg_unipc_step_delta measures against (csrc/ce_sched.hip)


def cfg_unipc_step_delta(v_cond: torch.Tensor, v_uncond: Optional[torch.Tensor], x: torch.Tensor, x_last: torch.Tensor, m0: torch.Tensor,
                         m1: torch.Tensor, coef: torch.Tensor, delta: torch.Tensor, x0_out: Optional[torch.Tensor] = None,
                         round_sigma_v: bool = True, bf16_state: bool = False, slot: Optional[int] = None,
                         table: Optional[torch.Tensor] = None, row: int = 0):
    """cfg_unipc_step with the guidance direction d = bf16(c - u) kept in `delta` (bf16, contiguous).
    v_uncond given: STORE - the outputs of cfg_unipc_step bit for bit, and delta (n elements) <- d.
    v_uncond None: REUSE - delta is only read: u' = bf16(c - d), v = bf16(u' + bf16(g * d)), then as cfg_unipc_step.
    slot / table given (with v_uncond): MEASURE - delta is a ring [A, n] (A <= 4) whose slot `slot` receives d; before that the pass sums
    (d - ring[(slot - a) % A])^2 for a = 1..A and d^2 over all elements (fp32, fixed order) into table[row] (table fp32 [rows, A + 1])."""
    _dev(v_cond, torch.bfloat16, "v_cond"), _dev(delta, torch.bfloat16, "delta")
    for name, t in (("x", x), ("x_last", x_last), ("m0", m0), ("m1", m1), ("coef", coef)):
        _dev(t, torch.float32, name)
        assert t.is_contiguous()
    if v_uncond is not None:
        _dev(v_uncond, torch.bfloat16, "v_uncond")
        assert v_uncond.is_contiguous()
    assert v_cond.is_contiguous() and delta.is_contiguous() and coef.numel() >= 10
    n = x.numel()
    assert v_cond.numel() == n == x_last.numel() == m0.numel() == m1.numel()
    assert v_uncond is None or v_uncond.numel() == n
    assert x0_out is None or (x0_out.dtype == torch.float32 and x0_out.is_contiguous() and x0_out.numel() == n)
    flags = int(round_sigma_v) | (2 if bf16_state else 0)
    if slot is None and table is None:
        if delta.numel() != n:
            raise ValueError(f"delta: need {n} elements, got shape {tuple(delta.shape)}")
        _launch("ce_cfg_unipc_step_delta", _ptr(v_cond), _ptr(v_uncond), _ptr(x), _ptr(x_last), _ptr(m0), _ptr(m1), _ptr(x0_out), _ptr(coef),
                _ptr(delta), n, flags, 0, 0, _ptr(None), 0, _ptr(None), 0, _stream())
        return x
    if v_uncond is None or slot is None or table is None:
        raise ValueError("measuring is an option of the store mode: it needs v_uncond, slot and table")
    A = delta.shape[0]
    if delta.dim() < 2 or not 1 <= A <= CFG_MAX_AGE or delta.numel() != A * n:
        raise ValueError(f"delta: measuring needs a ring [A, {n}] with 1 <= A <= {CFG_MAX_AGE}, got shape {tuple(delta.shape)}")
    _dev(table, torch.float32, "table")
    if table.dim() != 2 or table.shape[1] != A + 1 or not table.is_contiguous() or not 0 <= int(row) < table.shape[0]:
        raise ValueError(f"table: need contiguous fp32 [rows, {A + 1}] with rows > row = {row}, got shape {tuple(table.shape)}")
    if not 0 <= int(slot) < A:
        raise ValueError(f"slot {slot} is outside the ring of {A}")
    scratch = torch.empty((CFG_MAX_AGE + 1) * 2048, dtype=torch.float32, device=x.device)  # five sums per workgroup, at most 2048 of them
    _launch("ce_cfg_unipc_step_delta", _ptr(v_cond), _ptr(v_uncond), _ptr(x), _ptr(x_last), _ptr(m0), _ptr(m1), _ptr(x0_out), _ptr(coef),
            _ptr(delta), n, flags, A, int(slot), _ptr(scratch), scratch.numel() * 4, _ptr(table), int(row), _stream())
    return x


# ---- TeaCache step skipping (csrc/ce_tea.hip) ------------------------------------------------------------------------
def tea_rel_l1(rows: torch.Tensor, out: Optional[torch.Tensor] = None):
    """rows bf16 [S, n] (one time-projection row per scheduled step) -> fp32 [S, 2]: per step i >= 1 the sums of |bf16(row_i - row_{i-1})|
    and of |row_{i-1}|; row 0 is zeros."""
    _dev(rows, torch.bfloat16, "rows")
    if rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError(f"rows: need a contiguous 2-D tensor, got shape {tuple(rows.shape)} stride {rows.stride()}")
    S, n = rows.shape
    if out is None:
        out = torch.empty((S, 2), dtype=torch.float32, device=rows.device)
    _dev(out, torch.float32, "out")
    assert out.is_contiguous() and out.shape == (S, 2)
    _launch("ce_tea_rel_l1_bf16", _ptr(rows), S, n, _ptr(out), _stream())
    return out


def _tea_pair(x: torch.Tensor, r: torch.Tensor):
    _dev(x, torch.bfloat16, "x"), _dev(r, torch.bfloat16, "r")
    if not (x.is_contiguous() and r.is_contiguous()) or x.numel() != r.numel():
        raise ValueError(f"x / r: need two contiguous tensors of one size, got {tuple(x.shape)} and {tuple(r.shape)}")
    return x.numel()


def tea_store_(x: torch.Tensor, r: torch.Tensor):
    """r <- bf16(x - r), in place: r enters as the tokens saved in front of the block stack and leaves as the stack's residual."""
    n = _tea_pair(x, r)
    st = _prof_begin()
    _launch("ce_tea_store_bf16", _ptr(x), _ptr(r), n, _stream())
    _prof_end(st, f"tea_store_{n}", 6.0 * n)
    return r


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    pa, pb = a.data_ptr(), b.data_ptr()
    return pa < pb + b.numel() * b.element_size() and pb < pa + a.numel() * a.element_size()


def tea_store_dist_(x: torch.Tensor, r: torch.Tensor, prev: torch.Tensor, sums: torch.Tensor):
    """tea_store_ (the same bits in r) that also measures the new residual against the previous step's: sums (fp32 [2]) receives
    sum |r_new - prev| and sum |prev| over all elements, accumulated in fp32 in a fixed order.  prev is only read and overlaps neither r nor x."""
    n = _tea_pair(x, r)
    _dev(prev, torch.bfloat16, "prev"), _dev(sums, torch.float32, "sums")
    if not prev.is_contiguous() or prev.numel() != n:
        raise ValueError(f"prev: need a contiguous tensor of the size of x / r, got {tuple(prev.shape)} for {n} elements")
    if not sums.is_contiguous() or sums.numel() != 2:
        raise ValueError(f"sums: need two contiguous fp32 elements, got shape {tuple(sums.shape)} stride {sums.stride()}")
    if _overlap(prev, r) or _overlap(prev, x):
        raise ValueError("prev: the previous residual must not alias r or x (it is read after r has been written)")
    scratch = torch.empty(2 * 2048, dtype=torch.float32, device=x.device)  # one pair per workgroup, at most 2048 of them (csrc/ce_tea.hip)
    st = _prof_begin()
    _launch("ce_tea_store_dist_bf16", _ptr(x), _ptr(r), _ptr(prev), _ptr(sums), _ptr(scratch), scratch.numel() * 4, n, _stream())
    _prof_end(st, f"tea_store_dist_{n}", 8.0 * n)
    return r


def tea_apply_(x: torch.Tensor, r: torch.Tensor):
    """x <- bf16(x + r), in place: the cached residual added to the patch-embedded tokens of a skipped step."""
    n = _tea_pair(x, r)
    st = _prof_begin()
    _launch("ce_tea_apply_bf16", _ptr(x), _ptr(r), n, _stream())
    _prof_end(st, f"tea_apply_{n}", 6.0 * n)
    return x


# ---- image pre- / post-processing (csrc/ce_image.hip) ------------------------------------------------------------------
def image_resample_u8(src: torch.Tensor, axis: int, coeff: torch.Tensor, bounds: torch.Tensor, out: Optional[torch.Tensor] = None):
    """One 1-D pass of PIL's 8-bit resampler: src uint8 [H, W, 3] -> [H, out, 3] (axis 0, horizontal) or [out, W, 3] (axis 1, vertical),
    with coeff int32 [out, ksize] (22-bit fixed point) and bounds int32 [out, 2] = (first, count) on the device."""
    _dev(src, torch.uint8, "src"), _dev(coeff, torch.int32, "coeff"), _dev(bounds, torch.int32, "bounds")
    if src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise ValueError(f"src: need a contiguous [H, W, 3] tensor, got shape {tuple(src.shape)} stride {src.stride()}")
    if axis not in (0, 1):
        raise ValueError(f"axis: 0 (horizontal) or 1 (vertical), got {axis}")
    H, W, _ = src.shape
    n, ksize = coeff.shape
    if not (coeff.is_contiguous() and bounds.is_contiguous()) or bounds.shape != (n, 2):
        raise ValueError(f"coeff / bounds: need contiguous [out, ksize] and [out, 2], got {tuple(coeff.shape)} and {tuple(bounds.shape)}")
    shape = (H, n, 3) if axis == 0 else (n, W, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and tuple(out.shape) == shape and out.data_ptr() != src.data_ptr()
    st = _prof_begin()
    _launch("ce_image_resample_u8", _ptr(src), _ptr(out), axis, H, W, n, _ptr(coeff), _ptr(bounds), ksize, _stream())
    _prof_end(st, f"image_resample_{'hv'[axis]}_{H}x{W}_{n}", float(src.numel() + out.numel()))
    return out


def image_u8_lut_planar(src: torch.Tensor, lut: torch.Tensor, out: torch.Tensor, top: int = 0, left: int = 0):
    """out[c, y, x] = lut[c, src[top + y, left + x, c]]: src uint8 [H, W, 3], lut [3, 256] and out [3, h, w] both bf16 or both fp32."""
    _dev(src, torch.uint8, "src")
    if lut.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"lut: expected bfloat16 or float32, got {lut.dtype}")
    _dev(lut, lut.dtype, "lut"), _dev(out, lut.dtype, "out")
    if src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise ValueError(f"src: need a contiguous [H, W, 3] tensor, got shape {tuple(src.shape)} stride {src.stride()}")
    if tuple(lut.shape) != (3, 256) or not lut.is_contiguous():
        raise ValueError(f"lut: need a contiguous [3, 256] table, got {tuple(lut.shape)}")
    if out.dim() != 3 or out.shape[0] != 3 or not out.is_contiguous():
        raise ValueError(f"out: need a contiguous [3, h, w] tensor, got shape {tuple(out.shape)} stride {out.stride()}")
    H, W, _ = src.shape
    h, w = out.shape[1:]
    if top < 0 or left < 0 or top + h > H or left + w > W:
        raise ValueError(f"the {h}x{w} crop at ({top}, {left}) does not lie inside the {H}x{W} source")
    st = _prof_begin()
    _launch("ce_image_u8_lut_planar", _ptr(src), H, W, int(top), int(left), h, w, _ptr(lut), _ptr(out), int(lut.dtype == torch.float32), _stream())
    _prof_end(st, f"image_lut_{h}x{w}", float(3 * h * w * (1 + out.element_size())))
    return out


def video_to_u8(video: torch.Tensor, out: Optional[torch.Tensor] = None):
    """[B, 3, F, H, W] bf16 / fp32 in [-1, 1] -> uint8 [B, F, H, W, 3]: rint(clamp(v * 0.5 + 0.5, 0, 1) * 255), every operation rounded in fp32."""
    if video.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"video: expected bfloat16 or float32, got {video.dtype}")
    _dev(video, video.dtype, "video")
    if video.dim() != 5 or video.shape[1] != 3 or not video.is_contiguous():
        raise ValueError(f"video: need a contiguous [B, 3, F, H, W] tensor, got shape {tuple(video.shape)} stride {video.stride()}")
    B, _, F, H, W = video.shape
    if out is None:
        out = torch.empty((B, F, H, W, 3), dtype=torch.uint8, device=video.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and tuple(out.shape) == (B, F, H, W, 3)
    st = _prof_begin()
    _launch("ce_video_to_u8", _ptr(video), _ptr(out), B, F, H, W, int(video.dtype == torch.float32), _stream())
    _prof_end(st, f"video_to_u8_{B}x{F}x{H}x{W}", float(video.numel() * (video.element_size() + 1)))
    return out


# ---- region-limited edits (csrc/ce_region.hip) -------------------------------------------------------------------------
def region_weights_u8(mask: torch.Tensor, out: Optional[torch.Tensor] = None):
    """uint8 mask [H, W] (H, W multiples of 8) -> fp32 [H / 8, W / 8]: float(sum of the 64 bytes of a tile) / 16320, the 8x8 box mean."""
    _dev(mask, torch.uint8, "mask")
    if mask.dim() != 2 or not mask.is_contiguous():
        raise ValueError(f"mask: need a contiguous [H, W] tensor, got shape {tuple(mask.shape)} stride {mask.stride()}")
    H, W = mask.shape
    if out is None:
        out = torch.empty((H // 8, W // 8), dtype=torch.float32, device=mask.device)
    _dev(out, torch.float32, "out")
    assert out.is_contiguous() and out.numel() == (H // 8) * (W // 8)
    st = _prof_begin()
    _launch("ce_region_weights_u8", _ptr(mask), _ptr(out), H, W, _stream())
    _prof_end(st, f"region_weights_{H}x{W}", float(mask.numel() + 4 * out.numel()))
    return out


def region_blend_(x: torch.Tensor, z_src: torch.Tensor, eps: torch.Tensor, w: torch.Tensor, sigma_next: torch.Tensor, bf16_state: bool = False):
    """In place on x (fp32, [..., h, w]): k = (1 - s) * z_src + s * eps, x = w * x + (1 - w) * k, every operation rounded in fp32; s is the
    ONE fp32 element of the device tensor sigma_next, read by the kernel; w = fp32 [h, w], broadcast over the leading axes.
    bf16_state: x is rounded to a bf16 value (fp32 storage), as cfg_unipc_step's."""
    for name, t in (("x", x), ("z_src", z_src), ("eps", eps), ("w", w), ("sigma_next", sigma_next)):
        _dev(t, torch.float32, name)
        if not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous tensor, got shape {tuple(t.shape)} stride {t.stride()}")
    n, plane = x.numel(), w.numel()
    if z_src.numel() != n or eps.numel() != n or sigma_next.numel() != 1:
        raise ValueError(f"z_src / eps: need {n} elements each and ONE sigma, got {z_src.numel()}, {eps.numel()} and {sigma_next.numel()}")
    if w.dim() != 2 or x.dim() < 2 or tuple(x.shape[-2:]) != tuple(w.shape):
        raise ValueError(f"w: need [h, w] = the last two axes of x {tuple(x.shape)}, got {tuple(w.shape)}")
    st = _prof_begin()
    _launch("ce_region_blend_f32", _ptr(x), _ptr(z_src), _ptr(eps), _ptr(w), _ptr(sigma_next), n, plane, 2 if bf16_state else 0, _stream())
    _prof_end(st, f"region_blend_{n}", 16.0 * n)
    return x


def region_composite(video: torch.Tensor, src: torch.Tensor, mask: torch.Tensor, out: Optional[torch.Tensor] = None):
    """video [B, 3, F, H, W] bf16 / fp32, src bf16 [B, 3, H, W], mask uint8 [H, W] -> a NEW fp32 video: m = float(mask) / 255,
    out = m * video + (1 - m) * src, every operation rounded in fp32; mask and source broadcast over the frames."""
    if video.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"video: expected bfloat16 or float32, got {video.dtype}")
    _dev(video, video.dtype, "video"), _dev(src, torch.bfloat16, "src"), _dev(mask, torch.uint8, "mask")
    if video.dim() != 5 or video.shape[1] != 3 or not video.is_contiguous():
        raise ValueError(f"video: need a contiguous [B, 3, F, H, W] tensor, got shape {tuple(video.shape)} stride {video.stride()}")
    B, _, F, H, W = video.shape
    if tuple(src.shape) != (B, 3, H, W) or not src.is_contiguous():
        raise ValueError(f"src: need a contiguous [{B}, 3, {H}, {W}] tensor, got shape {tuple(src.shape)} stride {src.stride()}")
    if tuple(mask.shape) != (H, W) or not mask.is_contiguous():
        raise ValueError(f"mask: need a contiguous [{H}, {W}] tensor, got shape {tuple(mask.shape)} stride {mask.stride()}")
    if out is None:
        out = torch.empty(video.shape, dtype=torch.float32, device=video.device)
    _dev(out, torch.float32, "out")
    assert out.is_contiguous() and out.shape == video.shape and out.data_ptr() != video.data_ptr()
    st = _prof_begin()
    _launch("ce_region_composite", _ptr(video), int(video.dtype == torch.bfloat16), _ptr(src), _ptr(mask), _ptr(out), B, F, H, W, _stream())
    _prof_end(st, f"region_composite_{B}x{F}x{H}x{W}", float(video.numel() * (video.element_size() + 4) + src.numel() * 2 + mask.numel()))
    return out


# ---- focused region edits (csrc/ce_focus.hip) ---------------------------------------------------------------------------
def focus_resample_l8(src: torch.Tensor, axis: int, coeff: torch.Tensor, bounds: torch.Tensor, out: Optional[torch.Tensor] = None):
    """One 1-D pass of PIL's 8-bit resampler over single-channel bytes: src uint8 [H, W] with unit inner stride and ANY row stride >= W (a
    crop of a larger mask is a view, not a copy) -> a contiguous [H, out] (axis 0, horizontal) or [out, W] (axis 1, vertical); coeff and
    bounds as image_resample_u8 takes them."""
    _dev(src, torch.uint8, "src"), _dev(coeff, torch.int32, "coeff"), _dev(bounds, torch.int32, "bounds")
    if src.dim() != 2 or src.stride(1) != 1 or src.stride(0) < src.shape[1]:
        raise ValueError(f"src: need an [H, W] tensor with unit inner stride and a row stride >= W, got shape {tuple(src.shape)} stride {src.stride()}")
    if axis not in (0, 1):
        raise ValueError(f"axis: 0 (horizontal) or 1 (vertical), got {axis}")
    H, W = src.shape
    n, ksize = coeff.shape
    if not (coeff.is_contiguous() and bounds.is_contiguous()) or bounds.shape != (n, 2):
        raise ValueError(f"coeff / bounds: need contiguous [out, ksize] and [out, 2], got {tuple(coeff.shape)} and {tuple(bounds.shape)}")
    shape = (H, n) if axis == 0 else (n, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and tuple(out.shape) == shape and out.data_ptr() != src.data_ptr()
    st = _prof_begin()
    _launch("ce_focus_resample_l8", _ptr(src), src.stride(0), _ptr(out), axis, H, W, n, _ptr(coeff), _ptr(bounds), ksize, _stream())
    _prof_end(st, f"focus_resample_{'hv'[axis]}_{H}x{W}_{n}", float(src.numel() + out.numel()))
    return out


def focus_paste_u8(edit: torch.Tensor, src: torch.Tensor, mask: Optional[torch.Tensor], left: int, top: int, out: Optional[torch.Tensor] = None):
    """Image.paste(edit[f], (left, top), mask) into a copy of src, for every frame: edit uint8 [F, bh, bw, 3], src uint8 [SH, SW, 3], mask
    uint8 [SH, SW] at the SOURCE's size or None (the whole box is replaced) -> a new uint8 [F, SH, SW, 3]."""
    _dev(edit, torch.uint8, "edit"), _dev(src, torch.uint8, "src")
    if edit.dim() != 4 or edit.shape[3] != 3 or not edit.is_contiguous():
        raise ValueError(f"edit: need a contiguous [F, bh, bw, 3] tensor, got shape {tuple(edit.shape)} stride {edit.stride()}")
    if src.dim() != 3 or src.shape[2] != 3 or not src.is_contiguous():
        raise ValueError(f"src: need a contiguous [SH, SW, 3] tensor, got shape {tuple(src.shape)} stride {src.stride()}")
    F, bh, bw, _ = edit.shape
    SH, SW, _ = src.shape
    if mask is not None:
        _dev(mask, torch.uint8, "mask")
        if tuple(mask.shape) != (SH, SW) or not mask.is_contiguous():
            raise ValueError(f"mask: need a contiguous [{SH}, {SW}] tensor, got shape {tuple(mask.shape)} stride {mask.stride()}")
    if left < 0 or top < 0 or left + bw > SW or top + bh > SH:
        raise ValueError(f"the {bw}x{bh} box at ({left}, {top}) does not lie inside the {SW}x{SH} source")
    if out is None:
        out = torch.empty((F, SH, SW, 3), dtype=torch.uint8, device=src.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and tuple(out.shape) == (F, SH, SW, 3) and out.data_ptr() not in (edit.data_ptr(), src.data_ptr())
    st = _prof_begin()
    _launch("ce_focus_paste_u8", _ptr(edit), _ptr(src), _ptr(mask), _ptr(out), F, SH, SW, int(left), int(top), bw, bh, _stream())
    _prof_end(st, f"focus_paste_{F}x{SH}x{SW}", float(out.numel() + src.numel() + edit.numel()))
    return out


# ---- auto-focused edits (csrc/ce_autofocus.hip) -------------------------------------------------------------------------
def autofocus_bbox_u8(mask: torch.Tensor, out: Optional[torch.Tensor] = None):
    """mask uint8 [H, W] with unit inner stride and ANY row stride >= W (a box's view of a larger mask is reduced where it lies) -> int32
    [5] on the device: left, top, right, bottom (half open) of mask > 0 and the count of non-zero bytes; W, H, 0, 0, 0 for an empty mask.
    `out` needs no initialisation.  Nothing is read back here."""
    _dev(mask, torch.uint8, "mask")
    if mask.dim() != 2 or mask.stride(1) != 1 or mask.stride(0) < mask.shape[1] or mask.numel() == 0:
        raise ValueError(f"mask: need a non-empty [H, W] tensor with unit inner stride and a row stride >= W, got shape {tuple(mask.shape)} stride {mask.stride()}")
    if out is None:
        out = torch.empty(5, dtype=torch.int32, device=mask.device)
    _dev(out, torch.int32, "out")
    assert out.is_contiguous() and out.numel() == 5
    H, W = mask.shape
    st = _prof_begin()
    _launch("ce_autofocus_bbox_u8", _ptr(mask), mask.stride(0), H, W, _ptr(out), _stream())
    _prof_end(st, f"autofocus_bbox_{H}x{W}", float(mask.numel()))
    return out


def autofocus_restart(x0: torch.Tensor, eps: torch.Tensor, tables, s: float, bf16_state: bool = False, out: Optional[torch.Tensor] = None):
    """x0, eps fp32 [..., h, w] of one shape, tables = (ix0, ix1, fx, iy0, iy1, fy) on the device (int32 [w], int32 [w], fp32 [w], int32 [h],
    int32 [h], fp32 [h]: autofocus.restart_tables) -> a new fp32 tensor (1 - s) * R(x0) + s * eps, R the bilinear sample through the
    tables, every operation rounded in fp32; bf16_state: rounded to a bf16 value (fp32 storage).  One launch, no host read."""
    _f32c(x0, "x0"), _f32c(eps, "eps")
    if x0.dim() < 2 or tuple(eps.shape) != tuple(x0.shape) or x0.numel() == 0:
        raise ValueError(f"x0 / eps: need two non-empty [..., h, w] tensors of one shape, got {tuple(x0.shape)} and {tuple(eps.shape)}")
    h, w = x0.shape[-2:]
    ix0, ix1, fx, iy0, iy1, fy = tables
    for name, t, dt, n in (("ix0", ix0, torch.int32, w), ("ix1", ix1, torch.int32, w), ("fx", fx, torch.float32, w),
                           ("iy0", iy0, torch.int32, h), ("iy1", iy1, torch.int32, h), ("fy", fy, torch.float32, h)):
        _dev(t, dt, name)
        if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous [{n}] table, got shape {tuple(t.shape)} stride {t.stride()}")
    if out is None:
        out = torch.empty_like(x0)
    _f32c(out, "out")
    assert out.shape == x0.shape and out.data_ptr() != x0.data_ptr()
    st = _prof_begin()
    _launch("ce_autofocus_restart_f32", _ptr(x0), _ptr(eps), _ptr(out), _ptr(ix0), _ptr(ix1), _ptr(fx), _ptr(iy0), _ptr(iy1), _ptr(fy), float(s),
            x0.numel() // (h * w), h, w, int(bool(bf16_state)), _stream())
    _prof_end(st, f"autofocus_restart_{x0.numel()}", 12.0 * x0.numel())
    return out


# ---- sketch edits (csrc/ce_sketch.hip) -----------------------------------------------------------------------------------
def _plane(t: torch.Tensor, name: str):
    _dev(t, torch.uint8, name)
    if t.dim() != 2 or not t.is_contiguous() or t.numel() == 0:
        raise ValueError(f"{name}: need a non-empty contiguous [H, W] tensor, got shape {tuple(t.shape)} stride {t.stride()}")


def sketch_changed_u8(background: torch.Tensor, composite: torch.Tensor, threshold: int = 0, out: Optional[torch.Tensor] = None):
    """background, composite uint8 [SH, SW, 3] -> a new uint8 [SH, SW]: 255 where max over the channels of |composite - background| >
    threshold (0..254), else 0."""
    _dev(background, torch.uint8, "background"), _dev(composite, torch.uint8, "composite")
    for name, t in (("background", background), ("composite", composite)):
        if t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous() or t.numel() == 0:
            raise ValueError(f"{name}: need a non-empty contiguous [SH, SW, 3] tensor, got shape {tuple(t.shape)} stride {t.stride()}")
    if background.shape != composite.shape:
        raise ValueError(f"background {tuple(background.shape)} and composite {tuple(composite.shape)} differ in shape")
    if isinstance(threshold, bool) or not 0 <= int(threshold) <= 254:
        raise ValueError(f"threshold: an int in 0..254, got {threshold!r}")
    SH, SW, _ = background.shape
    if out is None:
        out = torch.empty((SH, SW), dtype=torch.uint8, device=background.device)
    _plane(out, "out")
    assert tuple(out.shape) == (SH, SW) and out.data_ptr() not in (background.data_ptr(), composite.data_ptr())
    st = _prof_begin()
    _launch("ce_sketch_changed_u8", _ptr(background), _ptr(composite), _ptr(out), SH * SW, int(threshold), _stream())
    _prof_end(st, f"sketch_changed_{SH}x{SW}", 7.0 * SH * SW)
    return out


def sketch_scratch_bytes(H: int, W: int, axis: int, radius: int) -> int:
    """The scratch a `sketch_dilate_u8` / `sketch_box_u8` call needs: the per-segment sums uint16 [ceil(H / 32), W] of a vertical pass whose
    window holds more than 128 rows; 0 otherwise."""
    return (H + 31) // 32 * W * 2 if axis == 1 and int(radius) >= 64 else 0


def _sketch_filter(fn_name: str, src: torch.Tensor, axis: int, radius: int, out: Optional[torch.Tensor], scratch: Optional[torch.Tensor]):
    _plane(src, "src")
    if axis not in (0, 1):
        raise ValueError(f"axis: 0 (horizontal) or 1 (vertical), got {axis}")
    if out is None:
        out = torch.empty_like(src)
    _plane(out, "out")
    assert out.shape == src.shape and out.data_ptr() != src.data_ptr()
    H, W = src.shape
    need = sketch_scratch_bytes(H, W, axis, radius)
    if scratch is None and need:
        scratch = torch.empty(need, dtype=torch.uint8, device=src.device)
    if scratch is not None:
        _dev(scratch, torch.uint8, "scratch")
        assert scratch.is_contiguous()
    st = _prof_begin()
    _launch(fn_name, _ptr(src), _ptr(out), H, W, int(axis), int(radius), _ptr(scratch), 0 if scratch is None else scratch.numel(), _stream())
    _prof_end(st, f"{fn_name[3:-3]}_{'hv'[axis]}_{H}x{W}_r{int(radius)}", 2.0 * src.numel())
    return out


def sketch_dilate_u8(src: torch.Tensor, axis: int, radius: int, out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """One axis (0: horizontal, 1: vertical) of the maximum filter of a 0 / 255 plane uint8 [H, W], window [i - radius, i + radius] clipped to
    the image, radius 0..4096 -> a new plane: 255 where the window holds a non-zero byte, else 0.  scratch: uint8, at least
    `sketch_scratch_bytes` (made here when not given)."""
    return _sketch_filter("ce_sketch_dilate_u8", src, axis, radius, out, scratch)


def sketch_box_u8(src: torch.Tensor, axis: int, radius: int, out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """One axis of PIL's BoxBlur(radius) for an integer radius 0..1024 over uint8 [H, W], edges replicated -> a new plane:
    (window sum * (2^24 // (2 radius + 1)) + 2^23) >> 24."""
    return _sketch_filter("ce_sketch_box_u8", src, axis, radius, out, scratch)


# ---- connected components (csrc/ce_components.hip) ------------------------------------------------------------------------
def _iplane(t: torch.Tensor, name: str, shape):
    _dev(t, torch.int32, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name}: need a contiguous int32 {list(shape)} tensor, got shape {tuple(t.shape)} stride {t.stride()}")


def components_scratch_bytes(H: int, W: int) -> int:
    """The scratch of one `components.filter` on the device: the label plane and the sums plane int32 [H, W], and 16 bytes of counters."""
    return 8 * int(H) * int(W) + 16


def components_roots_i32(plane: torch.Tensor, out: Optional[torch.Tensor] = None):
    """plane uint8 [H, W] -> int32 [H, W]: the smallest index y * W + x of the pixel's 8-connected component of non-zero bytes, -1 for a
    zero byte.  `out` needs no initialisation."""
    _plane(plane, "plane")
    H, W = plane.shape
    if H * W >= 1 << 31:
        raise ValueError(f"plane: need H * W < 2^31, got {H} x {W}")
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=plane.device)
    _iplane(out, "out", (H, W))
    st = _prof_begin()
    _launch("ce_components_roots_i32", _ptr(plane), _ptr(out), H, W, _stream())
    _prof_end(st, f"components_roots_{H}x{W}", 13.0 * H * W)
    return out


def components_sums_i32(roots: torch.Tensor, weight: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """roots int32 [H, W] (+ weight uint8 [H, W]; None: every pixel counts) -> int32 [H, W]: at a root's own position the number of its
    component's pixels with a non-zero weight byte, 0 elsewhere."""
    if roots.dim() != 2 or roots.numel() == 0:
        raise ValueError(f"roots: need a non-empty [H, W] tensor, got shape {tuple(roots.shape)}")
    H, W = roots.shape
    _iplane(roots, "roots", (H, W))
    if weight is not None:
        _plane(weight, "weight")
        if tuple(weight.shape) != (H, W):
            raise ValueError(f"weight: need shape {(H, W)}, got {tuple(weight.shape)}")
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=roots.device)
    _iplane(out, "out", (H, W))
    assert out.data_ptr() != roots.data_ptr()
    st = _prof_begin()
    _launch("ce_components_sums_i32", _ptr(roots), _ptr(weight), _ptr(out), H, W, _stream())
    _prof_end(st, f"components_sums_{H}x{W}", 9.0 * H * W)
    return out


def components_keep_u8(plane: torch.Tensor, roots: torch.Tensor, sums: torch.Tensor, min_weight: int, num: int = 0, den: int = 0,
                       out: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None):
    """-> (out uint8 [H, W], counters int32 [4]): plane where the component's weight is >= the least weight kept - min_weight (den == 0), or
    ceil(num * the largest weight / den), taken on the device -, else 0; counters = components kept, dropped, weight dropped, largest."""
    _plane(plane, "plane")
    H, W = plane.shape
    _iplane(roots, "roots", (H, W)), _iplane(sums, "sums", (H, W))
    if out is None:
        out = torch.empty_like(plane)
    _plane(out, "out")
    assert out.shape == plane.shape and out.data_ptr() != plane.data_ptr()
    if counters is None:
        counters = torch.empty(4, dtype=torch.int32, device=plane.device)
    _iplane(counters, "counters", (4,))
    if not ((den == 0 and min_weight >= 1) or (0 < num < den <= 65536)):
        raise ValueError(f"need min_weight >= 1, or a fraction 0 < num / den < 1 with den <= 65536, got {min_weight}, {num} / {den}")
    st = _prof_begin()
    _launch("ce_components_keep_u8", _ptr(plane), _ptr(roots), _ptr(sums), _ptr(out), _ptr(counters), int(min_weight), int(num), int(den), H, W,
            _stream())
    _prof_end(st, f"components_keep_{H}x{W}", 14.0 * H * W)
    return out, counters


def components_seeds(d: torch.Tensor, thr: torch.Tensor, out: Optional[torch.Tensor] = None):
    """d fp32 [h, w], thr one fp32 element on the device -> uint8 [h, w]: 255 where d > thr, else 0."""
    _f32c(d, "d"), _f32c(thr, "thr")
    if d.dim() != 2 or d.numel() == 0 or thr.numel() != 1:
        raise ValueError(f"need d [h, w] and one threshold, got {tuple(d.shape)} and {tuple(thr.shape)}")
    if out is None:
        out = torch.empty(tuple(d.shape), dtype=torch.uint8, device=d.device)
    _plane(out, "out")
    assert out.shape == d.shape
    _launch("ce_components_seeds_f32", _ptr(d), _ptr(thr), _ptr(out), d.numel(), _stream())
    return out


def components_masked(d: torch.Tensor, kept: torch.Tensor, out: Optional[torch.Tensor] = None):
    """d fp32 [h, w], kept uint8 [h, w] -> a new fp32 [h, w]: d where kept is non-zero, else -1."""
    _f32c(d, "d"), _plane(kept, "kept")
    if d.shape != kept.shape:
        raise ValueError(f"d {tuple(d.shape)} and kept {tuple(kept.shape)} differ in shape")
    if out is None:
        out = torch.empty_like(d)
    _f32c(out, "out")
    assert out.shape == d.shape and out.data_ptr() != d.data_ptr()
    _launch("ce_components_masked_f32", _ptr(d), _ptr(kept), _ptr(out), d.numel(), _stream())
    return out


# ---- one crop per group of stroke clusters (csrc/ce_clusters.hip) ---------------------------------------------------------
CLUSTERS_ROWS = 256  # rows of the cluster table (CL_ROWS of csrc/ce_clusters.hip)


def clusters_table_i32(roots: torch.Tensor, sums: torch.Tensor, kept: torch.Tensor, table: Optional[torch.Tensor] = None,
                       counters: Optional[torch.Tensor] = None):
    """roots, sums int32 [H, W], kept uint8 [H, W] -> (table int32 [256, 8], counters int32 [257]): one row per kept cluster in ascending
    label order (label, left, top, right, bottom, pixels, weight, 0), rows at and after the count 0; counters[0] = the exact number of kept
    clusters (the rest is scratch).  Neither needs initialisation; nothing is read back here."""
    if roots.dim() != 2 or roots.numel() == 0:
        raise ValueError(f"roots: need a non-empty [H, W] tensor, got shape {tuple(roots.shape)}")
    H, W = roots.shape
    _iplane(roots, "roots", (H, W)), _iplane(sums, "sums", (H, W)), _plane(kept, "kept")
    if tuple(kept.shape) != (H, W):
        raise ValueError(f"kept: need shape {(H, W)}, got {tuple(kept.shape)}")
    if H * W >= 1 << 31:
        raise ValueError(f"roots: need H * W < 2^31, got {H} x {W}")
    if table is None:
        table = torch.empty((CLUSTERS_ROWS, 8), dtype=torch.int32, device=roots.device)
    if counters is None:
        counters = torch.empty(1 + CLUSTERS_ROWS, dtype=torch.int32, device=roots.device)
    _iplane(table, "table", (CLUSTERS_ROWS, 8)), _iplane(counters, "counters", (1 + CLUSTERS_ROWS,))
    st = _prof_begin()
    _launch("ce_clusters_table_i32", _ptr(roots), _ptr(sums), _ptr(kept), _ptr(table), _ptr(counters), CLUSTERS_ROWS, H, W, _stream())
    _prof_end(st, f"clusters_table_{H}x{W}", 10.0 * H * W)
    return table, counters


def clusters_select_u8(roots: torch.Tensor, kept: torch.Tensor, table: torch.Tensor, group_of_row: torch.Tensor, g: int,
                       out: Optional[torch.Tensor] = None):
    """-> a new uint8 [H, W]: 255 where kept is non-zero and the pixel's root is the label of a row i of `table` with group_of_row[i] == g
    (int32 [256] on the device), else 0."""
    if roots.dim() != 2 or roots.numel() == 0:
        raise ValueError(f"roots: need a non-empty [H, W] tensor, got shape {tuple(roots.shape)}")
    H, W = roots.shape
    _iplane(roots, "roots", (H, W)), _plane(kept, "kept")
    _iplane(table, "table", (CLUSTERS_ROWS, 8)), _iplane(group_of_row, "group_of_row", (CLUSTERS_ROWS,))
    if tuple(kept.shape) != (H, W):
        raise ValueError(f"kept: need shape {(H, W)}, got {tuple(kept.shape)}")
    if isinstance(g, bool) or int(g) < 0:
        raise ValueError(f"g: a group index >= 0, got {g!r}")
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=roots.device)
    _plane(out, "out")
    assert tuple(out.shape) == (H, W) and out.data_ptr() != kept.data_ptr()
    st = _prof_begin()
    _launch("ce_clusters_select_u8", _ptr(roots), _ptr(kept), _ptr(table), _ptr(group_of_row), int(g), _ptr(out), H, W, _stream())
    _prof_end(st, f"clusters_select_{H}x{W}", 6.0 * H * W)
    return out


def clusters_paste_u8(edit: torch.Tensor, mask: Optional[torch.Tensor], canvas: torch.Tensor, left: int, top: int):
    """Image.paste(edit[f], (left, top), mask) into canvas[f] IN PLACE, for every frame: edit uint8 [F, bh, bw, 3], canvas uint8 [F, SH, SW, 3],
    mask uint8 [SH, SW] at the photo's size or None (the whole box is replaced) -> canvas.  Only the box's bytes are touched."""
    _dev(edit, torch.uint8, "edit"), _dev(canvas, torch.uint8, "canvas")
    if edit.dim() != 4 or edit.shape[3] != 3 or not edit.is_contiguous() or edit.numel() == 0:
        raise ValueError(f"edit: need a non-empty contiguous [F, bh, bw, 3] tensor, got shape {tuple(edit.shape)} stride {edit.stride()}")
    if canvas.dim() != 4 or canvas.shape[3] != 3 or not canvas.is_contiguous() or canvas.shape[0] != edit.shape[0]:
        raise ValueError(f"canvas: need a contiguous [{edit.shape[0]}, SH, SW, 3] tensor, got shape {tuple(canvas.shape)} stride {canvas.stride()}")
    F, bh, bw, _ = edit.shape
    _, SH, SW, _ = canvas.shape
    if mask is not None:
        _dev(mask, torch.uint8, "mask")
        if tuple(mask.shape) != (SH, SW) or not mask.is_contiguous():
            raise ValueError(f"mask: need a contiguous [{SH}, {SW}] tensor, got shape {tuple(mask.shape)} stride {mask.stride()}")
    if left < 0 or top < 0 or left + bw > SW or top + bh > SH:
        raise ValueError(f"the {bw}x{bh} box at ({left}, {top}) does not lie inside the {SW}x{SH} canvas")
    assert canvas.data_ptr() != edit.data_ptr()
    st = _prof_begin()
    _launch("ce_clusters_paste_u8", _ptr(edit), _ptr(mask), _ptr(canvas), F, SH, SW, int(left), int(top), bw, bh, _stream())
    _prof_end(st, f"clusters_paste_{F}x{bh}x{bw}", 7.0 * F * bh * bw)
    return canvas


# ---- sketch edits from an editor's layers (csrc/ce_layers.hip) -----------------------------------------------------------
def _layer_box(layer: torch.Tensor, left: int, top: int, SW: int, SH: int):
    _dev(layer, torch.uint8, "layer")
    if layer.dim() != 3 or layer.shape[2] != 4 or not layer.is_contiguous() or layer.numel() == 0:
        raise ValueError(f"layer: need a non-empty contiguous [bh, bw, 4] tensor, got shape {tuple(layer.shape)} stride {layer.stride()}")
    bh, bw, _ = layer.shape
    if isinstance(left, bool) or isinstance(top, bool) or left < 0 or top < 0 or left + bw > SW or top + bh > SH:
        raise ValueError(f"the {bw}x{bh} box at ({left}, {top}) does not lie inside the {SW}x{SH} photo")
    return bw, bh


def layers_strokes_u8(layer: torch.Tensor, left: int, top: int, plane: torch.Tensor, threshold: int = 0):
    """layer uint8 [bh, bw, 4] (RGBA, a layer's alpha bounding box at (left, top) of the photo), plane uint8 [SH, SW] -> plane, IN PLACE: 255
    where the layer's alpha > threshold (0..254), every other byte as it was.  Only the box's bytes are touched."""
    _plane(plane, "plane")
    SH, SW = plane.shape
    bw, bh = _layer_box(layer, left, top, SW, SH)
    if isinstance(threshold, bool) or not 0 <= int(threshold) <= 254:
        raise ValueError(f"threshold: an int in 0..254, got {threshold!r}")
    st = _prof_begin()
    _launch("ce_layers_strokes_u8", _ptr(layer), bw, bh, int(left), int(top), _ptr(plane), SW, SH, int(threshold), _stream())
    _prof_end(st, f"layers_strokes_{bh}x{bw}", 5.0 * bh * bw)
    return plane


def layers_over_u8(layer: torch.Tensor, left: int, top: int, canvas: torch.Tensor):
    """Image.alpha_composite(canvas, layer) over an opaque canvas, IN PLACE: layer uint8 [bh, bw, 4] at (left, top), canvas uint8 [SH, SW, 3]
    -> canvas.  Only the box's bytes are touched."""
    _dev(canvas, torch.uint8, "canvas")
    if canvas.dim() != 3 or canvas.shape[2] != 3 or not canvas.is_contiguous() or canvas.numel() == 0:
        raise ValueError(f"canvas: need a non-empty contiguous [SH, SW, 3] tensor, got shape {tuple(canvas.shape)} stride {canvas.stride()}")
    SH, SW, _ = canvas.shape
    bw, bh = _layer_box(layer, left, top, SW, SH)
    st = _prof_begin()
    _launch("ce_layers_over_u8", _ptr(layer), bw, bh, int(left), int(top), _ptr(canvas), SW, SH, _stream())
    _prof_end(st, f"layers_over_{bh}x{bw}", 10.0 * bh * bw)
    return canvas


# ---- automatic edit regions (csrc/ce_region_auto.hip) ------------------------------------------------------------------
def _f32c(t: torch.Tensor, name: str):
    _dev(t, torch.float32, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: need a contiguous tensor, got shape {tuple(t.shape)} stride {t.stride()}")


def auto_region_change(x0: torch.Tensor, z_src: torch.Tensor, frame: int = -1, out: Optional[torch.Tensor] = None):
    """x0, z_src fp32 [B, C, T, h, w] -> d fp32 [h, w] on latent frame `frame` (negative: from the end):
    d = max over b of ((sum over c, in order, of (x0 - z_src)^2) / C), every operation rounded in fp32."""
    _f32c(x0, "x0"), _f32c(z_src, "z_src")
    if x0.dim() != 5 or tuple(z_src.shape) != tuple(x0.shape):
        raise ValueError(f"x0 / z_src: need two [B, C, T, h, w] tensors of one shape, got {tuple(x0.shape)} and {tuple(z_src.shape)}")
    B, C, T, h, w = x0.shape
    f = int(frame) + T if frame < 0 else int(frame)
    if not 0 <= f < T:
        raise ValueError(f"frame: {frame} is outside the {T} latent frames")
    if out is None:
        out = torch.empty((h, w), dtype=torch.float32, device=x0.device)
    _f32c(out, "out")
    assert out.numel() == h * w
    st = _prof_begin()
    _launch("ce_auto_region_change_f32", _ptr(x0), _ptr(z_src), _ptr(out), B, C, T, h, w, f, _stream())
    _prof_end(st, f"auto_region_change_{B}x{C}x{h}x{w}", float(8 * B * C * h * w + 4 * h * w))
    return out


def auto_region_otsu(d: torch.Tensor, floor: float = 0.0, thr: Optional[torch.Tensor] = None, dmax: Optional[torch.Tensor] = None):
    """d fp32 (any shape, >= 0 or NaN) -> (thr, dmax), one device float each: Otsu's threshold over 256 bins of [0, dmax], at least floor^2;
    +inf when dmax == 0.  One workgroup, nothing read back."""
    _f32c(d, "d")
    if thr is None:
        thr = torch.empty(1, dtype=torch.float32, device=d.device)
    if dmax is None:
        dmax = torch.empty(1, dtype=torch.float32, device=d.device)
    _f32c(thr, "thr"), _f32c(dmax, "dmax")
    assert thr.numel() == 1 and dmax.numel() == 1
    st = _prof_begin()
    _launch("ce_auto_region_otsu_f32", _ptr(d), d.numel(), float(floor), _ptr(thr), _ptr(dmax), _stream())
    _prof_end(st, f"auto_region_otsu_{d.numel()}", float(8 * d.numel()))
    return thr, dmax


def auto_region_ramp(d: torch.Tensor, thr: torch.Tensor, dilate: int, feather: int, out: Optional[torch.Tensor] = None):
    """d fp32 [h, w], thr = ONE device float -> w fp32 [h, w]: 1 within `dilate` cells (Chebyshev) of a cell with d > thr, a linear ramp
    over the next `feather` cells, 0 beyond.  dilate + feather <= 8."""
    _f32c(d, "d"), _f32c(thr, "thr")
    if d.dim() != 2 or thr.numel() != 1:
        raise ValueError(f"d / thr: need an [h, w] map and ONE threshold, got {tuple(d.shape)} and {thr.numel()} elements")
    if dilate < 0 or feather < 0 or dilate + feather > 8:
        raise ValueError(f"dilate + feather must lie in 0..8, got {dilate} + {feather}")
    if out is None:
        out = torch.empty_like(d)
    _f32c(out, "out")
    assert out.numel() == d.numel() and out.data_ptr() != d.data_ptr()
    st = _prof_begin()
    _launch("ce_auto_region_ramp_f32", _ptr(d), _ptr(thr), _ptr(out), d.shape[0], d.shape[1], int(dilate), int(feather), _stream())
    _prof_end(st, f"auto_region_ramp_{d.shape[0]}x{d.shape[1]}_r{dilate + feather}", float(8 * d.numel()))
    return out


def auto_region_mask_u8(w: torch.Tensor, out: Optional[torch.Tensor] = None):
    """w fp32 [h, w] -> uint8 [8 h, 8 w]: byte = rint(255 * w) of the pixel's cell."""
    _f32c(w, "w")
    if w.dim() != 2:
        raise ValueError(f"w: need an [h, w] map, got {tuple(w.shape)}")
    h, wl = w.shape
    if out is None:
        out = torch.empty((8 * h, 8 * wl), dtype=torch.uint8, device=w.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and out.numel() == 64 * h * wl
    st = _prof_begin()
    _launch("ce_auto_region_mask_u8", _ptr(w), _ptr(out), h, wl, _stream())
    _prof_end(st, f"auto_region_mask_{h}x{wl}", float(4 * w.numel() + out.numel()))
    return out


# ---- live previews (csrc/ce_preview.hip) ---------------------------------------------------------------------------------
PREVIEW_SCALES = (1, 2, 4, 8)
PREVIEW_GRAM_SCRATCH = 1024 * 210 * 8  # the most ce_preview_gram_f64 uses: 1024 workgroups x 210 float64 partials


def preview_rgb_u8(x0: torch.Tensor, factors: torch.Tensor, scale: int = 2, frame: int = -1, w: Optional[torch.Tensor] = None,
                   z_src: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """x0 fp32 [B, 16, T, h, w] on latent frame `frame` (negative: from the end), factors fp32 [17, 3] -> uint8 [B, h scale, w scale, 3]:
    the projection per cell, a bilinear upsample, ce_video_to_u8's byte (preview.rgb_u8_reference, bit for bit).  w fp32 [h, w] and z_src
    (x0's shape), both or neither: cells show w * x0 + (1 - w) * z_src."""
    _f32c(x0, "x0"), _f32c(factors, "factors")
    if x0.dim() != 5 or x0.shape[1] != 16:
        raise ValueError(f"x0: need a [B, 16, T, h, w] tensor, got {tuple(x0.shape)}")
    if tuple(factors.shape) != (17, 3):
        raise ValueError(f"factors: need [17, 3] (16 channel rows and the bias), got {tuple(factors.shape)}")
    if int(scale) not in PREVIEW_SCALES:
        raise ValueError(f"scale: must be one of {PREVIEW_SCALES}, got {scale}")
    if (w is None) != (z_src is None):
        raise ValueError("w and z_src: the composite takes both or neither")
    B, C, T, h, wl = x0.shape
    f = int(frame) + T if frame < 0 else int(frame)
    if not 0 <= f < T:
        raise ValueError(f"frame: {frame} is outside the {T} latent frames")
    if w is not None:
        _f32c(w, "w"), _f32c(z_src, "z_src")
        if tuple(w.shape) != (h, wl) or tuple(z_src.shape) != tuple(x0.shape):
            raise ValueError(f"w / z_src: need [{h}, {wl}] and x0's shape, got {tuple(w.shape)} and {tuple(z_src.shape)}")
    s = int(scale)
    if out is None:
        out = torch.empty((B, h * s, wl * s, 3), dtype=torch.uint8, device=x0.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and out.numel() == B * h * s * wl * s * 3
    st = _prof_begin()
    _launch("ce_preview_rgb_u8", _ptr(x0), _ptr(z_src), _ptr(w), _ptr(factors), _ptr(out), B, C, T, f, h, wl, s, _stream())
    _prof_end(st, f"preview_rgb_{B}x{h}x{wl}_s{s}", float((1 if w is None else 2) * 64 * B * h * wl + out.numel()))
    return out


def preview_gram(z: torch.Tensor, y: torch.Tensor, frame: int = -1, out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """z fp32 [B, 16, T, h, w] on latent frame `frame`, y [B, 3, 8h, 8w] fp32 / bf16 -> float64 [20, 20] = sum over cells of v v^T,
    v = (z_0..z_15, 1, r, g, b) with r, g, b the fp32 8x8 box mean (preview.gram_reference).  Fixed summation order: the same bits every run."""
    _f32c(z, "z")
    if y.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"y: expected bfloat16 or float32, got {y.dtype}")
    _dev(y, y.dtype, "y")
    if z.dim() != 5 or z.shape[1] != 16:
        raise ValueError(f"z: need a [B, 16, T, h, w] tensor, got {tuple(z.shape)}")
    B, _, T, h, wl = z.shape
    if not y.is_contiguous() or tuple(y.shape) != (B, 3, 8 * h, 8 * wl):
        raise ValueError(f"y: need a contiguous [{B}, 3, {8 * h}, {8 * wl}] tensor, got shape {tuple(y.shape)} stride {y.stride()}")
    f = int(frame) + T if frame < 0 else int(frame)
    if not 0 <= f < T:
        raise ValueError(f"frame: {frame} is outside the {T} latent frames")
    if out is None:
        out = torch.empty((20, 20), dtype=torch.float64, device=z.device)
    _dev(out, torch.float64, "out")
    assert out.is_contiguous() and out.numel() == 400
    if scratch is None:
        scratch = torch.empty(PREVIEW_GRAM_SCRATCH, dtype=torch.uint8, device=z.device)
    _dev(scratch, torch.uint8, "scratch")
    st = _prof_begin()
    _launch("ce_preview_gram_f64", _ptr(z), f, _ptr(y), int(y.dtype == torch.bfloat16), _ptr(out), _ptr(scratch), scratch.numel(), B, T, h, wl,
            _stream())
    _prof_end(st, f"preview_gram_{B}x{h}x{wl}", float(64 * B * h * wl + y.numel() * y.element_size()))
    return out


# ---- guided detail lift (csrc/ce_lift.hip) --------------------------------------------------------------------------------
LIFT_CELL = 8  # floats per coefficient cell: abar_rgb, bbar_rgb, g, 0


def _lift_planes(L: torch.Tensor, E: torch.Tensor):
    _dev(L, torch.uint8, "L"), _dev(E, torch.uint8, "E")
    if L.dim() != 3 or L.shape[2] != 3 or not L.is_contiguous():
        raise ValueError(f"L: need a contiguous [H, W, 3] tensor, got shape {tuple(L.shape)} stride {L.stride()}")
    if E.dim() != 4 or tuple(E.shape[1:]) != tuple(L.shape) or not E.is_contiguous():
        raise ValueError(f"E: need a contiguous [F, {L.shape[0]}, {L.shape[1]}, 3] tensor, got shape {tuple(E.shape)} stride {E.stride()}")
    return E.shape[0], L.shape[0], L.shape[1]


def lift_fit_q16(L: torch.Tensor, E: torch.Tensor, radius: int, eps_q: int, max_gain: float, out: Optional[torch.Tensor] = None):
    """Stage 1 of lift.reference: L uint8 [H, W, 3], E uint8 [F, H, W, 3] -> int32 [F, H, W, 6] = rint(65536 a_rgb), rint(65536 b_rgb)."""
    F, H, W = _lift_planes(L, E)
    if out is None:
        out = torch.empty((F, H, W, 6), dtype=torch.int32, device=L.device)
    _dev(out, torch.int32, "out")
    assert out.is_contiguous() and tuple(out.shape) == (F, H, W, 6)
    st = _prof_begin()
    _launch("ce_lift_fit_q16", _ptr(L), _ptr(E), _ptr(out), F, H, W, int(radius), int(eps_q), float(max_gain), _stream())
    _prof_end(st, f"lift_fit_{F}x{H}x{W}_r{radius}", float(L.numel() + E.numel() + 4 * out.numel()))
    return out


def lift_smooth(L: torch.Tensor, E: torch.Tensor, AB: torch.Tensor, radius: int, coef: Optional[torch.Tensor] = None,
                R: Optional[torch.Tensor] = None):
    """Stage 2: -> (the cells fp32 [F, H, W, 8]: the box means of a and b, slots 6 and 7 zeroed; R int32 [F, H, W] = rint(256 min(res, 255)))."""
    F, H, W = _lift_planes(L, E)
    _dev(AB, torch.int32, "AB")
    if not AB.is_contiguous() or tuple(AB.shape) != (F, H, W, 6):
        raise ValueError(f"AB: need a contiguous [{F}, {H}, {W}, 6] tensor, got shape {tuple(AB.shape)} stride {AB.stride()}")
    if coef is None:
        coef = torch.empty((F, H, W, LIFT_CELL), dtype=torch.float32, device=L.device)
    if R is None:
        R = torch.empty((F, H, W), dtype=torch.int32, device=L.device)
    _dev(coef, torch.float32, "coef"), _dev(R, torch.int32, "R")
    assert coef.is_contiguous() and tuple(coef.shape) == (F, H, W, LIFT_CELL) and R.is_contiguous() and tuple(R.shape) == (F, H, W)
    st = _prof_begin()
    _launch("ce_lift_smooth_f32", _ptr(L), _ptr(E), _ptr(AB), _ptr(coef), _ptr(R), F, H, W, int(radius), _stream())
    _prof_end(st, f"lift_smooth_{F}x{H}x{W}_r{radius}", float(4 * (AB.numel() + coef.numel() + R.numel())))
    return coef, R


def lift_gate(R: torch.Tensor, coef: torch.Tensor, radius: int, t0: float, t1: float):
    """Stage 3: g = clamp((box mean of R / 256 - t0) / (t1 - t0), 0, 1) into slot 6 of the cells, in place."""
    _dev(R, torch.int32, "R"), _dev(coef, torch.float32, "coef")
    if R.dim() != 3 or not R.is_contiguous() or not coef.is_contiguous() or tuple(coef.shape) != tuple(R.shape) + (LIFT_CELL,):
        raise ValueError(f"R / coef: need contiguous [F, H, W] and [F, H, W, 8], got {tuple(R.shape)} and {tuple(coef.shape)}")
    F, H, W = R.shape
    st = _prof_begin()
    _launch("ce_lift_gate_f32", _ptr(R), _ptr(coef), F, H, W, int(radius), float(t0), float(t1), _stream())
    _prof_end(st, f"lift_gate_{F}x{H}x{W}_r{radius}", float(8 * R.numel()))
    return coef


def lift_apply_u8(P: torch.Tensor, coef: torch.Tensor, tables, U: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """Stage 4: P uint8 [SH, SW, 3], the cells fp32 [F, H, W, 8], tables = (ix0, ix1 int32 [SW], tx fp32 [SW], iy0, iy1 int32 [SH], ty fp32 [SH])
    on the device, U uint8 [F, SH, SW, 3] or None -> a new uint8 [F, SH, SW, 3]."""
    _dev(P, torch.uint8, "P"), _dev(coef, torch.float32, "coef")
    if P.dim() != 3 or P.shape[2] != 3 or not P.is_contiguous():
        raise ValueError(f"P: need a contiguous [SH, SW, 3] tensor, got shape {tuple(P.shape)} stride {P.stride()}")
    if coef.dim() != 4 or coef.shape[3] != LIFT_CELL or not coef.is_contiguous():
        raise ValueError(f"coef: need a contiguous [F, H, W, 8] tensor, got shape {tuple(coef.shape)} stride {coef.stride()}")
    SH, SW, _ = P.shape
    F, H, W, _ = coef.shape
    ix0, ix1, tx, iy0, iy1, ty = tables
    for t, dt, n, name in ((ix0, torch.int32, SW, "ix0"), (ix1, torch.int32, SW, "ix1"), (tx, torch.float32, SW, "tx"),
                           (iy0, torch.int32, SH, "iy0"), (iy1, torch.int32, SH, "iy1"), (ty, torch.float32, SH, "ty")):
        _dev(t, dt, name)
        if tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous [{n}] tensor, got shape {tuple(t.shape)}")
    if U is not None:
        _dev(U, torch.uint8, "U")
        if tuple(U.shape) != (F, SH, SW, 3) or not U.is_contiguous():
            raise ValueError(f"U: need a contiguous [{F}, {SH}, {SW}, 3] tensor, got shape {tuple(U.shape)} stride {U.stride()}")
    if out is None:
        out = torch.empty((F, SH, SW, 3), dtype=torch.uint8, device=P.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and tuple(out.shape) == (F, SH, SW, 3) and not _overlap(out, P) and (U is None or not _overlap(out, U))
    st = _prof_begin()
    _launch("ce_lift_apply_u8", _ptr(P), _ptr(U), _ptr(coef), _ptr(ix0), _ptr(ix1), _ptr(tx), _ptr(iy0), _ptr(iy1), _ptr(ty), _ptr(out),
            F, SH, SW, H, W, _stream())
    _prof_end(st, f"lift_apply_{F}x{SH}x{SW}", float(out.numel() + P.numel() + (0 if U is None else U.numel())))
    return out


# ---- guided detail lift inside a focus box (csrc/ce_boxlift.hip) -----------------------------------------------------------
def boxlift_apply_paste_u8(P: torch.Tensor, coef: torch.Tensor, tables, U: Optional[torch.Tensor], mask: Optional[torch.Tensor],
                           canvas: torch.Tensor, left: int, top: int, bw: int, bh: int):
    """Stage 4 of the lift fused with the paste, IN PLACE: P uint8 [SH, SW, 3] (the photo the crop was cut from), the cells fp32 [F, H, W, 8],
    tables = lift.tables((bw, bh), (H, W)) on the device, U uint8 [F, bh, bw, 3] or None, mask uint8 [SH, SW] or None (the whole box),
    canvas uint8 [F, SH, SW, 3] -> canvas.  Only the box's bytes are touched; under a mask byte of 0 nothing is computed or written."""
    _dev(P, torch.uint8, "P"), _dev(coef, torch.float32, "coef"), _dev(canvas, torch.uint8, "canvas")
    if P.dim() != 3 or P.shape[2] != 3 or not P.is_contiguous():
        raise ValueError(f"P: need a contiguous [SH, SW, 3] tensor, got shape {tuple(P.shape)} stride {P.stride()}")
    if coef.dim() != 4 or coef.shape[3] != LIFT_CELL or not coef.is_contiguous():
        raise ValueError(f"coef: need a contiguous [F, H, W, 8] tensor, got shape {tuple(coef.shape)} stride {coef.stride()}")
    SH, SW, _ = P.shape
    F, H, W, _ = coef.shape
    if tuple(canvas.shape) != (F, SH, SW, 3) or not canvas.is_contiguous():
        raise ValueError(f"canvas: need a contiguous [{F}, {SH}, {SW}, 3] tensor, got shape {tuple(canvas.shape)} stride {canvas.stride()}")
    left, top, bw, bh = int(left), int(top), int(bw), int(bh)
    if bw < 1 or bh < 1 or left < 0 or top < 0 or left + bw > SW or top + bh > SH:
        raise ValueError(f"the {bw}x{bh} box at ({left}, {top}) does not lie inside the {SW}x{SH} canvas")
    ix0, ix1, tx, iy0, iy1, ty = tables
    for t, dt, n, name in ((ix0, torch.int32, bw, "ix0"), (ix1, torch.int32, bw, "ix1"), (tx, torch.float32, bw, "tx"),
                           (iy0, torch.int32, bh, "iy0"), (iy1, torch.int32, bh, "iy1"), (ty, torch.float32, bh, "ty")):
        _dev(t, dt, name)
        if tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous [{n}] tensor, got shape {tuple(t.shape)}")
    if U is not None:
        _dev(U, torch.uint8, "U")
        if tuple(U.shape) != (F, bh, bw, 3) or not U.is_contiguous():
            raise ValueError(f"U: need a contiguous [{F}, {bh}, {bw}, 3] tensor, got shape {tuple(U.shape)} stride {U.stride()}")
    if mask is not None:
        _dev(mask, torch.uint8, "mask")
        if tuple(mask.shape) != (SH, SW) or not mask.is_contiguous():
            raise ValueError(f"mask: need a contiguous [{SH}, {SW}] tensor, got shape {tuple(mask.shape)} stride {mask.stride()}")
    assert not _overlap(canvas, P) and (U is None or not _overlap(canvas, U)) and (mask is None or not _overlap(canvas, mask))
    st = _prof_begin()
    _launch("ce_boxlift_apply_paste_u8", _ptr(P), _ptr(U), _ptr(coef), _ptr(ix0), _ptr(ix1), _ptr(tx), _ptr(iy0), _ptr(iy1), _ptr(ty), _ptr(mask),
            _ptr(canvas), F, SH, SW, left, top, bw, bh, H, W, _stream())
    _prof_end(st, f"boxlift_apply_paste_{F}x{bh}x{bw}", float(F * bh * bw * (9 if U is not None else 6) + bh * bw * 4))
    return canvas


# ---- mask-aware detail lift (csrc/ce_rimlift.hip) --------------------------------------------------------------------------
def _rimlift_planes(L: torch.Tensor, E: torch.Tensor, M: torch.Tensor):
    F, H, W = _lift_planes(L, E)
    _dev(M, torch.uint8, "M")
    if tuple(M.shape) != (H, W) or not M.is_contiguous():
        raise ValueError(f"M: need a contiguous [{H}, {W}] tensor, got shape {tuple(M.shape)} stride {M.stride()}")
    return F, H, W


def rimlift_fit_q16(L: torch.Tensor, E: torch.Tensor, M: torch.Tensor, radius: int, eps_q: int, max_gain: float,
                    out: Optional[torch.Tensor] = None):
    """Stage 1 of rimlift.py: L uint8 [H, W, 3], E uint8 [F, H, W, 3], M uint8 [H, W] (the edit-size weight plane) -> int32 [F, H, W, 6] =
    rint(65536 a_rgb), rint(65536 b_rgb) of the untapered map."""
    F, H, W = _rimlift_planes(L, E, M)
    if out is None:
        out = torch.empty((F, H, W, 6), dtype=torch.int32, device=L.device)
    _dev(out, torch.int32, "out")
    assert out.is_contiguous() and tuple(out.shape) == (F, H, W, 6)
    st = _prof_begin()
    _launch("ce_rimlift_fit_q16", _ptr(L), _ptr(E), _ptr(M), _ptr(out), F, H, W, int(radius), int(eps_q), float(max_gain), _stream())
    _prof_end(st, f"rimlift_fit_{F}x{H}x{W}_r{radius}", float(L.numel() + E.numel() + F * M.numel() + 4 * out.numel()))
    return out


def rimlift_smooth(L: torch.Tensor, E: torch.Tensor, M: torch.Tensor, AB: torch.Tensor, radius: int, coef: Optional[torch.Tensor] = None,
                   R: Optional[torch.Tensor] = None):
    """Stage 2 of rimlift.py: -> (the cells fp32 [F, H, W, 8]: the M-weighted box means of a and b, slots 6 and 7 zeroed; R int32 [F, H, W] =
    rint(256 min(res, 255)), the residual of the tapered model)."""
    F, H, W = _rimlift_planes(L, E, M)
    _dev(AB, torch.int32, "AB")
    if not AB.is_contiguous() or tuple(AB.shape) != (F, H, W, 6):
        raise ValueError(f"AB: need a contiguous [{F}, {H}, {W}, 6] tensor, got shape {tuple(AB.shape)} stride {AB.stride()}")
    if coef is None:
        coef = torch.empty((F, H, W, LIFT_CELL), dtype=torch.float32, device=L.device)
    if R is None:
        R = torch.empty((F, H, W), dtype=torch.int32, device=L.device)
    _dev(coef, torch.float32, "coef"), _dev(R, torch.int32, "R")
    assert coef.is_contiguous() and tuple(coef.shape) == (F, H, W, LIFT_CELL) and R.is_contiguous() and tuple(R.shape) == (F, H, W)
    st = _prof_begin()
    _launch("ce_rimlift_smooth_f32", _ptr(L), _ptr(E), _ptr(M), _ptr(AB), _ptr(coef), _ptr(R), F, H, W, int(radius), _stream())
    _prof_end(st, f"rimlift_smooth_{F}x{H}x{W}_r{radius}", float(4 * (AB.numel() + coef.numel() + R.numel()) + F * M.numel()))
    return coef, R


# ---- tiled edits (csrc/ce_tiles.hip) ---------------------------------------------------------------------------------------
def _tile_origins(xs, ys):
    """The origins as the host int arrays the launchers read (they check the geometry; a bad one is a HipKernelError 'bad argument')."""
    xs, ys = [int(v) for v in xs], [int(v) for v in ys]
    return len(xs), len(ys), (ctypes.c_int * max(len(xs), 1))(*xs), (ctypes.c_int * max(len(ys), 1))(*ys)


def _tile_latents(tiles: torch.Tensor, canvas: torch.Tensor, nx: int, ny: int):
    _dev(tiles, torch.float32, "tiles"), _dev(canvas, torch.float32, "canvas")
    if tiles.dim() < 3 or canvas.dim() < 2 or not tiles.is_contiguous() or not canvas.is_contiguous():
        raise ValueError(f"tiles / canvas: need contiguous [n, ..., th, tw] and [..., ch, cw], got {tuple(tiles.shape)} stride {tiles.stride()} and "
                         f"{tuple(canvas.shape)} stride {canvas.stride()}")
    if tiles.shape[0] != nx * ny or tuple(tiles.shape[1:-2]) != tuple(canvas.shape[:-2]):
        raise ValueError(f"tiles {tuple(tiles.shape)}: need {nx * ny} tiles whose middle axes are the canvas's {tuple(canvas.shape[:-2])}")
    planes = 1
    for s in canvas.shape[:-2]:
        planes *= int(s)
    return planes, int(tiles.shape[-2]), int(tiles.shape[-1]), int(canvas.shape[-2]), int(canvas.shape[-1])


def tiles_fuse(tiles: torch.Tensor, canvas: torch.Tensor, xs, ys):
    """tiles fp32 [n, ..., th, tw] (row-major over ys x xs, origins in cells) -> canvas fp32 [..., ch, cw], overwritten: per cell the mean of
    the covering tiles under integer tent weights, summed in double in ascending tile index (tiles.reference_fuse, bit for bit)."""
    nx, ny, ox, oy = _tile_origins(xs, ys)
    planes, th, tw, ch, cw = _tile_latents(tiles, canvas, nx, ny)
    st = _prof_begin()
    _launch("ce_tiles_fuse_f32", _ptr(tiles), _ptr(canvas), nx, ny, ox, oy, planes, th, tw, ch, cw, _stream())
    _prof_end(st, f"tiles_fuse_{nx}x{ny}_{planes}x{ch}x{cw}", 4.0 * (tiles.numel() + canvas.numel()))
    return canvas


def tiles_scatter(canvas: torch.Tensor, tiles: torch.Tensor, xs, ys):
    """canvas fp32 [..., ch, cw] -> tiles fp32 [n, ..., th, tw], overwritten: every tile cell takes its canvas cell (tiles.reference_scatter)."""
    nx, ny, ox, oy = _tile_origins(xs, ys)
    planes, th, tw, ch, cw = _tile_latents(tiles, canvas, nx, ny)
    st = _prof_begin()
    _launch("ce_tiles_scatter_f32", _ptr(canvas), _ptr(tiles), nx, ny, ox, oy, planes, th, tw, ch, cw, _stream())
    _prof_end(st, f"tiles_scatter_{nx}x{ny}_{planes}x{ch}x{cw}", 8.0 * tiles.numel())
    return tiles


def tiles_blend_u8(frames: torch.Tensor, xs, ys, target, out: Optional[torch.Tensor] = None):
    """frames uint8 [n, F, TH, TW, 3] (the decoded tiles, row-major over ys x xs, origins in pixels), target = (W, H) -> uint8 [F, H, W, 3]: the
    tent-weighted mean in exact integers, the canvas cropped to the target (tiles.reference_blend, the same bytes)."""
    _dev(frames, torch.uint8, "frames")
    if frames.dim() != 5 or frames.shape[4] != 3 or not frames.is_contiguous():
        raise ValueError(f"frames: need a contiguous [n, F, TH, TW, 3] tensor, got shape {tuple(frames.shape)} stride {frames.stride()}")
    nx, ny, ox, oy = _tile_origins(xs, ys)
    n, F, TH, TW, _ = frames.shape
    W, H = int(target[0]), int(target[1])
    if n != nx * ny:
        raise ValueError(f"frames: {n} tiles for a {nx}x{ny} grid")
    if out is None:
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=frames.device)
    _dev(out, torch.uint8, "out")
    assert out.is_contiguous() and tuple(out.shape) == (F, H, W, 3)
    st = _prof_begin()
    _launch("ce_tiles_blend_u8", _ptr(frames), _ptr(out), nx, ny, ox, oy, F, TH, TW, H, W, _stream())
    _prof_end(st, f"tiles_blend_{nx}x{ny}_{F}x{H}x{W}", float(frames.numel() + out.numel()))
    return out


# ---- Wan VAE ------------------------------------------------------------------------------------------------------
# ---- sparse region edits (csrc/ce_sparse.hip) ----------------------------------------------------------------------------
def _sparse_ids(ids: torch.Tensor):
    """ids on the device -> (Na, ids_i64).  Sorted / unique / in range is the caller's once-per-edit check (sparse_region.validate_ids)."""
    if not ids.is_cuda:
        raise HipKernelError("ids: tensor must live on the GPU (the HIP path has no CPU fallback)")
    if ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"ids: expected int32 or int64, got {ids.dtype}")
    if ids.dim() != 1 or not ids.is_contiguous() or ids.numel() == 0:
        raise ValueError(f"ids: need a non-empty contiguous 1-D tensor, got shape {tuple(ids.shape)} stride {ids.stride()}")
    return ids.numel(), int(ids.dtype == torch.int64)


def sparse_patchify(x: torch.Tensor, ids: torch.Tensor, kpad: int, out: Optional[torch.Tensor] = None):
    """x [C,T,H,W] bf16, ids [Na] -> [Na, kpad]: the rows `patchify` gives for the listed tokens."""
    _dev(x, torch.bfloat16, "x")
    assert x.is_contiguous() and x.dim() == 4
    C, T, H, W = x.shape
    na, i64 = _sparse_ids(ids)
    if out is None:
        out = torch.empty((na, kpad), dtype=torch.bfloat16, device=x.device)
    _dev(out, torch.bfloat16, "out")
    assert out.is_contiguous() and out.shape == (na, kpad)
    st = _prof_begin()
    _launch("ce_sparse_patchify_bf16", _ptr(x), _ptr(ids), i64, _ptr(out), C, T, H, W, kpad, na, _stream())
    _prof_end(st, f"sparse_patchify_{na}x{kpad}", 4.0 * na * kpad)
    return out


def sparse_scatter_rows_(dst: torch.Tensor, src: torch.Tensor, ids: torch.Tensor, batch: int = 1):
    """dst [batch*N, D], src [batch*Na, D] (row strides free), ids [Na]: dst[b*N + ids[a]] = src[b*Na + a]; other rows are not written."""
    _dev(dst, torch.bfloat16, "dst"), _dev(src, torch.bfloat16, "src")
    Md, D, ldd = _rows(dst, "dst")
    Ms, Ds, lds = _rows(src, "src")
    na, i64 = _sparse_ids(ids)
    if batch < 1 or Ds != D or Ms != batch * na or Md % batch or na > Md // batch:
        raise ValueError(f"sparse_scatter_rows_: src {tuple(src.shape)} / dst {tuple(dst.shape)} do not fit {na} ids and batch={batch}")
    st = _prof_begin()
    _launch("ce_sparse_scatter_rows_bf16", _ptr(src), lds, _ptr(dst), ldd, _ptr(ids), i64, na, Md // batch, batch, D, _stream())
    _prof_end(st, f"sparse_scatter_rows_{Ms}x{D}", 4.0 * Ms * D)
    return dst


def sparse_scatter_vt_(vt: torch.Tensor, src: torch.Tensor, ids: torch.Tensor, n_tokens: int, batch: int = 1, src_rows: bool = False):
    """vt [D, >= batch*n_tokens] (the cached V^T, row stride free), ids [Na]: vt[:, b*n_tokens + ids[a]] = V of sample b's active token a.
    src: V^T [D, batch*Na] as the transposed-store GEMM leaves it (row stride free), or - src_rows - row-major V [batch*Na, D]."""
    _dev(vt, torch.bfloat16, "vt"), _dev(src, torch.bfloat16, "src")
    D, cols, ldvt = _rows(vt, "vt")
    Ms, Ns, lds = _rows(src, "src")
    na, i64 = _sparse_ids(ids)
    want = (batch * na, D) if src_rows else (D, batch * na)
    if batch < 1 or (Ms, Ns) != want or na > n_tokens or cols < batch * n_tokens:
        raise ValueError(f"sparse_scatter_vt_: src {tuple(src.shape)} (expected {want}) / vt {tuple(vt.shape)} do not fit {na} ids of "
                         f"{n_tokens} tokens and batch={batch}")
    st = _prof_begin()
    _launch("ce_sparse_scatter_vt_bf16", _ptr(src), lds, int(bool(src_rows)), _ptr(vt), ldvt, _ptr(ids), i64, na, int(n_tokens), batch, D,
            _stream())
    _prof_end(st, f"sparse_scatter_vt_{batch * na}x{D}" + ("_rows" if src_rows else ""), 4.0 * batch * na * D)
    return vt


def sparse_unpatchify_(out: torch.Tensor, y: torch.Tensor, ids: torch.Tensor):
    """y [Na, >= 4*Cout] (head rows of the listed tokens), out [Cout,T,H,W]: the 2 x 2 cells of those tokens; nothing else is written."""
    _dev(y, torch.bfloat16, "y"), _dev(out, torch.bfloat16, "out")
    Ms, _, ldy = _rows(y, "y")
    na, i64 = _sparse_ids(ids)
    assert out.is_contiguous() and out.dim() == 4 and Ms == na, (out.shape, y.shape, na)
    cout, T, H, W = out.shape
    st = _prof_begin()
    _launch("ce_sparse_unpatchify_bf16", _ptr(y), ldy, _ptr(ids), i64, _ptr(out), cout, T, H, W, na, _stream())
    _prof_end(st, f"sparse_unpatchify_{na}x{4 * cout}", 16.0 * na * cout)
    return out


def conv3d_gemm(in_stack: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], out_stack: torch.Tensor,
                res_stack: Optional[torch.Tensor], *, T_out: int, H: int, W: int, Cin: int, Cout: int, KT: int, n_tile: int = 0):
    """Stride-1 3x3 / 3x3x3 conv of a wide layer as ONE large-tile GEMM over a contiguous stack of bordered frames (see
    include/chronoedit_hip.h: in_stack holds T_out + KT - 1 frames plus one zeroed slack frame)."""
    _dev(in_stack, torch.bfloat16, "in_stack")
    _dev(out_stack, torch.bfloat16, "out_stack")
    _dev(weight, torch.bfloat16, "weight")
    assert in_stack.is_contiguous() and out_stack.is_contiguous() and weight.is_contiguous() and weight.dim() == 2
    assert in_stack.shape[0] >= T_out + KT and tuple(in_stack.shape[1:]) == (H + 2, W + 2, Cin), in_stack.shape
    assert out_stack.shape[0] >= T_out and tuple(out_stack.shape[1:3]) == (H + 2, W + 2), out_stack.shape
    if res_stack is not None:
        _dev(res_stack, torch.bfloat16, "res_stack")
        assert res_stack.is_contiguous() and res_stack.shape[1:] == out_stack.shape[1:] and res_stack.shape[0] >= T_out
    st_ev = _prof_begin()
    _launch("ce_conv3d_gemm_bf16", _ptr(in_stack), _ptr(weight), weight.shape[1], _ptr(bias), _ptr(out_stack), _ptr(res_stack), T_out, H, W,
            Cin, Cout, KT, out_stack.shape[3], n_tile, _stream())
    _prof_end(st_ev, f"conv_{KT}x3x3_{Cin}->{Cout}_{T_out}x{H}x{W}", 2.0 * T_out * H * W * Cout * Cin * KT * 9)


def conv3d_gemm_rms_silu(in_stack: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], normed_stack: torch.Tensor, gamma: torch.Tensor, *,
                         T_out: int, H: int, W: int, Cin: int, Cout: int, KT: int, silu: bool = True, out_stack: Optional[torch.Tensor] = None,
                         res_stack: Optional[torch.Tensor] = None):
    """conv3d_gemm with the next layer's RMS_norm (+ SiLU) in its epilogue: normed_stack = silu(rms_norm(y) * gamma), y = bf16(conv + bias)
    [bf16(res + .)]; y itself goes to out_stack when one is given (the next block's shortcut operand), else it is never written.  96 output
    channels only (ce_conv3d_gemm_rms_silu_bf16)."""
    _dev(in_stack, torch.bfloat16, "in_stack")
    _dev(normed_stack, torch.bfloat16, "normed_stack")
    _dev(weight, torch.bfloat16, "weight")
    _dev(gamma, torch.float32, "gamma")
    assert in_stack.is_contiguous() and normed_stack.is_contiguous() and weight.is_contiguous() and weight.dim() == 2 and gamma.numel() == Cout
    assert in_stack.shape[0] >= T_out + KT and tuple(in_stack.shape[1:]) == (H + 2, W + 2, Cin), in_stack.shape
    assert normed_stack.shape[0] >= T_out and tuple(normed_stack.shape[1:3]) == (H + 2, W + 2), normed_stack.shape
    for t, nm in ((out_stack, "out_stack"), (res_stack, "res_stack")):
        if t is not None:
            _dev(t, torch.bfloat16, nm)
            assert t.is_contiguous() and t.shape[1:] == normed_stack.shape[1:] and t.shape[0] >= T_out, (nm, t.shape)
    assert res_stack is None or out_stack is not None
    st_ev = _prof_begin()
    _launch("ce_conv3d_gemm_rms_silu_bf16", _ptr(in_stack), _ptr(weight), weight.shape[1], _ptr(bias), _ptr(out_stack), _ptr(res_stack), _ptr(normed_stack),
            T_out, H, W, Cin, Cout, KT, normed_stack.shape[3], _ptr(gamma), int(bool(silu)), _stream())
    _prof_end(st_ev, f"conv_{KT}x3x3_{Cin}->{Cout}_{T_out}x{H}x{W}+norm", 2.0 * T_out * H * W * Cout * Cin * KT * 9)


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def conv_igemm(in_frames, weight: torch.Tensor, bias: Optional[torch.Tensor], out_frames, res_frames, *, Cin: int, Cout: int,
               KT: int, KH: int, KW: int, st: int, ss: int, H_out: int, W_out: int, in_Wp: int, in_off: int, out_Wp: int,
               out_border: int, out_cstride: int, out_coff: int = 0):
    """Implicit-GEMM conv over lists of channels-last frames (see include/chronoedit_hip.h)."""
    for t in list(in_frames) + list(out_frames) + list(res_frames or []):
        _dev(t, torch.bfloat16, "frame")
    _dev(weight, torch.bfloat16, "weight")
    assert weight.is_contiguous() and weight.numel() >= Cout * KT * KH * KW * Cin
    ia, oa = _ptr_array(in_frames), _ptr_array(out_frames)
    ra = _ptr_array(res_frames) if res_frames else None
    st_ev = _prof_begin()
    _launch("ce_conv_igemm_bf16", ia, len(in_frames), _ptr(weight), _ptr(bias), oa, len(out_frames), ra, Cin, Cout, KT, KH, KW,
            st, ss, H_out, W_out, in_Wp, in_off, in_off, out_Wp, out_border, out_cstride, out_coff,
            _stream())
    _prof_end(st_ev, f"conv_{KT}x{KH}x{KW}_{Cin}->{Cout}_{len(out_frames)}x{H_out}x{W_out}",
              2.0 * len(out_frames) * H_out * W_out * Cout * Cin * KT * KH * KW)


def conv3d_head(in_frames, weight: torch.Tensor, bias: Optional[torch.Tensor], out_frames, *, Cin: int, Cout: int, KT: int, H_out: int,
                W_out: int, in_Wp: int, out_Wp: int, out_border: int, out_cstride: int, out_coff: int = 0):
    """Stride-1 3x3(x3) conv of 96 channels onto <= 4 (the VAE decoder's head conv) - ce_conv3d_head_bf16, see include/chronoedit_hip.h."""
    for t in list(in_frames) + list(out_frames):
        _dev(t, torch.bfloat16, "frame")
    _dev(weight, torch.bfloat16, "weight")
    assert weight.is_contiguous() and weight.numel() >= Cout * KT * 9 * Cin
    ia, oa = _ptr_array(in_frames), _ptr_array(out_frames)
    st_ev = _prof_begin()
    _launch("ce_conv3d_head_bf16", ia, len(in_frames), _ptr(weight), _ptr(bias), oa, len(out_frames), Cin, Cout, KT, H_out, W_out, in_Wp,
            out_Wp, out_border, out_cstride, out_coff, _stream())
    _prof_end(st_ev, f"conv_head_{KT}x3x3_{Cin}->{Cout}_{len(out_frames)}x{H_out}x{W_out}", 2.0 * len(out_frames) * H_out * W_out * Cout * Cin * KT * 9)


def rms_silu(x: torch.Tensor, gamma: torch.Tensor, out: torch.Tensor, T: int, C: int, H: int, W: int, in_border: int,
             out_border: int, silu: bool = True):
    _dev(x, torch.bfloat16, "x"), _dev(out, torch.bfloat16, "out"), _dev(gamma, torch.float32, "gamma")
    st = _prof_begin()
    _launch("ce_rms_silu_bf16", _ptr(x), _ptr(out), _ptr(gamma), T * H * W, C, H, W, in_border, out_border, int(silu), _stream())
    _prof_end(st, f"rms_silu_{C}ch_{T}x{H}x{W}", 4.0 * T * H * W * C)  # (work: bytes read + written, bf16)
    return out


def zero_border(frames: torch.Tensor, T: int, H: int, W: int, C: int):
    """Zero the one-pixel border of T bordered channels-last frames [T, H+2, W+2, ld] (channels [0, C))."""
    _dev(frames, torch.bfloat16, "frames")
    assert frames.is_contiguous() and tuple(frames.shape[:3]) == (T, H + 2, W + 2)
    st = _prof_begin()
    _launch("ce_zero_border_bf16", _ptr(frames), T, H, W, C, frames.shape[3], _stream())
    _prof_end(st, f"zero_border_{C}ch_{T}x{H}x{W}", 2.0 * T * (2 * (W + 2) + 2 * H) * C)
    return frames


def upsample2x(x: torch.Tensor, out: torch.Tensor, T: int, C: int, H: int, W: int):
    _dev(x, torch.bfloat16, "x"), _dev(out, torch.bfloat16, "out")
    st = _prof_begin()
    _launch("ce_upsample2x_bf16", _ptr(x), _ptr(out), T, C, H, W, _stream())
    _prof_end(st, f"upsample2x_{C}ch_{T}x{H}x{W}", 2.0 * T * H * W * C * 5)  # (read once, written four times)
    return out


def softmax_rows(scores: torch.Tensor, probs: torch.Tensor, n: int, scale: float):
    _dev(scores, torch.float32, "scores"), _dev(probs, torch.bfloat16, "probs")
    M, _, ld = _rows(scores, "scores")
    _, npad, ldp = _rows(probs, "probs")
    _launch("ce_softmax_rows_f32_bf16", _ptr(scores), _ptr(probs), M, n, npad, ld, ldp, float(scale), _stream())
    return probs


_attn1_ws = {}  # (device index, floats) -> fp32 scratch of the key split of attention_1head: one per shape, allocated outside capture and NEVER
                # freed or replaced (a captured graph of an earlier shape keeps writing through its pointer)


def attention_1head(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None,
                    split_keys: bool = True):
    """softmax(q k^T * scale) v for one head of dimension C in {128, 384} (the Wan VAE mid-block): q [Nq, C], k [Nk, C] row views,
    vt [C, >= 64 ceil(Nk / 64)] = v transposed with zero padding columns; flash-style, nothing of size Nq x Nk is materialised.
    split_keys: hand the library a scratch (4 Nq (C + 2) floats per device and shape, allocated once, shared by the launches of ONE stream) so that it may split the key axis over
    several workgroups per query block when the query blocks alone do not fill the chip (ce_attention_1head_bf16)."""
    _dev(q, torch.bfloat16, "q"), _dev(k, torch.bfloat16, "k"), _dev(vt, torch.bfloat16, "vt")
    Nq, C, ldq = _rows(q, "q")
    Nk, C2, ldk = _rows(k, "k")
    Cv, _, ldvt = _rows(vt, "vt")
    assert C == C2 == Cv, (C, C2, Cv)
    if out is None:
        out = torch.empty((Nq, C), dtype=torch.bfloat16, device=q.device)
    _dev(out, torch.bfloat16, "out")
    _, _, ldo = _rows(out, "out")
    ws = None
    if split_keys:
        dev = q.device.index if q.device.index is not None else torch.cuda.current_device()
        need = 4 * Nq * (C + 2)
        ws = _attn1_ws.get((dev, need))
        if ws is None and not torch.cuda.is_current_stream_capturing():
            ws = _attn1_ws[(dev, need)] = torch.empty(need, dtype=torch.float32, device=q.device)
        # (first seen under capture: no scratch - one workgroup per query block walks all keys)
    st = _prof_begin()
    _launch("ce_attention_1head_bf16", _ptr(q), _ptr(k), _ptr(vt), _ptr(out), Nq, Nk, C, ldq, ldk, ldvt, ldo, float(scale), _ptr(ws),
            0 if ws is None else ws.numel() * 4, _stream())
    _prof_end(st, f"attention_1head_{Nq}x{Nk}x{C}", 4.0 * Nq * Nk * C)
    return out


def gemm_f32(a: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None):
    """out[M,N] (fp32) = a[M,K] @ w[N,K]^T, no bias (CE_EPI_F32)."""
    _dev(a, torch.bfloat16, "a"), _dev(w, torch.bfloat16, "w")
    M, K, lda = _rows(a, "a")
    N, K2, ldw = _rows(w, "w")
    assert K == K2
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _, _, ldc = _rows(out, "out")
    ws, ws_bytes = _gemm_scratch(a.device)
    _launch("ce_gemm_bf16", _ptr(a), _ptr(w), _ptr(out), _ptr(None), 4, _ptr(None), _ptr(None), M, N, K, lda, ldw, ldc, 0, 0, 0, 0, 0, 0,
            ws, ws_bytes, _stream())
    return out


# ------------------------------------------------------------------------------------------
# conditioning encoders (once per edit)
# ------------------------------------------------------------------------------------------
def gemm_batched(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor, M: int, N: int, K: int, lda: int, ldw: int, ldc: int,
                 batch: tuple, stride_a: tuple, stride_w: tuple, stride_c: tuple, f32_out: bool = False,
                 bias: Optional[torch.Tensor] = None):
    """batch[0] x batch[1] products out_z[M,N] = a_z[M,K] @ w_z[N,K]^T; operand z = (z0, z1) starts stride[0]*z0 + stride[1]*z1
    elements into its tensor (flat storage offsets; see ce_gemm_batched_bf16).  Raw-pointer form: the caller states the geometry."""
    _dev(a, torch.bfloat16, "a"), _dev(w, torch.bfloat16, "w")
    _dev(out, torch.float32 if f32_out else torch.bfloat16, "out")
    if bias is not None:
        _dev(bias, torch.float32, "bias")
    st = _prof_begin()
    _launch("ce_gemm_batched_bf16", _ptr(a), _ptr(w), _ptr(out), _ptr(bias), EPI_F32 if f32_out else EPI_BIAS, M, N, K, lda, ldw, ldc,
            batch[0], batch[1], stride_a[0], stride_a[1], stride_w[0], stride_w[1], stride_c[0], stride_c[1],
            _stream())
    _prof_end(st, f"gemm_batched_{batch[0] * batch[1]}x{M}x{N}x{K}", 2.0 * M * N * K * batch[0] * batch[1])
    return out


def im2col_patch2d(img: torch.Tensor, patch: int, kpad: int, out: Optional[torch.Tensor] = None):
    """img [B,C,H,W] bf16 contiguous -> cols [B*(H/P)*(W/P), kpad] (column = c*P*P + y*P + x, zero padded)."""
    _dev(img, torch.bfloat16, "img")
    if img.dim() != 4 or not img.is_contiguous():
        raise ValueError("im2col_patch2d: need a contiguous [B,C,H,W] tensor")
    B, C, H, W = img.shape
    if out is None:
        out = torch.empty((B * (H // patch) * (W // patch), kpad), dtype=torch.bfloat16, device=img.device)
    _launch("ce_im2col_patch2d_bf16", _ptr(img), _ptr(out), B, C, H, W, patch, kpad, _stream())
    return out


def gather_rows(table: torch.Tensor, ids: torch.Tensor, out: Optional[torch.Tensor] = None):
    """out[i] = table[ids[i]] (bf16 rows, int64 ids)."""
    _dev(table, torch.bfloat16, "table"), _dev(ids, torch.int64, "ids")
    V, D, ldt = _rows(table, "table")
    ids = ids.reshape(-1).contiguous()
    if out is None:
        out = torch.empty((ids.numel(), D), dtype=torch.bfloat16, device=table.device)
    _, _, ldo = _rows(out, "out")
    _launch("ce_gather_rows_bf16", _ptr(table), _ptr(ids), _ptr(out), ids.numel(), D, ldt, ldo, V, _stream())
    return out


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None):
    """T5LayerNorm: out = bf16(bf16(x * rsqrt(mean(x^2) + eps)) * w); x, w, out bf16."""
    _dev(x, torch.bfloat16, "x"), _dev(w, torch.bfloat16, "w")
    M, D, ldx = _rows(x, "x")
    assert w.numel() == D and w.is_contiguous()
    if out is None:
        out = torch.empty((M, D), dtype=torch.bfloat16, device=x.device)
    _, _, ldy = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_rmsnorm_bf16", _ptr(x), _ptr(out), _ptr(w), M, D, ldx, ldy, float(eps), _stream())
    _prof_end(st, f"rmsnorm_{M}x{D}", 4.0 * M * D)
    return out


def softmax_t5(scores: torch.Tensor, probs: torch.Tensor, batch: int, heads: int, Lq: int, Lk: int,
               bucket_lut: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None,
               valid_len: Optional[torch.Tensor] = None):
    """probs = softmax(scores + relative-position bias) over the valid keys; scores [batch*heads*Lq, ld] fp32, probs [.., ldp] bf16."""
    _dev(scores, torch.float32, "scores"), _dev(probs, torch.bfloat16, "probs")
    rows, _, ld = _rows(scores, "scores")
    rows_p, _, ldp = _rows(probs, "probs")
    assert rows == rows_p == batch * heads * Lq
    for t, dt, n in ((bucket_lut, torch.int32, "bucket_lut"), (valid_len, torch.int32, "valid_len"), (table, torch.float32, "table")):
        if t is not None:
            _dev(t, dt, n)
            assert t.is_contiguous()
    if table is not None:
        assert bucket_lut.numel() == Lq + Lk - 1 and table.shape[-1] == heads
    _launch("ce_softmax_t5_bf16", _ptr(scores), _ptr(probs), batch, heads, Lq, Lk, ld, ldp, _ptr(bucket_lut), _ptr(table),
            _ptr(valid_len), _stream())
    return probs


# ------------------------------------------------------------------------------------------
# fp8 (OCP e4m3) GEMM path
# ------------------------------------------------------------------------------------------
def quant_rows_fp8(x: torch.Tensor, out: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """x [M,K] bf16 -> (q [M,K] uint8 holding fp8 e4m3, s [M] fp32) with x ~= q * s[:, None] and max |q| = 448 per row."""
    _dev(x, torch.bfloat16, "x")
    M, K, ldx = _rows(x, "x")
    if out is None:
        out = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty((M,), dtype=torch.float32, device=x.device)
    _dev(out, torch.uint8, "out"), _dev(scale, torch.float32, "scale")
    _, _, ldq = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_quant_rows_fp8", _ptr(x), _ptr(out), _ptr(scale), M, K, ldx, ldq, _stream())
    _prof_end(st, f"quant_fp8_{M}x{K}", 3.0 * M * K)
    return out, scale


def ln_affine_fp8(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, eps: float, out: torch.Tensor, scale: torch.Tensor,
                  ab_rows: int = 0, ab_stride: int = 0):
    """ln_affine + quant_rows_fp8 in one pass: out (uint8 fp8 e4m3) and scale (fp32 per row) of LN(x) * a + b rounded to bf16."""
    _dev(x, torch.bfloat16, "x"), _dev(a, torch.float32, "a"), _dev(b, torch.float32, "b")
    _dev(out, torch.uint8, "out"), _dev(scale, torch.float32, "scale")
    M, D, ldx = _rows(x, "x")
    _, _, ldq = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_ln_affine_fp8", _ptr(x), _ptr(out), _ptr(scale), _ptr(a), _ptr(b), M, D, ldx, ldq, float(eps), int(ab_rows),
            int(ab_stride), _stream())
    _prof_end(st, f"ln_affine_fp8_{M}x{D}", 3.0 * M * D)
    return out, scale


def mx_scale_bytes(rows: int, K: int) -> int:
    """Size of the tiled E8M0 scale buffer of a [rows, K] MX operand ([ceil(rows/128)][K/128][4][16][8] bytes)."""
    return (rows + 127) // 128 * (K // 128) * 512


def mx_scales_to_rows(scale8: torch.Tensor, rows: int, K: int, w_order: bool = False) -> torch.Tensor:
    """The tiled scale buffer as a plain [rows, K/32] uint8 matrix (E8M0 bytes; for tests and tools - not on the hot path).
    w_order: the buffer is in the W order ([rb][kt][g][128 rows], `quant_rows_mxfp8(..., w_order=True)`), else in the A order."""
    rb, kt = (rows + 127) // 128, K // 128
    if w_order:
        t = scale8[: rb * kt * 512].view(rb, kt, 4, 128)            # [rb][kt][g][row % 128]
        return t.permute(0, 3, 1, 2).reshape(rb * 128, kt * 4)[:rows]
    t = scale8[: rb * kt * 512].view(rb, kt, 4, 16, 8)          # [rb][kt][g][fr][F]
    return t.permute(0, 4, 3, 1, 2).reshape(rb * 128, kt * 4)[:rows]  # row = rb*128 + F*16 + fr, block = kt*4 + g


def quant_rows_mxfp8(x: torch.Tensor, out: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, w_order: bool = False):
    """x [M,K] bf16 -> (q [M,K] uint8 holding e4m3, scale8 uint8: one E8M0 byte per 32 consecutive elements of a row, tiled layout of
    `gemm_mxfp8`): the OCP MX contract of oracle.dit_oracle.mx_quant.  K % 128 == 0.  w_order=True: the scale order of the GEMM's WEIGHT
    operand (ce_quant_rows_mxfp8_w; weights are quantised once at load time), else of its activation operand."""
    _dev(x, torch.bfloat16, "x")
    M, K, ldx = _rows(x, "x")
    if out is None:
        out = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty((mx_scale_bytes(M, K),), dtype=torch.uint8, device=x.device)
    _dev(out, torch.uint8, "out"), _dev(scale, torch.uint8, "scale")
    assert scale.is_contiguous() and scale.numel() >= mx_scale_bytes(M, K)
    _, _, ldq = _rows(out, "out")
    st = _prof_begin()
    # (an A/B build with the staged epilogue of rounds 3-5, -DF8_EPI_LDS=1 = ce_build_info bit 2, reads the W scales in the A order)
    w_order = w_order and not getattr(lib(), "ce_build_info")() & 4  # (returns flags, not a status: not a _launch)
    _launch("ce_quant_rows_mxfp8_w" if w_order else "ce_quant_rows_mxfp8", _ptr(x), _ptr(out), _ptr(scale), M, K, ldx, ldq, _stream())
    _prof_end(st, f"quant_mxfp8_{M}x{K}", 3.0 * M * K)
    return out, scale


def ln_affine_mxfp8(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, eps: float, out: torch.Tensor, scale: torch.Tensor,
                    ab_rows: int = 0, ab_stride: int = 0):
    """ln_affine + quant_rows_mxfp8 in one pass: out (uint8 e4m3) and the tiled E8M0 scales of LN(x) * a + b rounded to bf16."""
    _dev(x, torch.bfloat16, "x"), _dev(a, torch.float32, "a"), _dev(b, torch.float32, "b")
    _dev(out, torch.uint8, "out"), _dev(scale, torch.uint8, "scale")
    M, D, ldx = _rows(x, "x")
    assert scale.is_contiguous() and scale.numel() >= mx_scale_bytes(M, D)
    _, _, ldq = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_ln_affine_mxfp8", _ptr(x), _ptr(out), _ptr(scale), _ptr(a), _ptr(b), M, D, ldx, ldq, float(eps), int(ab_rows),
            int(ab_stride), _stream())
    _prof_end(st, f"ln_affine_mxfp8_{M}x{D}", 3.0 * M * D)
    return out, scale


def gemm_mxfp8(aq: torch.Tensor, sa: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, bias: Optional[torch.Tensor],
               out: Optional[torch.Tensor] = None, epilogue: int = EPI_BIAS, gate: Optional[torch.Tensor] = None,
               res: Optional[torch.Tensor] = None, gate_rows: int = 0):
    """out[M,N] (bf16) = epilogue(MX-scaled aq @ wq^T + bias); aq [M,K], wq [N,K] uint8 (e4m3) with their tiled E8M0 scale buffers: sa in the
    A order (every activation producer writes it), sw in the W order (`quant_rows_mxfp8(w, w_order=True)`)."""
    _dev(aq, torch.uint8, "aq"), _dev(wq, torch.uint8, "wq"), _dev(sa, torch.uint8, "sa"), _dev(sw, torch.uint8, "sw")
    M, K, lda = _rows(aq, "aq")
    N, K2, ldw = _rows(wq, "wq")
    if K != K2 or sa.numel() < mx_scale_bytes(M, K) or sw.numel() < mx_scale_bytes(N, K):
        raise ValueError("gemm_mxfp8: operand / scale shapes do not match")
    if bias is not None:
        _dev(bias, torch.float32, "bias")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=aq.device)
    _dev(out, torch.bfloat16, "out")
    _, _, ldc = _rows(out, "out")
    ldres = 0
    if epilogue == EPI_GATE_RES:
        if res is None:
            raise ValueError("EPI_GATE_RES needs res")
        _dev(res, torch.bfloat16, "res")
        _, _, ldres = _rows(res, "res")
        if gate is not None:
            _dev(gate, torch.float32, "gate")
    ws, ws_bytes = _gemm_scratch(aq.device)
    st = _prof_begin()
    _launch("ce_gemm_mxfp8", _ptr(aq), _ptr(wq), _ptr(out), _ptr(sa), _ptr(sw), _ptr(bias), epilogue, _ptr(gate), _ptr(res), M, N, K, lda, ldw,
            ldc, ldres, int(gate_rows), ws, ws_bytes, _stream())
    _prof_end(st, f"gemm_mxfp8_{M}x{N}x{K}_epi{epilogue}", 2.0 * M * N * K)
    return out


def gemm_mxfp8_gelu_quant(aq: torch.Tensor, sa: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, bias: Optional[torch.Tensor],
                          out: torch.Tensor, scale: torch.Tensor):
    """quant_rows_mxfp8(gelu_tanh(aq @ wq^T + bias) rounded to bf16) with the quantisation fused into the GEMM epilogue: `out` (uint8 e4m3
    [M, N]) and `scale` (tiled E8M0 bytes of an [M, N] operand) are the next GEMM's A operand; no bf16 matrix is written.  N % 128 == 0."""
    _dev(aq, torch.uint8, "aq"), _dev(wq, torch.uint8, "wq"), _dev(sa, torch.uint8, "sa"), _dev(sw, torch.uint8, "sw")
    _dev(out, torch.uint8, "out"), _dev(scale, torch.uint8, "scale")
    M, K, lda = _rows(aq, "aq")
    N, K2, ldw = _rows(wq, "wq")
    Mo, No, ldq = _rows(out, "out")
    if K != K2 or (Mo, No) != (M, N) or sa.numel() < mx_scale_bytes(M, K) or sw.numel() < mx_scale_bytes(N, K) or scale.numel() < mx_scale_bytes(M, N):
        raise ValueError("gemm_mxfp8_gelu_quant: operand / scale shapes do not match")
    if bias is not None:
        _dev(bias, torch.float32, "bias")
    ws, ws_bytes = _gemm_scratch(aq.device)
    st = _prof_begin()
    _launch("ce_gemm_mxfp8_gelu_quant", _ptr(aq), _ptr(wq), _ptr(sa), _ptr(sw), _ptr(bias), _ptr(out), _ptr(scale), M, N, K, lda, ldw, ldq,
            ws, ws_bytes, _stream())
    _prof_end(st, f"gemm_mxfp8_{M}x{N}x{K}_gelu_quant", 2.0 * M * N * K)
    return out, scale


def set_gemm_fp8_variant(v: int) -> int:
    """Main loop of `gemm_fp8`: 0 = 8 waves / 4 phases, 1 = one wave per SIMD (ce_gemm_fp8w4.hip); returns the previous setting."""
    return _set_knob("ce_set_gemm_fp8_variant", v)


def gemm_fp8(aq: torch.Tensor, sa: torch.Tensor, wq: torch.Tensor, sw: torch.Tensor, bias: Optional[torch.Tensor],
             out: Optional[torch.Tensor] = None, epilogue: int = EPI_BIAS, gate: Optional[torch.Tensor] = None,
             res: Optional[torch.Tensor] = None, gate_rows: int = 0):
    """out[M,N] (bf16) = epilogue(sa[:,None] * sw[None,:] * (aq @ wq^T) + bias); aq [M,K], wq [N,K] uint8 (fp8 e4m3)."""
    _dev(aq, torch.uint8, "aq"), _dev(wq, torch.uint8, "wq"), _dev(sa, torch.float32, "sa"), _dev(sw, torch.float32, "sw")
    M, K, lda = _rows(aq, "aq")
    N, K2, ldw = _rows(wq, "wq")
    if K != K2 or sa.numel() != M or sw.numel() != N:
        raise ValueError("gemm_fp8: operand / scale shapes do not match")
    if bias is not None:
        _dev(bias, torch.float32, "bias")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=aq.device)
    _dev(out, torch.bfloat16, "out")
    _, _, ldc = _rows(out, "out")
    ldres = 0
    if epilogue == EPI_GATE_RES:
        if res is None:
            raise ValueError("EPI_GATE_RES needs res")
        _dev(res, torch.bfloat16, "res")
        _, _, ldres = _rows(res, "res")
        if gate is not None:
            _dev(gate, torch.float32, "gate")
    ws, ws_bytes = _gemm_scratch(aq.device)  # the one-wave-per-SIMD loop cuts a partially filled last round of tiles along K (as ce_gemm_bf16)
    st = _prof_begin()
    _launch("ce_gemm_fp8", _ptr(aq), _ptr(wq), _ptr(out), _ptr(sa), _ptr(sw), _ptr(bias), epilogue, _ptr(gate), _ptr(res), M, N, K,
            lda, ldw, ldc, ldres, int(gate_rows), ws, ws_bytes, _stream())
    _prof_end(st, f"gemm_fp8_{M}x{N}x{K}_epi{epilogue}", 2.0 * M * N * K)
    return out


# ------------------------------------------------------------------------------------------
# MXFP8 self-attention (fp8 mode; contract: chronoedit_amd/csrc/ce_attn_fp8.hip, oracle.dit_oracle.attention_mxfp8)
# ------------------------------------------------------------------------------------------
MXFP8_Q_SCALE = 128 ** -0.5 * 1.4426950408889634  # softmax_scale * log2(e): what the q producer multiplies in (head_dim 128)


def rmsnorm_rope_mxfp8(x: torch.Tensor, w: torch.Tensor, cos_sin: Optional[torch.Tensor], head_dim: int, eps: float,
                       out: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, post_scale: float = 1.0):
    """RMSNorm across heads (+ RoPE) of x [M, D] (bf16, row stride free), times post_scale -> (q8 [M, D] uint8 e4m3, s8 [M, D/32]
    uint8 E8M0): MXFP8 blocks of 32 head channels.  The attention kernel expects q produced with post_scale = MXFP8_Q_SCALE
    (scores then come out of the matrix pipe in the exp2 domain) and k with 1."""
    _dev(x, torch.bfloat16, "x"), _dev(w, torch.float32, "w")
    M, D, ldx = _rows(x, "x")
    rope_rows = 0
    if cos_sin is not None:
        _dev(cos_sin, torch.float32, "cos_sin")
        assert cos_sin.is_contiguous() and cos_sin.shape[1:] == (head_dim // 2, 2) and M % cos_sin.shape[0] == 0
        rope_rows = cos_sin.shape[0]
    if out is None:
        out = torch.empty((M, D), dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty((M, D // 32), dtype=torch.uint8, device=x.device)
    _dev(out, torch.uint8, "out"), _dev(scale, torch.uint8, "scale")
    assert scale.is_contiguous() and scale.shape == (M, D // 32)
    _, _, ldq = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_rmsnorm_rope_mxfp8", _ptr(x), _ptr(w), _ptr(cos_sin), _ptr(out), _ptr(scale), M, D, ldx, ldq, head_dim, float(eps), rope_rows,
            float(post_scale), _stream())
    _prof_end(st, f"rmsnorm_rope_mxfp8_{M}x{D}", 3.0 * M * D)
    return out, scale


def v_mxfp8_transpose(v: torch.Tensor, n_tokens: int, batch: int, heads: int, out: Optional[torch.Tensor] = None,
                      scale: Optional[torch.Tensor] = None):
    """v [batch*n_tokens, heads*128] bf16 (row stride free) -> (v8t [batch, heads, 128, npad] uint8, sv [batch, heads, npad/64, 128, 2] uint8),
    npad = n_tokens rounded up to 64: V^T tiles in the key order of the attention kernel's P operand, MXFP8 blocks of 32 consecutive keys
    (sv[.., t, d, beta] = E8M0 scale of keys 64 t + 32 beta .. of channel d)."""
    _dev(v, torch.bfloat16, "v")
    Mv, Dv, ldv = _rows(v, "v")
    assert Mv == batch * n_tokens and Dv == heads * 128
    npad = (n_tokens + 63) // 64 * 64
    if out is None:
        out = torch.empty((batch, heads, 128, npad), dtype=torch.uint8, device=v.device)
    if scale is None:
        scale = torch.empty((batch, heads, npad // 64, 128, 2), dtype=torch.uint8, device=v.device)
    assert out.is_contiguous() and scale.is_contiguous() and out.shape == (batch, heads, 128, npad) and scale.shape == (batch, heads, npad // 64, 128, 2)
    st = _prof_begin()
    _launch("ce_v_mxfp8_transpose", _ptr(v), ldv, _ptr(out), _ptr(scale), n_tokens, batch, heads, npad, _stream())
    _prof_end(st, f"v_mxfp8_transpose_{Mv}x{Dv}", 3.0 * Mv * Dv)
    return out, scale


def set_attention_mxfp8_variant(v: int) -> int:
    """0: plain loop (exact running maximum every tile), 1: software-pipelined with the speculative offset (default); returns the
    previous setting.  (A one-wave-per-SIMD form, 4 waves x 64 rows, measured 1.20 vs 1.71 PFLOP/s at 28 800 keys and was removed:
    profiles/r02_microbench_attn_mxfp8.txt.)"""
    return _set_knob("ce_set_attention_mxfp8_variant", v)


def set_attention_mxfp8_persistent(n: int) -> int:
    """(diagnostic build) workgroups of the persistent MXFP8 attention form: 0 = one workgroup per work item, default 512; returns the previous value."""
    return _set_knob("ce_set_attention_mxfp8_persistent", n)


def attention_mxfp8(q8: torch.Tensor, sq: torch.Tensor, k8: torch.Tensor, sk: torch.Tensor, v8t: torch.Tensor, sv: torch.Tensor,
                    heads: int, out: Optional[torch.Tensor] = None, batch: int = 1, out8: Optional[torch.Tensor] = None,
                    scale8: Optional[torch.Tensor] = None, add: Optional[torch.Tensor] = None):
    """Attention on the MX-fp8 matrix instruction from the operands the two producers above write (q with post_scale =
    MXFP8_Q_SCALE); out [batch*Nq, heads*128] bf16 - or, with out8 / scale8, the same values as the MX fp8 operand of the out-projection
    (e4m3 rows + tiled E8M0 block scales, bit-identical to quant_rows_mxfp8 of the bf16 output).
    add: bf16 rows [batch*Nq, heads*128] added to this call's bf16-rounded result before it is stored / quantised - the second segment of the
    cross-attention (`add` = the text segment's result; `out` may be `add` itself)."""
    for n, t in (("q8", q8), ("sq", sq), ("k8", k8), ("sk", sk), ("v8t", v8t), ("sv", sv)):
        _dev(t, torch.uint8, n)
    Mq, D, ldq = _rows(q8, "q8")
    Mk, _, ldk = _rows(k8, "k8")
    assert D == heads * 128 and Mq % batch == 0 and Mk % batch == 0
    nq, nkv = Mq // batch, Mk // batch
    npad = v8t.shape[-1]
    assert sq.is_contiguous() and sk.is_contiguous() and v8t.is_contiguous() and sv.is_contiguous()
    assert sq.shape == (Mq, D // 32) and sk.shape == (Mk, D // 32) and v8t.shape == (batch, heads, 128, npad) and sv.shape == (batch, heads, npad // 64, 128, 2)
    if add is not None:
        _dev(add, torch.bfloat16, "add")
        Ma, Da, lda = _rows(add, "add")
        assert (Ma, Da) == (Mq, D)
        ld8 = ldo = 0
        if out8 is not None:
            _dev(out8, torch.uint8, "out8"), _dev(scale8, torch.uint8, "scale8")
            _, D8, ld8 = _rows(out8, "out8")
            assert out8.shape[0] == Mq and D8 == D and scale8.is_contiguous() and scale8.numel() >= mx_scale_bytes(Mq, D)
        else:
            if out is None:
                out = add
            _dev(out, torch.bfloat16, "out")
            _, _, ldo = _rows(out, "out")
        st = _prof_begin()
        _launch("ce_attention_mxfp8_add", _ptr(q8), _ptr(sq), _ptr(k8), _ptr(sk), _ptr(v8t), _ptr(sv), _ptr(add), lda, _ptr(out) if out8 is None else None,
                ldo, _ptr(out8), _ptr(scale8) if out8 is not None else None, ld8, nq, nkv, npad, heads, 128, ldq, ldk, batch,
                _stream())
        _prof_end(st, f"attention_mxfp8_{nq}x{nkv}_h{heads}" + (f"_b{batch}" if batch > 1 else "") + "_add" + ("_mxq" if out8 is not None else ""),
                  4.0 * nq * nkv * 128 * heads * batch)
        return out8 if out8 is not None else out
    if out8 is not None:
        _dev(out8, torch.uint8, "out8"), _dev(scale8, torch.uint8, "scale8")
        _, D8, ld8 = _rows(out8, "out8")
        assert out8.shape[0] == Mq and D8 == D and scale8.is_contiguous() and scale8.numel() >= mx_scale_bytes(Mq, D)
        st = _prof_begin()
        _launch("ce_attention_mxfp8_quant", _ptr(q8), _ptr(sq), _ptr(k8), _ptr(sk), _ptr(v8t), _ptr(sv), _ptr(out8), _ptr(scale8), nq, nkv, npad,
                heads, 128, ldq, ldk, ld8, batch, _stream())
        _prof_end(st, f"attention_mxfp8_{nq}x{nkv}_h{heads}" + (f"_b{batch}" if batch > 1 else "") + "_mxq", 4.0 * nq * nkv * 128 * heads * batch)
        return out8
    if out is None:
        out = torch.empty((Mq, D), dtype=torch.bfloat16, device=q8.device)
    _dev(out, torch.bfloat16, "out")
    _, _, ldo = _rows(out, "out")
    st = _prof_begin()
    _launch("ce_attention_mxfp8", _ptr(q8), _ptr(sq), _ptr(k8), _ptr(sk), _ptr(v8t), _ptr(sv), _ptr(out), nq, nkv, npad, heads, 128, ldq, ldk, ldo,
            batch, _stream())
    _prof_end(st, f"attention_mxfp8_{nq}x{nkv}_h{heads}" + (f"_b{batch}" if batch > 1 else ""), 4.0 * nq * nkv * 128 * heads * batch)
    return out


# ------------------------------------------------------------------------------------------
# weight-side LoRA merge (csrc/ce_lora.hip)
# ------------------------------------------------------------------------------------------
LORA_RANK_MULT = 32   # ce_lora_merge_bf16 walks the rank in chunks of one MFMA contraction
LORA_MAX_RANK = 512
LORA_MAX_ADAPTERS = 8


def lora_pad_rank(a: torch.Tensor, b: torch.Tensor):
    """(A [r, K], B [N, r]) -> the same pair with r zero-padded to the next multiple of 32 (zero ranks add exact zeros to the
    product), contiguous.  A pair that already fits is returned as it is."""
    r = a.shape[0]
    rp = (r + LORA_RANK_MULT - 1) // LORA_RANK_MULT * LORA_RANK_MULT
    if rp == r:
        return a.contiguous(), b.contiguous()
    a2 = torch.zeros((rp, a.shape[1]), dtype=a.dtype, device=a.device)
    a2[:r] = a
    b2 = torch.zeros((b.shape[0], rp), dtype=b.dtype, device=b.device)
    b2[:, :r] = b
    return a2, b2


def lora_merge(w0: torch.Tensor, adapters, out: Optional[torch.Tensor] = None):
    """out[N,K] = bf16(fp32(w0) + sum_i scale_i * (b_i @ a_i)) for adapters = [(a_i [r_i, K], b_i [N, r_i], scale_i), ...], all bf16 on
    the GPU: the rank products accumulate in fp32 on the MFMA, each is multiplied by its scale and added onto fp32(w0) in list order,
    one rounding (the contract of ce_lora_merge_bf16).  out may be w0 itself or a row view of a taller buffer; an empty list copies w0.
    Ranks that are no multiple of 32 are zero-padded here (callers that switch often pad once with lora_pad_rank)."""
    _dev(w0, torch.bfloat16, "w0")
    N, K, ldw0 = _rows(w0, "w0")
    if out is None:
        out = torch.empty((N, K), dtype=torch.bfloat16, device=w0.device)
    _dev(out, torch.bfloat16, "out")
    No, Ko, ldw = _rows(out, "out")
    if (No, Ko) != (N, K) or out.device != w0.device:
        raise ValueError(f"lora_merge: out is {tuple(out.shape)} on {out.device}, w0 {tuple(w0.shape)} on {w0.device}")
    adapters = list(adapters)
    if len(adapters) > LORA_MAX_ADAPTERS:
        raise ValueError(f"lora_merge: {len(adapters)} adapters in one merge (at most {LORA_MAX_ADAPTERS})")
    keep, ranks, scales = [], [], []
    for i, (a, b, s) in enumerate(adapters):
        _dev(a, torch.bfloat16, f"a[{i}]"), _dev(b, torch.bfloat16, f"b[{i}]")
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != K or b.shape[0] != N or a.shape[0] != b.shape[1]:
            raise ValueError(f"lora_merge: adapter {i} has A {tuple(a.shape)} / B {tuple(b.shape)} for a [{N}, {K}] weight")
        if a.device != w0.device or b.device != w0.device:
            raise ValueError(f"lora_merge: adapter {i} is not on {w0.device}")
        a, b = lora_pad_rank(a, b)
        if a.shape[0] > LORA_MAX_RANK:
            raise ValueError(f"lora_merge: adapter {i} has rank {a.shape[0]} (at most {LORA_MAX_RANK})")
        keep.append((a, b))
        ranks.append(a.shape[0])
        scales.append(float(s))
    n = len(keep)
    st = _prof_begin()
    _launch("ce_lora_merge_bf16", _ptr(w0), ldw0, _ptr(out), ldw, N, K, n, _ptr_array([b for _, b in keep]), _ptr_array([a for a, _ in keep]),
            (ctypes.c_int * max(n, 1))(*ranks), (ctypes.c_float * max(n, 1))(*scales), _stream())
    _prof_end(st, f"lora_merge_{N}x{K}_r{sum(ranks)}", 4.0 * N * K)
    return out
