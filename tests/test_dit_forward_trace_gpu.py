"""The launch sequence of DiTEngine.forward, traced on the device: which op runs when, on which buffer, at which offset, shape and stride, in
every mode that is different Python in chronoedit_amd/transformer.py.  The companion of tests/test_loop_trace_cpu.py and
tests/test_call_trace_cpu.py for the engine's hot path (the engine refuses a CPU model, so this one needs the GPU).  The numbers are
tests/test_dit_wiring_gpu.py's business; here only the wiring of the launches is pinned, so that moving host code around shows at once.

The recorder replaces the name `ops` inside chronoedit_amd.transformer with a proxy.  For every call it appends one line - the op name and
one entry per argument - and then calls the real op.  The arguments are bound to the op's signature first: the required ones are shown in
order, an optional one as name=value, and only where it differs from its default - `ab_rows=0` spelled out and left out are one launch and
one line.  Scalars, None, tuples and lists are shown by value; a tensor as

    owner+element_offset[shape]/stride        ("+0" and the stride of a contiguous tensor are left out)

`owner` is found by address range in a table built in front of the traced forward, behind at least one warm-up forward, in this order:
the call's inputs (`in.*`, with the compacted text's rows, counts and weights), every tensor attribute of the engine (`eng.*`), every field
of every block pack (`blk<li>.*`), the fields of the current workspace (`ws.*`), the context buffers and cached contexts (`cb<i>.*`,
`cc<form>.*`), the TeaCache buffers (`tea.*`) and the sparse state (`sp.k`, `sp.vt`, `sp.ws.*`, `sp.ids`, `sp.cs`).  Where ranges alias the
first registered owner wins: `xs` shows as a range of `ws.ffn`, layer 1's context K as an offset into layer 0's view.  A tensor that
nobody owns - what an op returned, or what torch made inside the forward - is named t0, t1, ... in order of appearance with its storage as
its range; the recorder keeps it (and every table entry) alive until the forward ends, so no address appears under two names.

Shape: tests/wiring_util.CFG (2 heads x 128, ffn 512, 2 layers: D = 256 and F = 512 meet the fp8 modes' multiple-of-256 rule) at case T2 -
2 latent frames of 16 x 16, N = 128 tokens, 48 text rows, 257 image rows; LONG_TEXT["T2"] (128 text rows, 8 real) where compaction must be
active; sparse ids of a rectangle with margin 1: 40 of 128 tokens.  The traced forward is the second of its kind, except where the mode is
a sequence of its own (cache miss then hit, TeaCache compute then skip, measure step 0 then 1, refresh then sparse).  The sharded (Ulysses
/ CFG-parallel) branches need several ranks and are tests/test_ulysses.py's.

The expected traces are tests/golden/dit_forward_traces.json, {mode: [lines]}, recorded by running this module as a script
(`python tests/test_dit_forward_trace_gpu.py [out.json]`) at commit c570bb5 - the last one in which the block stack was written out three
times (forward, _forward_sparse, _block0_shared_prefix) - and unchanged since: the refactor that gave every launch group one method had
to reproduce it line by line, and did.

Mutants.  Each mistake was applied to a scratch copy of transformer.py, never committed, and this file run on an MI355X (33 tests, 3 s).
All three sit in code that computes finite numbers of the right shape either way; the trace names the first differing line:

    mistake                                                      failing traces
    the V^T self-attention norms into ws.att instead of ws.h     16: every mode that runs the bf16 V^T self-attention - default,
                                                                 row_major_cross_v, no_image, no_cross_attn_norm, stacked_pair, shared_pair,
                                                                 compaction, compaction_shared_pair, cache_miss, cache_hit, tea_compute_*,
                                                                 tea_measure_step0 / 1, sparse_refresh_* (first differing line: its ln_affine)
    rmsnorm_rope_ in front of the V^T GEMM                       the same 16 (first differing line: the V^T GEMM's place)
    res_rows=N dropped from the block-0 fan-out                  4: shared_pair, compaction_shared_pair, tea_compute_shared,
                                                                 sparse_refresh_shared (line 33, the fan-out's out-projection)

The 17 (29) others pass: row_major_v, the fp8 GEMM and fp8 attention modes and the sparse steps run another self-attention, a skipped step
runs no block, and only the shared pair has a fan-out.
"""
import contextlib
import inspect
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import wiring_util as W

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_forward_traces.json")
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------------------------------
# the recorder
# ------------------------------------------------------------------------------------------------------------------------------------
def _extent(t: torch.Tensor) -> int:
    """Bytes from the tensor's first element to one past its last."""
    if t.numel() == 0:
        return 0
    return (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()


def _walk(prefix: str, obj, out: list):
    """(name, tensor) of every tensor inside obj, depth first in the containers' own order."""
    if isinstance(obj, torch.Tensor):
        out.append((prefix, obj))
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            _walk(f"{prefix}.{i}", v, out)
    elif isinstance(obj, dict):
        for i, v in enumerate(obj.values()):
            _walk(f"{prefix}.{i}", v, out)
    elif isinstance(obj, SimpleNamespace):
        for k, v in vars(obj).items():
            _walk(f"{prefix}.{k}", v, out)


_ENGINE_SECTIONS = ("model", "blk", "_ws", "_ctx_bufs", "_ctx_cache", "_tea_res", "_tea_prev", "_tea_sums", "_sparse")


def owner_table(eng, inputs: dict, rows: int) -> list:
    found: list = []
    for k, v in inputs.items():
        _walk("in." + k, v, found)
        cmp = getattr(v, "_ce_compact", None)
        if cmp is not None:
            _walk(f"in.{k}.c", SimpleNamespace(text=cmp.text, valid=cmp.valid, w=cmp.w), found)
    for k, v in vars(eng).items():
        if k not in _ENGINE_SECTIONS:
            _walk("eng." + k, v, found)
    for li, p in enumerate(eng.blk):
        _walk(f"blk{li}", p, found)
    _walk("ws", eng._ws.get(rows), found)
    for i, b in enumerate(eng._ctx_bufs.values()):
        _walk(f"cb{i}", b, found)
    for form, (_, ctx, _) in eng._ctx_cache.items():
        _walk(f"cc{form}", SimpleNamespace(kv=ctx.kv), found)
    _walk("tea", SimpleNamespace(res=eng._tea_res, prev=eng._tea_prev, sums=eng._tea_sums), found)
    st = eng._sparse
    if st is not None:
        _walk("sp", SimpleNamespace(k=st.k, vt=st.vt, ws=st.ws, ids=st.ids, cs=st.cs), found)
    return [(name, t.data_ptr(), t.data_ptr() + _extent(t), t) for name, t in found if t.is_cuda and t.numel()]


class Recorder:
    """Stands in for `chronoedit_amd.transformer.ops`.  Idle (lines is None) it hands every attribute through."""

    def __init__(self, real):
        self._real = real
        self.lines = None
        self._owners, self._temps = [], []

    def start(self, owners):
        self.lines, self._owners, self._temps = [], owners, []

    def stop(self):
        lines, self.lines, self._owners, self._temps = self.lines, None, [], []
        return lines

    def _tensor(self, t: torch.Tensor) -> str:
        p = t.data_ptr()
        name = None
        if t.is_cuda and t.numel():
            for table in (self._owners, self._temps):
                for n, lo, hi, _ in table:
                    if lo <= p < hi:
                        name, base = n, lo
                        break
                if name is not None:
                    break
            if name is None:
                st = t.untyped_storage()
                name, base = f"t{len(self._temps)}", st.data_ptr()
                self._temps.append((name, base, base + st.nbytes(), t))
            off = (p - base) // t.element_size()
        else:
            name, off = ("host" if not t.is_cuda else "empty"), 0
        s = name + (f"+{off}" if off else "") + "[" + ",".join(str(n) for n in t.shape) + "]"
        if not t.is_contiguous():
            s += "/" + ",".join(str(n) for n in t.stride())
        return s

    def _fmt(self, v) -> str:
        if isinstance(v, torch.Tensor):
            return self._tensor(v)
        if isinstance(v, (tuple, list)):
            return "(" + ",".join(self._fmt(x) for x in v) + ")"
        return repr(v)

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if self.lines is None or not callable(attr) or isinstance(attr, type):
            return attr
        sig = inspect.signature(attr)

        def call(*a, **kw):
            entries = []
            for k, v in sig.bind(*a, **kw).arguments.items():
                default = sig.parameters[k].default
                if default is inspect.Parameter.empty:
                    entries.append(self._fmt(v))
                elif isinstance(v, torch.Tensor) or type(v) is not type(default) or v != default:
                    entries.append(f"{k}={self._fmt(v)}")
            self.lines.append(name + "(" + ", ".join(entries) + ")")
            out = attr(*a, **kw)
            self._fmt(out)  # (names what nobody owns, and keeps it alive)
            return out
        return call


# ------------------------------------------------------------------------------------------------------------------------------------
# models, inputs, modes
# ------------------------------------------------------------------------------------------------------------------------------------
def make_model(setup=None, **ctor):
    from chronoedit_amd.transformer import ChronoEditTransformer3DModel
    cfg = W.CFG
    m = ChronoEditTransformer3DModel(
        num_attention_heads=cfg.num_attention_heads, attention_head_dim=cfg.attention_head_dim, in_channels=cfg.in_channels,
        out_channels=cfg.out_channels, text_dim=cfg.text_dim, freq_dim=cfg.freq_dim, ffn_dim=cfg.ffn_dim, num_layers=cfg.num_layers,
        image_dim=cfg.image_dim, added_kv_proj_dim=cfg.added_kv_proj_dim, rope_temporal_skip_len=cfg.rope_temporal_skip_len,
        device=DEV, dtype=BF, **ctor)
    params = W.state("T2")[0]
    m.load_synthetic_({k: params[k].to(DEV) for k, _ in m.named_parameters()})
    if setup is not None:
        setup(m)
    return m


def make_inputs(kind: str = "single", long_text: bool = False, image: bool = True) -> dict:
    """single: B = 1.  stacked: B = 2, two prompts, everything its own tensor.  shared: the guidance pair as the loop builds it."""
    from chronoedit_amd import loop
    case = (W.LONG_TEXT if long_text else W.CASES)["T2"]
    a, b = W.make_inputs(W.CFG, case), W.make_inputs(W.CFG, case, text_b=True)
    d = lambda t: t.to(DEV)
    if kind == "single":
        text = d(a["text"])
        if long_text:
            loop.compact_text_context(text)
        x = dict(hidden=d(a["lat"]), ts=torch.tensor([a["ts"]], device=DEV), text=text, image=d(a["image"]))
    elif kind == "stacked":
        x = dict(hidden=torch.cat([d(a["lat"]), d(b["lat"])], 0), ts=torch.tensor([a["ts"], 50], device=DEV),
                 text=torch.cat([d(a["text"]), d(b["text"])], 0), image=torch.cat([d(a["image"]), d(b["image"])], 0))
    else:
        text, image2 = loop.make_cfg_inputs(d(a["text"]), d(b["text"]), d(a["image"]))
        x = dict(hidden=torch.cat([d(a["lat"]), d(a["lat"])], 0), ts=torch.tensor([a["ts"], a["ts"]], device=DEV), text=text, image=image2)
    if not image:
        x["image"] = None
    x["shared"] = kind == "shared"
    return x


def recorder(monkeypatch) -> Recorder:
    import chronoedit_amd.transformer as TR
    rec = Recorder(TR.ops)
    monkeypatch.setattr(TR, "ops", rec)
    return rec


def forward(m, x, rec=None, tea=None, sparse=None):
    """One forward under the per-call flags, set as chronoedit_amd/loop.py sets them; rec: traced, returns the lines."""
    from chronoedit_amd import loop
    eng = m.engine()
    if rec is not None:
        B, _, T, Hh, Ww = x["hidden"].shape
        rows = B * T * (Hh // 2) * (Ww // 2)
        rec.start(owner_table(eng, {k: x[k] for k in ("hidden", "ts", "text", "image")}, rows))
    m._tea_mode, m._sparse_mode = tea, sparse
    try:
        with (loop._shared_inputs(m) if x["shared"] else contextlib.nullcontext()):
            m(x["hidden"], x["ts"], x["text"], x["image"], return_dict=False)
            if x["shared"]:
                assert eng._share_image(x["text"], x["image"])  # sharing is active
    finally:
        m._tea_mode = m._sparse_mode = None
        lines = rec.stop() if rec is not None else None
    torch.cuda.synchronize()
    return lines


def second(m, x, rec, **kw):
    forward(m, x, **kw)
    return forward(m, x, rec, **kw)


def sparse_ids():
    from chronoedit_amd import sparse_region
    case = W.CASES["T2"]
    w = torch.zeros((case.h, case.w), dtype=torch.float32)
    w[4:8, 4:10] = 1.0  # patches rows 2..3, columns 2..4; margin 1: 4 x 5 patches in each of the 2 frames
    ids, n = sparse_region.active_tokens(w, case.T, 1)
    N = case.T * (case.h // 2) * (case.w // 2)
    assert n == ids.numel() == 40 and ids.numel() % 8 == 0 and ids.numel() < N
    return ids


def _compacts(m, x):
    assert m.engine()._text_compact(x["text"], x["image"]) is not None  # compaction is active
    return x


def record_all(rec) -> dict:
    """{mode: lines} of every mode, in the order of the golden file."""
    out = {}
    case = W.CASES["T2"]

    def plain(name, setup=None, kind="single", **kw):
        ctor = kw.pop("ctor", {})
        m = make_model(setup, **ctor)
        x = make_inputs(kind, **kw)
        out[name] = second(m, x, rec)
        return m, x

    # bf16, B = 1
    plain("default")
    plain("row_major_v", lambda m: m.enable_transposed_v(False))
    plain("row_major_cross_v", lambda m: m.enable_cross_vt(False))
    plain("no_image", image=False)
    plain("no_cross_attn_norm", ctor=dict(cross_attn_norm=False))
    # bf16, B = 2
    plain("stacked_pair", kind="stacked")
    plain("shared_pair", kind="shared")
    # compaction
    _compacts(*plain("compaction", long_text=True))
    _compacts(*plain("compaction_shared_pair", kind="shared", long_text=True))
    # cache_context: a miss (other tensors than the warm-up's), then a hit
    m = make_model(lambda m: setattr(m, "cache_context", True))
    forward(m, make_inputs())
    x = make_inputs()
    n0 = m.engine().ctx_projections
    out["cache_miss"] = forward(m, x, rec)
    assert m.engine().ctx_projections == n0 + 1
    out["cache_hit"] = forward(m, x, rec)
    assert m.engine().ctx_projections == n0 + 1
    # TeaCache: compute then skip, on the stacked and on the shared pair; measure, two consecutive steps
    for kind in ("stacked", "shared"):
        m, x = make_model(), make_inputs(kind)
        forward(m, x, tea="compute")
        out[f"tea_compute_{kind}"] = forward(m, x, rec, tea="compute")
        out[f"tea_skip_{kind}"] = forward(m, x, rec, tea="skip")
    m, x = make_model(), make_inputs()
    forward(m, x)
    m.engine().tea_measure_begin(2)
    for row in range(2):
        m.engine()._tea_row = row
        out[f"tea_measure_step{row}"] = forward(m, x, rec, tea="measure")
    m.engine().tea_measure_end()
    # sparse region: refresh on the shared and on the stacked pair, sparse at B = 1 and B = 2
    ids = sparse_ids()
    for kind in ("shared", "stacked"):
        m, x = make_model(), make_inputs(kind)
        m.engine().sparse_begin(ids, 2, case.T, case.h, case.w)
        out[f"sparse_refresh_{kind}"] = second(m, x, rec, sparse="refresh")
        if kind == "shared":
            out["sparse_b2"] = second(m, x, rec, sparse="sparse")
    m, x = make_model(), make_inputs()
    m.engine().sparse_begin(ids, 1, case.T, case.h, case.w)
    forward(m, x, sparse="refresh")
    out["sparse_b1"] = second(m, x, rec, sparse="sparse")
    # fp8 GEMMs

    def unfused(m):
        m.fp8_fuse_quant = m.fp8_fuse_attn_quant = False
        m.enable_fp8_gemms(mx=True)
    plain("fp8_rowscale", lambda m: m.enable_fp8_gemms(mx=False))
    plain("mxfp8_fused", lambda m: m.enable_fp8_gemms(mx=True))
    plain("mxfp8_unfused", unfused)
    plain("mxfp8_mixed", lambda m: m.enable_fp8_gemms(mx=True, linears=("qkv", "q2", "o2", "f1")))  # o1 and f2 stay bf16
    # fp8 attention
    plain("fp8_attn", lambda m: m.enable_fp8_attention())
    plain("fp8_attn_cross", lambda m: m.enable_fp8_attention(cross=True))
    plain("fp8_attn_cross_no_image", lambda m: m.enable_fp8_attention(cross=True), image=False)
    # ... and with the MX GEMMs' fused operands on top (the attention kernels emit the out-projections' operands)
    plain("mxfp8_fp8_attn_cross", lambda m: m.enable_fp8_gemms(mx=True).enable_fp8_attention(cross=True))
    plain("mxfp8_fp8_attn_cross_no_image", lambda m: m.enable_fp8_gemms(mx=True).enable_fp8_attention(cross=True), image=False)
    return out


MODES = ("default", "row_major_v", "row_major_cross_v", "no_image", "no_cross_attn_norm", "stacked_pair", "shared_pair", "compaction",
         "compaction_shared_pair", "cache_miss", "cache_hit", "tea_compute_stacked", "tea_skip_stacked", "tea_compute_shared",
         "tea_skip_shared", "tea_measure_step0", "tea_measure_step1", "sparse_refresh_shared", "sparse_b2", "sparse_refresh_stacked",
         "sparse_b1", "fp8_rowscale", "mxfp8_fused", "mxfp8_unfused", "mxfp8_mixed", "fp8_attn", "fp8_attn_cross",
         "fp8_attn_cross_no_image", "mxfp8_fp8_attn_cross", "mxfp8_fp8_attn_cross_no_image")


@pytest.fixture(scope="module")
def traces():
    mp = pytest.MonkeyPatch()
    try:
        yield record_all(recorder(mp))
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_mode_is_recorded_and_pinned(traces, golden):
    assert tuple(traces) == MODES and tuple(golden) == MODES


@pytest.mark.parametrize("mode", MODES)
def test_trace(traces, golden, mode):
    got, want = traces[mode], golden[mode]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"{mode}: first difference at line {i}\n  got:      {g}\n  expected: {w}")
        assert g == w, f"{mode} line {i}"
    assert len(got) == len(want), f"{mode}: {len(got)} lines, expected {len(want)}; first extra: {(got + want)[min(len(got), len(want))]}"


@pytest.mark.parametrize("kind", ["stacked", "shared"])
def test_a_skipped_step_launches_no_block(traces, kind):
    names = [line.split("(", 1)[0] for line in traces[f"tea_skip_{kind}"]]
    assert "tea_apply_" in names and names[-1] == "unpatchify"
    assert not [n for n in names if n.startswith("attention") or n.startswith("rmsnorm")]
    assert names.count("gemm") == 2  # the patch embedding and the head


if __name__ == "__main__":
    _mp = pytest.MonkeyPatch()
    _traces = record_all(recorder(_mp))
    _mp.undo()
    assert tuple(_traces) == MODES, [k for k in _traces if k not in MODES]
    _path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(_path, "w") as f:
        json.dump(_traces, f, indent=0)
        f.write("\n")
    print(f"wrote {_path}: {len(_traces)} modes, {sum(len(v) for v in _traces.values())} lines, {os.path.getsize(_path)} bytes")
