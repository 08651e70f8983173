"""The wiring of chronoedit_amd/transformer.py: which kernel gets which tensor, modulation row, eps, bias, context segment, RoPE table and norm
weight - one wire at a time, in every bf16 host path, against the fp32 oracle (tests/wiring_util.py has the recipe and the wire list,
tests/test_dit_wiring_cpu.py the conditions it meets on the oracle alone).

Per wire and mode: the engine is built as tests/test_dit_forward_gpu.py builds it, the base and the perturbed set are loaded
(`load_synthetic_`), both forwards run, and with delta = out(perturbed) - out(base)

    err_engine = |delta_engine - delta_fp32| / |delta_fp32|   <=   3 x err_eager + 0.02

where err_eager is the same figure of the bf16-eager ORACLE for that wire (the reference's arithmetic, not the engine's; the same 3 x over
eager as test_dit_forward_gpu.py).  err_eager <= 0.15 (CPU conditions), so no cap exceeds 0.47: an ignored wire (1.0) or a crossed one
(~1.4) cannot pass.  Once per mode and case the engine's base output at the loud parameters is held to 3 x e_eager + 2e-3 of fp32.

Modes (each is different Python in transformer.py):
  default             the V^T self-attention and the V^T two-segment cross-attention;
  row_major_v         enable_transposed_v(False);
  row_major_cross_v   enable_cross_vt(False);
  cache_context       cache_context = True.  The engine first runs the BASE set with the very tensors of the perturbed forward, then the
                      perturbed set is loaded and the SECOND of two calls is compared: a context that survived the reload is a dead wire;
  compaction          `loop.compact_text_context` on the text tensor, compaction active (asserted).  128 text rows of which 8 are real:
                      `loop.text_compaction_plan` compacts only when a 64-key tile is saved, which the cases' 48 rows never do;
  compaction_off      the same tensors with enable_text_compaction(False);
  stacked_pair        one B = 2 forward, two different prompts; both samples against their own oracle forwards, plus the `s1:` wires that
                      perturb sample 1's text / image / latents only: sample 0 bit-unchanged, sample 1 inside its cap;
  shared_pair         the guidance pair as the loop runs it (`loop.make_cfg_inputs`, `loop._shared_inputs`, enable_shared_guidance(True);
                      sharing asserted active), both samples against their own oracle forwards, plus `s1:text_row`.

Measured on an MI355X (`python -m pytest tests/test_dit_wiring_gpu.py -m gpu -q -s`): 2002 tests, 27 s including every oracle forward
on the host; slowest test 0.45 s (the first engine build), a wire 0.02 - 0.06 s.  No wire exceeded its cap: nothing in transformer.py
changed.  Worst err_engine per mode, with the worst err_eager of the same mode (both at `in:latent_voxel_last`, T = 8: one token of 768),
the largest err_engine - err_eager of any wire, and the base output against fp32 (engine / eager oracle, T = 2 and T = 8):

    mode                worst err_engine   worst err_eager   largest excess   base T = 2            base T = 8
    default             0.114              0.112             0.006            1.177e-2 / 1.176e-2   1.450e-2 / 1.394e-2
    row_major_v         0.116              0.112             0.006            1.177e-2 / 1.176e-2   1.451e-2 / 1.394e-2
    row_major_cross_v   0.115              0.112             0.005            1.187e-2 / 1.176e-2   1.451e-2 / 1.394e-2
    cache_context       0.114              0.112             0.006            1.177e-2 / 1.176e-2   1.450e-2 / 1.394e-2
    compaction          0.112              0.112             0.006            1.129e-2 / 1.121e-2   1.458e-2 / 1.419e-2
    compaction_off      0.116              0.112             0.006            1.144e-2 / 1.121e-2   1.444e-2 / 1.419e-2
    stacked_pair        0.125              0.124             0.006            1.146e-2 / 1.120e-2   1.392e-2 / 1.367e-2   (sample 1)
    shared_pair         0.125              0.124             0.006            1.146e-2 / 1.120e-2   1.392e-2 / 1.367e-2   (sample 1)

The engine reproduces every change as well as the reference's own bf16 arithmetic does; the largest err_engine / cap is 0.33.

Mutants.  Each mistake was applied to a scratch copy of transformer.py (the softmax scale: the default of the attention wrappers in ops.py,
where it lives), never committed, and this file and tests/test_dit_forward_gpu.py (8 tests: the three goldens, the full-width block at 720p,
40 blocks, LoRA round trip, B = 2, signature) were run on an MI355X.  tests/test_bench_shapes_gpu.py and test_width_depth_gpu.py hold the
same whole-output bound with the same weight recipe at larger shapes and were not run under the mutants.  "new" = failures of the 2002
tests here, every mode failing alike; all 16 base-output tests fail under every mutant:

    mistake                                                    new          test_dit_forward_gpu.py
    two gate rows swapped (self-attention <-> FFN)             1970         6 (goldens, 720p block, 40 blocks, LoRA)
    norm_added_k weight replaced by norm_k's                   1970         0   <- only the new tests
    key bias of the self-attention dropped                     1858         0   <- only the new tests
    image / text segments take each other's K / V projections  1970         6
    softmax scale of head_dim 64                               1892         3 (small_T2 golden, 720p block, 40 blocks; the tiny goldens pass)
    RoPE height and width tables swapped                       1962         1 (720p block: 45 x 80 patches; every square shape passes)
    `1 + scale` written as `scale`                             1970         6
    the head's shift and scale swapped                         1986         6

Nearly every wire fails under every mutant, not just the mutated one: at the loud parameters a mistake in one branch moves the base output
by several per cent (the dropped key bias: 9.2e-2 in the fp32 oracle with the same edit at T = 2, where the older tests' weights leave it
inside their 2e-2), and every other wire's change runs through the mistaken branch.  What still passes are wires that ADD to the stream
behind the mistake, whose change does not depend on it: `proj_out.bias` and the head's shift row under every mutant, the late biases and
block 1's FFN rows under the dropped key bias.
"""
import pytest
import torch

import wiring_util as W

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

MODES = ("default", "row_major_v", "row_major_cross_v", "cache_context", "compaction", "compaction_off", "stacked_pair", "shared_pair")
PAIR_MODES = ("stacked_pair", "shared_pair")


def cases_of(mode):
    return [c.name for c in W.LONG_TEXT.values()] if mode.startswith("compaction") else list(W.CASES)


def wires_of(mode, case):
    ws = [w.name for w in W.wires_of(case)]
    if mode == "stacked_pair":
        ws += [w.name for w in W.sample1_wires()]
    if mode == "shared_pair":
        ws += ["s1:text_row"]  # (the pair's latents, timestep and image are one tensor each)
    return ws


class _Runner:
    """One mode at one case: its model(s), what is loaded, the device copies of every host tensor, the base outputs."""

    def __init__(self, mode, case):
        self.mode, self.case = mode, case
        self.pair = mode in PAIR_MODES
        self.models, self.loaded, self.dev, self.pairs, self.base_out = {}, {}, {}, {}, {}

    def _dev(self, t):
        hit = self.dev.get(id(t))
        if hit is None:
            hit = self.dev[id(t)] = (t, t.to("cuda:0"))  # (the host tensor is kept: its id stays its own)
        return hit[1]

    def model(self, cfg):
        key = cfg.rope_temporal_skip_len
        if key not in self.models:
            from chronoedit_amd.transformer import ChronoEditTransformer3DModel
            m = ChronoEditTransformer3DModel(
                num_attention_heads=cfg.num_attention_heads, attention_head_dim=cfg.attention_head_dim, in_channels=cfg.in_channels,
                out_channels=cfg.out_channels, text_dim=cfg.text_dim, freq_dim=cfg.freq_dim, ffn_dim=cfg.ffn_dim,
                num_layers=cfg.num_layers, image_dim=cfg.image_dim, added_kv_proj_dim=cfg.added_kv_proj_dim,
                rope_temporal_skip_len=cfg.rope_temporal_skip_len, device="cuda:0", dtype=BF)
            if self.mode == "row_major_v":
                m.enable_transposed_v(False)
            elif self.mode == "row_major_cross_v":
                m.enable_cross_vt(False)
            elif self.mode == "cache_context":
                m.cache_context = True
            elif self.mode == "compaction_off":
                m.enable_text_compaction(False)
            elif self.mode == "shared_pair":
                m.enable_shared_guidance(True)
            self.models[key] = m
        return key, self.models[key]

    def _load(self, key, m, params):
        if self.loaded.get(key) is not params:
            m.load_synthetic_({k: self._dev(v) for k, v in params.items()})
            self.loaded[key] = params

    def _pair(self, name, a, b):
        """The two samples' device tensors as one batch, one tensor per pair of host tensors (so a context cache could recognise it)."""
        k = (name, id(a), id(b))
        if k not in self.pairs:
            self.pairs[k] = torch.cat([self._dev(a), self._dev(b)], 0)
        return self.pairs[k]

    def _once(self, m, xs):
        from chronoedit_amd import loop
        x0, x1 = xs[0], xs[-1]
        ts = torch.tensor([x["ts"] for x in xs], device="cuda:0")
        if self.mode == "shared_pair":
            assert x0["lat"] is x1["lat"] and x0["image"] is x1["image"] and x0["ts"] == x1["ts"]
            k = ("cfg", id(x0["text"]), id(x1["text"]), id(x0["image"]))
            if k not in self.pairs:
                self.pairs[k] = loop.make_cfg_inputs(self._dev(x0["text"]), self._dev(x1["text"]), self._dev(x0["image"]))
            text, image = self.pairs[k]
            with loop._shared_inputs(m):
                out = m(self._pair("lat", x0["lat"], x0["lat"]), ts, text, image, return_dict=False)[0]
                assert m.engine()._share_image(text, image)
        elif self.pair:
            out = m(self._pair("lat", x0["lat"], x1["lat"]), ts, self._pair("text", x0["text"], x1["text"]),
                    self._pair("image", x0["image"], x1["image"]), return_dict=False)[0]
        else:
            text, image = self._dev(x0["text"]), self._dev(x0["image"])
            if self.mode.startswith("compaction"):
                loop.compact_text_context(text)
            out = m(self._dev(x0["lat"]), ts, text, image, return_dict=False)[0]
            if self.mode.startswith("compaction"):
                assert (m.engine()._text_compact(text, image) is not None) == (self.mode == "compaction")
        assert out.dtype == BF
        return out.float().cpu()

    def forward(self, states, prime=None):
        """states: one (params, inputs, cfg) per sample (same params and cfg) -> one output per sample.  prime (cache_context): a state whose
        forward runs first, on the same model, so that the engine holds a cached context of OTHER parameters when `states` are loaded."""
        params, _, cfg = states[0]
        key, m = self.model(cfg)
        xs = [s[1] for s in states]
        if self.mode == "cache_context":
            if prime is not None:
                self._load(key, m, prime[0][0])
                self._once(m, [s[1] for s in prime])
            self._load(key, m, params)
            first, out = self._once(m, xs), self._once(m, xs)
            assert torch.equal(first, out)  # (the cached context is the computed one)
        else:
            self._load(key, m, params)
            out = self._once(m, xs)
        return [out[i:i + 1] for i in range(len(states))]

    def states(self, base, wire=None):
        if not self.pair:
            return [W.state(self.case, base, wire)]
        s1only = wire is not None and W.WIRE_BY_NAME[wire].sample1
        s0, s1 = W.state(self.case, base, None if s1only else wire), W.state(self.case, base, wire, True)
        for k, v in s0[0].items():
            assert torch.equal(v, s1[0][k]), k  # (one set of parameters for both samples)
        if self.mode == "shared_pair":  # one tensor for what the pair shares
            assert torch.equal(s0[1]["lat"], s1[1]["lat"]) and torch.equal(s0[1]["image"], s1[1]["image"])
            s1 = (s0[0], dict(s1[1], lat=s0[1]["lat"], image=s0[1]["image"]), s0[2])
        return [s0, (s0[0], s1[1], s0[2])]

    def base(self, base):
        if base not in self.base_out:
            self.base_out[base] = self.forward(self.states(base))
        return self.base_out[base]

    def perturbed(self, wire):
        w = W.WIRE_BY_NAME[wire]
        st = self.states(w.base, wire)
        prime = None
        if self.mode == "cache_context":  # the base parameters under the perturbed forward's own inputs and config
            prime = [(W.state(self.case, w.base)[0], s[1], s[2]) for s in st]
        return self.forward(st, prime)


_RUNNERS = {}
_WORST = {}  # mode -> [worst err_engine, its err_eager, its cap, wire]


def runner(mode, case) -> _Runner:
    if (mode, case) not in _RUNNERS:
        _RUNNERS[(mode, case)] = _Runner(mode, case)
    return _RUNNERS[(mode, case)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for mode, (e, ee, cap, name) in _WORST.items():
        print(f"\nwiring {mode}: worst err_engine / cap {e:.3f} / {cap:.3f} (err_eager {ee:.3f}) at {name}")
    _RUNNERS.clear()


@pytest.mark.parametrize("mode,case", [(m, c) for m in MODES for c in cases_of(m)])
def test_base_output_at_loud_parameters(mode, case):
    got = runner(mode, case).base("loud")
    for s, out in enumerate(got):
        ref32, ref_bf = W.reference(case, "loud", None, s == 1)
        e, e_eager = W.rel_l2(out, ref32), W.rel_l2(ref_bf, ref32)
        print(f"{mode} {case} sample {s}: hip-vs-fp32 {e:.3e}  bf16-eager-oracle-vs-fp32 {e_eager:.3e}")
        assert out.shape == ref32.shape and torch.isfinite(out).all()
        assert e <= 3 * e_eager + 2e-3


@pytest.mark.parametrize("mode,case,wire", [pytest.param(m, c, w, id=f"{m}-{c}-{w}") for m in MODES for c in cases_of(m) for w in wires_of(m, c)])
def test_wire(mode, case, wire):
    r = runner(mode, case)
    w = W.WIRE_BY_NAME[wire]
    got_b, got_p = r.base(w.base), r.perturbed(wire)
    for s in range(len(got_b)):
        if w.sample1 and s == 0:
            assert torch.equal(got_p[0], got_b[0])  # nothing of sample 1 reaches sample 0
            continue
        text_b = s == 1
        ref_b, ref_p = W.reference(case, w.base, None, text_b)[0], W.reference(case, w.base, wire, text_b)[0]
        if not w.sample1 and torch.equal(ref_b, ref_p):
            assert False, f"{wire} does not reach sample {s} of the oracle"
        size, err = W.delta_err(got_b[s], got_p[s], ref_b, ref_p)
        _, err_eager = W.wire_figures(case, w, text_b)
        cap = 3 * err_eager + 0.02
        print(f"{mode} {case} {wire} sample {s}: size {size:.3f}  err_engine {err:.3f}  err_eager {err_eager:.3f}  cap {cap:.3f}")
        if mode not in _WORST or err / cap > _WORST[mode][0] / _WORST[mode][2]:
            _WORST[mode] = [err, err_eager, cap, f"{case} {wire} sample {s}"]
        assert err <= cap
