"""Wiring checks of the DiT forward: loud parameters, one perturbed wire at a time, and the CHANGE of the output compared.

With `oracle.dit_oracle.make_synthetic_params` (Linear weights ~N(0, 0.02^2)) every branch of a block is a whisper next to the residual
stream: replacing a whole projection moves the output by well under the 2e-2 whole-output bound of the model-level tests.  Two changes
make every wire audible (neither touches the engine):

  * `loud_params`: every branch contributes at the size of the residual stream and attention is peaked;
  * `delta_err`: for one wire at a time, perturb it and compare delta = out(perturbed) - out(base) of the engine with the fp32 oracle's,
        size = |delta_ref| / |out_ref|        err = |delta_got - delta_ref| / |delta_ref|
    A wire the forward ignores gives err = 1, one that goes to the wrong place err ~ 1.4; bf16 arithmetic stays far below.

A wire is a named function (params, inputs, cfg) -> (params', inputs', cfg') on top of one of the BASES below; `perturbations(cfg)`
lists them.  The oracle's fp32 and bf16-eager outputs of every (case, base, wire, text) are computed once per process (`reference`).

Bases: "loud" is `loud_params` itself.  "flat_img" sets the image rows between the first and the last to ONE constant row: among 257
distinct keys under a peaked softmax a single row moves the output by 0.004 - 0.04; next to 255 copies of one key the two end rows carry
weight, and a forward that drops or misplaces the first or the last image row shows.  The "small" bases exist for the eps of the norms,
which is invisible while the normalised rows have rms ~1: they scale what FEEDS a norm down until the row's variance is comparable to
the eps, and their wires scale it part of the way back up ("toward normal size"), so the change of the output depends on the eps at first
order (tests/test_dit_wiring_cpu.py: a tenfold cfg.eps misses every such wire's cap):
  * small_patch:   `patch_embedding` x 1e-3 - the tokens in front of block 0's norm1 (cfg.eps), wire x 3;
  * small:<proj>:  ONE of `to_q` / `to_k` of the two attentions and `add_k_proj` of a block, weight and bias, x 3e-4 - its RMS norm
                   (cfg.eps), wire x 10.  One base per projection: with all of them small at once the scores are flat and a single
                   projection's change moves the output by 0.02 - 0.06 only;
  * small_img:     the image rows x 3e-3 and `image_embedder.ff.net.2` x 3e-3 - the image embedder's two layer norms (1e-5), wires x 3.
Not reachable through parameters alone, and left out: norm1 of deeper blocks, norm2 and norm3 of every block and the head's norm - their
input is the residual stream behind at least one branch of normal size (the self-attention's out-projection bias alone has rms 0.3), and
scaling every branch in front of them down leaves nothing of the forward to perturb.

Cases (tiny widths: 2 heads x 128, ffn 512, 2 layers, text_dim 128, image_dim 64): T = 2 at 16 x 16 latents (the temporal-skip RoPE
indices {0, skip_len - 1}) and T = 8 at 16 x 24 (the plain indices; h != w, so swapped height / width tables cannot cancel), 48 text rows
of which 8 are real.  `text_len=128` gives the variants the text-compaction mode needs: `loop.text_compaction_plan` compacts only when
every sample walks at least one 64-key tile less, which 48 rows never do.
"""
from __future__ import annotations

import dataclasses
import zlib
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from oracle import dit_oracle as O

BF = torch.bfloat16
CFG = O.DiTConfig(num_attention_heads=2, ffn_dim=512, num_layers=2, text_dim=128, image_dim=64, added_kv_proj_dim=256)
TIMESTEP = 500

SIZE_FLOOR = 0.05      # every wire moves the fp32 oracle's output by at least this (relative to its norm)
EAGER_CAP = 0.15       # the bf16-eager oracle reproduces every delta to within this
BASE_EAGER_CAP = 2e-2  # bf16-eager against fp32 oracle at the loud parameters, whole output


class Case(NamedTuple):
    name: str
    param_seed: int
    T: int
    h: int
    w: int
    text_len: int = 48
    real_text: int = 8


CASES = {"T2": Case("T2", 21, 2, 16, 16), "T8": Case("T8", 5, 8, 16, 24)}
LONG_TEXT = {k: c._replace(name=k + "_long", text_len=128) for k, c in CASES.items()}  # (module docstring: text compaction)
ALL_CASES = {**CASES, **{c.name: c for c in LONG_TEXT.values()}}


def _seed(*parts) -> int:
    return zlib.crc32("/".join(str(p) for p in parts).encode()) & 0x7FFFFFFF


def _randn(shape, *seed_parts) -> torch.Tensor:
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(_seed(*seed_parts)))


def _store(name: str, t: torch.Tensor) -> torch.Tensor:
    """Round to what the model holds: fp32 for the keep-fp32 names, bf16 otherwise (as make_synthetic_params)."""
    return t.to(torch.float32 if O.keep_fp32(name) else BF)


# ------------------------------------------------------------------------------------------------------------------------------------
# loud parameters
# ------------------------------------------------------------------------------------------------------------------------------------
QK_NORM_GAIN = 2.5


def loud_params(cfg: O.DiTConfig, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded parameters with which every branch is as large as the residual stream: Linear / conv weights ~N(0, 1 / fan_in);
    scale_shift_table (blocks and head) ~0.5 N(0, 1); biases ~0.3 N(0, 1); norm weights 1 + 0.5 N(0, 1), those of norm_q / norm_k /
    norm_added_k times 2.5 on top (scores spread over several units: peaked attention).  bf16 values, the keep-fp32 names in fp32."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in O.param_shapes(cfg).items():
        n = torch.randn(shape, generator=g)
        if name.endswith("scale_shift_table"):
            t = 0.5 * n
        elif "norm" in name and name.endswith(".weight"):
            t = 1.0 + 0.5 * n
            if any(k in name for k in ("norm_q", "norm_k", "norm_added_k")):
                t = QK_NORM_GAIN * t
        elif name.endswith(".bias"):
            t = 0.3 * n
        else:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            t = n / fan_in ** 0.5
        out[name] = _store(name, t)
    return out


TEXT_B_SEED = 3  # the second sample's text of the two-sample modes


def make_inputs(cfg: O.DiTConfig, case: Case, text_b: bool = False) -> dict:
    """{"lat", "ts", "text", "image"}: oracle.make_synthetic_inputs in bf16 (zero rows behind the real text).  text_b: another prompt of
    the same length (the second sample of a guidance pair)."""
    lat, text, image = O.make_synthetic_inputs(cfg, case.T, case.h, case.w, dtype=BF, text_len=case.text_len, real_text=case.real_text)
    if text_b:
        text = torch.randn((1, case.text_len, cfg.text_dim), generator=torch.Generator().manual_seed(TEXT_B_SEED))
        text[:, case.real_text:] = 0
        text = text.to(BF)
    return {"lat": lat, "ts": TIMESTEP, "text": text, "image": image}


# ------------------------------------------------------------------------------------------------------------------------------------
# bases and wires
# ------------------------------------------------------------------------------------------------------------------------------------
def _scaled(params, inputs, names, factor, image_factor=None):
    p = dict(params)
    for n in names:
        p[n] = _store(n, params[n].float() * factor)
    if image_factor is not None:
        inputs = dict(inputs, image=(inputs["image"].float() * image_factor).to(BF))
    return p, inputs


def _qk_names(cfg, i):
    b = f"blocks.{i}."
    return [b + "attn1.to_q", b + "attn1.to_k", b + "attn2.to_q", b + "attn2.to_k", b + "attn2.add_k_proj"]


def _wb(stems):
    return [s + e for s in stems for e in (".weight", ".bias")]


SMALL, SMALL_QK, SMALL_IMG = 1e-3, 3e-4, 3e-3
_FF2 = "condition_embedder.image_embedder.ff.net.2"


def _flat_image(x):
    t = x["image"].clone()
    t[0, 1:-1] = (_randn((t.shape[2],), "flat_img") * t.float().pow(2).mean().sqrt()).to(BF)
    return dict(x, image=t)


BASES: Dict[str, Callable] = {
    "loud": lambda p, x, cfg: (p, x),
    "small_patch": lambda p, x, cfg: _scaled(p, x, _wb(["patch_embedding"]), SMALL),
    "flat_img": lambda p, x, cfg: (p, _flat_image(x)),
    "small_img": lambda p, x, cfg: _scaled(p, x, _wb([_FF2]), SMALL_IMG, image_factor=SMALL_IMG),
}
for _i in range(CFG.num_layers):
    for _stem in _qk_names(CFG, _i):
        BASES["small:" + _stem] = (lambda stem: lambda p, x, cfg: _scaled(p, x, _wb([stem]), SMALL_QK))(_stem)


class Wire(NamedTuple):
    name: str
    base: str
    fn: Callable  # (params, inputs, cfg) -> (params', inputs', cfg')
    cases: Optional[Tuple[str, ...]] = None  # None = every case
    sample1: bool = False  # two-sample modes only: perturbs sample 1's inputs and nothing of sample 0


# A wire whose change of the fp32 oracle's output misses SIZE_FLOOR at the default factor gets a larger one here (never a lower floor).
# The key biases are the weakest wires: in front of the RMS norm a key bias shifts every key of a segment alike, and a softmax ignores what
# all its scores share; only what the norm makes of the shift is left.  8 x rms instead of the biases' 4 x.
FACTOR = {f"blocks.{i}.{stem}.bias": 8.0 for i in range(CFG.num_layers) for stem in ("attn1.to_k", "attn2.to_k", "attn2.add_k_proj")}


def _param_noise(name, factor, rows=None):
    def fn(params, inputs, cfg):
        p = dict(params)
        t = params[name].float()
        sel = t if rows is None else t[:, rows]
        noise = _randn(sel.shape, "param", name, rows) * sel.pow(2).mean().sqrt() * factor
        t = t.clone()
        if rows is None:
            t += noise
        else:
            t[:, rows] += noise
        p[name] = _store(name, t)
        return p, inputs, cfg
    return fn


def _input(fn):
    def wrapped(params, inputs, cfg):
        x = dict(inputs)
        fn(x, cfg)
        return params, x, cfg
    return wrapped


def _set_ts(v):
    def fn(x, cfg):
        x["ts"] = v
    return fn


def _text_row(row):
    def fn(x, cfg):
        t = x["text"].clone()
        t[0, row] = _randn((t.shape[2],), "text_row", row).to(BF)
        x["text"] = t
    return fn


def _text_padding(x, cfg):
    """Every padding row (the trailing run of equal rows) set to ANOTHER constant row: compaction still applies."""
    t = x["text"].clone()
    same = (t[0] == t[0, -1]).all(-1)
    first = int((~same).nonzero().max()) + 1
    t[0, first:] = _randn((t.shape[2],), "text_padding").to(BF)
    x["text"] = t


def _image_row(row):
    def fn(x, cfg):
        t = x["image"].clone()
        t[0, row] = (_randn((t.shape[2],), "image_row", row) * t.float().pow(2).mean().sqrt()).to(BF)
        x["image"] = t
    return fn


def _image_all(x, cfg):
    t = x["image"]
    x["image"] = (_randn(t.shape, "image_all") * t.float().pow(2).mean().sqrt()).to(BF)


def _lat_channels(lo, hi):
    def fn(x, cfg):
        t = x["lat"].clone()
        t[:, lo:hi] = (t[:, lo:hi].float() + _randn(t[:, lo:hi].shape, "lat", lo, hi)).to(BF)
        x["lat"] = t
    return fn


VOXEL_GAIN = 64.0  # (gain 1 moves the T = 8 output by 0.034, gain 16 by 0.052 - 0.057: one token of 768; a louder voxel replaces its token outright)


def _lat_voxel(x, cfg):
    """One latent voxel, all channels, at the last frame / last row / last column: patchify / unpatchify index order."""
    t = x["lat"].clone()
    t[0, :, -1, -1, -1] = (VOXEL_GAIN * _randn((t.shape[1],), "lat_voxel")).to(BF)
    x["lat"] = t


def _scale_wire(names, factor, image_factor=None):
    def fn(params, inputs, cfg):
        p, x = _scaled(params, inputs, names, factor, image_factor)
        return p, x, cfg
    return fn


def _skip_len(v):
    def fn(params, inputs, cfg):
        return params, inputs, dataclasses.replace(cfg, rope_temporal_skip_len=v)
    return fn


EPS_STEP, EPS_QK_STEP = 3.0, 10.0  # a small-signal wire scales its target this far back toward normal size


def perturbations(cfg: O.DiTConfig = CFG) -> List[Wire]:
    wires: List[Wire] = []
    # every parameter, one at a time: 1 x rms seeded noise; biases 4 x rms
    for name in O.param_shapes(cfg):
        f = FACTOR.get(name, 4.0 if name.endswith(".bias") else 1.0)
        wires.append(Wire(name, "loud", _param_noise(name, f)))
    # the rows of the modulation tables one by one (a whole-table perturbation averages swapped rows away)
    for i in range(cfg.num_layers):
        for r in range(6):
            n = f"blocks.{i}.scale_shift_table"
            wires.append(Wire(f"{n}[{r}]", "loud", _param_noise(n, FACTOR.get(f"{n}[{r}]", 1.0), rows=r)))
    for r in range(2):
        wires.append(Wire(f"scale_shift_table[{r}]", "loud", _param_noise("scale_shift_table", FACTOR.get(f"scale_shift_table[{r}]", 1.0), rows=r)))
    # inputs
    wires += [
        Wire("in:timestep=50", "loud", _input(_set_ts(50))),
        Wire("in:timestep=999", "loud", _input(_set_ts(999))),
        Wire("in:text_row", "loud", _input(_text_row(3))),
        Wire("in:text_padding", "loud", _input(_text_padding)),
        Wire("in:image_row_first", "flat_img", _input(_image_row(0))),
        Wire("in:image_row_last", "flat_img", _input(_image_row(-1))),
        Wire("in:latent_channels", "loud", _input(_lat_channels(0, 16))),
        Wire("in:condition_channels", "loud", _input(_lat_channels(16, 36))),
        Wire("in:latent_voxel_last", "loud", _input(_lat_voxel)),
    ]
    # config
    wires.append(Wire("cfg:rope_temporal_skip_len=5", "loud", _skip_len(5), cases=("T2", "T2_long")))
    # small-signal eps wires (module docstring)
    wires.append(Wire("eps:norm1[patch_embedding]", "small_patch", _scale_wire(_wb(["patch_embedding"]), EPS_STEP)))
    for i in range(cfg.num_layers):
        for stem in _qk_names(cfg, i):
            wires.append(Wire(f"eps:{stem}", "small:" + stem, _scale_wire(_wb([stem]), EPS_QK_STEP)))
    wires.append(Wire("eps:image_embedder.norm1[image rows]", "small_img", _scale_wire([], 1.0, image_factor=EPS_STEP)))
    wires.append(Wire("eps:image_embedder.norm2[ff.net.2]", "small_img", _scale_wire(_wb([_FF2]), EPS_STEP)))
    return wires


def sample1_wires() -> List[Wire]:
    """Two-sample modes: wires that touch sample 1 only (applied to sample 1's inputs; sample 0 must come out bit-unchanged)."""
    return [
        Wire("s1:timestep=50", "loud", _input(_set_ts(50)), sample1=True),  # (the per-sample modulation and gate rows)
        Wire("s1:text_row", "loud", _input(_text_row(3)), sample1=True),
        Wire("s1:image", "loud", _input(_image_all), sample1=True),
        Wire("s1:latent_channels", "loud", _input(_lat_channels(0, 16)), sample1=True),
    ]


WIRES: List[Wire] = perturbations(CFG)
WIRE_BY_NAME = {w.name: w for w in WIRES + sample1_wires()}


def wires_of(case_name: str) -> List[Wire]:
    return [w for w in WIRES if w.cases is None or case_name in w.cases]


# ------------------------------------------------------------------------------------------------------------------------------------
# evaluation
# ------------------------------------------------------------------------------------------------------------------------------------
def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def delta_err(got_base, got_pert, ref_base, ref_pert) -> Tuple[float, float]:
    """(size, err) of module docstring, in fp64."""
    gb, gp, rb, rp = (t.double().cpu() for t in (got_base, got_pert, ref_base, ref_pert))
    d_ref = rp - rb
    size = float(d_ref.norm() / (rb.norm() + 1e-300))
    err = float(((gp - gb) - d_ref).norm() / (d_ref.norm() + 1e-300))
    return size, err


_STATE: dict = {}
_REF: dict = {}


def state(case_name: str, base: str = "loud", wire: Optional[str] = None, text_b: bool = False):
    """(params, inputs, cfg) of a base, or of one wire applied to its base.  Cached; treat as read-only."""
    key = (case_name, base, wire, text_b)
    if key not in _STATE:
        case = ALL_CASES[case_name]
        if wire is None:
            pkey = ("loud_params", case.param_seed)  # one set of tensors per seed: an unchanged parameter is the SAME tensor in every state
            if pkey not in _STATE:
                _STATE[pkey] = loud_params(CFG, case.param_seed)
            p, x = BASES[base](_STATE[pkey], make_inputs(CFG, case, text_b), CFG)
            _STATE[key] = (p, x, CFG)
        else:
            w = WIRE_BY_NAME[wire]
            assert w.base == base, (wire, base)
            _STATE[key] = w.fn(*state(case_name, base, None, text_b))
    return _STATE[key]


def oracle(params, inputs, cfg, dtype) -> torch.Tensor:
    """The oracle's forward in fp32 arithmetic (dtype=torch.float32) or as the reference's bf16-eager run (dtype=BF, keep-fp32 names fp32)."""
    if dtype == torch.float32:
        params = {k: v.float() for k, v in params.items()}
    cast = lambda t: t.to(dtype)
    with torch.no_grad():
        return O.dit_forward(params, cfg, cast(inputs["lat"]), torch.tensor([inputs["ts"]]), cast(inputs["text"]), cast(inputs["image"]))


def reference(case_name: str, base: str = "loud", wire: Optional[str] = None, text_b: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp32 oracle output, bf16-eager oracle output) of a state, each computed once per process."""
    key = (case_name, base, wire, text_b)
    if key not in _REF:
        st = state(*key)
        _REF[key] = (oracle(*st, torch.float32), oracle(*st, BF))
    return _REF[key]


def wire_figures(case_name: str, wire: Wire, text_b: bool = False) -> Tuple[float, float]:
    """(size, err_eager) of a wire: how far it moves the fp32 oracle's output, and how well the bf16-eager oracle reproduces that change."""
    rb32, rbbf = reference(case_name, wire.base, None, text_b)
    rp32, rpbf = reference(case_name, wire.base, wire.name, text_b)
    return delta_err(rbbf, rpbf, rb32, rp32)
