"""Switchable LoRA adapters, host side (no GPU): the state machine of set_adapters / disable_lora / enable_lora / delete_adapters on a
model whose tensors are all on the CPU (a switch on such a model is recorded and merged once the model is on the device, so nothing
here reaches a kernel), the effective-scale rule, and the registration of the merge kernel's entry point."""
import pytest
import torch

from chronoedit_amd import hiplib, weights
from chronoedit_amd.transformer import ChronoEditTransformer3DModel

TINY = dict(num_attention_heads=2, attention_head_dim=128, in_channels=36, out_channels=16, text_dim=64, freq_dim=32, ffn_dim=512,
            num_layers=2, image_dim=48, added_kv_proj_dim=256)


def tiny(seed=0):
    torch.manual_seed(seed)
    m = ChronoEditTransformer3DModel(**TINY)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape).to(p.dtype) * 0.05)
    return m


def _lora(m, targets, r=4, alpha=None, seed=1):
    g = torch.Generator().manual_seed(seed)
    mods = dict(m.named_modules())
    sd = {}
    for t in targets:
        sd[f"transformer.{t}.lora_A.weight"] = torch.randn(r, mods[t].in_features, generator=g) * 0.1
        sd[f"transformer.{t}.lora_B.weight"] = torch.randn(mods[t].out_features, r, generator=g) * 0.1
        if alpha is not None:
            sd[f"transformer.{t}.alpha"] = torch.tensor(float(alpha))
    return sd


def _loaded():
    m = tiny()
    m.load_lora_weights(_lora(m, ["blocks.0.attn1.to_q"], seed=1), adapter_name="a")
    m.load_lora_weights(_lora(m, ["blocks.0.attn1.to_q", "blocks.1.ffn.net.2"], seed=2, alpha=2.0), adapter_name="b")
    m.load_lora_weights(_lora(m, ["blocks.1.attn2.to_k"], seed=3), adapter_name="c")
    return m


def test_unknown_adapter_raises_key_error():
    m = _loaded()
    with pytest.raises(KeyError, match="no adapter"):
        m.set_adapters(["a", "zzz"])
    with pytest.raises(KeyError, match="no adapter"):
        m.set_adapters("zzz")
    with pytest.raises(KeyError, match="no adapter"):
        m.delete_adapters(["zzz"])
    assert m.get_active_adapters() == []


def test_activating_a_fused_adapter_raises_value_error():
    m = _loaded()
    m.fuse_lora(adapter_names=["a"], lora_scale=1.0)
    with pytest.raises(ValueError, match="fused"):
        m.set_adapters(["a"])
    with pytest.raises(ValueError, match="fused"):
        m.set_adapters(["b", "a"], [1.0, 0.5])
    assert m.get_active_adapters() == []
    m.set_adapters(["b"])  # the others still switch
    assert m.get_active_adapters() == ["b"]


def test_adapter_weights_of_the_wrong_length_raise_value_error():
    m = _loaded()
    with pytest.raises(ValueError, match="adapter weights"):
        m.set_adapters(["a", "b"], [1.0])
    with pytest.raises(ValueError, match="adapter weights"):
        m.set_adapters("a", [1.0, 2.0])
    with pytest.raises(ValueError, match="twice"):
        m.set_adapters(["a", "a"])
    assert m.get_active_adapters() == []


def test_bookkeeping_across_set_disable_enable_delete():
    m = _loaded()
    w0 = {k: p.detach().clone() for k, p in m.named_parameters()}
    assert m.get_list_adapters() == ["a", "b", "c"] and m.get_active_adapters() == []
    m.set_adapters(["b", "a"], [0.5, 2.0])
    assert m.get_active_adapters() == ["b", "a"]
    assert m._lora_rt.weights == {"b": 0.5, "a": 2.0}
    m.set_adapters("c")                      # a single name, weight 1.0; replaces the set
    assert m.get_active_adapters() == ["c"] and m._lora_rt.weights == {"c": 1.0}
    m.set_adapters(["a", "c"], 0.25)         # one number for all
    assert m._lora_rt.weights == {"a": 0.25, "c": 0.25}
    m.disable_lora()
    assert m.get_active_adapters() == [] and m.get_list_adapters() == ["a", "b", "c"]
    m.enable_lora()
    assert m.get_active_adapters() == ["a", "c"]
    m.delete_adapters("a")
    assert m.get_active_adapters() == ["c"] and m.get_list_adapters() == ["b", "c"]
    m.delete_adapters(["b"])                 # an inactive one
    assert m.get_active_adapters() == ["c"] and m.get_list_adapters() == ["c"]
    m.unfuse_lora()
    assert m.get_active_adapters() == []
    m.enable_lora()
    assert m.get_active_adapters() == ["c"]
    m.delete_adapters(["c"])
    assert m.get_active_adapters() == [] and m.get_list_adapters() == []
    # all of it on the host: no weight was touched (the merge runs on the device only), nothing is pending for an empty set
    assert all(torch.equal(p, w0[k]) for k, p in m.named_parameters())
    assert not m._lora_rt.dirty


def test_switch_on_a_host_model_is_pending_and_blocks_fuse():
    m = _loaded()
    m.set_adapters(["a"])
    assert m._lora_rt.dirty and m._lora_rt.merged == ()
    with pytest.raises(RuntimeError, match="unfuse_lora"):
        m.fuse_lora(adapter_names=["b"])
    m.unfuse_lora()
    assert not m._lora_rt.dirty
    m.fuse_lora(adapter_names=["b"])


def test_a_refused_set_is_not_reported_active():
    """A target the merge kernel does not take (an fp32 island) is refused before the record changes."""
    m = _loaded()
    m.load_lora_weights(_lora(m, ["condition_embedder.time_embedder.linear_1"], seed=4), adapter_name="t")
    m.set_adapters(["a"], [0.5])
    with pytest.raises(NotImplementedError, match="bf16 weight"):
        m.set_adapters(["b", "t"])
    assert m.get_active_adapters() == ["a"] and m._lora_rt.weights == {"a": 0.5}


def test_scale_scope_restores_the_record_when_the_block_raises_under_capture(monkeypatch):
    """The way out of lora_scale() must not raise over the block's own exception: under capture it only puts the weights' record back
    and leaves the merge to the next engine() call."""
    m = _loaded()
    m.set_adapters(["a", "b"], [1.0, 0.5])
    with pytest.raises(ValueError, match="from the block"):
        with m.lora_scale(0.5):
            assert m._lora_rt.weights == {"a": 0.5, "b": 0.25}
            monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
            monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            raise ValueError("from the block")
    monkeypatch.undo()
    assert m._lora_rt.weights == {"a": 1.0, "b": 0.5} and m._lora_rt.dirty
    with m.lora_scale(1.0), m.lora_scale(None):  # no-ops
        assert m._lora_rt.weights == {"a": 1.0, "b": 0.5}


def test_pipeline_forwards_the_adapter_surface():
    from chronoedit_amd.pipeline import ChronoEditPipeline
    m = _loaded()
    pipe = ChronoEditPipeline(transformer=m)
    pipe.set_adapters(["a", "b"], [1.0, 0.5])
    assert pipe.get_active_adapters() == ["a", "b"] and pipe.get_list_adapters() == {"transformer": ["a", "b", "c"]}
    pipe.disable_lora()
    assert pipe.get_active_adapters() == []
    pipe.enable_lora()
    pipe.delete_adapters(["a"])
    assert pipe.get_active_adapters() == ["b"]
    pipe.unfuse_lora()
    assert pipe.get_active_adapters() == []


@pytest.mark.parametrize("weight,alpha,rank,want", [(1.0, None, 4, 1.0), (0.5, None, 128, 0.5), (1.0, 8.0, 4, 2.0), (0.7, 2.0, 16, 0.7 * 0.125),
                                                    (2.0, 64.0, 32, 4.0)])
def test_effective_scale_rule(weight, alpha, rank, want):
    """adapter_weight * alpha / r, or adapter_weight alone without alpha: the rule of fuse_lora (lora_scale in the weight's place)."""
    assert weights.LoraMixin.lora_effective_scale(weight, alpha, rank) == pytest.approx(want, rel=1e-12)


def test_merge_entry_point_is_registered_everywhere():
    assert "ce_lora_merge_bf16" in hiplib.header_symbols()
    assert "ce_lora_merge_bf16" in hiplib.SIGNATURES and len(hiplib.SIGNATURES["ce_lora_merge_bf16"]) == 12
    assert "ce_lora.hip" in hiplib.SOURCES
    path = hiplib.build()
    assert "ce_lora_merge_bf16" in hiplib.exported_symbols(path)
    assert "ce_lora_merge_bf16" in hiplib.exported_symbols(hiplib.DIAG_LIB_PATH)
