"""CPU: the Qwen2 family (Qwen2BiDense / Qwen2BiSparse, /root/reference/scaling_retriever/modeling/llm_encoder.py:204-209,528-533)
without a device - the oracle restatement the GPU tests lean on against the reference's goldens, and the host side of the loaders."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import llama_bi as LB
from qwen2_common import CASES, BiasHooks, load_case, rel


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", CASES)
def test_oracle_with_bias_hook_matches_reference_qwen2_heads(name, side):
    """oracle.llama_bi + a `lin` that adds the q / k / v bias = the reference's Qwen2 heads, to the bar the Llama oracle is held to
    in tests/test_oracle.py: 4e-6 absolute on both heads.

    Measured (max abs, dense / sparse): hd64 left 8.2e-8 / 3.4e-6, hd64 right 1.2e-7 / 2.6e-6, hd128 left 8.6e-8 / 4.6e-7, hd128
    right 1.0e-7 / 4.3e-7.  The largest is one near-zero maximum logit (rep 0.0403: a sum of 128 products of magnitude ~1 that
    cancels), i.e. the fp32 rounding of the reference's own run; the hook's linear layers accumulate in float64 so that the
    restatement adds none of its own there (with fp32 GEMMs in the hook that element was 4.005e-6)."""
    z, cfg, w = load_case(name)
    ids, mask = z[f"{side}:input_ids"], z[f"{side}:attention_mask"]
    hooks = BiasHooks(w)
    d = LB.dense_encode(w, cfg, ids, mask, hooks)
    s = LB.sparse_encode(w, cfg, ids, mask, hooks)
    print(name, side, "dense max abs", np.abs(d - z[f"{side}:dense"]).max(), "sparse max abs", np.abs(s - z[f"{side}:sparse"]).max())
    assert np.abs(d - z[f"{side}:dense"]).max() <= 4e-6
    assert np.abs(s - z[f"{side}:sparse"]).max() <= 4e-6
    # the fixture is about the bias: without it the oracle is far off
    assert rel(LB.dense_encode(w, cfg, ids, mask), z[f"{side}:dense"]) > 0.1


def test_bf16_bias_hook_tracks_reference_autocast():
    """Hooks(bf16=True) + bias (cast to bf16, added to the fp32 accumulator, one rounding) stays as close to the reference's
    autocast run as that run is to its fp32 run (r_autocast), up to the factor the GPU tests allow the product."""
    for name in CASES:
        z, cfg, w = load_case(name)
        r = float(z["r_autocast"])
        for side in ("left", "right"):
            ids, mask = z[f"{side}:input_ids"], z[f"{side}:attention_mask"]
            d = LB.dense_encode(w, cfg, ids, mask, BiasHooks(w, bf16=True))
            assert rel(d, z[f"{side}:dense_bf16autocast"]) < 2.5 * r, (name, side, rel(d, z[f"{side}:dense_bf16autocast"]), r)


def test_model_config_struct_ends_in_attention_bias():
    from scaling_retriever_amd import _lib
    assert _lib.SrModelConfig._fields_[-1] == ("attention_bias", ctypes.c_int32)
    assert _lib.SrModelConfig(vocab_size=16).attention_bias == 0
    assert "sr_gemm_qkv_rope_bias" in _lib.SIGNATURES


def _write_dir(tmp_path, cfg, w, name="qwen2_base"):
    from safetensors.numpy import save_file
    d = tmp_path / name
    os.makedirs(d)
    save_file({k: np.ascontiguousarray(v) for k, v in w.items()}, str(d / "model.safetensors"))
    json.dump(cfg, open(d / "config.json", "w"))
    return str(d)


def test_qwen2_classes_build_host_side_models(tmp_path):
    from scaling_retriever_amd.modeling import llm_encoder as LE
    z, cfg, w = load_case("enc_qwen2_hd64")
    assert LE.Qwen2BiDense.TRANSFORMER_CLS == "Qwen2BiModel" and LE.Qwen2BiSparse.TRANSFORMER_CLS == "Qwen2BiForMNTP"
    assert LE.Qwen2BiHybrid.TRANSFORMER_CLS == "Qwen2BiForMNTP"
    assert LE.Qwen2BiDenseForNCE is LE.Qwen2BiDense and LE.Qwen2BiSparseForNCE is LE.Qwen2BiSparse
    assert LE.Qwen2BiDense.TARGET_MODULES == LE.LlamaBiDense.TARGET_MODULES
    plain = {k: v for k, v in cfg.items() if k != "model_type"}
    m = LE.Qwen2BiDense.from_weights(plain, w)                      # Qwen2Config has no attention_bias field: the family implies it
    assert m.base_model.config.attention_bias is True and m.base_model._c_config().attention_bias == 1
    assert m.hidden_size == cfg["hidden_size"]
    assert LE.LlamaBiDense.from_weights(plain, {k: v for k, v in w.items() if not k.endswith(".bias")}) \
        .base_model._c_config().attention_bias == 0
    d = _write_dir(tmp_path, cfg, w)
    for cls in (LE.Qwen2BiDense, LE.Qwen2BiSparse, LE.Qwen2BiHybrid):
        m = cls.load(d)
        c = m.base_model._c_config()
        assert c.attention_bias == 1 and c.rope_theta == 1000000.0
        assert "model.layers.1.self_attn.k_proj.bias" in m.base_model._weights
    assert LE.retriever_class(d, "dense") is LE.Qwen2BiDense and LE.retriever_class(d, "sparse") is LE.Qwen2BiSparse


def test_a_class_refuses_the_other_family(tmp_path):
    from scaling_retriever_amd.modeling import llm_encoder as LE
    z, cfg, w = load_case("enc_qwen2_hd64")
    d = _write_dir(tmp_path, cfg, w)
    with pytest.raises(ValueError, match="qwen2"):
        LE.LlamaBiDense.load(d)
    with pytest.raises(ValueError, match="qwen2"):
        LE.LlamaBiSparse.load(d)
    llama = _write_dir(tmp_path, dict(cfg, model_type="llama"), {k: v for k, v in w.items() if not k.endswith(".bias")}, "llama_base")
    with pytest.raises(ValueError, match="llama"):
        LE.Qwen2BiDense.load(llama)
    assert LE.retriever_class(llama, "dense") is LE.LlamaBiDense
    LE.LlamaBiDense.load(llama)


def test_unsupported_config_flags_raise_instead_of_dropping_tensors():
    from scaling_retriever_amd.modeling.llm_encoder import LlamaConfigLite
    z, cfg, w = load_case("enc_qwen2_hd64")
    with pytest.raises(NotImplementedError, match="sliding"):
        LlamaConfigLite.from_dict(dict(cfg, use_sliding_window=True))
    assert LlamaConfigLite.from_dict(dict(cfg, use_sliding_window=False)).attention_bias is True
    with pytest.raises(NotImplementedError, match="mlp_bias"):
        LlamaConfigLite.from_dict(dict(cfg, mlp_bias=True))
    with pytest.raises(NotImplementedError, match="o_proj"):
        LlamaConfigLite.from_dict(dict(cfg, model_type="llama", attention_bias=True))
    assert LlamaConfigLite.from_dict(dict(cfg, model_type="llama")).attention_bias is False
