#!/usr/bin/env python3
"""Generate the Qwen2 golden vectors (tests/golden/enc_qwen2_*.npz) from the REFERENCE code.

The recipe of make_golden.py for the second backbone family: runs ONLY where the reference tree is present (read-only),
copies nothing from it - it imports the reference's own Qwen2BiDense / Qwen2BiSparse head classes
(scaling_retriever/modeling/llm_encoder.py:204-209,528-533), wraps them around a stock HF Qwen2Model / Qwen2ForCausalLM
driven with the reference's bidirectional key-padding mask (BiWrap, make_golden.py), eager attention, fp32 on the CPU, and
stores inputs + outputs as .npz data, plus the `*_bf16autocast` outputs the Llama fixtures carry.

Weights: the matrices come from golden_weights.make_weights(config, weight_seed) like every other encoder fixture (stored
whole, the two cases would take 1.4 and 4.6 MB; a committed file may hold 1 MiB), the q / k / v BIASES - what these fixtures
are about - are drawn N(0, 1) here and stored in the .npz (`bias:<tensor name>`).  At that size a dropped or misplaced bias
moves the output far beyond any tolerance: the generator asserts that the reference's own output with the biases zeroed
differs from the real one by a relative L2 > 0.1 on every case, head and padding side.

Also stored: `r_autocast` = the largest relative L2 between the reference's bf16-autocast and fp32 outputs over a case's
heads and sides (the GPU test's bf16 bar is max(1.5e-2, 2.5 r) with r the largest over the cases).

Usage:  python tests/golden/make_golden_qwen2.py
"""
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402
from golden_weights import make_weights  # noqa: E402

CASES = {
    # head_dim 64 (Qwen2.5-0.5B geometry), GQA 2:1, tied head; left / right padding, lengths include 1 and the full width
    "enc_qwen2_hd64": (dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                            num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=256,
                            rope_theta=1000000.0, rms_norm_eps=1e-6, tie_word_embeddings=True),
                       24, [24, 9, 1, 17, 24]),
    # head_dim 128 (1.5B / 7B geometry), GQA 2:1, untied head, L = 70: the fp32 attention's > 64-token path
    "enc_qwen2_hd128": (dict(vocab_size=320, hidden_size=256, intermediate_size=384, num_hidden_layers=2,
                             num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=512,
                             rope_theta=1000000.0, rms_norm_eps=1e-6, tie_word_embeddings=False),
                        70, [70, 3, 64, 65, 31]),
}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _biases(ckw, seed):
    rng = np.random.default_rng(seed)
    nh, nkv = ckw["num_attention_heads"], ckw["num_key_value_heads"]
    hd = ckw["hidden_size"] // nh
    out = {}
    for i in range(ckw["num_hidden_layers"]):
        for nm, n in (("q", nh * hd), ("k", nkv * hd), ("v", nkv * hd)):
            out[f"model.layers.{i}.self_attn.{nm}_proj.bias"] = rng.standard_normal(n, dtype=np.float32)
    return out


def _load(lm, ckw, w, b):
    sd = {k: torch.from_numpy(v) for k, v in {**w, **b}.items()}
    if ckw.get("tie_word_embeddings", False):
        sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    missing, unexpected = lm.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("rotary" in m or "inv_freq" in m for m in missing), missing
    if ckw.get("tie_word_embeddings", False):
        lm.tie_weights()


def main():
    from transformers import Qwen2Config, Qwen2ForCausalLM
    from scaling_retriever.modeling import llm_encoder as le
    for ci, (name, (ckw, L, lengths)) in enumerate(CASES.items()):
        cfg = Qwen2Config(**ckw)
        cfg._attn_implementation = "eager"
        assert not getattr(cfg, "use_sliding_window", False)
        assert all(t == "full_attention" for t in getattr(cfg, "layer_types", ["full_attention"]))
        lm = Qwen2ForCausalLM(cfg).eval()
        names = [n for n, _ in lm.named_parameters() if n.endswith(".bias")]
        assert names and all(".self_attn." in n and n.split(".")[-2] in ("q_proj", "k_proj", "v_proj") for n in names), names
        seed = 300 + ci
        w, b = make_weights(ckw, seed), _biases(ckw, 1000 + seed)
        zero_b = {k: np.zeros_like(v) for k, v in b.items()}
        V = cfg.vocab_size
        rng = np.random.default_rng(70 + ci)
        out = {"config_json": np.array(json.dumps(dict(ckw, model_type="qwen2"))), "weight_seed": seed}
        for k, v in b.items():
            out["bias:" + k] = v
        dense, sparse = le.Qwen2BiDense(MG.BiWrap(lm.model)), le.Qwen2BiSparse(MG.BiWrap(lm))
        r = 0.0
        for side in ["left", "right"]:
            ids, mask = MG._make_batch(rng, V, L, lengths, side, pad_id=V - 1)
            t = dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask))
            with torch.no_grad():
                _load(lm, ckw, w, b)
                d, s = dense.doc_encode(**t), sparse.doc_encode(**t)
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    d16, s16 = dense.doc_encode(**t), sparse.doc_encode(**t)
                _load(lm, ckw, w, zero_b)
                d0, s0 = dense.doc_encode(**t), sparse.doc_encode(**t)
            assert d.dtype == torch.float32 and s.dtype == torch.float32
            d, s, d16, s16 = d.numpy(), s.numpy(), d16.float().numpy(), s16.float().numpy()
            drop_d, drop_s = _rel(d0.numpy(), d), _rel(s0.numpy(), s)
            assert drop_d > 0.1 and drop_s > 0.1, (name, side, drop_d, drop_s)      # the biases matter
            r = max(r, _rel(d16, d), _rel(s16, s))
            out[f"{side}:input_ids"], out[f"{side}:attention_mask"] = ids, mask
            out[f"{side}:dense"], out[f"{side}:sparse"] = d, s
            out[f"{side}:dense_bf16autocast"], out[f"{side}:sparse_bf16autocast"] = d16, s16
            print(name, side, "zeroed-bias rel L2 dense %.3f sparse %.3f" % (drop_d, drop_s),
                  "autocast vs fp32 dense %.2e sparse %.2e" % (_rel(d16, d), _rel(s16, s)))
        out["r_autocast"] = np.float64(r)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
        print(name, "r_autocast %.3e" % r, "bytes", os.path.getsize(os.path.join(OUT, name + ".npz")))


if __name__ == "__main__":
    MG._install_stubs()
    torch.manual_seed(0)
    main()
