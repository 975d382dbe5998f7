"""GPU: eval_dense.py / eval_sparse.py on a `model_type: qwen2` checkpoint - the flow of tests/test_eval_drivers.py.  The drivers
read model_type from config.json and pick Qwen2BiDense / Qwen2BiSparse (the reference's own drivers name the Llama classes only,
eval_dense.py:180,201, eval_sparse.py:87-92,128-132: this is an extension); adapters name Qwen2BiModel / Qwen2BiForMNTP."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import llama_bi as LB
from qwen2_common import BiasHooks, load_case
from test_eval_drivers import ROOT, _encode_oracle, _make_tokenizer, _texts


def _write_qwen2(tmp, cfg, w, rng):
    from safetensors.numpy import save_file
    out = {}
    for kind, bare, prefix, base_cls in [("dense", True, "base_model.model.", "Qwen2BiModel"),
                                         ("sparse", False, "base_model.model.model.", "Qwen2BiForMNTP")]:
        base, lora = os.path.join(tmp, f"base_{kind}"), os.path.join(tmp, f"lora_{kind}")
        os.makedirs(base), os.makedirs(lora)
        sd = {(k[len("model."):] if bare else k): np.ascontiguousarray(v) for k, v in w.items() if not (bare and k.startswith("lm_head"))}
        save_file(sd, os.path.join(base, "model.safetensors"))
        for d in (base, lora):
            json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
        ad, merged = {}, dict(w)
        for i in range(cfg["num_hidden_layers"]):
            for mod in ("self_attn.q_proj", "self_attn.v_proj", "mlp.down_proj"):
                name = f"model.layers.{i}.{mod}.weight"
                o, inn = w[name].shape
                A = (rng.standard_normal((4, inn)) / inn ** 0.5).astype(np.float32)
                B = (rng.standard_normal((o, 4)) * 0.2).astype(np.float32)
                ad[f"{prefix}layers.{i}.{mod}.lora_A.weight"], ad[f"{prefix}layers.{i}.{mod}.lora_B.weight"] = A, B
                merged[name] = LB.lora_merge(w[name], A, B, lora_alpha=8, r=4)
        save_file(ad, os.path.join(lora, "adapter_model.safetensors"))
        json.dump({"base_model_name_or_path": base, "r": 4, "lora_alpha": 8, "peft_type": "LORA",
                   "auto_mapping": {"base_model_class": base_cls}}, open(os.path.join(lora, "adapter_config.json"), "w"))
        _make_tokenizer(lora)
        out[kind] = (lora, merged)
    return out


@pytest.mark.gpu
def test_eval_drivers_on_a_qwen2_checkpoint(tmp_path):
    sys.path.insert(0, ROOT)
    import eval_dense
    import eval_sparse
    from scaling_retriever_amd.modeling import llm_encoder as LE
    from scaling_retriever_amd.utils.utils import obtain_doc_vec_dir_files
    z, cfg, w = load_case("enc_qwen2_hd64")
    assert cfg["model_type"] == "qwen2"
    rng = np.random.default_rng(3)
    models = _write_qwen2(str(tmp_path), cfg, w, rng)
    docs, queries = _texts(rng, 60, 3, 20), _texts(rng, 6, 2, 6)
    with open(tmp_path / "corpus.tsv", "w") as f:
        for i, t in enumerate(docs):
            f.write(f"d{i}\t{t}\n")
    with open(tmp_path / "queries.tsv", "w") as f:
        for i, t in enumerate(queries):
            f.write(f"q{i}\t{t}\n")
    from transformers import AutoTokenizer

    lora, merged = models["dense"]
    assert LE.retriever_class(lora, "dense") is LE.Qwen2BiDense
    with pytest.raises(ValueError, match="qwen2"):
        LE.LlamaBiDense.load(os.path.join(str(tmp_path), "base_dense"))
    emb_dir, out_dir = str(tmp_path / "embs"), str(tmp_path / "out_dense")
    eval_dense.main(["--task_name", "write_doc_embeds", "--model_name_or_path", lora, "--corpus_path", str(tmp_path / "corpus.tsv"),
                     "--doc_embed_dir", emb_dir, "--eval_batch_size", "16", "--doc_max_length", "16", "--chunk_size", "32",
                     "--token_budget", "0"])
    vf, idf = obtain_doc_vec_dir_files(emb_dir)
    got = {str(p): v for f_, g_ in zip(vf, idf) for p, v in zip(np.load(g_), np.load(f_))}
    assert set(got) == {f"d{i}" for i in range(60)}
    tok = AutoTokenizer.from_pretrained(lora)
    hooks = BiasHooks(merged)

    def dense_fn(w_, cfg_, ids, mask):
        return LB.dense_encode(w_, cfg_, ids, mask, hooks)
    d_ref = _encode_oracle(dense_fn, merged, cfg, tok, docs, 16)
    for i in range(len(docs)):
        err = np.linalg.norm(got[f"d{i}"] - d_ref[i]) / np.linalg.norm(d_ref[i])
        assert err < 1.5e-2, (i, err)                                      # the bf16-regime tolerance of tests/test_eval_drivers.py
    eval_dense.main(["--task_name", "retrieval", "--model_name_or_path", lora, "--query_path", str(tmp_path / "queries.tsv"),
                     "--doc_embed_dir", emb_dir, "--out_dir", out_dir, "--top_k", "10", "--query_max_length", "8"])
    run = json.load(open(os.path.join(out_dir, "run.json")))
    q_ref = _encode_oracle(dense_fn, merged, cfg, tok, queries, 8)
    ref_scores = q_ref @ d_ref.T
    for qi in range(len(queries)):
        hit = run[f"q{qi}"]
        assert len(hit) == 10
        assert len(set(np.argsort(-ref_scores[qi])[:10]) & {int(k[1:]) for k in hit}) >= 8
        for k, v in hit.items():
            assert abs(v - ref_scores[qi, int(k[1:])]) < 2e-2

    lora_s, merged_s = models["sparse"]
    assert LE.retriever_class(lora_s, "sparse") is LE.Qwen2BiSparse
    index_dir, out_s = str(tmp_path / "sp_index"), str(tmp_path / "out_sparse")
    eval_sparse.main(["--task_name", "indexing", "--model_name_or_path", lora_s, "--corpus_path", str(tmp_path / "corpus.tsv"),
                      "--index_dir", index_dir, "--eval_batch_size", "8", "--doc_max_length", "16", "--token_budget", "0"])
    assert os.path.exists(os.path.join(index_dir, "doc_ids.pkl")) and os.path.exists(os.path.join(index_dir, "index_stats.json"))
    eval_sparse.main(["--task_name", "retrieval", "--model_name_or_path", lora_s, "--query_path", str(tmp_path / "queries.tsv"),
                      "--index_dir", index_dir, "--out_dir", out_s, "--top_k", "10", "--query_max_length", "8"])
    run_s = json.load(open(os.path.join(out_s, "run.json")))
    hooks_s = BiasHooks(merged_s)

    def sparse_fn(w_, cfg_, ids, mask):
        return LB.sparse_encode(w_, cfg_, ids, mask, hooks_s)
    tok_s = AutoTokenizer.from_pretrained(lora_s)
    ds, qs = _encode_oracle(sparse_fn, merged_s, cfg, tok_s, docs, 16), _encode_oracle(sparse_fn, merged_s, cfg, tok_s, queries, 8)
    ref_s = qs @ ds.T
    for qi in range(len(queries)):
        hit = run_s[f"q{qi}"]
        assert len(hit) == 10
        assert len(set(np.argsort(-ref_s[qi])[:10]) & {int(k[1:]) for k in hit}) >= 8
