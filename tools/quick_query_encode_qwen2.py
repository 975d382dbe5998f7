#!/usr/bin/env python3
"""Query-encode time at Qwen2.5-1.5B dims (28 layers, H 1536, 12 : 2 heads of 128, MLP 8960, q / k / v biases) for the 6 980
synthetic Dev queries of tools/quick_query_encode.py, one batch, both regimes.  FLOP per token = 2 x the layers' linear parameters
(the way DESIGN.md 4.4 counts Llama); the fraction is of the 16-bit MFMA peak, with the fp32 regime's plane products counted as
work.  There is no reference number for this workload.
python tools/quick_query_encode_qwen2.py"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from scaling_retriever_amd.modeling.llm_encoder import Qwen2BiDense  # noqa: E402

dev = torch.device("cuda", 0)
cfg = dict(vocab_size=151936, hidden_size=1536, intermediate_size=8960, num_hidden_layers=28, num_attention_heads=12,
           num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6, rope_theta=1000000.0, tie_word_embeddings=True,
           model_type="qwen2")
w = bench.random_weights(cfg, dev, 0)
g = torch.Generator(device=dev).manual_seed(1)
nq, nkv = cfg["num_attention_heads"] * cfg["head_dim"], cfg["num_key_value_heads"] * cfg["head_dim"]
for li in range(cfg["num_hidden_layers"]):
    for nm, n in (("q", nq), ("k", nkv), ("v", nkv)):
        w[f"model.layers.{li}.self_attn.{nm}_proj.bias"] = torch.randn((n,), device=dev, generator=g)
H, I = cfg["hidden_size"], cfg["intermediate_size"]
flop_per_token = 2.0 * cfg["num_hidden_layers"] * ((nq + 2 * nkv) * H + H * nq + 3 * I * H)
model = Qwen2BiDense.from_weights(cfg, w, max_batch_tokens=65536, max_batch_seqs=8192).to(dev).eval()
segs = model.base_model.weight_segments()
batches, lens = bench.synth_batches(6980, 6980, 2.1, 0.35, 4, 64, cfg["vocab_size"], 2, dev)
for prec in ("bf16", "fp32"):
    model.base_model.precision = prec
    for rep in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i, m in batches:
            model.query_encode(input_ids=i, attention_mask=m)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    nprod = 1.0 if prec == "bf16" else sum(segs) / len(segs)
    tf = float(lens.sum()) * flop_per_token * nprod / dt / 1e12
    print(f"qwen2.5-1.5b dims, 6980 queries, {prec}: {dt * 1e3:8.1f} ms  ({int(lens.sum())} tokens, {nprod:.2f} plane products, "
          f"{tf:7.1f} TFLOP/s of 16-bit MFMA work = {tf / bench.PEAK_BF16_MFMA_TF:.3f} of peak)", flush=True)
