#!/usr/bin/env python3
"""Query-encode time at Lion-DS-1B dims for the 6 980 synthetic Dev queries: bf16 regime vs the fp32 regime, per query-batch
size.  planes: 16 (default) = two fp16 planes of power-of-two scaled rows, 2 / 3 = bf16 planes.  The plane products per GEMM
come from the model (sr_model_weight_segments): with fp16 planes, 2 for a matrix whose low plane is all zero (the bench's
bf16-valued weights), else 3.
python tools/quick_query_encode.py [planes ...]
python tools/quick_query_encode.py --ab N     fp16 planes, batch 6 980, fp32 regime: N alternating rounds of a model forced to
                                              3 segments (SR_F16_WEIGHT_SEGS=3) and the default model, same weights
python tools/quick_query_encode.py --ab-lib N OTHER.so [OUT.json]
                                              fp16 planes, batch 6 980, fp32 regime: N alternating rounds of a model on another build
                                              of the library (tools/build_variant.sh) and a model on the product build, same process,
                                              same weights; the rounds are written to OUT.json"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense  # noqa: E402

dev = torch.device("cuda", 0)
cfg = dict(bench.LION_1B)
w = bench.random_weights(cfg, dev, 0)


def products(model, prec):
    """Plane products per GEMM, averaged over the layers' matrices weighted by their MACs (1 in the bf16 regime)."""
    if prec != "fp32":
        return 1.0
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    hd = cfg["head_dim"]
    nq, nkv = cfg["num_attention_heads"] * hd, cfg["num_key_value_heads"] * hd
    macs = [(nq + 2 * nkv) * H, H * nq, 2 * I * H, H * I]
    segs = model.base_model.weight_segments()      # = plane products of each matrix's GEMM
    tot = 0.0
    for li in range(cfg["num_hidden_layers"]):
        for j, mac in enumerate(macs):
            tot += mac * segs[4 * li + j]
    return tot / (sum(macs) * cfg["num_hidden_layers"])


def make(planes, force3=False):
    keep = {k: os.environ.get(k) for k in ("SR_DEV_SWITCHES", "SR_F16_WEIGHT_SEGS")}
    if force3:      # read by sr_model_finalize, i.e. while .to(dev) builds the engine
        os.environ["SR_DEV_SWITCHES"], os.environ["SR_F16_WEIGHT_SEGS"] = "1", "3"
    try:
        return LlamaBiDense.from_weights(cfg, dict(w), max_batch_tokens=65536, max_batch_seqs=8192, fp32_planes=planes).to(dev).eval()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def timed(model, batches, prec):
    model.base_model.precision = prec
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i, m in batches:
        model.query_encode(input_ids=i, attention_mask=m)
    torch.cuda.synchronize()
    return time.perf_counter() - t


if len(sys.argv) > 2 and sys.argv[1] == "--ab":
    rounds = int(sys.argv[2])
    models = {"forced-3": make(16, force3=True), "default": make(16)}
    batches, lens = bench.synth_batches(6980, 6980, 2.1, 0.35, 4, 64, cfg["vocab_size"], 2, dev)
    for name, model in models.items():
        print(f"{name}: segments per matrix {sorted(set(model.base_model.weight_segments()))}", flush=True)
        timed(model, batches, "fp32")       # warm-up (workspace allocation)
    times = {k: [] for k in models}
    for r in range(rounds):
        for name, model in models.items():
            dt = timed(model, batches, "fp32")
            times[name].append(dt * 1e3)
            print(f"round {r} {name:8s}: {dt * 1e3:8.1f} ms", flush=True)
    for name, ts in times.items():
        ts = sorted(ts)
        print(f"{name:8s}: median {ts[len(ts) // 2]:8.1f} ms  min {ts[0]:8.1f}  max {ts[-1]:8.1f}  ({int(lens.sum())} tokens)", flush=True)
    sys.exit(0)

if len(sys.argv) > 3 and sys.argv[1] == "--ab-lib":
    import json

    from scaling_retriever_amd import _lib
    rounds, other = int(sys.argv[2]), os.path.abspath(sys.argv[3])
    with _lib.library(other):               # a model keeps the library it was built on
        models = {"other": make(16)}
    models["product"] = make(16)
    batches, lens = bench.synth_batches(6980, 6980, 2.1, 0.35, 4, 64, cfg["vocab_size"], 2, dev)
    outs = {}
    for name, model in models.items():
        timed(model, batches, "fp32")       # warm-up (workspace allocation)
        i, m = batches[0]
        outs[name] = model.query_encode(input_ids=i, attention_mask=m)
    same = bool(torch.equal(outs["other"], outs["product"]))
    print(f"query rows of the two builds bit-identical: {same}", flush=True)
    times = {k: [] for k in models}
    for r in range(rounds):
        for name, model in models.items():
            dt = timed(model, batches, "fp32")
            times[name].append(round(dt * 1e3, 3))
            print(f"round {r} {name:8s}: {dt * 1e3:8.2f} ms", flush=True)
    spread = max(max(ts) - min(ts) for ts in times.values())
    gain = min(times["other"]) - max(times["product"])
    res = {"tool": "quick_query_encode.py --ab-lib", "other_lib": os.path.basename(other), "queries": 6980, "tokens": int(lens.sum()),
           "rounds_ms": times, "bit_identical_query_rows": same, "larger_spread_ms": round(spread, 3),
           "other_fastest_minus_product_slowest_ms": round(gain, 3), "counts_as_faster": bool(gain > 5 * spread)}
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(0)

for planes in [int(a) for a in sys.argv[1:]] or [16]:
    model = make(planes)
    for qb in (512, 2048, 6980):
        batches, lens = bench.synth_batches(6980, qb, 2.1, 0.35, 4, 64, cfg["vocab_size"], 2, dev)
        for prec in ("bf16", "fp32"):
            for rep in range(3):
                dt = timed(model, batches, prec)
            nprod = products(model, prec)
            tf = lens.sum() * bench.FLOP_PER_TOKEN_1B * nprod / dt / 1e12
            print(f"planes {planes} batch {qb:5d} {prec}: {dt * 1e3:8.1f} ms  ({int(lens.sum())} tokens, {nprod:.2f} plane products, "
                  f"{tf:7.1f} TFLOP/s of bf16 MFMA work)", flush=True)
    del model
    torch.cuda.empty_cache()
