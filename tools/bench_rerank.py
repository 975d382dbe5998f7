#!/usr/bin/env python3
"""Pair scoring on the resident indexes, measured: rerank a Dev-sized run (6 980 queries x 1 000 candidates taken from an actual
search) with sr_dense_score_pairs / sr_sparse_score_pairs, on synthetic indexes in the shapes bench.py uses for BASELINE.json
configs[1] (dense: 8 841 823 x 2048 fp32 rows) and configs[2] (sparse: V = 128 256, Zipf(1.0), 128 postings per doc, 32 query terms).

Per head: milliseconds per rerank (HIP events around the call, median of --reps runs after warm-up), bytes gathered, their rate as
a fraction of the HBM peak bench.py uses (8 000 GB/s), and whether EVERY score equals the bits the search returned for that pair.
For scale the present route - rerank_forward, which encodes the query and the document of every pair again - is timed on a sample
of pairs with the 1B-shaped random-init encoder.  Writes one JSON document (default profiles/rerank_pairs.json) and prints it.

  python tools/bench_rerank.py                       # full size, one MI355X (dense leg: 72 GB of rows + the filter's 36 GB plane)
  python tools/bench_rerank.py --scale 0.01 --nq 300 --baseline-pairs 256 --layers 2     # a small box
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from synth import build_index, build_queries, dense_queries, dense_rows  # noqa: E402

PEAK_HBM_GBPS = 8000.0       # bench.py's figure for its streaming leg (HBM3E spec peak)
STREAM_KERNEL_GBPS = 5900.0  # what dense_stream.hip reaches on contiguous rows


def timed(fn, reps, warmup=2):
    """Median / min / max milliseconds of fn() between two events on the current stream."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": reps}


def rate(bytes_, ms):
    gbps = bytes_ / (ms * 1e-3) / 1e9
    return {"bytes_gathered": int(bytes_), "achieved_GBps": round(gbps, 1), "peak_GBps": PEAK_HBM_GBPS,
            "frac_of_hbm_peak": round(gbps / PEAK_HBM_GBPS, 4), "frac_of_streaming_kernel": round(gbps / STREAM_KERNEL_GBPS, 4)}


def dense_leg(a, dev):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    N = max(4 * a.k, int(a.n_docs * a.scale))
    D = dense_rows("gauss", N, a.hidden, dev, 1)
    idx = DenseIndexHIP(a.hidden, device=dev)
    idx.add_device_rows(D)
    idx.set_precision("fp32_filtered")                   # what the retrieval drivers use; the same bits as the exact kernel
    Q = dense_queries("gauss", a.nq, a.hidden, dev, 2)
    s, ids = idx.search(Q, a.k)
    indptr = torch.arange(a.nq + 1, dtype=torch.int64, device=dev) * a.k
    flat = ids.reshape(-1).contiguous()
    got, t = timed(lambda: idx.score_pairs(Q, indptr, flat), a.reps)
    pairs = int(flat.numel())
    out = {"n_docs": N, "hidden": a.hidden, "nq": a.nq, "k": a.k, "pairs": pairs, "kernel": "dense_pairs_kernel", **t,
           "pairs_per_s": round(pairs / (t["median_ms"] * 1e-3), 1),
           "all_scores_equal_the_searchs": bool(torch.equal(got.view(torch.int32), s.reshape(-1).view(torch.int32))),
           **rate(pairs * (a.hidden * 4 + 8 + 4) + a.nq * a.hidden * 4, t["median_ms"])}
    # the same pairs with each list's candidates in ascending row order: what the gather costs without the run's rank order
    srt = torch.sort(ids, dim=1).values.reshape(-1).contiguous()
    _, t2 = timed(lambda: idx.score_pairs(Q, indptr, srt), a.reps)
    out["candidates_sorted_by_row_median_ms"] = t2["median_ms"]
    idx.close()
    del D, idx, Q, s, ids, flat, srt
    torch.cuda.empty_cache()
    return out


def sparse_leg(a, dev):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    N = max(8 * (a.k + 1024), int(a.n_docs * a.scale))        # the certified scorer (and its forward index) needs 8 (k + 1024) docs
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    q_indptr, q_cols, q_vals = build_queries(a.vocab, a.nq, a.l0_q, dev, 4)
    idx = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    s, ids, cnt = idx.search(q_indptr, q_cols, q_vals, a.k)
    valid = torch.arange(a.k, device=dev)[None, :] < cnt[:, None]
    ci = torch.zeros(a.nq + 1, dtype=torch.int64, device=dev)
    ci[1:] = torch.cumsum(cnt.to(torch.int64), 0)
    flat, want = ids[valid].contiguous(), s[valid]
    pairs = int(flat.numel())
    row_len = torch.bincount(doc_ids.long(), minlength=N)
    fwd_bytes = int(row_len[flat].sum().item()) * 8 + pairs * (16 + 8 + 4)
    has_fwd = idx.cert_stats()["present"] == 1
    got, t = timed(lambda: idx.score_pairs(q_indptr, q_cols, q_vals, ci, flat), a.reps)
    out = {"n_docs": N, "vocab": a.vocab, "postings": int(doc_ids.numel()), "L0_d": a.l0_d, "L0_q": a.l0_q, "nq": a.nq, "k": a.k,
           "pairs": pairs, "kernel": "sparse_pairs_kernel", "route": "forward index" if has_fwd else "posting lists", **t,
           "pairs_per_s": round(pairs / (t["median_ms"] * 1e-3), 1),
           "all_scores_equal_the_searchs": bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))}
    if has_fwd:
        out.update(rate(fwd_bytes, t["median_ms"]))
        out["bytes_note"] = "forward rows of the candidates (8 B per posting) + row bounds, id and score per pair; the query's terms are cache-resident"
    # the other route (dev switch): lane = query term, binary search in its posting list
    os.environ["SR_DEV_SWITCHES"], os.environ["SR_PAIR_SPARSE_ROUTE"] = "1", "postings"
    got2, t2 = timed(lambda: idx.score_pairs(q_indptr, q_cols, q_vals, ci, flat), max(3, a.reps // 2), warmup=1)
    del os.environ["SR_PAIR_SPARSE_ROUTE"]
    out["posting_list_route"] = {**t2, "all_scores_equal_the_searchs": bool(torch.equal(got2.view(torch.int32), want.view(torch.int32)))}
    idx.close()
    del indptr, doc_ids, vals, idx
    torch.cuda.empty_cache()
    return out


def baseline_leg(a, dev):
    """rerank_forward as it stands (scaling_retriever_amd/modeling/llm_encoder.py: both sides of every pair encoded again), dense
    head, 1B-shaped random-init encoder, bf16 autocast, batches of 128 pairs with Dev-like query and passage lengths."""
    import bench
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    cfg = dict(bench.LION_1B)
    if a.layers:
        cfg["num_hidden_layers"] = a.layers
    model = LlamaBiDense.from_weights(cfg, bench.random_weights(cfg, dev, seed=0), max_batch_tokens=65536, max_batch_seqs=8192).to(dev).eval()
    n = a.baseline_pairs
    qb, _ = bench.synth_batches(n, 128, 2.1, 0.35, 4, 64, cfg["vocab_size"], 2, dev)
    db, dl = bench.synth_batches(n, 128, 4.25, 0.35, 8, 192, cfg["vocab_size"], 5, dev)

    def run():
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):
            return [model.rerank_forward(tokenized_queries={"input_ids": q[0], "attention_mask": q[1]},
                                         tokenized_docs={"input_ids": d[0], "attention_mask": d[1]}) for q, d in zip(qb, db)]
    _, t = timed(run, 3, warmup=1)
    return {"route": "rerank_forward: re-encode the query and the document of every pair", "pairs": n, "layers": cfg["num_hidden_layers"],
            "mean_passage_tokens": round(float(np.mean(dl)), 1), **t, "pairs_per_s": round(n / (t["median_ms"] * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (both indexes)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7, help="timed runs per leg after warm-up (median reported; at least 5)")
    ap.add_argument("--baseline-pairs", type=int, default=2048, help="0: skip the re-encoding baseline")
    ap.add_argument("--layers", type=int, default=0, help="encoder layers of the baseline (0: the 1B shape's 16)")
    ap.add_argument("--legs", type=str, default="dense,sparse,baseline")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "rerank_pairs.json"))
    a = ap.parse_args()
    a.reps = max(5, a.reps)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    res = {"what": "pair scoring on the resident indexes: one rerank of nq x k candidates taken from a search (tools/bench_rerank.py)",
           "device": torch.cuda.get_device_name(0), "n_gpus": 1, "scale": a.scale, "data": "synthetic",
           "timing": f"HIP events around the call, median of {a.reps} runs after 2 warm-up runs"}
    legs = a.legs.split(",")
    if "dense" in legs:
        res["dense"] = dense_leg(a, dev)
        print("[dense]", json.dumps(res["dense"]), file=sys.stderr, flush=True)
    if "sparse" in legs:
        res["sparse"] = sparse_leg(a, dev)
        print("[sparse]", json.dumps(res["sparse"]), file=sys.stderr, flush=True)
    if "baseline" in legs and a.baseline_pairs > 0:
        res["re_encoding_baseline"] = baseline_leg(a, dev)
        for head in ("dense", "sparse"):
            if head in res:
                res[head]["speedup_over_re_encoding"] = round(res[head]["pairs_per_s"] / res["re_encoding_baseline"]["pairs_per_s"], 1)
    res["all_scores_equal_the_searchs"] = all(res[h]["all_scores_equal_the_searchs"] for h in ("dense", "sparse") if h in res)
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
