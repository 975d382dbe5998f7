#!/usr/bin/env python3
"""The exact hybrid search, measured (scaling_retriever_amd/hybrid.py over csrc/hybrid_fuse.hip), on synthetic indexes in the shapes
bench.py uses for BASELINE.json configs[1] (dense: 8 841 823 x 2048 fp32 rows) and configs[2] (sparse: V = 128 256, Zipf(1.0), 128
postings per doc, 32 query terms); the two indexes number the same documents in independent random orders.

  (a) union + ranking of one round: sr_hybrid_union + sr_hybrid_rank against the torch route of HybridRetriever.retrieve_fused
      (torch.unique over nq x 2k keys, then rerank.drop_repeats and rank_candidates: a scatter_reduce and three stable sorts), on the
      SAME two top-k lists and the same pair scores.  The pair scorers are common to both routes and not in either figure.
  (b) a whole hybrid.search_fused call at --nq (6 980) and at 64 queries, k = 1 000, default depths, with the queries per route.
  (c) the range route: --range-nq (8) queries with depths = (k,), which this data leaves uncertified.

HIP events around each call, the routes alternated in one process, median of --reps runs after warm-up.  Independent Gaussian / Zipf
scores are the hard case for the certificate (the two heads agree on nothing); how often real embeddings certify at the first depth is
not measured here.  Writes one JSON document (default profiles/hybrid_search.json) and prints it.

  python tools/bench_hybrid.py                    # full size, one MI355X
  python tools/bench_hybrid.py --scale 0.02 --nq 300
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


def alternated(fns, reps, warmup=2):
    """{name: stats} of the given callables, run in turn (a, b, a, b, ...) between two events each."""
    ms = {n: [] for n in fns}
    for r in range(warmup + reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ms[n].append(a.elapsed_time(b))
    return {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs": reps}
            for n, v in ms.items()}


def torch_union(sp, sc, dp, s2d, d2s, n_dense):
    """The union of HybridRetriever.retrieve_fused, as it stands there."""
    dev, nq = sp.device, sp.shape[0]
    sp_valid = (sp >= 0) & (torch.arange(sp.shape[1], device=dev)[None, :] < sc[:, None])
    rows_s = torch.arange(nq, device=dev)[:, None].expand_as(sp)[sp_valid]
    sp_as_dense = s2d[sp[sp_valid]]
    if bool((sp_as_dense < 0).any()):
        raise KeyError("the inverted index holds a document the dense index does not")
    rows_d = torch.arange(nq, device=dev)[:, None].expand_as(dp)[dp >= 0]
    keys = torch.unique(torch.cat([rows_s * n_dense + sp_as_dense, rows_d * n_dense + dp[dp >= 0]]))
    row, dpos = keys // max(1, n_dense), keys % max(1, n_dense)
    indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(row, minlength=nq), 0)
    spos = d2s[dpos]
    tie = torch.where(spos >= 0, spos, int(s2d.numel()) + dpos)
    return indptr, dpos, spos, tie


def torch_rank(dense_s, sparse_s, dpos, spos, tie, indptr, w, k):
    from scaling_retriever_amd.rerank import drop_repeats, fused_scores, rank_candidates
    sparse_s = torch.where(spos >= 0, sparse_s, torch.zeros_like(sparse_s))
    scores, positions, ties, ip = drop_repeats(fused_scores(dense_s, sparse_s, w), dpos, tie, indptr)
    order, counts = rank_candidates(scores, ties, ip, k)
    return scores[order], positions[order], counts


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--range-nq", type=int, default=8, help="queries of the range-route leg (0: skip it)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "hybrid_search.json"))
    a = ap.parse_args()
    from scaling_retriever_amd import hybrid
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP, hybrid_rank, hybrid_union
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    N = max(8 * (a.k + 1024), int(a.n_docs * a.scale))
    dense = DenseIndexHIP(a.hidden, device=dev)
    dense.add_device_rows(dense_rows("gauss", N, a.hidden, dev, 1))
    dense.set_precision("fp32_filtered")
    Q = dense_queries("gauss", a.nq, a.hidden, dev, 2)
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    q_indptr, q_cols, q_vals = build_queries(a.vocab, a.nq, a.l0_q, dev, 4)
    sparse = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    s2d = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    d2s = torch.empty_like(s2d)
    d2s[s2d] = torch.arange(N, device=dev)
    w, k = (1.0, 1.0), a.k
    res = {"what": "exact hybrid search: union + ranking kernels against retrieve_fused's torch route, and whole search_fused calls "
                   "(tools/bench_hybrid.py)", "device": torch.cuda.get_device_name(0), "n_gpus": 1, "scale": a.scale, "data": "synthetic",
           "n_docs": N, "hidden": a.hidden, "vocab": a.vocab, "L0_d": a.l0_d, "L0_q": a.l0_q, "k": k, "weights": list(w),
           "timing": f"HIP events around each call, routes alternated in one process, median of {a.reps} runs after 2 warm-up runs"}

    # (a) one round at depth k on the same lists
    ds, dp = dense.search(Q, k)
    ss, sp, sc = sparse.search(q_indptr, q_cols, q_vals, k, threshold=0.0)
    n_dense = int(d2s.numel())
    u_hip = hybrid_union(dp, sp, sc, s2d, d2s)
    u_torch = torch_union(sp, sc, dp, s2d, d2s, n_dense)
    same_union = all(torch.equal(x, y) for x, y in zip(u_hip, u_torch))
    ip, dpos, spos, tie = u_hip
    dense_s = dense.score_pairs(Q, ip, dpos)
    sparse_s = sparse.score_pairs(q_indptr, q_cols, q_vals, ip, torch.clamp(spos, min=0))
    D, S = ds[:, k - 1].contiguous(), torch.where(sc == k, ss[:, k - 1], torch.zeros_like(ss[:, 0]))
    complete = torch.zeros(a.nq, dtype=torch.bool, device=dev)
    r_hip = hybrid_rank(ip, dpos, spos, tie, dense_s, sparse_s, w, k, D, S, complete, int(s2d.numel()), dense.id_end)
    r_torch = torch_rank(dense_s, sparse_s, dpos, spos, tie, ip, w, k)
    valid = torch.arange(k, device=dev)[None, :] < r_hip[2][:, None]
    same_rank = bool(torch.equal(r_hip[1][valid], r_torch[1]) and torch.equal(r_hip[0][valid].view(torch.int32), r_torch[0].view(torch.int32))
                     and torch.equal(r_hip[2].to(torch.int64), r_torch[2]))
    t = alternated({"union_hip": lambda: hybrid_union(dp, sp, sc, s2d, d2s), "union_torch": lambda: torch_union(sp, sc, dp, s2d, d2s, n_dense),
                    "rank_hip": lambda: hybrid_rank(ip, dpos, spos, tie, dense_s, sparse_s, w, k, D, S, complete, int(s2d.numel()), dense.id_end),
                    "rank_torch": lambda: torch_rank(dense_s, sparse_s, dpos, spos, tie, ip, w, k)}, a.reps)
    hip_ms = t["union_hip"]["median_ms"] + t["rank_hip"]["median_ms"]
    torch_ms = t["union_torch"]["median_ms"] + t["rank_torch"]["median_ms"]
    res["union_and_rank"] = {"nq": a.nq, "list_entries": int(a.nq * 2 * k), "union_entries": int(dpos.numel()), **t,
                             "hip_union_plus_rank_ms": round(hip_ms, 3), "torch_union_plus_rank_ms": round(torch_ms, 3),
                             "torch_over_hip": round(torch_ms / hip_ms, 2), "same_union": same_union, "same_ranking": same_rank,
                             "certified_at_depth_k": int(r_hip[3].sum().item())}
    print("[union_and_rank]", json.dumps(res["union_and_rank"]), file=sys.stderr, flush=True)
    del u_hip, u_torch, r_hip, r_torch, dense_s, sparse_s
    torch.cuda.empty_cache()

    # (b) whole calls
    res["search_fused"] = {}
    for nq in sorted({min(64, a.nq), a.nq}, reverse=True):
        qp = q_indptr[:nq + 1].contiguous()
        args = (dense, sparse, d2s, s2d, Q[:nq], qp, q_cols[:int(qp[-1])], q_vals[:int(qp[-1])], k)
        out = {}

        def call():
            out["r"] = hybrid.search_fused(*args, weights=w)
        tt = alternated({"search_fused": call}, max(3, a.reps if nq <= 64 else 3), warmup=1)
        stats = out["r"][3]
        routes = {("range" if d < 0 else f"depth_{stats['depths'][d]}"): int((stats["depth"] == d).sum()) for d in np.unique(stats["depth"])}
        res["search_fused"][f"nq_{nq}"] = {"nq": nq, "depths": list(stats["depths"]), **tt["search_fused"], "queries_per_route": routes,
                                           "mean_candidates_ranked": round(float(stats["union"].mean()), 1),
                                           "mean_range_hits_on_the_range_route": round(float(stats["range_hits"][stats["depth"] < 0].mean()), 1)
                                           if (stats["depth"] < 0).any() else 0.0}
        print(f"[search_fused nq={nq}]", json.dumps(res["search_fused"][f"nq_{nq}"]), file=sys.stderr, flush=True)
    # (c) the range route at this size: depths = (k,) leaves (nearly) every query of this data uncertified, a few queries only - a
    # query's candidates are then a sizeable part of the collection, ranked by one workgroup
    nq = min(a.range_nq, a.nq)
    if nq > 0:
        qp = q_indptr[:nq + 1].contiguous()
        args = (dense, sparse, d2s, s2d, Q[:nq], qp, q_cols[:int(qp[-1])], q_vals[:int(qp[-1])], k)
        out = {}

        def call_range():
            out["r"] = hybrid.search_fused(*args, weights=w, depths=(k,))
        tt = alternated({"search_fused": call_range}, 3, warmup=1)
        stats = out["r"][3]
        on_range = stats["depth"] < 0
        res["range_route"] = {"nq": nq, "depths": [k], **tt["search_fused"], "queries_on_the_range_route": int(on_range.sum()),
                              "mean_range_hits": round(float(stats["range_hits"][on_range].mean()), 1) if on_range.any() else 0.0,
                              "max_range_hits": int(stats["range_hits"].max()), "fallback_bytes": 1 << 30}
        print("[range_route]", json.dumps(res["range_route"]), file=sys.stderr, flush=True)
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
