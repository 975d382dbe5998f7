#!/usr/bin/env python3
"""Collapsed search (top-k distinct groups, csrc/topk_collapse.hip + scaling_retriever_amd/collapse.py), measured
(profiles/collapse_search.json) on the synthetic indexes of tools/bench_hybrid.py: dense 8 841 823 x 2 048 fp32 rows (config 2,
fp32_filtered), sparse V = 128 256, Zipf(1.0), 128 postings per document (config 3), 6 980 queries, k = 1 000.

(a) the kernel: sr_topk_collapse on [6 980, 4 000] and [6 980, 16 000] rows (ids: runs of 4 consecutive documents sampled over the
    collection, shuffled; scores descending), k = 1 000, keys = id // 8 and random groups of mean size 8, against the same computation written in torch on the device
    (gather the keys, stable sort by key, first-occurrence flags, ordered compaction).  The outputs are asserted identical before timing.
(b) whole search_collapsed calls on both heads for 6 980 and 64 queries, next to the plain search at k = 1 000 and at the first depth,
    with the route statistics; once with the default schedule and once with --alt-depths, whose first depth stays inside the limit of the
    dense certified filter.

HIP events around each call, variants alternated in one process, median of --reps (7) runs after a warm-up.  No target: the file records
what the hardware says.  Reads nothing outside the repository.

  python tools/bench_collapse.py                   # full size, one MI355X
  python tools/bench_collapse.py --scale 0.02 --nq 300
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

FLT_MAX = float(np.finfo(np.float32).max)


def alternated(fns, reps, warmup=1):
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
    return {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs": len(v)}
            for n, v in ms.items()}


def torch_collapse(scores, ids, keys, k):
    """sr_topk_collapse of full rows (no padding) in torch ops on the device."""
    nq, L = ids.shape
    g = keys[ids].to(torch.int64)
    gs, at = torch.sort(g, dim=1, stable=True)                  # equal keys keep their rank order: the first of a run is the best passage
    first = torch.ones_like(gs, dtype=torch.bool)
    first[:, 1:] = gs[:, 1:] != gs[:, :-1]
    flag = torch.zeros_like(first)
    flag.scatter_(1, at, first)                                 # back in rank order
    pos = torch.cumsum(flag, 1) - 1
    keep = flag & (pos < k)
    rows = torch.arange(nq, device=ids.device)[:, None].expand_as(ids)[keep]
    out_s = torch.full((nq, k), -FLT_MAX, dtype=torch.float32, device=ids.device)
    out_i = torch.full((nq, k), -1, dtype=torch.int64, device=ids.device)
    out_k = torch.full((nq, k), -1, dtype=torch.int32, device=ids.device)
    out_s[rows, pos[keep]], out_i[rows, pos[keep]], out_k[rows, pos[keep]] = scores[keep], ids[keep], g[keep].to(torch.int32)
    n = flag.sum(1)
    counts = torch.clamp(n, max=k).to(torch.int32)
    return out_s, out_i, out_k, counts, (n >= k).to(torch.int32)


def routes(stats):
    return {("full_ranking" if d < 0 else f"depth_{stats['depths'][d]}"): int((stats["depth"] == d).sum()) for d in np.unique(stats["depth"])}


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
    ap.add_argument("--row-lens", type=int, nargs="+", default=[4000, 16000])
    ap.add_argument("--alt-depths", type=int, nargs="+", default=[1365, 4000],
                    help="a second schedule for leg (b): its first depth inside the dense certified filter's limit (k <= 1 365)")
    ap.add_argument("--skip-searches", action="store_true", help="the kernel leg (a) alone")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "collapse_search.json"))
    a = ap.parse_args()
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP, topk_collapse
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    N = max(8 * (a.k + 1024), int(a.n_docs * a.scale), 16 * max(a.row_lens))
    k, nq = a.k, a.nq
    gen = torch.Generator(device=dev).manual_seed(9)
    key_tables = {"id_div_8": (torch.arange(N, device=dev) // 8).to(torch.int32),
                  "random_mean_8": torch.randint(0, max(1, N // 8), (N,), device=dev, generator=gen).to(torch.int32)}
    res = {"what": "collapsed search: sr_topk_collapse against the same computation in torch, and whole search_collapsed calls on both heads "
                   "(tools/bench_collapse.py)", "device": torch.cuda.get_device_name(0), "n_gpus": 1, "scale": a.scale, "data": "synthetic",
           "n_docs": N, "hidden": a.hidden, "vocab": a.vocab, "L0_d": a.l0_d, "L0_q": a.l0_q, "k": k,
           "timing": f"HIP events around each call, variants alternated in one process, median of {a.reps} runs after a warm-up run",
           "not_measured": ["real group-size distributions (a chunked corpus)", "the full-ranking route at this size",
                            "search_collapsed under filters at this size"]}

    # (a) the kernel on rows of its own: ids distinct inside a row, scores descending with ties
    res["kernel"] = {}
    for L in a.row_lens:
        # L / 4 runs of 4 consecutive ids, one run per stratum of the collection, the columns shuffled: neighbours share a group
        n_runs, width = L // 4, (N // 4) // (L // 4)
        runs = torch.randint(0, width, (nq, n_runs), device=dev, generator=gen) + torch.arange(n_runs, device=dev)[None, :] * width
        ids = (runs[:, :, None] * 4 + torch.arange(4, device=dev)[None, None, :]).reshape(nq, 4 * n_runs)
        ids = ids[:, torch.randperm(4 * n_runs, device=dev, generator=gen)].contiguous()
        L = ids.shape[1]
        scores = (-(torch.arange(L, device=dev) // 3).to(torch.float32))[None, :].expand(nq, L).contiguous()
        for name, keys in key_tables.items():
            hip = topk_collapse(scores, ids, keys, k)
            ref = torch_collapse(scores, ids, keys, k)
            same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                       for x, y in zip(hip, ref))
            assert same, ("sr_topk_collapse and the torch route differ", L, name)
            t = alternated({"hip": lambda: topk_collapse(scores, ids, keys, k), "torch": lambda: torch_collapse(scores, ids, keys, k)}, a.reps)
            cell = {"nq": nq, "row_len": L, "keys": name, **t, "torch_over_hip": round(t["torch"]["median_ms"] / t["hip"]["median_ms"], 2),
                    "same_outputs": same, "rows_complete": int(hip[4].sum()), "mean_groups": round(float(hip[3].float().mean()), 1),
                    # what the kernel must move: ids, the gathered keys, and the k kept entries in and out
                    "min_bytes": int(nq * (L * 12 + k * 20))}
            res["kernel"][f"L{L}_{name}"] = cell
            print(f"[kernel L={L} {name}]", json.dumps(cell), file=sys.stderr, flush=True)
        del ids, scores
    torch.cuda.empty_cache()

    if not a.skip_searches:
        dense = DenseIndexHIP(a.hidden, device=dev)
        dense.add_device_rows(dense_rows("gauss", N, a.hidden, dev, 1))
        dense.set_precision("fp32_filtered")
        Q = dense_queries("gauss", nq, a.hidden, dev, 2)
        indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
        qi, qc, qv = build_queries(a.vocab, nq, a.l0_q, dev, 4)
        sparse = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
        keys = key_tables["id_div_8"]
        res["search_collapsed"] = {"keys": "id // 8"}
        for n in sorted({min(64, nq), nq}, reverse=True):
            qp = qi[:n + 1].contiguous()
            sq = (qp, qc[:int(qp[-1])], qv[:int(qp[-1])])
            dq = Q[:n].contiguous()
            out = {}

            def dense_collapsed():
                out["d"] = dense.search_collapsed(dq, k, keys)

            def sparse_collapsed():
                out["s"] = sparse.search_collapsed(*sq, k, keys)
            alt = tuple(d for d in a.alt_depths if d >= k)

            def dense_collapsed_alt():
                out["da"] = dense.search_collapsed(dq, k, keys, depths=alt)

            def sparse_collapsed_alt():
                out["sa"] = sparse.search_collapsed(*sq, k, keys, depths=alt)
            dense_collapsed()
            d0 = out["d"][4]["depths"][0]
            reps = a.reps if n <= 64 else 3
            t = alternated({"dense_collapsed": dense_collapsed, "dense_search_k": lambda: dense.search(dq, k),
                            "dense_search_first_depth": lambda: dense.search(dq, min(d0, N)),
                            "sparse_collapsed": sparse_collapsed, "sparse_search_k": lambda: sparse.search(*sq, k),
                            "sparse_search_first_depth": lambda: sparse.search(*sq, min(d0, N)),
                            **({"dense_collapsed_alt_depths": dense_collapsed_alt, "sparse_collapsed_alt_depths": sparse_collapsed_alt} if alt else {})},
                           reps)
            cell = {"nq": n, "depths": list(out["d"][4]["depths"]), **t, "dense_routes": routes(out["d"][4]), "sparse_routes": routes(out["s"][4]),
                    "dense_mean_groups": round(float(out["d"][4]["groups_seen"].mean()), 1),
                    "sparse_mean_groups": round(float(out["s"][4]["groups_seen"].mean()), 1)}
            if alt:
                cell.update(alt_depths=list(alt), dense_routes_alt_depths=routes(out["da"][4]), sparse_routes_alt_depths=routes(out["sa"][4]))
            res["search_collapsed"][f"nq_{n}"] = cell
            print(f"[search_collapsed nq={n}]", json.dumps(cell), file=sys.stderr, flush=True)
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
