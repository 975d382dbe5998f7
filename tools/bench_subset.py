#!/usr/bin/env python3
"""Search within a document subset, measured: sr_dense_search_subset / sr_sparse_search_subset on synthetic indexes in the shapes
bench.py uses for BASELINE.json configs[1] (dense: 8 841 823 x 2048 fp32 rows) and configs[2] (sparse: V = 128 256, Zipf(1.0), 128
postings per doc, 32 query terms), for m in {1 000, 100 000, 1 000 000} documents drawn uniformly, nq in {1, 64, 6 980}, k = 1 000.

Per (head, m, nq): milliseconds of the subset search (HIP events around the call, median of --reps runs after warm-up) next to two
baselines measured in the same run: the pair scorer over the same nq x m pairs (sr_*_score_pairs; scores only, no ranking - where the
nq x m scores fit --pairs-limit) and the unrestricted search with the same k (what "search with a larger k and filter on the host"
starts from; its time does not depend on m).  Per (head, nq) the smallest measured m at which the unrestricted search is the faster of
the two is reported as well.  Writes one JSON document (default profiles/subset_search.json) and prints it; a leg left out with --legs
keeps its record from the file being rewritten (marked as kept), or reads "unmeasured".

  python tools/bench_subset.py                                  # full size, one MI355X (dense leg: 72 GB of rows)
  python tools/bench_subset.py --scale 0.02 --nqs 1,64,300      # a small box
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from synth import build_index, build_queries, dense_queries, dense_rows  # noqa: E402


def timed(fn, reps, warmup=1):
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


def draw_subset(n_docs, m, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.sort(torch.randperm(n_docs, device=dev, generator=g)[:m]).values.to(torch.int64).contiguous()


def crossover(rows):
    """Per nq: the smallest measured m whose subset search took longer than the unrestricted search (None: none did)."""
    out = {}
    for r in rows:
        slower = r["subset"]["median_ms"] > r["unrestricted_search"]["median_ms"]
        cur = out.setdefault(str(r["nq"]), None)
        if slower and (cur is None or r["m"] < cur):
            out[str(r["nq"])] = r["m"]
    return out


def dense_leg(a, dev):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    N = max(2 * a.k, int(a.n_docs * a.scale))
    D = dense_rows("gauss", N, a.hidden, dev, 1)
    idx = DenseIndexHIP(a.hidden, device=dev)
    idx.add_device_rows(D)
    idx.set_precision("fp32_filtered")                   # what the retrieval drivers use for the unrestricted search
    rows, full = [], {}
    for nq in a.nqs:
        Q = dense_queries("gauss", nq, a.hidden, dev, 2)
        _, full[nq] = timed(lambda: idx.search(Q, a.k), a.reps)
        for m in a.ms:
            if m > N:
                continue
            sub = draw_subset(N, m, dev, m)
            (s, i), t = timed(lambda: idx.search(Q, a.k, subset=sub), a.reps)
            row = {"m": m, "nq": nq, "k": a.k, "subset": t, "unrestricted_search": full[nq],
                   "row_bytes_per_pass": m * a.hidden * 4, "passes_over_the_subset": -(-nq // 16)}
            if nq * m <= a.pairs_limit:
                indptr = torch.arange(nq + 1, dtype=torch.int64, device=dev) * m
                flat = sub.repeat(nq)
                got, tp = timed(lambda: idx.score_pairs(Q, indptr, flat), a.reps)
                row["score_pairs_same_pairs"] = tp
                # the returned scores are the pair scorer's bits
                pos = torch.searchsorted(sub, i.clamp(min=0))
                want = got.view(nq, m).gather(1, pos.clamp(max=m - 1))
                row["scores_equal_score_pairs"] = bool(torch.equal(torch.where(i >= 0, want, s).view(torch.int32), s.view(torch.int32)))
                del indptr, flat, got
            else:
                row["score_pairs_same_pairs"] = f"not measured: {nq * m} scores exceed --pairs-limit"
            rows.append(row)
            print("[dense]", json.dumps(row), file=sys.stderr, flush=True)
            del sub
        del Q
    out = {"n_docs": N, "hidden": a.hidden, "kernel": "dense_subset_kernel", "rows": rows,
           "smallest_measured_m_where_the_unrestricted_search_is_faster": crossover(rows)}
    idx.close()
    del D, idx
    torch.cuda.empty_cache()
    return out


def sparse_leg(a, dev):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    N = max(8 * (a.k + 1024), int(a.n_docs * a.scale))
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    idx = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    rows, full = [], {}
    for nq in a.nqs:
        q_indptr, q_cols, q_vals = build_queries(a.vocab, nq, a.l0_q, dev, 4)
        _, full[nq] = timed(lambda: idx.search(q_indptr, q_cols, q_vals, a.k), a.reps)
        for m in a.ms:
            if m > N:
                continue
            sub = draw_subset(N, m, dev, m + 1)
            _, t = timed(lambda: idx.search(q_indptr, q_cols, q_vals, a.k, subset=sub), a.reps)
            row = {"m": m, "nq": nq, "k": a.k, "route": "array" if m * 16 >= N else "pairs", "subset": t, "unrestricted_search": full[nq]}
            if nq * m <= a.pairs_limit:
                ci = torch.arange(nq + 1, dtype=torch.int64, device=dev) * m
                flat = sub.repeat(nq)
                _, row["score_pairs_same_pairs"] = timed(lambda: idx.score_pairs(q_indptr, q_cols, q_vals, ci, flat), a.reps)
                del ci, flat
            else:
                row["score_pairs_same_pairs"] = f"not measured: {nq * m} scores exceed --pairs-limit"
            rows.append(row)
            print("[sparse]", json.dumps(row), file=sys.stderr, flush=True)
            del sub
    out = {"n_docs": N, "vocab": a.vocab, "postings": int(doc_ids.numel()), "L0_d": a.l0_d, "L0_q": a.l0_q,
           "forward_index": idx.cert_stats()["present"] == 1, "rows": rows,
           "smallest_measured_m_where_the_unrestricted_search_is_faster": crossover(rows)}
    idx.close()
    del indptr, doc_ids, vals, idx
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (both indexes)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--nqs", type=str, default="1,64,6980")
    ap.add_argument("--ms", type=str, default="1000,100000,1000000")
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7, help="timed runs per figure after one warm-up run (median reported)")
    ap.add_argument("--pairs-limit", type=int, default=500_000_000, help="largest nq x m the pair-scorer baseline is run for (12 bytes each)")
    ap.add_argument("--legs", type=str, default="dense,sparse")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "subset_search.json"))
    a = ap.parse_args()
    a.nqs = [int(x) for x in a.nqs.split(",")]
    a.ms = [int(x) for x in a.ms.split(",")]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    res = {"what": "top-k within a subset of m documents shared by all queries (tools/bench_subset.py)",
           "device": torch.cuda.get_device_name(0), "n_gpus": 1, "scale": a.scale, "data": "synthetic, subsets drawn uniformly",
           "timing": f"HIP events around the call, median of {a.reps} runs after 1 warm-up run"}
    earlier = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            earlier = json.load(f)
    for leg, fn in (("dense", dense_leg), ("sparse", sparse_leg)):
        if leg in a.legs.split(","):
            res[leg] = fn(a, dev)
        elif isinstance(earlier.get(leg), dict) and earlier.get("scale") == a.scale:
            res[leg] = dict(earlier[leg], kept_from_an_earlier_run_of_this_tool=True)      # --legs: the other leg's record stays
        else:
            res[leg] = "unmeasured"
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
