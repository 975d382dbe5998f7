#!/usr/bin/env python3
"""Dense range search against the exact top-k search of the same batch, one process, one GPU (profiles/range_search.json).

Synthetic index in the shape of config 2 (8 841 823 x 2 048, fp32 rows, tools/synth.py "gauss").  For nq in {1, 64, 6 980} the
thresholds come from a top-k search of the same queries: each query's 100th and 10 000th best score, so a query has 99 and 9 999
hits (fewer where that score is tied).  Timed with HIP events: sr_dense_range_count (kernel + scan + its 8-byte read-back) and sr_dense_range_fill separately, and
sr_dense_search in SR_PRECISION_FP32 with k = 1 000 for the same batch - each pass of the range search runs the exact kernel's
product once, so that search is the yardstick (ratio = pass / search).  One warm-up, then the median of --reps (7); a call that
takes over a second is timed once, after a warm-up of the same kernels on its first 130 queries.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from synth import dense_queries, dense_rows  # noqa: E402


def _timed(fn, reps, once_over_ms=1000.0):
    """(result of the last call, {median / min / max ms, runs}) of fn() between two events; the first timed call decides: over
    once_over_ms it is the only one."""
    ms, out = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        if ms[0] > once_over_ms:
            break
    return out, {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--nqs", type=int, nargs="+", default=[1, 64, 6980])
    ap.add_argument("--ranks", type=int, nargs="+", default=[100, 10000])
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import DenseIndexHIP, _ptr
    dev = torch.device("cuda", 0)
    N, H = a.n_docs, a.hidden
    D = dense_rows("gauss", N, H, dev, 1)
    idx = DenseIndexHIP(H, device=dev)
    idx.add_device_rows(D)
    lib, h = idx.lib, idx._h
    out = {"metric": "dense range search (count pass, fill pass) against sr_dense_search SR_PRECISION_FP32 of the same batch",
           "n_gpus": 1, "N": N, "H": H, "rows": "fp32", "data": "synthetic gauss", "reps": a.reps, "k_search": a.k,
           "device": torch.cuda.get_device_name(0), "row_bytes_per_pass": N * H * 4, "batches": []}
    for nq in a.nqs:
        Q = dense_queries("gauss", nq, H, dev, 2).contiguous()
        warm = Q[:min(nq, 130)].contiguous() if nq > 130 else None      # the same kernels (query tile of 256) on a short batch
        # thresholds: the rank-th best score of each query (tiled k order: what the range search computes)
        idx.set_batch_invariant(True)
        top, _ = idx.search(Q, max(a.ranks))
        idx.set_batch_invariant(False)
        if warm is not None:
            idx.search(warm, a.k)
        else:
            idx.search(Q, a.k)
        _, t_search = _timed(lambda: idx.search(Q, a.k), a.reps)
        row = {"nq": nq, "search_fp32_k": t_search, "thresholds": []}
        for rank in a.ranks:
            thr = top[:, rank - 1].contiguous()
            lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
            total = ctypes.c_int64(0)

            def count(q=Q, t=thr, lm=lims):
                _lib.check(lib.sr_dense_range_count(h, _ptr(q), q.shape[0], _ptr(t), _ptr(lm), ctypes.byref(total), _lib.stream_ptr()))
                return total.value
            if warm is not None:
                wl = torch.empty(warm.shape[0] + 1, dtype=torch.int64, device=dev)
                n = count(warm, thr[:warm.shape[0]].contiguous(), wl)
                ws, wi = torch.empty(max(1, n), dtype=torch.float32, device=dev), torch.empty(max(1, n), dtype=torch.int64, device=dev)
                _lib.check(lib.sr_dense_range_fill(h, _ptr(warm), warm.shape[0], _ptr(thr[:warm.shape[0]].contiguous()), _ptr(wl), _ptr(ws),
                                                   _ptr(wi), n, _lib.stream_ptr()))
            else:
                count()
            n, t_count = _timed(count, a.reps)
            scores = torch.empty(max(1, n), dtype=torch.float32, device=dev)
            ids = torch.empty(max(1, n), dtype=torch.int64, device=dev)

            def fill():
                _lib.check(lib.sr_dense_range_fill(h, _ptr(Q), nq, _ptr(thr), _ptr(lims), _ptr(scores), _ptr(ids), n, _lib.stream_ptr()))
            if warm is None:
                fill()
            _, t_fill = _timed(fill, a.reps)
            # the lists are the search's: every hit scores above the threshold, and a query has as many as its top-k list holds above it
            # (rank - 1 unless the rank-th score is tied)
            counts = lims[1:] - lims[:-1]
            ok = bool(torch.equal(counts, (top > thr[:, None]).sum(1))) and bool((scores[:n] > torch.repeat_interleave(thr, counts)).all())
            r = {"rank": rank, "total_hits": n, "result_GB": round(n * 12 / 1e9, 6), "hit_counts_equal_the_search": ok,
                 "count": t_count, "fill": t_fill,
                 "count_over_search": round(t_count["median_ms"] / t_search["median_ms"], 4),
                 "fill_over_search": round(t_fill["median_ms"] / t_search["median_ms"], 4),
                 "count_row_GBps": round(N * H * 4 / t_count["median_ms"] / 1e6, 1),
                 "fill_row_GBps": round(N * H * 4 / t_fill["median_ms"] / 1e6, 1),
                 "count_TFLOPs": round(2.0 * nq * N * H / t_count["median_ms"] / 1e9, 2)}
            row["thresholds"].append(r)
            print(json.dumps({"nq": nq, **r}), file=sys.stderr, flush=True)
            del scores, ids
        out["batches"].append(row)
        del Q, top
    idx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
