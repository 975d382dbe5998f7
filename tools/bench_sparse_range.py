#!/usr/bin/env python3
"""Sparse range search against the top-k search of the same batch, one process, one GPU (profiles/sparse_range.json).

Synthetic index in the shape of config 3 (V = 128 256 terms, N = 8 841 823 docs, 128 postings per doc, Zipf(1.0) document
frequencies, tools/synth.py), queries of 32 distinct terms.  For nq in {1, 64, 6 980} the thresholds come from a top-k search of the
same queries: each query's 100th and 10 000th best score, so a query has 99 and 9 999 hits (fewer where that score is tied).  Timed
with HIP events: sr_sparse_range_count (kernel + scan + its 8-byte read-back) and sr_sparse_range_fill separately, and sr_sparse_search
with k = 1 000 for the same batch, once as routed by default (the certified two-stage scorer where the index has one) and once on the
exact kernels (dev switch SR_SPARSE_CERT_SEARCH=0 on the same handle: the per-call form of SR_SPARSE_CERT=0) - the reference point for
a pass that computes every score.  Per threshold also: hits, result bytes, and the share of (query, chunk) cells without a hit, which
the fill pass leaves before it touches a posting.  For one query also the route numba_score_float took before: a search with k = the
number of documents that can score at all.  One warm-up, then the median of --reps (7); a call that takes over a second is timed once.
Prints one JSON line.
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

from synth import build_index, build_queries  # noqa: E402

TILE_DOCS = 8192


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


_ENV_BEFORE = {}


def _exact_kernels(on):
    """Dev switch SR_SPARSE_CERT_SEARCH=0 around the exact-kernel timing; both variables get their earlier values back."""
    names = ("SR_DEV_SWITCHES", "SR_SPARSE_CERT_SEARCH")
    if on:
        _ENV_BEFORE.update({n: os.environ.get(n) for n in names})
        os.environ["SR_DEV_SWITCHES"], os.environ["SR_SPARSE_CERT_SEARCH"] = "1", "0"
    else:
        for n in names:
            if _ENV_BEFORE.get(n) is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = _ENV_BEFORE[n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=128256)
    ap.add_argument("--N", type=int, default=8_841_823)
    ap.add_argument("--L0-d", type=int, default=128)
    ap.add_argument("--L0-q", type=int, default=32)
    ap.add_argument("--nqs", type=int, nargs="+", default=[6980, 64, 1])
    ap.add_argument("--ranks", type=int, nargs="+", default=[100, 10000])
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import SparseIndexHIP, _ptr
    dev = torch.device("cuda", 0)
    indptr, doc_ids, vals, _ = build_index(a.V, a.N, a.L0_d, dev, 3)
    idx = SparseIndexHIP(indptr, doc_ids, vals, a.N)
    lib, h = idx.lib, idx._h
    n_tiles = (a.N + TILE_DOCS - 1) // TILE_DOCS
    lens = indptr[1:] - indptr[:-1]
    out = {"metric": "sparse range search (count pass, fill pass) against sr_sparse_search of the same batch",
           "n_gpus": 1, "V": a.V, "N": a.N, "L0_d": a.L0_d, "L0_q": a.L0_q, "postings": int(doc_ids.numel()), "data": "synthetic Zipf(1.0)",
           "reps": a.reps, "k_search": a.k, "doc_tiles": n_tiles, "device": torch.cuda.get_device_name(0), "batches": []}
    for nq in a.nqs:
        qp, qc, qv = build_queries(a.V, nq, a.L0_q, dev, 4)
        touched = float(lens[qc.long()].sum().item())
        top, _, top_n = idx.search(qp, qc, qv, max(a.ranks))         # thresholds: the rank-th best score of each query
        idx.search(qp, qc, qv, a.k)
        _, t_default = _timed(lambda: idx.search(qp, qc, qv, a.k), a.reps)
        _exact_kernels(True)
        idx.search(qp, qc, qv, a.k)
        _, t_exact = _timed(lambda: idx.search(qp, qc, qv, a.k), a.reps)
        _exact_kernels(False)
        row = {"nq": nq, "postings_of_the_query_terms": touched, "search_k_default_routing": t_default, "search_k_exact_kernels": t_exact,
               "thresholds": []}
        for rank in a.ranks:
            thr = top[:, rank - 1].contiguous()
            lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
            total = ctypes.c_int64(0)

            def count():
                _lib.check(lib.sr_sparse_range_count(h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(thr), _ptr(lims), ctypes.byref(total),
                                                     _lib.stream_ptr()))
                return total.value
            count()
            n, t_count = _timed(count, a.reps)
            scores = torch.empty(max(1, n), dtype=torch.float32, device=dev)
            ids = torch.empty(max(1, n), dtype=torch.int64, device=dev)

            def fill():
                _lib.check(lib.sr_sparse_range_fill(h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(thr), _ptr(lims), 0, 1, _ptr(scores), _ptr(ids),
                                                    n, _lib.stream_ptr()))
            fill()
            _, t_fill = _timed(fill, a.reps)
            # the lists are the search's: every hit scores above the threshold, and a query has as many as its top-k list holds above it
            counts = lims[1:] - lims[:-1]
            ok = bool(torch.equal(counts, (top > thr[:, None]).sum(1))) and bool((scores[:n] > torch.repeat_interleave(thr, counts)).all())
            query = torch.repeat_interleave(torch.arange(nq, device=dev), counts, output_size=n)
            cells = int(torch.unique(query * n_tiles + ids[:n] // TILE_DOCS).numel())          # one tile per chunk (the default)
            del query
            r = {"rank": rank, "total_hits": n, "result_GB": round(n * 12 / 1e9, 6), "hit_counts_equal_the_search": ok,
                 "count": t_count, "fill": t_fill, "cells": nq * n_tiles, "cells_skipped_by_fill": round(1.0 - cells / (nq * n_tiles), 6),
                 "count_over_exact_search": round(t_count["median_ms"] / t_exact["median_ms"], 4),
                 "fill_over_exact_search": round(t_fill["median_ms"] / t_exact["median_ms"], 4),
                 "count_posting_GBps": round(8.0 * touched / t_count["median_ms"] / 1e6, 1)}
            row["thresholds"].append(r)
            print(json.dumps({"nq": nq, **r}), file=sys.stderr, flush=True)
            del scores, ids
        if nq == 1:
            # what numba_score_float did before: a search with k = every document that can score, then an argsort by id on the host
            k_all = max(1, min(a.N, int(touched)))
            idx.search(qp, qc, qv, k_all)
            _, t_old = _timed(lambda: idx.search(qp, qc, qv, k_all), a.reps)
            row["search_k_collection"] = dict(t_old, k=k_all)
        out["batches"].append(row)
        del top
    idx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
