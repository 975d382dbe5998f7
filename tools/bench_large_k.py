#!/usr/bin/env python3
"""Search time at large k (top-k beyond sr_max_topk() = 4096 runs the global-memory select and sort of csrc/topk_large.hip).

  dense:  H = 2048 (full MSMARCO width), N = 8 841 823 synthetic rows (72 GB in HBM), 6 980 queries, exact fp32 kernel
  sparse: the configuration of tools/bench_sparse.py (V = 128 256, Zipf(1.0) document frequencies, L0_d = 128, L0_q = 32)

Prints one JSON line: per k, search ms and queries/s of each (one timed search after a warm-up at the first k).  For the share
of the top-k kernels, run the dense leg alone under `rocprofv3 --kernel-trace --stats -- python tools/bench_large_k.py
--skip-sparse --ks 10000`.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _time(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8_841_823)
    ap.add_argument("--H", type=int, default=2048)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--ks", type=str, default="1000,4096,10000,100000")
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--skip-dense", action="store_true")
    ap.add_argument("--skip-sparse", action="store_true")
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",")]
    dev = torch.device("cuda", 0)
    out = {"metric": "search at large k", "unit": "ms / queries/s", "n_gpus": 1, "nq": a.nq, "data": "synthetic"}
    if not a.skip_dense:
        from scaling_retriever_amd.scoring import DenseIndexHIP
        g = torch.Generator(device=dev).manual_seed(0)
        D = torch.empty((a.N, a.H), dtype=torch.float32, device=dev)
        for r0 in range(0, a.N, 1 << 20):
            D[r0:r0 + (1 << 20)].normal_(generator=g)
        Q = torch.randn((a.nq, a.H), dtype=torch.float32, device=dev, generator=g)
        idx = DenseIndexHIP(a.H)
        idx.add_device_rows(D)
        idx.search(Q, ks[0])                            # warm-up
        res = {}
        for k in ks:
            dt = _time(lambda: idx.search(Q, k), a.steps)
            res[str(k)] = {"ms": round(dt * 1e3, 1), "qps": round(a.nq / dt, 1)}
            print("dense", k, res[str(k)], file=sys.stderr, flush=True)
        out["dense"] = {"H": a.H, "N": a.N, "precision": "fp32", "k": res}
        del idx, D, Q
        torch.cuda.empty_cache()
    if not a.skip_sparse:
        from synth import build_index, build_queries
        from scaling_retriever_amd.scoring import SparseIndexHIP
        V, L0_d, L0_q, N = 128256, 128, 32, 8_841_823
        indptr, doc_ids, vals, _ = build_index(V, N, L0_d, dev, 3)
        q_indptr, q_cols, q_vals = build_queries(V, a.nq, L0_q, dev, 4)
        idx = SparseIndexHIP(indptr, doc_ids, vals, N)
        idx.search(q_indptr, q_cols, q_vals, ks[0])     # warm-up
        res = {}
        for k in ks:
            dt = _time(lambda: idx.search(q_indptr, q_cols, q_vals, k), a.steps)
            res[str(k)] = {"ms": round(dt * 1e3, 1), "qps": round(a.nq / dt, 1)}
            print("sparse", k, res[str(k)], file=sys.stderr, flush=True)
        out["sparse"] = {"V": V, "N": N, "L0_d": L0_d, "L0_q": L0_q, "k": res}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
