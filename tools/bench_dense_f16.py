#!/usr/bin/env python3
"""fp16-stored rows against fp32-stored rows, both indexes in one process on one GPU (profiles/dense_f16.json).

The fp32 index holds the fp16 rows widened to fp32 ("the twin"), so every pair of measurements is also a check: ids and score
bits of the two indexes must be identical.  Synthetic rows ~ N(0, 0.5 / sqrt(H)) as the embeddings' scale, N = 8 841 823 x 2048
by default (72.4 + 36.2 GB of rows, 36.2 GB of filter plane each).

  streaming pass    nq in {1, 16, 64}, k = 100: per search the summed time of the score-kernel launches (the library's per-launch HIP
                    events, sr_dense_index_profile) and the whole search (HIP events around the call); GB/s = row bytes / kernel time
  tiled exact pass  nq = 6 980, k = 1000, SR_PRECISION_FP32
  filtered search   nq = 6 980, k = 1000, SR_PRECISION_FP32_FILTERED
  resident bytes    rows + sr_dense_index_owned_bytes in the four configurations

Every figure: one warm-up, then the median of --reps (7) repetitions; min and max are recorded next to it.  Prints one JSON line.
For the kernel's own row, run `rocprofv3 --kernel-trace --stats -- python tools/bench_dense_f16.py --only stream`.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _measure(idx, q, k, reps):
    """(median / min / max ms of the whole search, the same of the score kernels alone, (scores, ids) of the last run)"""
    lib, h = idx.lib, idx._h
    n, ms, fl, by = ctypes.c_int64(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    idx.search(q, k)                                   # warm-up: workspaces, code objects, the filter's query buffers
    lib.sr_dense_index_profile(h, 1)
    lib.sr_dense_index_profile_read(h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by))
    whole, kern = [], []
    out = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = idx.search(q, k)
        e1.record()
        e1.synchronize()
        whole.append(e0.elapsed_time(e1))
        lib.sr_dense_index_profile_read(h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by))
        kern.append(ms.value)
    lib.sr_dense_index_profile(h, 0)

    def stat(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return stat(whole), stat(kern), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8_841_823)
    ap.add_argument("--H", type=int, default=2048)
    ap.add_argument("--nq-large", type=int, default=6980)
    ap.add_argument("--k-large", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["all", "stream", "large"], default="all")
    a = ap.parse_args()
    from scaling_retriever_amd.scoring import DenseIndexHIP
    dev = torch.device("cuda", 0)
    N, H = a.N, a.H
    g = torch.Generator(device=dev).manual_seed(0)
    D16 = torch.empty((N, H), dtype=torch.float16, device=dev)
    D32 = torch.empty((N, H), dtype=torch.float32, device=dev)
    for r0 in range(0, N, 1 << 19):                    # piecewise: no third copy of the matrix
        piece = torch.randn((min(1 << 19, N - r0), H), dtype=torch.float32, device=dev, generator=g) * (0.5 / H ** 0.5)
        D16[r0:r0 + piece.shape[0]] = piece.half()
        D32[r0:r0 + piece.shape[0]] = D16[r0:r0 + piece.shape[0]].float()
    del piece
    Q = torch.randn((a.nq_large, H), dtype=torch.float32, device=dev, generator=g) / H ** 0.5
    f16, f32 = DenseIndexHIP(H), DenseIndexHIP(H)
    f16.add_device_rows(D16)
    f32.add_device_rows(D32)
    out = {"metric": "dense index, fp16-stored rows against fp32-stored rows (the twin)", "n_gpus": 1, "N": N, "H": H, "data": "synthetic",
           "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    rows = {"fp32": N * H * 4, "fp16": N * H * 2}
    resident = {"fp32": {"rows": rows["fp32"], "owned": f32.owned_bytes()}, "fp16": {"rows": rows["fp16"], "owned": f16.owned_bytes()}}

    def both(nq, k):
        q = Q[:nq].contiguous()
        w32, k32, o32 = _measure(f32, q, k, a.reps)
        w16, k16, o16 = _measure(f16, q, k, a.reps)
        same = bool(torch.equal(o16[1], o32[1]) and torch.equal(o16[0].view(torch.int32), o32[0].view(torch.int32)))
        r = {"nq": nq, "k": k, "identical_results": same,
             "fp32": {"search": w32, "score_kernels": k32, "row_GBps": round(rows["fp32"] / k32["median_ms"] / 1e6, 1)},
             "fp16": {"search": w16, "score_kernels": k16, "row_GBps": round(rows["fp16"] / k16["median_ms"] / 1e6, 1)},
             "ratio_score_kernels": round(k16["median_ms"] / k32["median_ms"], 4),
             "ratio_search": round(w16["median_ms"] / w32["median_ms"], 4),
             "fp32_spread_ms": round(w32["max_ms"] - w32["min_ms"], 4),
             "fp16_minus_fp32_ms": round(w16["median_ms"] - w32["median_ms"], 4)}
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r
    if a.only in ("all", "stream"):
        out["streaming_pass"] = [both(nq, 100) for nq in (1, 16, 64)]
    if a.only in ("all", "large"):
        out["tiled_exact_pass"] = both(a.nq_large, a.k_large)
        for idx in (f32, f16):
            idx.set_precision("fp32_filtered")
        out["filtered_search"] = both(a.nq_large, a.k_large)
        out["filtered_search"]["queries_certified"] = {"fp32": f32.filter_query_stats()[0], "fp16": f16.filter_query_stats()[0]}
        resident["fp32_filtered"] = {"rows": rows["fp32"], "owned": f32.owned_bytes()}
        resident["fp16_filtered"] = {"rows": rows["fp16"], "owned": f16.owned_bytes()}
    for v in resident.values():
        v["total_GB"] = round((v["rows"] + v["owned"]) / 1e9, 2)
    out["resident_bytes"] = resident
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
