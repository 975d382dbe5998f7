#!/usr/bin/env python3
"""The sparse head's per-row term budget, measured: sr_sparse_compact_topm on one query group's representations - synthetic
reps [2048, 128 256] fp32 with exactly nnz non-zeros per row, nnz in {64, 1 000, 20 000}, budgets m in {32, 128}.

Three routes over the same input, each timed with HIP events around the whole route (1 warm-up, median of --reps runs; every route
ends in a stream synchronise of its own, so the window holds the device work and the call's host side):
  a  sr_sparse_compact                  every non-zero (two passes over a row: count, fill) - the yardstick, unchanged code
  b  sr_sparse_compact_topm             the budget inside the compaction (csrc/sparse_prune.hip)
  c  torch.topk + sort by column + gather + sr_sparse_compact over the [B, m] values: what a caller had to write without it
Per route: milliseconds and B * V * 4 / time in GB/s (the bytes of ONE pass over the input, whatever the route reads).  Per cell
also the passes route b makes over a row, and whether b and c kept the same entries (torch.topk does not promise the lower column
among equal values; the synthetic values are continuous, so they agree unless two values collide).
Writes one JSON document (default profiles/sparse_prune.json) and prints it.

  python tools/bench_sparse_prune.py
  python tools/bench_sparse_prune.py --rows 64 --reps 3          # a quick look
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scaling_retriever_amd import _lib  # noqa: E402

STAGE_KEYS = 7168        # csrc/sparse_prune.hip TOPM_STAGE: a row with more non-zeros is read again by the two later radix steps


def timed(fn, reps, warmup=1):
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
    return out, {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def synth_reps(B, V, nnz, dev, seed):
    """Exactly nnz non-zeros per row at random columns, values uniform in (0.001, 3.001)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    reps = torch.zeros((B, V), dtype=torch.float32, device=dev)
    for r0 in range(0, B, 256):
        r1 = min(B, r0 + 256)
        cols = torch.rand((r1 - r0, V), device=dev, generator=g).argsort(dim=1)[:, :nnz]
        vals = torch.rand((r1 - r0, nnz), device=dev, generator=g) * 3.0 + 1e-3
        reps[r0:r1].scatter_(1, cols, vals)
    return reps


class Buffers:
    def __init__(self, B, cap, dev):
        self.row_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        self.cols = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
        self.vals = torch.empty(max(1, cap), dtype=torch.float32, device=dev)
        self.cap = cap
        self.n = ctypes.c_int64(0)

    def result(self):
        n = self.n.value
        return self.row_ptr.clone(), self.cols[:n].clone(), self.vals[:n].clone()


def route_all(lib, x, buf):
    B, V = x.shape
    _lib.check(lib.sr_sparse_compact(x.data_ptr(), B, V, buf.row_ptr.data_ptr(), buf.cols.data_ptr(), buf.vals.data_ptr(), buf.cap,
                                     ctypes.byref(buf.n), _lib.stream_ptr()), "sr_sparse_compact")
    torch.cuda.current_stream().synchronize()


def route_topm(lib, x, m, buf):
    B, V = x.shape
    _lib.check(lib.sr_sparse_compact_topm(x.data_ptr(), B, V, m, buf.row_ptr.data_ptr(), buf.cols.data_ptr(), buf.vals.data_ptr(),
                                          buf.cap, ctypes.byref(buf.n), _lib.stream_ptr()), "sr_sparse_compact_topm")


def route_torch(lib, x, m, buf):
    """topk, order the kept entries by column, compact the [B, m] values (rows under budget carry zeros), map positions to columns."""
    B, V = x.shape
    k = min(m, V)
    vals, idx = torch.topk(x, k, dim=1)
    idx, perm = idx.sort(dim=1)
    vals = vals.gather(1, perm).contiguous()
    route_all(lib, vals, buf)
    n = buf.n.value
    rows = torch.repeat_interleave(torch.arange(B, device=x.device), buf.row_ptr[1:] - buf.row_ptr[:-1])
    cols = idx.reshape(-1)[rows * k + buf.cols[:n]].to(torch.int32)
    torch.cuda.current_stream().synchronize()
    return buf.row_ptr, cols, buf.vals[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--nnz", type=str, default="64,1000,20000")
    ap.add_argument("--budgets", type=str, default="32,128")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "sparse_prune.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    lib = _lib.load()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, V = a.rows, a.vocab
    one_pass = B * V * 4
    t0 = time.time()

    def with_rate(t):
        return {**t, "GBps_of_one_input_pass": round(one_pass / (t["median_ms"] * 1e-3) / 1e9, 1)}
    res = {"what": "per-row term budget inside the sparse compaction: sr_sparse_compact_topm against sr_sparse_compact and the torch route "
                   "(tools/bench_sparse_prune.py)",
           "device": torch.cuda.get_device_name(0), "n_gpus": 1, "data": "synthetic", "rows": B, "vocab": V, "input_bytes": one_pass,
           "timing": f"HIP events around each route, median of {a.reps} runs after 1 warm-up run; GB/s = input_bytes / time",
           "quality": "the effect of a budget on MRR / nDCG is NOT measured (no checkpoint available)", "cells": []}
    for nnz in [int(x) for x in a.nnz.split(",")]:
        x = synth_reps(B, V, min(nnz, V), dev, seed=nnz)
        full = Buffers(B, B * min(nnz, V), dev)
        _, ta = timed(lambda: route_all(lib, x, full), a.reps)
        for m in [int(x_) for x_ in a.budgets.split(",")]:
            buf_b, buf_c = Buffers(B, B * min(m, V), dev), Buffers(B, B * min(m, V), dev)
            _, tb = timed(lambda: route_topm(lib, x, m, buf_b), a.reps)
            got_c, tc = timed(lambda: route_torch(lib, x, m, buf_c), a.reps)
            got_b = buf_b.result()
            same = all(torch.equal(p, q) for p, q in zip(got_b, got_c))
            passes = 2 + (2 if (nnz > m and nnz > STAGE_KEYS) else 0)
            cell = {"nnz_per_row": nnz, "max_terms": m, "kept_entries": int(buf_b.n.value),
                    "a_sparse_compact": with_rate(ta), "b_sparse_compact_topm": with_rate(tb), "c_torch_topk_route": with_rate(tc),
                    "b_passes_over_a_row": passes,
                    "b_passes_note": ("count + fill from HBM" if passes == 2 else
                                      "count + fill from HBM, two radix steps over the row again (L2)") +
                                     ("" if nnz > m else "; no row is over budget, no select runs"),
                    "a_passes_over_a_row": 2, "b_over_a": round(tb["median_ms"] / ta["median_ms"], 3),
                    "c_over_b": round(tc["median_ms"] / tb["median_ms"], 3), "b_beats_c": tb["median_ms"] < tc["median_ms"],
                    "b_and_c_keep_the_same_entries": bool(same)}
            res["cells"].append(cell)
            print("[cell]", json.dumps(cell), file=sys.stderr, flush=True)
        del x, full
        torch.cuda.empty_cache()
    res["b_beats_c_everywhere"] = all(c["b_beats_c"] for c in res["cells"])
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
