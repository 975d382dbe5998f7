#!/usr/bin/env python3
"""Dense search under per-query document filters (sr_dense_search_grouped), measured (profiles/grouped_search.json) on the synthetic
config-2 index of tools/bench_subset.py: 8 841 823 x 2 048 fp32 rows, fp32_filtered, 6 980 queries, k = 1 000.

One cell per (G, mask kind): G in {1, 8, 100, 1 000} groups, the queries dealt to them round-robin; every group has a mask of its own -
random 50 %, random 10 %, or one band of 10 % of the ids (another band per group).  Per cell, alternated in one process:

  grouped_pass      sr_dense_search_grouped, SR_GROUPED_DENSE_ROUTE=pass: one pass over the rows for all groups
  grouped_loop      the same call, SR_GROUPED_DENSE_ROUTE=loop: the gather route group by group
  per_group_masked  the baseline - what a caller had before this entry point: one sr_dense_search_masked per group over that group's
                    queries (gathered beforehand, outside the timed region), on whatever route each call picks
  unrestricted      sr_dense_search of all queries, no filter
  masked            G = 1 only: sr_dense_search_masked on the same mask, mask route forced - grouped_pass / masked is the price of the
                    per-query offset

HIP events around each variant, median of --reps (7) runs after a warm-up; two runs where the warm-up shows a variant at over a second.
No target: the file records what the hardware says.  The child process that measures runs under a time limit; if it fails or runs out of
time nothing more is started on the GPU and the file says so.

  python tools/bench_grouped.py                       # full size, one MI355X
  python tools/bench_grouped.py --scale 0.02 --nq 300 --groups 1 8
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MASKS = {"random_50pct": "random 50 % per group", "random_10pct": "random 10 % per group", "band_10pct": "one band of 10 % of the ids per group"}
CROSSOVER = 6980 * 130000            # SR_SUBSET_DENSE_CROSSOVER (csrc/dense_restrict.hip): what the auto rule compares the pairs with


def alternated(fns, reps, warmup=1, once_over_ms=1000.0):
    """{name: stats} of the given callables, run in turn between two events each; a variant whose warm-up run takes over once_over_ms
    is timed twice instead of `reps` times."""
    import torch
    ms, runs = {n: [] for n in fns}, {n: reps for n in fns}
    for r in range(warmup + reps):
        for n, fn in fns.items():
            if r >= warmup + runs[n]:
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
            if r >= warmup:
                ms[n].append(t)
            elif t > once_over_ms:
                runs[n] = min(reps, 2)
    return {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs": len(v)}
            for n, v in ms.items()}


def group_words(kind, G, N, dev, seed):
    """int32 [G, ceil(N / 32)] on the device, packed group by group (a bool [G, N] would be 8.8 GB at G = 1 000)."""
    import torch
    from scaling_retriever_amd.scoring import pack_doc_mask
    gen = torch.Generator(device=dev).manual_seed(seed)
    words = torch.empty((G, (N + 31) // 32), dtype=torch.int32, device=dev)
    counts = []
    for g in range(G):
        if kind == "band_10pct":
            m = torch.zeros(N, dtype=torch.bool, device=dev)
            start = (g * (N // max(G, 1))) % (N - N // 10)
            m[start:start + N // 10] = True
        else:
            m = torch.rand(N, device=dev, generator=gen) < (0.5 if kind == "random_50pct" else 0.1)
        counts.append(int(m.sum()))
        words[g] = pack_doc_mask(m)
    return words, counts


def measure(a):
    import torch
    from scaling_retriever_amd.scoring import DenseIndexHIP
    from synth import dense_queries, dense_rows
    os.environ["SR_DEV_SWITCHES"] = "1"
    dev = torch.device("cuda", 0)
    N, H, nq, k = max(4096, int(a.n_docs * a.scale)), a.hidden, a.nq, a.k
    idx = DenseIndexHIP(H, device=dev)
    idx.set_precision("fp32_filtered")
    idx.add_device_rows(dense_rows("gauss", N, H, dev, 1))
    Q = dense_queries("gauss", nq, H, dev, 2).contiguous()
    out = {"N": N, "H": H, "nq": nq, "k": k, "rows": "fp32", "precision": "fp32_filtered", "cells": []}

    def route(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
    for G in a.groups:
        groups = torch.arange(nq, device=dev) % G
        q_of = [Q[g::G].contiguous() for g in range(G)]            # the baseline's per-group batches, gathered outside the timed region
        for kind in a.masks:
            words, counts = group_words(kind, G, N, dev, 100 + G)
            pairs = sum(counts[g] * int(q_of[g].shape[0]) for g in range(G))
            got = {}

            def grouped(r):
                route("SR_GROUPED_DENSE_ROUTE", r)
                got[r] = idx.search_grouped(Q, k, words, groups)
                route("SR_GROUPED_DENSE_ROUTE", None)

            def per_group():
                for g in range(G):
                    if q_of[g].shape[0]:
                        idx.search(q_of[g], k, mask=words[g])

            def masked():
                route("SR_SUBSET_DENSE_ROUTE", "mask")
                got["masked"] = idx.search(Q, k, mask=words[0])
                route("SR_SUBSET_DENSE_ROUTE", None)
            fns = {"grouped_pass": lambda: grouped("pass"), "grouped_loop": lambda: grouped("loop"), "per_group_masked": per_group,
                   "unrestricted": lambda: idx.search(Q, k)}
            if G == 1:
                fns["masked"] = masked
            before = idx.filter_stats()
            grouped("pass")
            after = idx.filter_stats()
            t = alternated(fns, a.reps)
            same = torch.equal(got["pass"][1], got["loop"][1]) and torch.equal(got["pass"][0].view(torch.int32), got["loop"][0].view(torch.int32))
            cell = {"G": G, "mask": MASKS[kind], "allowed_per_group_mean": round(sum(counts) / G, 1), "pairs": pairs,
                    "auto_route": "pass" if pairs >= CROSSOVER else "loop",
                    "filter_stats_delta_of_one_pass_call": [after[0] - before[0], after[1] - before[1]],
                    "pass_equals_loop_bit_for_bit": bool(same), **t,
                    "ratios": {"grouped_pass_over_per_group_masked": round(t["grouped_pass"]["median_ms"] / t["per_group_masked"]["median_ms"], 4),
                               "grouped_loop_over_per_group_masked": round(t["grouped_loop"]["median_ms"] / t["per_group_masked"]["median_ms"], 4),
                               "grouped_pass_over_unrestricted": round(t["grouped_pass"]["median_ms"] / t["unrestricted"]["median_ms"], 4)}}
            if G == 1:
                same_m = torch.equal(got["pass"][1], got["masked"][1]) and torch.equal(got["pass"][0].view(torch.int32), got["masked"][0].view(torch.int32))
                cell["pass_equals_masked_bit_for_bit"] = bool(same_m)
                cell["ratios"]["grouped_pass_over_masked"] = round(t["grouped_pass"]["median_ms"] / t["masked"]["median_ms"], 4)
            print("[grouped]", json.dumps(cell), file=sys.stderr, flush=True)
            print("CELL " + json.dumps(cell), flush=True)          # the parent keeps the finished cells if this process is ended early
            out["cells"].append(cell)
            del words, got
    idx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8, 100, 1000])
    ap.add_argument("--masks", nargs="+", default=list(MASKS), choices=list(MASKS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=1080, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process and print the JSON")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "grouped_search.json"))
    a = ap.parse_args()
    if a.child:
        import torch
        torch.cuda.set_device(0)
        t0 = time.time()
        res = measure(a)
        res["seconds"] = round(time.time() - t0, 1)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        return 0
    res = {"what": "dense top-k under per-query document filters (sr_dense_search_grouped) against one sr_dense_search_masked per group "
                   "(tools/bench_grouped.py)", "n_gpus": 1, "data": "synthetic", "scale": a.scale,
           "timing": f"HIP events around each variant, variants alternated in one process, median of {a.reps} runs after a warm-up (2 runs "
                     "where a variant takes over a second)",
           "baseline": "per_group_masked: one sr_dense_search_masked per group over that group's queries, each call on the route it picks"}
    rc, stdout = 0, b""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], stdout=subprocess.PIPE, timeout=a.timeout)
        stdout = p.stdout
        if p.returncode != 0:
            res["incomplete"] = f"the measuring process ended with exit status {p.returncode}"
            rc = p.returncode
    except subprocess.TimeoutExpired as e:
        stdout = e.stdout or b""
        res["incomplete"] = f"the measuring process was ended at its time limit of {a.timeout} s"
        rc = 124
    lines = stdout.decode().strip().splitlines()
    if rc == 0:
        res.update(json.loads(lines[-1]))
    else:                                                # the cells that were finished
        res["cells"] = [json.loads(ln[5:]) for ln in lines if ln.startswith("CELL ")]
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
