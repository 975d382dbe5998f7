#!/usr/bin/env python3
"""Diversified dense search, measured: sr_dense_mmr - one kernel, one workgroup per query, all k greedy steps - against
the per-step composition a caller had before it (scaling_retriever_amd.mmr.mmr_by_steps: k x (score_pairs with the picked rows as
queries + torch operations for the maximum, the marginal value and the selection)), on the synthetic dense index of BASELINE.json
configs[1] (8 841 823 x 2048 rows, fp32 and fp16 storage), candidates taken from an actual search.

Per shape (nq, n, k): the outputs of the two are compared for equal bytes first; then HIP events around each call, the variants
alternating inside every round, median of --reps rounds.  The composition is timed twice per round: the difference of the two medians is
the spread a comparison has to exceed.  Also: search(fetch_k = n) alone, the whole search_mmr, and the bytes the kernel gathers per second.
Writes one JSON document (default profiles/mmr_search.json) and prints it.

  python tools/bench_mmr.py                               # full size, one MI355X
  python tools/bench_mmr.py --scale 0.01 --shapes 1:128:10,64:128:10
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

from synth import dense_queries, dense_rows  # noqa: E402

SHAPES = "1:128:10,64:128:10,6980:128:10,6980:1000:100,64:1000:100"
# MI355X, rows gathered into LDS tiles by index, GB/s per compute unit (256 units): from the XCD's L2 / the Infinity Cache / HBM
GATHER_GBPS_PER_CU = {"l2": 66.0, "infinity_cache": 33.5, "hbm": 23.0}


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def alternating(variants, reps, warmup=1):
    """{name: [ms per round]}: every round runs each variant once, in the given order."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    ms = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            ms[name].append(once(fn)[1])
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def same_bytes(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def shape_leg(idx, Q, nq, n, k, lam, reps, elem, dtype):
    from scaling_retriever_amd.mmr import mmr_by_steps
    q = Q[:nq].contiguous()
    (rel, ids), _ = once(lambda: idx.search(q, n))
    search_ms = [once(lambda: idx.search(q, n))[1] for _ in range(3)]
    got = idx.mmr(ids, rel, k, lam)
    equal = same_bytes(got, mmr_by_steps(idx, ids, rel, k, lam))
    assert equal, f"sr_dense_mmr and the per-step composition differ: {dtype} rows, (nq, n, k) = ({nq}, {n}, {k}); nothing was timed"
    ms = alternating({"kernel": lambda: idx.mmr(ids, rel, k, lam), "composition": lambda: mmr_by_steps(idx, ids, rel, k, lam),
                      "composition_again": lambda: mmr_by_steps(idx, ids, rel, k, lam)}, reps)
    whole_ms = [once(lambda: idx.search_mmr(q, k, n, lam))[1] for _ in range(3)]
    kern, comp, comp2 = summary(ms["kernel"]), summary(ms["composition"]), summary(ms["composition_again"])
    spread = abs(comp["median_ms"] - comp2["median_ms"])
    chains = nq * sum(n - t for t in range(1, k))                  # step t scores the n - t candidates still unselected
    gathered = chains * idx.dim * elem + nq * (k - 1) * idx.dim * elem
    gbps = gathered / (kern["median_ms"] * 1e-3) / 1e9
    cus = min(nq, torch.cuda.get_device_properties(0).multi_processor_count)
    return {"nq": nq, "n": n, "k": k, "lambda": lam, "outputs_equal_bytes": equal, "kernel": kern, "composition": comp,
            "composition_again": comp2, "composition_spread_ms": round(spread, 3),
            "kernel_speedup_over_composition": round(min(comp["median_ms"], comp2["median_ms"]) / kern["median_ms"], 2),
            "kernel_not_slower_beyond_the_spread": bool(kern["median_ms"] <= min(comp["median_ms"], comp2["median_ms"]) + spread),
            "search_fetch_k": summary(search_ms), "search_mmr_whole": summary(whole_ms),
            "chains": chains, "bytes_gathered": int(gathered), "gathered_GBps": round(gbps, 1), "workgroups_busy_at_most": cus,
            "gathered_GBps_per_busy_cu": round(gbps / cus, 2), "working_set_bytes_per_query": n * idx.dim * elem}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--shapes", type=str, default=SHAPES, help="nq:n:k, comma separated")
    ap.add_argument("--dtypes", type=str, default="fp32,fp16")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mmr_search.json"))
    a = ap.parse_args()
    from scaling_retriever_amd.scoring import DenseIndexHIP
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    N = max(4096, int(a.n_docs * a.scale))
    t0 = time.time()
    res = {"what": "exact greedy MMR on the device (sr_dense_mmr) against the per-step composition k x (score_pairs + torch select) "
                   "(tools/bench_mmr.py)",
           "device": torch.cuda.get_device_name(0), "n_gpus": 1, "n_docs": N, "hidden": a.hidden, "data": "synthetic (gauss), candidates = "
           "the top n of a search", "timing": f"HIP events around each call; variants alternate inside a round; median of {a.reps} rounds "
           "after 1 warm-up round; searches: median of 3", "gather_rates_GBps_per_cu_to_plan_with": GATHER_GBPS_PER_CU, "legs": {}}
    Q = dense_queries("gauss", max(s[0] for s in shapes), a.hidden, dev, 2)
    for dtype in a.dtypes.split(","):
        D = dense_rows("gauss", N, a.hidden, dev, 1)
        if dtype == "fp16":
            D = D.to(torch.float16)
        idx = DenseIndexHIP(a.hidden, device=dev, row_dtype=dtype)
        idx.add_device_rows(D)
        idx.set_precision("fp32_filtered")                 # what the retrieval drivers use; the same bits as the exact kernel
        legs = []
        for nq, n, k in shapes:
            legs.append(shape_leg(idx, Q, nq, n, k, a.lam, a.reps, 2 if dtype == "fp16" else 4, dtype))
            print(f"[{dtype}]", json.dumps(legs[-1]), file=sys.stderr, flush=True)
        res["legs"][dtype] = legs
        idx.close()
        del D, idx
        torch.cuda.empty_cache()
    every = [leg for legs in res["legs"].values() for leg in legs]
    res["outputs_equal_bytes"] = all(leg["outputs_equal_bytes"] for leg in every)
    res["kernel_not_slower_at_any_shape"] = all(leg["kernel_not_slower_beyond_the_spread"] for leg in every)
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
