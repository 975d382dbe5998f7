#!/usr/bin/env python3
"""Diversified sparse search, measured: sr_sparse_mmr - one kernel, one workgroup per query, all k greedy picks on the
documents' forward rows - against the per-step composition a caller had before it (scaling_retriever_amd.mmr.sparse_mmr_by_steps: k x
(the picked rows gathered into a query CSR + score_pairs + torch operations for the maximum, the marginal value and the selection)), on
the synthetic sparse index of BASELINE.json configs[2] (8 841 823 documents x 128 terms over 128 256), candidates taken from an actual
search, both similarities.

Per shape (nq, n, k) and similarity: the outputs of the two are compared for equal bytes first; then HIP events around each call, the
variants alternating inside every round, median of --reps rounds.  The composition is timed twice per round: the difference of the two
medians is the spread a comparison has to exceed.  Also: search(fetch_k = n) alone, the whole search_mmr, the one-off forward_rows()
build, and the bytes of row entries the kernel gathers per second - counted from the picks it made (a candidate picked at pick t was
scored t times, an unpicked one k - 1 times; every pick but the last is staged once; cosine reads every row once more for its norm).
Writes one JSON document (default profiles/mmr_sparse_search.json) and prints it.

  python tools/bench_mmr_sparse.py                               # full size, one MI355X
  python tools/bench_mmr_sparse.py --scale 0.01 --shapes 1:128:10,64:128:10
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

from synth import build_index, build_queries  # noqa: E402

SHAPES = "1:128:10,64:128:10,6980:128:10,6980:1000:100,64:1000:100"
# MI355X, rows gathered by index, GB/s per compute unit (256 units): from the XCD's L2 / the Infinity Cache / HBM
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
    return all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def gathered_bytes(fwd_indptr, ids, counts, got, k, sim):
    """8 bytes per row entry the kernel loads, from the picks it made."""
    nq, n = ids.shape
    valid = (ids >= 0) & (torch.arange(n, device=ids.device)[None, :] < counts[:, None])
    at = ids.clamp(min=0)
    lens = (fwd_indptr[at + 1] - fwd_indptr[at]) * valid
    scored = torch.full((nq, n + 1), k - 1, dtype=torch.int64, device=ids.device)   # an unpicked candidate: every round; column n: padding picks
    pos, picks = got[3].to(torch.int64), got[4].to(torch.int64)
    made = torch.arange(k, device=ids.device)[None, :] < picks[:, None]
    at_pos = torch.where(made, pos, torch.full_like(pos, n))
    rounds = torch.arange(k, device=ids.device).expand(nq, k).contiguous()          # picked at pick t: scored in rounds 1 .. t
    scored.scatter_(1, at_pos, rounds)
    staged = torch.zeros((nq, n + 1), dtype=torch.int64, device=ids.device)
    staged.scatter_(1, at_pos, (rounds < k - 1).to(torch.int64))                   # every pick but the k-th is staged once
    entries = (lens * (scored[:, :n] + staged[:, :n] + (1 if sim == "cosine" else 0))).sum()
    return 8 * int(entries), round(float(lens.sum()) / max(1, int(valid.sum())), 1)


def shape_leg(idx, fwd, Q, l0_q, nq, n, k, lam, sim, reps):
    from scaling_retriever_amd.mmr import sparse_mmr_by_steps
    q = (Q[0][:nq + 1], Q[1][:nq * l0_q], Q[2][:nq * l0_q])
    (rel, ids, counts), _ = once(lambda: idx.search(*q, n))
    search_ms = [once(lambda: idx.search(*q, n))[1] for _ in range(3)]
    got = idx.mmr(ids, rel, k, lam, counts=counts, sim=sim)
    equal = same_bytes(got, sparse_mmr_by_steps(idx, ids, rel, k, lam, counts=counts, sim=sim))
    assert equal, f"sr_sparse_mmr and the per-step composition differ: sim = {sim}, (nq, n, k) = ({nq}, {n}, {k}); nothing was timed"
    ms = alternating({"kernel": lambda: idx.mmr(ids, rel, k, lam, counts=counts, sim=sim),
                      "composition": lambda: sparse_mmr_by_steps(idx, ids, rel, k, lam, counts=counts, sim=sim),
                      "composition_again": lambda: sparse_mmr_by_steps(idx, ids, rel, k, lam, counts=counts, sim=sim)}, reps)
    whole_ms = [once(lambda: idx.search_mmr(*q, k, n, lam, sim=sim))[1] for _ in range(3)]
    kern, comp, comp2 = summary(ms["kernel"]), summary(ms["composition"]), summary(ms["composition_again"])
    spread = abs(comp["median_ms"] - comp2["median_ms"])
    gathered, mean_len = gathered_bytes(fwd[0], ids, counts, got, k, sim)
    gbps = gathered / (kern["median_ms"] * 1e-3) / 1e9
    cus = min(nq, torch.cuda.get_device_properties(0).multi_processor_count)
    return {"nq": nq, "n": n, "k": k, "lambda": lam, "sim": sim, "outputs_equal_bytes": equal, "kernel": kern, "composition": comp,
            "composition_again": comp2, "composition_spread_ms": round(spread, 3),
            "kernel_speedup_over_composition": round(min(comp["median_ms"], comp2["median_ms"]) / kern["median_ms"], 2),
            "kernel_not_slower_beyond_the_spread": bool(kern["median_ms"] <= min(comp["median_ms"], comp2["median_ms"]) + spread),
            "search_fetch_k": summary(search_ms), "search_mmr_whole": summary(whole_ms),
            "mean_candidates_per_query": round(float(counts.sum()) / nq, 1), "mean_terms_per_candidate": mean_len,
            "bytes_gathered": gathered, "gathered_GBps": round(gbps, 2), "workgroups_busy_at_most": cus,
            "gathered_GBps_per_busy_cu": round(gbps / cus, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--shapes", type=str, default=SHAPES, help="nq:n:k, comma separated")
    ap.add_argument("--sims", type=str, default="cosine,ip")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mmr_sparse_search.json"))
    a = ap.parse_args()
    from scaling_retriever_amd.scoring import SparseIndexHIP
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    N = max(4096, int(a.n_docs * a.scale))
    t0 = time.time()
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    idx = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    builds = []                                            # the one-off build, three times: host clock around a call that ends synchronised
    for _ in range(3):
        idx.drop_forward_rows()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fwd = idx.forward_rows()
        torch.cuda.synchronize()
        builds.append(round((time.perf_counter() - t) * 1e3, 1))
    res = {"what": "exact greedy MMR on the sparse head (sr_sparse_mmr) against the per-step composition k x (gather + score_pairs + torch "
                   "select) (tools/bench_mmr_sparse.py)",
           "device": torch.cuda.get_device_name(0), "n_gpus": 1, "n_docs": N, "vocab": a.vocab, "postings": int(indptr[-1]),
           "data": "synthetic (Zipf index), candidates = the top n of a search",
           "timing": f"HIP events around each call; variants alternate inside a round; median of {a.reps} rounds after 1 warm-up round; "
                     "searches and whole search_mmr calls: median of 3",
           "forward_rows_build_ms": builds, "forward_rows_bytes": int(sum(t.numel() * t.element_size() for t in fwd)),
           "gather_rates_GBps_per_cu_to_compare_with": GATHER_GBPS_PER_CU, "legs": []}
    Q = build_queries(a.vocab, max(s[0] for s in shapes), a.l0_q, dev, 4)
    for sim in a.sims.split(","):
        for nq, n, k in shapes:
            res["legs"].append(shape_leg(idx, fwd, Q, a.l0_q, nq, n, k, a.lam, sim, a.reps))
            print(json.dumps(res["legs"][-1]), file=sys.stderr, flush=True)
    res["outputs_equal_bytes"] = all(leg["outputs_equal_bytes"] for leg in res["legs"])
    res["kernel_not_slower_at_any_shape"] = all(leg["kernel_not_slower_beyond_the_spread"] for leg in res["legs"])
    res["shapes_that_lose"] = [{k_: leg[k_] for k_ in ("nq", "n", "k", "sim")} for leg in res["legs"] if not leg["kernel_not_slower_beyond_the_spread"]]
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
    idx.close()


if __name__ == "__main__":
    main()
