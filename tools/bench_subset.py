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


def dense_routes_leg(a, dev):
    """The two routes of the dense subset search, each forced (SR_SUBSET_DENSE_ROUTE), for nq in {64, 6 980} and m in {100 000, 1 000 000,
    half the collection, all documents}, next to the unrestricted search of the same index in the same process (k = 1 000: the unchanged
    instantiation of the filter's pass - the yardstick of the mask route at "all documents allowed").  The filter is given as a packed
    bitmap (sr_dense_search_masked), so the gather route's time includes the bitmap -> list expansion and the mask route's the same.
    A route whose warm-up run takes longer than --slow-ms is timed with --slow-reps runs."""
    from scaling_retriever_amd.scoring import DenseIndexHIP, pack_doc_mask
    os.environ["SR_DEV_SWITCHES"] = "1"
    N = max(2 * a.k, int(a.n_docs * a.scale))
    D = dense_rows("gauss", N, a.hidden, dev, 1)
    idx = DenseIndexHIP(a.hidden, device=dev)
    idx.add_device_rows(D)
    idx.set_precision("fp32_filtered")
    rows = []
    for nq in a.route_nqs:
        Q = dense_queries("gauss", nq, a.hidden, dev, 2)
        _, full = timed(lambda: idx.search(Q, a.k), a.reps)
        for m in [x for x in a.route_ms if x < N // 2] + [N // 2, N]:
            flags = torch.zeros(N, dtype=torch.bool, device=dev)
            flags[draw_subset(N, m, dev, m)] = True
            words = pack_doc_mask(flags)
            row = {"m": m, "nq": nq, "k": a.k, "unrestricted_search": full}
            outs = {}
            for route in ("mask", "gather"):
                os.environ["SR_SUBSET_DENSE_ROUTE"] = route
                before = idx.filter_stats()
                t0 = time.perf_counter()
                idx.search(Q, a.k, mask=words)
                torch.cuda.synchronize()
                first_ms = (time.perf_counter() - t0) * 1e3
                outs[route], row[route] = timed(lambda: idx.search(Q, a.k, mask=words), a.slow_reps if first_ms > a.slow_ms else a.reps, warmup=0)
                after = idx.filter_stats()
                row[route]["served_by_the_filter_pass"] = after[0] + after[1] > before[0] + before[1]
            os.environ.pop("SR_SUBSET_DENSE_ROUTE", None)
            row["routes_equal_bit_for_bit"] = bool(torch.equal(outs["mask"][1], outs["gather"][1]) and
                                                    torch.equal(outs["mask"][0].view(torch.int32), outs["gather"][0].view(torch.int32)))
            row["mask_over_unrestricted"] = round(row["mask"]["median_ms"] / full["median_ms"], 4)
            rows.append(row)
            print("[dense routes]", json.dumps(row), file=sys.stderr, flush=True)
            del flags, words, outs
        del Q
    out = {"n_docs": N, "hidden": a.hidden, "kernel": "dense_split_kernel<true, true> (mask) / dense_subset_kernel (gather)", "rows": rows}
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


def timed_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def sparse_routes_leg(a, dev):
    """The three routes of the sparse subset search, each forced (SR_SUBSET_SPARSE_ROUTE=pairs|array|mask), the rule's own choice and the
    unrestricted sr_sparse_search of the same index in the same process (which launches the unmasked instantiation of the scorer's
    kernel), for nq in --sparse-route-nqs and m in --sparse-route-ms, then half the collection and all of it.  The filter is given as a
    packed bitmap (sr_sparse_search_masked), so a list route's time includes the bitmap -> list expansion.  Per m the legs ALTERNATE:
    one run of each per round, --reps rounds after one warm-up run each; a leg whose warm-up run takes longer than --slow-ms is timed
    with --slow-reps runs instead.  The three forced routes must return equal ids and score bits on every cell (asserted)."""
    from scaling_retriever_amd.scoring import SparseIndexHIP, pack_doc_mask
    os.environ["SR_DEV_SWITCHES"] = "1"
    N = max(8 * (a.k + 1024), int(a.n_docs * a.scale))
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    idx = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    legs = ("pairs", "array", "mask", "rule", "unrestricted_search")
    rows = []
    for nq in a.sparse_route_nqs:
        q_indptr, q_cols, q_vals = build_queries(a.vocab, nq, a.l0_q, dev, 4)
        for m in [x for x in a.sparse_route_ms if x < N // 2] + [N // 2, N]:
            flags = torch.zeros(N, dtype=torch.bool, device=dev)
            flags[draw_subset(N, m, dev, m + 1)] = True
            words = pack_doc_mask(flags)

            def run(leg):
                if leg in ("pairs", "array", "mask"):
                    os.environ["SR_SUBSET_SPARSE_ROUTE"] = leg
                else:
                    os.environ.pop("SR_SUBSET_SPARSE_ROUTE", None)
                if leg == "unrestricted_search":
                    return idx.search(q_indptr, q_cols, q_vals, a.k)
                return idx.search(q_indptr, q_cols, q_vals, a.k, mask=words)
            outs, ms, slow = {}, {leg: [] for leg in legs}, {}
            before = idx.cert_stats()
            for leg in legs:                                  # warm-up, and which legs are slow
                outs[leg], first_ms = timed_once(lambda: run(leg))
                slow[leg] = first_ms > a.slow_ms
                after = idx.cert_stats()
                if leg == "mask":
                    handed_back = after["redone_exact"] - before["redone_exact"]
                    through_the_scorer = after["queries"] - before["queries"]
                if leg == "rule":                             # the scorer saw the queries: the rule chose the mask route
                    rule_chose = "mask" if after["queries"] > before["queries"] else ("array" if m * 16 >= N else "pairs")
                before = after
            for r in range(a.reps):
                for leg in legs:
                    if not slow[leg] or r < a.slow_reps:
                        ms[leg].append(timed_once(lambda: run(leg))[1])
            os.environ.pop("SR_SUBSET_SPARSE_ROUTE", None)
            row = {"m": m, "nq": nq, "k": a.k}
            for leg in legs:
                row[leg] = {"median_ms": round(statistics.median(ms[leg]), 3), "min_ms": round(min(ms[leg]), 3), "max_ms": round(max(ms[leg]), 3),
                            "runs": len(ms[leg])}
            row["mask"]["queries_through_the_scorer"] = through_the_scorer
            row["mask"]["share_handed_back"] = round(handed_back / through_the_scorer, 4) if through_the_scorer else None
            row["rule_chooses"] = rule_chose
            for other in ("array", "mask"):
                assert torch.equal(outs["pairs"][1], outs[other][1]) and torch.equal(outs["pairs"][2], outs[other][2]) and \
                    torch.equal(outs["pairs"][0].view(torch.int32), outs[other][0].view(torch.int32)), f"routes pairs and {other} differ at nq={nq} m={m}"
            row["routes_equal_bit_for_bit"] = True
            fastest = min(row[r_]["median_ms"] for r_ in ("pairs", "array", "mask"))
            row["rule_over_fastest_forced"] = round(row["rule"]["median_ms"] / fastest, 4)
            row["mask_over_unrestricted"] = round(row["mask"]["median_ms"] / row["unrestricted_search"]["median_ms"], 4)
            rows.append(row)
            print("[sparse routes]", json.dumps(row), file=sys.stderr, flush=True)
            del flags, words, outs
    out = {"n_docs": N, "vocab": a.vocab, "postings": int(doc_ids.numel()), "L0_d": a.l0_d, "L0_q": a.l0_q,
           "kernel": "cert_score_kernel<KS, true> (mask) / sparse_subset_array_kernel (array) / sparse_subset_pairs_kernel (pairs)",
           "certified_scorer": idx.cert_stats()["present"] == 1, "rows": rows}
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
    ap.add_argument("--legs", type=str, default="dense,sparse", help="dense, sparse, dense_routes (both routes of the dense search forced), sparse_routes (the three routes of the sparse search forced)")
    ap.add_argument("--route-nqs", type=str, default="64,6980")
    ap.add_argument("--route-ms", type=str, default="100000,1000000", help="dense_routes: these, then half the collection and all of it")
    ap.add_argument("--sparse-route-nqs", type=str, default="6980,64")
    ap.add_argument("--sparse-route-ms", type=str, default="1000,10000,100000,1000000", help="sparse_routes: these, then half the collection and all of it")
    ap.add_argument("--slow-ms", type=float, default=1000.0, help="dense_routes / sparse_routes: a search slower than this is timed with --slow-reps runs")
    ap.add_argument("--slow-reps", type=int, default=1)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "subset_search.json"))
    a = ap.parse_args()
    a.nqs = [int(x) for x in a.nqs.split(",")]
    a.ms = [int(x) for x in a.ms.split(",")]
    a.route_nqs = [int(x) for x in a.route_nqs.split(",")]
    a.route_ms = [int(x) for x in a.route_ms.split(",")]
    a.sparse_route_nqs = [int(x) for x in a.sparse_route_nqs.split(",")]
    a.sparse_route_ms = [int(x) for x in a.sparse_route_ms.split(",")]
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
    for leg, fn in (("dense", dense_leg), ("sparse", sparse_leg), ("dense_routes", dense_routes_leg), ("sparse_routes", sparse_routes_leg)):
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
