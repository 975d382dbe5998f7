#!/usr/bin/env python3
"""Range searches and the exact hybrid search under per-query document filters (filter groups), measured
(profiles/grouped_range.json), on the synthetic indexes of tools/bench_masked_range.py: dense N x 2 048 fp32 rows (config 2), sparse
V = 128 256, Zipf(1.0), 128 postings per document, 32 query terms (config 3); N = 8 841 823 x --scale.  Legs, each in a child process
of its own under its own time limit; a leg that fails or runs out of time ends the run (nothing more is started on the GPU), and the
file says which legs ran.

  dense   --nq queries dealt round-robin over G = 1 / 8 / 100 groups; masks random 50 %, random 10 %, and one contiguous band per group
          (N / G ids, each group's beginning elsewhere).  Thresholds at each query's rank-th best allowed score.  Timed: the grouped
          count, and the grouped count + fill, against one masked count (+ fill) per group over that group's queries.  In every cell
          both routes must return the same bytes (lims, ids, score bits): asserted.
  sparse  the same cells on the sparse head.
  hybrid  hybrid.search_fused for 64 queries in 8 groups (random 50 % masks) against one search_fused(mask=) per group; same rows: asserted.
  parent  (with --parent-lib PATH, the parent commit's libsr_hip.so) the unrestricted and the masked dense and sparse range count + fill
          of this library against the parent's, both libraries in this one process, alternated; the parent runs twice (p, p2), so the
          file holds the spread of two identical runs next to the ratios.

HIP events around each call, the variants alternated in one process, median of --reps (7) runs after a warm-up; two runs where a call
takes over a second.

  python tools/bench_grouped_range.py                      # full size, one MI355X
  python tools/bench_grouped_range.py --scale 0.05 --nq 512 --parent-lib /path/to/parent/libsr_hip.so
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_masked_range import alternated      # noqa: E402

KINDS = ("r50", "r10", "band")


def group_masks(kind, n, n_groups, dev, seed):
    """bool [G, n] on the device."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    if kind == "band":
        out = torch.zeros((n_groups, n), dtype=torch.bool, device=dev)
        width = max(1, n // n_groups)
        for i in range(n_groups):
            out[i, i * width:(i + 1) * width] = True
        return out
    share = 0.5 if kind == "r50" else 0.1
    return torch.stack([torch.rand(n, device=dev, generator=g) < share for _ in range(n_groups)])


def same_bytes(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def scatter_lists(parts, members, nq, dev):
    """Per-group CSR results (lims, scores, ids) of the member queries -> one CSR in query order."""
    import torch
    counts = torch.zeros(nq, dtype=torch.int64, device=dev)
    for (lims, _, _), sel in zip(parts, members):
        counts[sel] = lims[1:] - lims[:-1]
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    lims[1:] = torch.cumsum(counts, 0)
    scores = torch.empty(int(lims[-1]), dtype=torch.float32, device=dev)
    ids = torch.empty(int(lims[-1]), dtype=torch.int64, device=dev)
    for (pl, ps, pi), sel in zip(parts, members):
        n = pl[1:] - pl[:-1]
        dst = torch.repeat_interleave(lims[sel] - pl[:-1], n, output_size=int(pl[-1])) + torch.arange(int(pl[-1]), device=dev)
        scores[dst], ids[dst] = ps, pi
    return lims, scores, ids


def cells(a, run_grouped, run_loop, thresholds, n, dev, tag):
    """The (mask kind, G) grid of one head.  run_grouped(words, groups, thr, fill) / run_loop(words, members, thr, fill) -> CSR result."""
    import torch
    from scaling_retriever_amd.scoring import pack_doc_masks
    rows = []
    for kind in KINDS:
        for G in a.groups:
            flags = group_masks(kind, n, G, dev, 100 + G)
            words = pack_doc_masks(flags)
            groups = (torch.arange(a.nq, device=dev) % G).to(torch.int32)
            members = [torch.nonzero(groups == g)[:, 0] for g in range(G)]
            members = [m for m in members if m.numel()]
            used = [int(groups[m[0]]) for m in members]
            thr = thresholds(flags, groups)
            got = {}
            t_count = alternated({"grouped": lambda: got.__setitem__("gc", run_grouped(words, groups, thr, False)),
                                  "loop": lambda: got.__setitem__("lc", run_loop(words, used, members, thr, False))}, a.reps)
            t_pair = alternated({"grouped": lambda: got.__setitem__("g", run_grouped(words, groups, thr, True)),
                                 "loop": lambda: got.__setitem__("l", run_loop(words, used, members, thr, True))}, a.reps)
            loop = scatter_lists(got["l"], members, a.nq, dev)
            assert same_bytes(got["g"], loop), (tag, kind, G, "the grouped pass and the per-group loop differ")
            row = {"masks": kind, "G": G, "nq": a.nq, "total_hits": int(got["g"][0][-1]), "same_bytes": True,
                   "count": t_count, "count_plus_fill": t_pair,
                   "grouped_over_loop": {"count": round(t_count["grouped"]["median_ms"] / t_count["loop"]["median_ms"], 4),
                                         "count_plus_fill": round(t_pair["grouped"]["median_ms"] / t_pair["loop"]["median_ms"], 4)}}
            print(f"[{tag}]", json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
            del flags, words, got, loop
    return rows


def leg_dense(a):
    import torch
    from scaling_retriever_amd.scoring import DenseIndexHIP
    from synth import dense_queries, dense_rows
    dev = torch.device("cuda", 0)
    N, H = max(4096, int(a.n_docs * a.scale)), a.hidden
    idx = DenseIndexHIP(H, device=dev)
    idx.add_device_rows(dense_rows("gauss", N, H, dev, 1))
    Q = dense_queries("gauss", a.nq, H, dev, 2).contiguous()

    def thresholds(flags, groups):
        return idx.search_grouped(Q, a.rank, flags, groups)[0][:, a.rank - 1].contiguous()      # -FLT_MAX where a group allows fewer: every allowed document

    def run_grouped(words, groups, thr, fill):
        q, t, lims, n = idx.range_count(Q, thr, masks=words, query_group=groups)
        return (lims,) + idx.range_fill(q, t, lims, n, masks=words, query_group=groups) if fill else (lims, None, None)

    def run_loop(words, used, members, thr, fill):
        out = []
        for g, sel in zip(used, members):
            q, t, lims, n = idx.range_count(Q[sel], thr[sel], mask=words[g])
            out.append((lims,) + idx.range_fill(q, t, lims, n, mask=words[g]) if fill else (lims, None, None))
        return out
    out = {"N": N, "H": H, "rows": "fp32", "rank": a.rank, "cells": cells(a, run_grouped, run_loop, thresholds, N, dev, "dense")}
    idx.close()
    return out


def leg_sparse(a):
    import torch
    from scaling_retriever_amd.scoring import SparseIndexHIP
    from synth import build_index, build_queries
    dev = torch.device("cuda", 0)
    N = max(8192, int(a.n_docs * a.scale))
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    idx = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    qp, qc, qv = build_queries(a.vocab, a.nq, a.l0_q, dev, 4)
    qp, qc, qv = qp.to(torch.int64).contiguous(), qc.to(torch.int32).contiguous(), qv.to(torch.float32).contiguous()
    from scaling_retriever_amd.hybrid import _csr_rows

    def thresholds(flags, groups):
        ss, _, sc = idx.search_grouped(qp, qc, qv, a.rank, flags, groups, threshold=0.0)
        return torch.where(sc == a.rank, ss[:, a.rank - 1], torch.zeros_like(ss[:, 0])).contiguous()

    def run_grouped(words, groups, thr, fill):      # the sparse front end has no separate halves: the count alone is timed through thr = +inf
        return idx.range_search(qp, qc, qv, thr if fill else float("inf"), masks=words, query_group=groups)

    def run_loop(words, used, members, thr, fill):
        out = []
        for g, sel in zip(used, members):
            sub = _csr_rows(qp, qc, qv, sel)
            out.append(idx.range_search(*sub, thr[sel] if fill else float("inf"), mask=words[g]))
        return out
    out = {"N": N, "V": a.vocab, "L0_d": a.l0_d, "L0_q": a.l0_q, "rank": a.rank,
           "note": "count = a call whose thresholds are +inf (the count pass runs, the fill has nothing to write)",
           "cells": cells(a, run_grouped, run_loop, thresholds, N, dev, "sparse")}
    idx.close()
    return out


def leg_hybrid(a):
    import numpy as np
    import torch
    from scaling_retriever_amd import hybrid
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP, pack_doc_masks
    from synth import build_index, build_queries, dense_queries, dense_rows
    dev = torch.device("cuda", 0)
    k, w, nq, G = a.k, (1.0, 1.0), 64, 8
    N = max(8 * (k + 1024), int(a.n_docs * a.scale))
    dense = DenseIndexHIP(a.hidden, device=dev)
    dense.add_device_rows(dense_rows("gauss", N, a.hidden, dev, 1))
    dense.set_precision("fp32_filtered")
    Q = dense_queries("gauss", nq, a.hidden, dev, 2)
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    sparse = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    qp, qc, qv = build_queries(a.vocab, nq, a.l0_q, dev, 4)
    qp = qp.to(torch.int64)
    s2d = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    d2s = torch.empty_like(s2d)
    d2s[s2d] = torch.arange(N, device=dev)
    words = pack_doc_masks(group_masks("r50", N, G, dev, 7))
    groups = np.arange(nq) % G
    got = {}

    def grouped():
        got["g"] = hybrid.search_fused(dense, sparse, d2s, s2d, Q, qp, qc, qv, k, weights=w, masks=words, query_group=groups)

    def loop():
        got["l"] = []
        for g in range(G):
            sel = torch.from_numpy(np.flatnonzero(groups == g)).to(dev)
            sub = hybrid._csr_rows(qp, qc, qv, sel)
            got["l"].append(hybrid.search_fused(dense, sparse, d2s, s2d, Q[sel], *sub, k, weights=w, mask=words[g]))
    t = alternated({"grouped": grouped, "loop": loop}, a.reps)
    for g in range(G):
        sel = np.flatnonzero(groups == g)
        one = got["l"][g]
        assert np.array_equal(one[1], got["g"][1][sel]) and np.array_equal(one[0].view(np.int32), got["g"][0][sel].view(np.int32)), g
        assert np.array_equal(one[2], got["g"][2][sel]) and np.array_equal(one[3]["depth"], got["g"][3]["depth"][sel]), g
    stats = got["g"][3]
    routes = {("range" if d < 0 else f"depth_{stats['depths'][d]}"): int((stats["depth"] == d).sum()) for d in np.unique(stats["depth"])}
    out = {"N": N, "k": k, "nq": nq, "G": G, "masks": "r50", "search_fused": t, "same_rows_and_routes": True, "queries_per_route": routes,
           "grouped_over_loop": round(t["grouped"]["median_ms"] / t["loop"]["median_ms"], 4)}
    print("[hybrid]", json.dumps(out), file=sys.stderr, flush=True)
    return out


def leg_parent(a):
    """The unrestricted and masked range entry points: this library against the parent's, in one process."""
    import torch
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP, pack_doc_mask
    from synth import build_index, build_queries, dense_queries, dense_rows
    dev = torch.device("cuda", 0)
    N, H = max(8192, int(a.n_docs * a.scale)), a.hidden
    rows = dense_rows("gauss", N, H, dev, 1)
    Q = dense_queries("gauss", a.nq, H, dev, 2).contiguous()
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    qp, qc, qv = build_queries(a.vocab, a.nq, a.l0_q, dev, 4)
    qp, qc, qv = qp.to(torch.int64).contiguous(), qc.to(torch.int32).contiguous(), qv.to(torch.float32).contiguous()
    mask = pack_doc_mask(torch.rand(N, device=dev, generator=torch.Generator(device=dev).manual_seed(9)) < 0.5)

    def make():
        d = DenseIndexHIP(H, device=dev)
        d.add_device_rows(rows)                      # the rows are not copied: both libraries read the same tensor
        return d, SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    here = make()
    import ctypes
    plib = ctypes.CDLL(os.path.abspath(a.parent_lib))
    for name, (res, args) in _lib.SIGNATURES.items():              # the parent lacks the entries this change adds
        fn = getattr(plib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    keep, _lib._lib = _lib._lib, plib
    try:
        parent = make()                              # an index keeps the library it was created with
    finally:
        _lib._lib = keep
    thr_d = here[0].search(Q, a.rank)[0][:, a.rank - 1].contiguous()
    ss, _, sc = here[1].search(qp, qc, qv, a.rank, threshold=0.0)
    thr_s = torch.where(sc == a.rank, ss[:, a.rank - 1], torch.zeros_like(ss[:, 0])).contiguous()
    out = {"N": N, "nq": a.nq, "parent_lib": "libsr_hip.so of the parent commit", "entries": {}}
    for name, fn in (("dense_range", lambda ix, m: ix[0].range_search(Q, thr_d, mask=m)),
                     ("sparse_range", lambda ix, m: ix[1].range_search(qp, qc, qv, thr_s, mask=m))):
        for label, m in (("unrestricted", None), ("masked_r50", mask)):
            got = {}
            t = alternated({"p": lambda: got.__setitem__("p", fn(parent, m)), "new": lambda: got.__setitem__("new", fn(here, m)),
                            "p2": lambda: got.__setitem__("p2", fn(parent, m))}, a.reps)
            assert same_bytes(got["p"], got["new"]), (name, label, "this library and the parent's differ")
            p = t["p"]["median_ms"]
            spread = abs(t["p2"]["median_ms"] / p - 1.0)
            row = {**t, "new_over_parent": round(t["new"]["median_ms"] / p, 4), "parent_again_over_parent": round(t["p2"]["median_ms"] / p, 4),
                   "allowed_margin": round(spread + 0.01, 4), "within_margin": bool(t["new"]["median_ms"] / p <= 1.0 + spread + 0.01),
                   "same_bytes": True}
            print(f"[parent] {name} {label}", json.dumps(row), file=sys.stderr, flush=True)
            out["entries"][f"{name}_{label}"] = row
    return out


LEGS = {"dense": leg_dense, "sparse": leg_sparse, "hybrid": leg_hybrid, "parent": leg_parent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (every index)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8, 100])
    ap.add_argument("--rank", type=int, default=100, help="thresholds: each query's rank-th best allowed score")
    ap.add_argument("--k", type=int, default=1000, help="topk of the hybrid leg")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", type=str, default=None, help="the parent commit's libsr_hip.so: enables the `parent` leg")
    ap.add_argument("--legs", nargs="+", default=None, choices=list(LEGS))
    ap.add_argument("--leg-timeout", type=int, default=540, help="seconds a leg's child process may take")
    ap.add_argument("--leg", choices=list(LEGS), help="(internal) run this leg in this process and print its JSON")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "grouped_range.json"))
    a = ap.parse_args()
    if a.leg:
        import torch
        torch.cuda.set_device(0)
        t0 = time.time()
        res = LEGS[a.leg](a)
        res["seconds"] = round(time.time() - t0, 1)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        return 0
    legs = a.legs or [x for x in LEGS if x != "parent" or a.parent_lib]
    if "parent" in legs and not a.parent_lib:
        ap.error("the parent leg needs --parent-lib")
    res = {}
    if os.path.exists(a.out):                       # legs measured by an earlier run are kept: a leg can be run on its own
        with open(a.out) as f:
            res = json.load(f)
    res.update({"what": "range searches and the exact hybrid search under filter groups against one masked call per group, and the "
                        "existing range entry points against the parent commit's library (tools/bench_grouped_range.py)", "n_gpus": 1,
                "data": "synthetic",
                "timing": f"HIP events around each call, variants alternated in one process, median of {a.reps} runs after a warm-up "
                          "(2 runs where a call takes over a second); one child process per leg"})
    res.setdefault("legs_not_run", {})
    passed = [x for x in sys.argv[1:]]
    rc = 0
    for leg in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + passed
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            res["legs_not_run"][leg] = f"ended at its time limit of {a.leg_timeout} s"
            rc = 124
            break
        if p.returncode != 0:
            res["legs_not_run"][leg] = f"exit status {p.returncode}"
            rc = p.returncode
            break                                    # nothing more is started after a failure
        res[leg] = json.loads(p.stdout.decode().strip().splitlines()[-1])
        res[leg]["scale"] = a.scale
        res["legs_not_run"].pop(leg, None)
    for leg in LEGS:
        if leg not in res and leg not in res["legs_not_run"]:
            res["legs_not_run"][leg] = "not started"
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
