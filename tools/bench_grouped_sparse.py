#!/usr/bin/env python3
"""Sparse search under per-query document filters (sr_sparse_search_grouped), measured (profiles/grouped_sparse_search.json) on the
synthetic config-3 index of tools/bench_subset.py: 8 841 823 documents, V = 128 256, Zipf(1.0), 6 980 queries of 32 terms, k = 1 000.

One cell per (nq, G, mask kind): G in {1, 8, 100, 1 000} groups at 6 980 queries (and a 64-query row per mask kind at --small-groups),
the queries dealt to the groups round-robin; every group has a mask of its own - random 50 %, random 10 %, or one band of 10 % of the
positions (another band per group).  Per cell, alternated in one process:

  grouped_pass      sr_sparse_search_grouped, SR_GROUPED_SPARSE_ROUTE=pass: one pass of the certified scorer for all groups
  grouped_loop      the same call, SR_GROUPED_SPARSE_ROUTE=loop: the body of sr_sparse_search_masked group by group
  per_group_masked  the baseline - what a caller had before this entry point: one sr_sparse_search_masked per group over that group's
                    queries (their CSR gathered beforehand, outside the timed region), on whatever route each call picks
  unrestricted      sr_sparse_search of all queries, no filter
  masked            G = 1 only: sr_sparse_search_masked on the same mask, mask route forced - grouped_pass / masked is the price of the
                    per-query word

pass and loop must return equal counts, ids and score bits in every cell (asserted).  HIP events around each variant, median of --reps
(7) runs after a warm-up; two runs where the warm-up shows a variant at over --slow-ms.

--parent-lib PATH (a build of the parent commit: tools/build_variant.sh in a checkout of it) adds the comparison against the parent: the
unrestricted sr_sparse_search and the single-mask sr_sparse_search_masked (mask route forced, random 50 %) of BOTH libraries in this one
process, each library with its own index over the same device arrays, alternating call by call, and the parent against itself (two
indexes of the parent's library) for the spread of two identical runs.

No target: the file records what the hardware says.  The child process that measures runs under a time limit; if it fails or runs out of
time nothing more is started on the GPU and the file says so.  Reads nothing outside the repository.

  python tools/bench_grouped_sparse.py                       # full size, one MI355X
  python tools/bench_grouped_sparse.py --scale 0.02 --nq 300 --groups 1 8
  python tools/bench_grouped_sparse.py --merge a.json b.json      # the cells of several invocations (--groups 1 8 / --groups 100 ...) in one file
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MASKS = {"random_50pct": "random 50 % per group", "random_10pct": "random 10 % per group", "band_10pct": "one band of 10 % of the positions per group"}
CROSSOVER = 64 * 1000000             # SR_SUBSET_SPARSE_MASK_CROSSOVER (csrc/subset_search.hip): what the auto rule compares sum nq_g m_g with


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


def sub_csr(q_indptr, q_cols, q_vals, sel):
    """The CSR of the queries `sel` (int64 tensor) alone."""
    import torch
    lens = (q_indptr[1:] - q_indptr[:-1])[sel]
    ip = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=q_indptr.device)
    ip[1:] = torch.cumsum(lens, 0)
    take = torch.repeat_interleave(q_indptr[:-1][sel] - ip[:-1], lens) + torch.arange(int(ip[-1]), device=q_indptr.device)
    return ip, q_cols[take].contiguous(), q_vals[take].contiguous()


def same(a, b):
    import torch
    return bool(torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))


def route(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def cells(a, idx, N, dev, nq, group_counts, out):
    import torch
    from synth import build_queries
    qi, qc, qv = build_queries(a.vocab, nq, a.l0_q, dev, 4)
    for G in group_counts:
        groups = torch.arange(nq, device=dev) % G
        q_of = [sub_csr(qi, qc, qv, torch.arange(g, nq, G, device=dev)) for g in range(G)]     # the baseline's per-group batches
        for kind in a.masks:
            words, counts = group_words(kind, G, N, dev, 100 + G)
            pairs = sum(counts[g] * (int(q_of[g][0].numel()) - 1) for g in range(G))
            got = {}

            def grouped(r):
                route("SR_GROUPED_SPARSE_ROUTE", r)
                got[r] = idx.search_grouped(qi, qc, qv, a.k, words, groups)
                route("SR_GROUPED_SPARSE_ROUTE", None)

            def per_group():
                for g in range(G):
                    if q_of[g][0].numel() > 1:
                        idx.search(*q_of[g], a.k, mask=words[g])

            def masked():
                route("SR_SUBSET_SPARSE_ROUTE", "mask")
                got["masked"] = idx.search(qi, qc, qv, a.k, mask=words[0])
                route("SR_SUBSET_SPARSE_ROUTE", None)
            fns = {"grouped_pass": lambda: grouped("pass"), "grouped_loop": lambda: grouped("loop"), "per_group_masked": per_group,
                   "unrestricted": lambda: idx.search(qi, qc, qv, a.k)}
            if G == 1:
                fns["masked"] = masked
            before = idx.cert_stats()
            grouped("pass")
            torch.cuda.synchronize()
            after = idx.cert_stats()
            t = alternated(fns, a.reps, once_over_ms=a.slow_ms)
            assert same(got["pass"], got["loop"]), f"pass and loop differ at nq={nq} G={G} mask={kind}"
            cell = {"nq": nq, "G": G, "mask": MASKS[kind], "allowed_per_group_mean": round(sum(counts) / G, 1), "pairs": pairs,
                    "auto_route": "pass" if pairs >= CROSSOVER else "loop",
                    "one_pass_call": {"scorer_searches": after["searches"] - before["searches"], "queries": after["queries"] - before["queries"],
                                      "handed_back": after["redone_exact"] - before["redone_exact"]},
                    "pass_equals_loop_bit_for_bit": True, **t,
                    "ratios": {"grouped_pass_over_per_group_masked": round(t["grouped_pass"]["median_ms"] / t["per_group_masked"]["median_ms"], 4),
                               "grouped_loop_over_per_group_masked": round(t["grouped_loop"]["median_ms"] / t["per_group_masked"]["median_ms"], 4),
                               "grouped_pass_over_unrestricted": round(t["grouped_pass"]["median_ms"] / t["unrestricted"]["median_ms"], 4)}}
            if G == 1:
                assert same(got["pass"], got["masked"]), f"pass and the masked search differ at nq={nq} mask={kind}"
                cell["pass_equals_masked_bit_for_bit"] = True
                cell["ratios"]["grouped_pass_over_masked"] = round(t["grouped_pass"]["median_ms"] / t["masked"]["median_ms"], 4)
            print("[grouped sparse]", json.dumps(cell), file=sys.stderr, flush=True)
            print("CELL " + json.dumps(cell), flush=True)          # the parent process keeps the finished cells if this one is ended early
            out["cells"].append(cell)
            del words, got


def against_parent(a, arrays, N, dev):
    """The unrestricted and the single-mask search of this build and of the parent's, and the parent against itself."""
    import torch
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import SparseIndexHIP
    from synth import build_queries
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    for name, (res, args) in _lib.SIGNATURES.items():              # the parent lacks the entry this change adds
        fn = getattr(parent, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args

    def parent_index():
        keep, _lib._lib = _lib._lib, parent
        try:
            return SparseIndexHIP(*arrays, N, device=dev)
        finally:
            _lib._lib = keep
    idx = {"this": SparseIndexHIP(*arrays, N, device=dev), "parent": parent_index(), "parent_again": parent_index()}
    qi, qc, qv = build_queries(a.vocab, a.nq, a.l0_q, dev, 4)
    words, _ = group_words("random_50pct", 1, N, dev, 101)
    route("SR_SUBSET_SPARSE_ROUTE", "mask")
    fns = {}
    for name, ix in idx.items():
        fns[f"unrestricted_{name}"] = lambda ix=ix: ix.search(qi, qc, qv, a.k)
        fns[f"masked_{name}"] = lambda ix=ix: ix.search(qi, qc, qv, a.k, mask=words[0])
    t = alternated(fns, a.reps, once_over_ms=a.slow_ms)
    route("SR_SUBSET_SPARSE_ROUTE", None)
    for kind in ("unrestricted", "masked"):
        p = t[f"{kind}_parent"]["median_ms"]
        t[f"{kind}_this_over_parent"] = round(t[f"{kind}_this"]["median_ms"] / p, 4)
        t[f"{kind}_parent_again_over_parent"] = round(t[f"{kind}_parent_again"]["median_ms"] / p, 4)
    for ix in idx.values():
        ix.close()
    return t


def measure(a):
    import torch
    from scaling_retriever_amd.scoring import SparseIndexHIP
    from synth import build_index
    os.environ["SR_DEV_SWITCHES"] = "1"
    dev = torch.device("cuda", 0)
    N = max(8 * (a.k + 1024), int(a.n_docs * a.scale))
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    out = {"N": N, "vocab": a.vocab, "postings": int(doc_ids.numel()), "L0_d": a.l0_d, "L0_q": a.l0_q, "k": a.k, "cells": []}
    if a.parent_lib:
        out["against_parent"] = against_parent(a, (indptr, doc_ids, vals), N, dev)
        print("PARENT " + json.dumps(out["against_parent"]), flush=True)
    idx = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    out["certified_scorer"] = idx.cert_stats()["present"] == 1
    cells(a, idx, N, dev, a.nq, a.groups, out)
    cells(a, idx, N, dev, a.small_nq, a.small_groups, out)
    idx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8, 100, 1000])
    ap.add_argument("--small-nq", type=int, default=64)
    ap.add_argument("--small-groups", type=int, nargs="*", default=[8], help="group counts of the 64-query rows")
    ap.add_argument("--masks", nargs="+", default=list(MASKS), choices=list(MASKS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slow-ms", type=float, default=1000.0)
    ap.add_argument("--parent-lib", type=str, default=None, help="a build of the parent commit's library, for the comparison against it")
    ap.add_argument("--timeout", type=int, default=1080, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process and print the JSON")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "grouped_sparse_search.json"))
    ap.add_argument("--merge", nargs="+", default=None, help="files written by several invocations (a part of the cells each): one file of all")
    a = ap.parse_args()
    if a.merge:
        parts = [json.load(open(f)) for f in a.merge]
        res = parts[0]
        res["invocations"] = [{"argv_groups": sorted({c["G"] for c in p_["cells"]}), "seconds": p_.get("seconds")} for p_ in parts]
        for p_ in parts[1:]:
            res["cells"] += p_["cells"]
            if "against_parent" in p_:
                res["against_parent"] = p_["against_parent"]
        res.pop("seconds", None)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return 0
    if a.child:
        import torch
        torch.cuda.set_device(0)
        t0 = time.time()
        res = measure(a)
        res["seconds"] = round(time.time() - t0, 1)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        return 0
    res = {"what": "sparse top-k under per-query document filters (sr_sparse_search_grouped) against one sr_sparse_search_masked per group "
                   "(tools/bench_grouped_sparse.py)", "n_gpus": 1, "data": "synthetic", "scale": a.scale,
           "timing": f"HIP events around each variant, variants alternated in one process, median of {a.reps} runs after a warm-up (2 runs "
                     f"where a variant takes over {a.slow_ms:.0f} ms)",
           "baseline": "per_group_masked: one sr_sparse_search_masked per group over that group's queries, each call on the route it picks"}
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
    else:                                                # what was finished
        res["cells"] = [json.loads(ln[5:]) for ln in lines if ln.startswith("CELL ")]
        for ln in lines:
            if ln.startswith("PARENT "):
                res["against_parent"] = json.loads(ln[7:])
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
