#!/usr/bin/env python3
"""Range search and exact hybrid search under a document bitmap, measured (profiles/masked_range.json), on the synthetic full-size
indexes of tools/bench_range.py / tools/bench_hybrid.py: dense 8 841 823 x 2 048 fp32 rows (config 2), sparse V = 128 256, Zipf(1.0),
128 postings per document, 32 query terms (config 3).  Three legs, each in a child process of its own under its own time limit; a
leg that fails or runs out of time ends the run (nothing more is started on the GPU), and the file says which legs ran.

  dense   64 and 6 980 queries, thresholds at each query's 100th best ALLOWED score; the count pass and the fill pass under
          (a) no mask - the existing entry points, run twice (a, a2) so that the file holds the spread between two identical runs,
          (b) every bit set, (c) random 50 %, (d) random 1 %, (e) one contiguous band of 10 % of the ids.
  sparse  the same five variants at the config-3 shape.
  hybrid  whole hybrid.search_fused calls for 64 queries under (a), (c) and (e), and one call with the range route forced on 8 queries
          (depths = (k,)) under (c), as tools/bench_hybrid.py does unmasked.

HIP events around each call, the variants alternated in one process, median of --reps (7) runs after a warm-up; where one call takes
over a second (the dense passes at 6 980 queries) two runs.  What to read: b / a per pass next to a2 / a (the price of the bit test
against the noise of two identical runs), e / a (whether the tile skip pays: the share of non-empty tiles is about 0.1), and c / a, d / a
(expected at about 1: under a uniformly random filter every 256-row tile, and every 8 192-document tile, holds an allowed document).

  python tools/bench_masked_range.py                      # full size, one MI355X
  python tools/bench_masked_range.py --scale 0.02 --nqs 64 300
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

VARIANTS = ("a", "a2", "b", "c", "d", "e")
WHAT = {"a": "no mask (existing entry points)", "a2": "no mask, again", "b": "every bit set", "c": "random 50 %", "d": "random 1 %",
        "e": "one band of 10 % of the ids"}


def alternated(fns, reps, warmup=1, once_over_ms=1000.0):
    """{name: stats} of the given callables, run in turn (a, b, ..., a, b, ...) between two events each; when the warm-up round shows a
    call of over once_over_ms, two timed rounds instead of `reps`."""
    import torch
    ms = {n: [] for n in fns}
    r, rounds = 0, warmup + reps
    while r < rounds:
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t = a.elapsed_time(b)
            if r >= warmup:
                ms[n].append(t)
            elif t > once_over_ms:
                rounds = warmup + min(reps, 2)
        r += 1
    return {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs": len(v)}
            for n, v in ms.items()}


def make_masks(n, dev, seed):
    """variant -> bool tensor [n] on the device (None: no mask)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(n, device=dev, generator=g)
    band = torch.zeros(n, dtype=torch.bool, device=dev)
    band[n // 2:n // 2 + n // 10] = True
    return {"a": None, "a2": None, "b": torch.ones(n, dtype=torch.bool, device=dev), "c": u < 0.5, "d": u < 0.01, "e": band}


def tile_share(m, tile):
    """Share of the `tile`-document tiles of a bool mask that hold a set bit."""
    import torch
    n = m.numel()
    padded = torch.zeros((n + tile - 1) // tile * tile, dtype=torch.bool, device=m.device)
    padded[:n] = m
    return round(float(padded.view(-1, tile).any(1).float().mean()), 4)


def ratios(per_variant, key):
    base = per_variant["a"][key]["median_ms"]
    return {f"{v}_over_a": round(per_variant[v][key]["median_ms"] / base, 4) for v in VARIANTS if v != "a"}


def leg_dense(a):
    import torch
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import DenseIndexHIP, _ptr, pack_doc_mask
    from synth import dense_queries, dense_rows
    dev = torch.device("cuda", 0)
    N, H = max(4096, int(a.n_docs * a.scale)), a.hidden
    idx = DenseIndexHIP(H, device=dev)
    idx.add_device_rows(dense_rows("gauss", N, H, dev, 1))
    lib, h = idx.lib, idx._h
    masks = make_masks(N, dev, 11)
    words = {v: (None if m is None else pack_doc_mask(m)) for v, m in masks.items()}
    tiles = {v: (1.0 if m is None else tile_share(m, 256)) for v, m in masks.items()}
    out = {"N": N, "H": H, "rows": "fp32", "row_bytes_per_pass": N * H * 4, "share_of_256_row_tiles_with_an_allowed_row": tiles, "batches": []}
    for nq in a.nqs:
        Q = dense_queries("gauss", nq, H, dev, 2).contiguous()
        st = {}
        deep = min(N, max(a.rank, int(lib.sr_max_topk())))
        idx.set_batch_invariant(True)                         # the tiled k order: what the range search computes
        top_s, top_i = idx.search(Q, deep)
        idx.set_batch_invariant(False)
        for v in VARIANTS:
            # the rank-th best ALLOWED score: read off the unrestricted list where it holds that many allowed documents for every query,
            # else from a masked search (pair-score bits for every nq)
            m, thr = masks[v], None
            if m is None:
                thr = top_s[:, a.rank - 1]
            else:
                seen = m[top_i].cumsum(1)
                if bool((seen[:, -1] >= a.rank).all()):
                    thr = top_s.gather(1, (seen >= a.rank).int().argmax(1, keepdim=True))[:, 0]
                else:
                    thr = idx.search(Q, a.rank, mask=words[v])[0][:, a.rank - 1]
            st[v] = {"thr": thr.contiguous(), "lims": torch.empty(nq + 1, dtype=torch.int64, device=dev), "total": ctypes.c_int64(0)}
        del top_s, top_i, seen

        def count(v):
            s, w = st[v], words[v]
            if w is None:
                _lib.check(lib.sr_dense_range_count(h, _ptr(Q), nq, _ptr(s["thr"]), _ptr(s["lims"]), ctypes.byref(s["total"]), _lib.stream_ptr()))
            else:
                _lib.check(lib.sr_dense_range_count_masked(h, _ptr(Q), nq, _ptr(s["thr"]), _ptr(w), N, _ptr(s["lims"]), ctypes.byref(s["total"]),
                                                           _lib.stream_ptr()))

        def fill(v):                                          # the handle holds one count: each fill is timed behind its own
            s, w = st[v], words[v]
            if w is None:
                _lib.check(lib.sr_dense_range_fill(h, _ptr(Q), nq, _ptr(s["thr"]), _ptr(s["lims"]), _ptr(s["scores"]), _ptr(s["ids"]),
                                                   s["total"].value, _lib.stream_ptr()))
            else:
                _lib.check(lib.sr_dense_range_fill_masked(h, _ptr(Q), nq, _ptr(s["thr"]), _ptr(w), N, _ptr(s["lims"]), _ptr(s["scores"]),
                                                          _ptr(s["ids"]), s["total"].value, _lib.stream_ptr()))
        t_count = alternated({v: (lambda v=v: count(v)) for v in VARIANTS}, a.reps)
        for v in VARIANTS:
            n = st[v]["total"].value
            st[v]["scores"] = torch.empty(max(1, n), dtype=torch.float32, device=dev)
            st[v]["ids"] = torch.empty(max(1, n), dtype=torch.int64, device=dev)
        # count + fill together per variant (a fill needs ITS count on the handle); the fill's time is the pair's minus the count's
        t_pair = alternated({v: (lambda v=v: (count(v), fill(v))) for v in VARIANTS}, a.reps)
        per = {}
        for v in VARIANTS:
            s = st[v]
            ok = bool((s["scores"][:s["total"].value] > torch.repeat_interleave(s["thr"], s["lims"][1:] - s["lims"][:-1])).all())
            if masks[v] is not None:
                ok = ok and bool(masks[v][s["ids"][:s["total"].value]].all())
            fill_ms = {k: round(t_pair[v][k] - t_count[v][k], 3) for k in ("median_ms",)}
            per[v] = {"mask": WHAT[v], "total_hits": s["total"].value, "every_hit_is_allowed_and_above_its_threshold": ok,
                      "count": t_count[v], "count_plus_fill": t_pair[v], "fill": fill_ms}
        row = {"nq": nq, "rank": a.rank, "variants": per, "count_ratios": ratios(per, "count"), "fill_ratios": ratios(per, "fill")}
        print("[dense]", json.dumps(row), file=sys.stderr, flush=True)
        out["batches"].append(row)
        del st, Q
    idx.close()
    return out


def leg_sparse(a):
    import torch
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import SparseIndexHIP, _ptr, pack_doc_mask
    from synth import build_index, build_queries
    dev = torch.device("cuda", 0)
    N = max(8192, int(a.n_docs * a.scale))
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    idx = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    lib, h = idx.lib, idx._h
    masks = make_masks(N, dev, 12)
    words = {v: (None if m is None else pack_doc_mask(m)) for v, m in masks.items()}
    tiles = {v: (1.0 if m is None else tile_share(m, 8192)) for v, m in masks.items()}
    out = {"N": N, "V": a.vocab, "L0_d": a.l0_d, "L0_q": a.l0_q, "share_of_8192_document_tiles_with_an_allowed_document": tiles, "batches": []}
    for nq in a.nqs:
        qp, qc, qv = build_queries(a.vocab, nq, a.l0_q, dev, 4)
        qp, qc, qv = qp.to(torch.int64).contiguous(), qc.to(torch.int32).contiguous(), qv.to(torch.float32).contiguous()
        st = {}
        for v in VARIANTS:
            ss, _, sc = idx.search(qp, qc, qv, a.rank, threshold=0.0, mask=masks[v])
            thr = torch.where(sc == a.rank, ss[:, a.rank - 1], torch.zeros_like(ss[:, 0])).contiguous()
            st[v] = {"thr": thr, "lims": torch.empty(nq + 1, dtype=torch.int64, device=dev), "total": ctypes.c_int64(0)}

        def count(v):
            s, w = st[v], words[v]
            if w is None:
                _lib.check(lib.sr_sparse_range_count(h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(s["thr"]), _ptr(s["lims"]), ctypes.byref(s["total"]),
                                                     _lib.stream_ptr()))
            else:
                _lib.check(lib.sr_sparse_range_count_masked(h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(s["thr"]), _ptr(w), N, _ptr(s["lims"]),
                                                            ctypes.byref(s["total"]), _lib.stream_ptr()))

        def fill(v):
            s, w = st[v], words[v]
            if w is None:
                _lib.check(lib.sr_sparse_range_fill(h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(s["thr"]), _ptr(s["lims"]), 0, 1, _ptr(s["scores"]),
                                                    _ptr(s["ids"]), s["total"].value, _lib.stream_ptr()))
            else:
                _lib.check(lib.sr_sparse_range_fill_masked(h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(s["thr"]), _ptr(w), N, _ptr(s["lims"]), 0, 1,
                                                           _ptr(s["scores"]), _ptr(s["ids"]), s["total"].value, _lib.stream_ptr()))
        t_count = alternated({v: (lambda v=v: count(v)) for v in VARIANTS}, a.reps)
        for v in VARIANTS:
            n = st[v]["total"].value
            st[v]["scores"] = torch.empty(max(1, n), dtype=torch.float32, device=dev)
            st[v]["ids"] = torch.empty(max(1, n), dtype=torch.int64, device=dev)
        t_pair = alternated({v: (lambda v=v: (count(v), fill(v))) for v in VARIANTS}, a.reps)
        per = {}
        for v in VARIANTS:
            s = st[v]
            ok = bool((s["scores"][:s["total"].value] > torch.repeat_interleave(s["thr"], s["lims"][1:] - s["lims"][:-1])).all())
            if masks[v] is not None:
                ok = ok and bool(masks[v][s["ids"][:s["total"].value]].all())
            per[v] = {"mask": WHAT[v], "total_hits": s["total"].value, "every_hit_is_allowed_and_above_its_threshold": ok,
                      "count": t_count[v], "count_plus_fill": t_pair[v],
                      "fill": {"median_ms": round(t_pair[v]["median_ms"] - t_count[v]["median_ms"], 3)}}
        row = {"nq": nq, "rank": a.rank, "variants": per, "count_ratios": ratios(per, "count"), "fill_ratios": ratios(per, "fill")}
        print("[sparse]", json.dumps(row), file=sys.stderr, flush=True)
        out["batches"].append(row)
    idx.close()
    return out


def leg_hybrid(a):
    import numpy as np
    import torch
    from scaling_retriever_amd import hybrid
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP, pack_doc_mask
    from synth import build_index, build_queries, dense_queries, dense_rows
    dev = torch.device("cuda", 0)
    k, w, nq = a.k, (1.0, 1.0), 64
    N = max(8 * (k + 1024), int(a.n_docs * a.scale))
    dense = DenseIndexHIP(a.hidden, device=dev)
    dense.add_device_rows(dense_rows("gauss", N, a.hidden, dev, 1))
    dense.set_precision("fp32_filtered")
    Q = dense_queries("gauss", nq, a.hidden, dev, 2)
    indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
    sparse = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
    qp, qc, qv = build_queries(a.vocab, nq, a.l0_q, dev, 4)
    s2d = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    d2s = torch.empty_like(s2d)
    d2s[s2d] = torch.arange(N, device=dev)
    masks = make_masks(N, dev, 13)
    words = {v: (None if masks[v] is None else pack_doc_mask(masks[v])) for v in ("a", "c", "e")}
    got = {}

    def call(v, n, depths):
        p = qp[:n + 1].contiguous()
        got[v] = hybrid.search_fused(dense, sparse, d2s, s2d, Q[:n], p, qc[:int(p[-1])], qv[:int(p[-1])], k, weights=w, depths=depths, mask=words[v])
    t = alternated({v: (lambda v=v: call(v, nq, None)) for v in ("a", "c", "e")}, a.reps)
    out = {"N": N, "k": k, "weights": list(w), "search_fused_64_queries": {}}
    for v in ("a", "c", "e"):
        stats = got[v][3]
        routes = {("range" if d < 0 else f"depth_{stats['depths'][d]}"): int((stats["depth"] == d).sum()) for d in np.unique(stats["depth"])}
        allowed_ok = True if masks[v] is None else bool(masks[v][torch.from_numpy(got[v][1][got[v][1] >= 0]).to(dev)].all())
        out["search_fused_64_queries"][v] = {"mask": WHAT[v], **t[v], "queries_per_route": routes, "every_returned_document_is_allowed": allowed_ok,
                                             "mean_candidates_ranked": round(float(stats["union"].mean()), 1)}
    base = t["a"]["median_ms"]
    out["search_fused_64_queries"]["ratios"] = {f"{v}_over_a": round(t[v]["median_ms"] / base, 4) for v in ("c", "e")}
    print("[hybrid]", json.dumps(out["search_fused_64_queries"]), file=sys.stderr, flush=True)
    n = min(a.range_nq, nq)
    if n > 0:
        tr = alternated({v: (lambda v=v: call(v, n, (k,))) for v in ("a", "c")}, 3)
        out["range_route"] = {}
        for v in ("a", "c"):
            stats = got[v][3]
            on = stats["depth"] < 0
            out["range_route"][v] = {"mask": WHAT[v], "nq": n, "depths": [k], **tr[v], "queries_on_the_range_route": int(on.sum()),
                                     "mean_range_hits": round(float(stats["range_hits"][on].mean()), 1) if on.any() else 0.0}
        print("[hybrid range]", json.dumps(out["range_route"]), file=sys.stderr, flush=True)
    return out


LEGS = {"dense": leg_dense, "sparse": leg_sparse, "hybrid": leg_hybrid}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (every index)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--nqs", type=int, nargs="+", default=[64, 6980])
    ap.add_argument("--rank", type=int, default=100, help="thresholds: each query's rank-th best allowed score")
    ap.add_argument("--k", type=int, default=1000, help="topk of the hybrid leg")
    ap.add_argument("--range-nq", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--leg-timeout", type=int, default=540, help="seconds a leg's child process may take")
    ap.add_argument("--leg", choices=list(LEGS), help="(internal) run this leg in this process and print its JSON")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "masked_range.json"))
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
    res = {}
    if os.path.exists(a.out):                       # legs measured by an earlier run are kept: a leg can be run on its own
        with open(a.out) as f:
            res = json.load(f)
    res.update({"what": "range search and exact hybrid search under a document bitmap against the unrestricted entry points "
                        "(tools/bench_masked_range.py)", "n_gpus": 1, "data": "synthetic", "scale": a.scale,
                "timing": f"HIP events around each call, variants alternated in one process, median of {a.reps} runs after a warm-up "
                          "(2 runs where a call takes over a second); one child process per leg"})
    res.setdefault("legs_not_run", {})
    passed = [x for x in sys.argv[1:]]
    rc = 0
    for leg in a.legs:
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
