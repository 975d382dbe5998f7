#!/usr/bin/env python3
"""Pseudo-relevance feedback, measured: sr_sparse_feedback and sr_dense_feedback - one workgroup per query - against the
per-step compositions a caller had before them (scaling_retriever_amd.prf.sparse_feedback_by_steps: per document rank one gather-add into
dense [rows, V] buffers, the formula in torch, sparse_reps_to_csr; dense_feedback_by_steps: per rank the stored rows added in torch), on
the synthetic indexes of BASELINE.json configs[2] (sparse: 8 841 823 documents x 128 256 terms, L0_d = 128, L0_q = 32) and configs[1]
(dense: 8 841 823 x 2048 rows, fp32 and fp16 storage), the feedback lists taken from an actual search.

Per shape (nq, n_pos, max_terms): the outputs of the two are compared for equal bytes first; then HIP events around each call, the
variants alternating inside every round, median of --reps rounds.  The composition is timed twice per round: the difference of the two
medians is the spread a comparison has to exceed.  Also: the one-off forward_rows() build, and whole search_prf calls against their two
searches alone.  Writes one JSON document (default profiles/prf_search.json) and prints it.

  python tools/bench_prf.py                               # full size, one MI355X
  python tools/bench_prf.py --scale 0.01 --shapes 1:3:32,64:10:128
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

SHAPES = "1:3:32,1:10:128,1:50:0,64:3:32,64:10:128,64:50:0,6980:3:32,6980:10:128,6980:50:0"


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


def compared(kernel, composition, reps, what):
    """The two variants of one shape: equal bytes first, then the alternating timing and the ratios."""
    got, want = kernel(), composition()
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert same_bytes(got, want), f"kernel and per-step composition differ: {what}; nothing was timed"
    ms = alternating({"kernel": kernel, "composition": composition, "composition_again": composition}, reps)
    kern, comp, comp2 = summary(ms["kernel"]), summary(ms["composition"]), summary(ms["composition_again"])
    spread = abs(comp["median_ms"] - comp2["median_ms"])
    return {"outputs_equal_bytes": True, "kernel": kern, "composition": comp, "composition_again": comp2,
            "composition_spread_ms": round(spread, 3),
            "kernel_speedup_over_composition": round(min(comp["median_ms"], comp2["median_ms"]) / kern["median_ms"], 2),
            "kernel_not_slower_beyond_the_spread": bool(kern["median_ms"] <= min(comp["median_ms"], comp2["median_ms"]) + spread)}


def sparse_legs(a, N, shapes, dev):
    from scaling_retriever_amd.prf import sparse_feedback_by_steps
    from scaling_retriever_amd.scoring import SparseIndexHIP, sparse_feedback
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
    out = {"n_docs": N, "vocab": a.vocab, "postings": int(indptr[-1]), "forward_rows_build_ms": builds,
           "forward_rows_bytes": int(sum(t.numel() * t.element_size() for t in fwd)), "legs": []}
    Q = build_queries(a.vocab, max(s[0] for s in shapes), a.l0_q, dev, 4)
    for nq, n_pos, max_terms in shapes:
        q = (Q[0][:nq + 1], Q[1][:nq * a.l0_q], Q[2][:nq * a.l0_q])
        kw = dict(n_pos=n_pos, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=max_terms)
        (_, fb, counts), _ = once(lambda: idx.search(*q, n_pos))
        leg = {"nq": nq, "n_pos": n_pos, "max_terms": max_terms}
        leg.update(compared(lambda: sparse_feedback(*q, *fwd, a.vocab, fb, counts, **kw),
                            lambda: sparse_feedback_by_steps(*q, *fwd, a.vocab, fb, counts, **kw), a.reps, f"sparse {leg}"))
        new = sparse_feedback(*q, *fwd, a.vocab, fb, counts, **kw)
        leg["expanded_terms_per_query"] = round(new[1].numel() / nq, 1)
        used = (fb >= 0) & (torch.arange(n_pos, device=dev)[None, :] < counts[:, None])
        rows = fb.clamp(min=0)
        leg["entries_per_query"] = round(a.l0_q + float(((fwd[0][rows + 1] - fwd[0][rows]) * used).sum()) / nq, 1)
        ms = alternating({"search_prf": lambda: idx.search_prf(*q, a.k, fb_depth=n_pos, **kw),
                          "two_searches": lambda: (idx.search(*q, n_pos), idx.search(*new, a.k))}, 3)
        leg["search_prf_whole"], leg["its_two_searches_alone"] = summary(ms["search_prf"]), summary(ms["two_searches"])
        out["legs"].append(leg)
        print("[sparse]", json.dumps(leg), file=sys.stderr, flush=True)
    idx.close()
    return out


def dense_legs(a, N, shapes, dev, dtype):
    from scaling_retriever_amd.prf import dense_feedback_by_steps
    from scaling_retriever_amd.scoring import DenseIndexHIP
    D = dense_rows("gauss", N, a.hidden, dev, 1)
    if dtype == "fp16":
        D = D.to(torch.float16)
    idx = DenseIndexHIP(a.hidden, device=dev, row_dtype=dtype)
    idx.add_device_rows(D)
    idx.set_precision("fp32_filtered")                     # what the retrieval drivers use; the same bits as the exact kernel
    Q = dense_queries("gauss", max(s[0] for s in shapes), a.hidden, dev, 2)
    legs = []
    for nq, n_pos in sorted({(s[0], s[1]) for s in shapes}):
        q = Q[:nq].contiguous()
        kw = dict(n_pos=n_pos, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0)
        (_, fb), _ = once(lambda: idx.search(q, n_pos))
        leg = {"nq": nq, "n_pos": n_pos}
        leg.update(compared(lambda: idx.feedback(q, fb, None, **kw), lambda: dense_feedback_by_steps(idx, q, fb, None, **kw), a.reps,
                            f"dense {dtype} {leg}"))
        moved = nq * n_pos * a.hidden * (2 if dtype == "fp16" else 4)
        leg["row_bytes_read"] = moved
        leg["rows_GBps"] = round(moved / (leg["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
        new = idx.feedback(q, fb, None, **kw)
        ms = alternating({"search_prf": lambda: idx.search_prf(q, a.k, fb_depth=n_pos, **kw),
                          "two_searches": lambda: (idx.search(q, n_pos), idx.search(new, a.k))}, 3)
        leg["search_prf_whole"], leg["its_two_searches_alone"] = summary(ms["search_prf"]), summary(ms["two_searches"])
        legs.append(leg)
        print(f"[dense {dtype}]", json.dumps(leg), file=sys.stderr, flush=True)
    idx.close()
    del D, idx
    torch.cuda.empty_cache()
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (both indexes)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--k", type=int, default=1000, help="depth of the second search of the whole search_prf calls")
    ap.add_argument("--shapes", type=str, default=SHAPES, help="nq:n_pos:max_terms, comma separated (the dense legs use nq:n_pos)")
    ap.add_argument("--heads", type=str, default="sparse,fp32,fp16", help="sparse and / or the dense row types")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "prf_search.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    N = max(4096, int(a.n_docs * a.scale))
    t0 = time.time()
    res = {"what": "Rocchio feedback on the device (sr_sparse_feedback, sr_dense_feedback) against the per-step compositions "
                   "(tools/bench_prf.py)",
           "device": torch.cuda.get_device_name(0), "n_gpus": 1, "n_docs": N, "data": "synthetic (Zipf index / gauss rows), feedback lists = "
           "the top n_pos of a search", "timing": f"HIP events around each call; variants alternate inside a round; median of {a.reps} rounds "
           "after 1 warm-up round; whole search_prf calls: median of 3", "sparse": None, "dense": {}}
    for head in a.heads.split(","):
        if head == "sparse":
            res["sparse"] = sparse_legs(a, N, shapes, dev)
            torch.cuda.empty_cache()
        else:
            res["dense"][head] = dense_legs(a, N, shapes, dev, head)
    every = (res["sparse"]["legs"] if res["sparse"] else []) + [leg for legs in res["dense"].values() for leg in legs]
    res["outputs_equal_bytes"] = all(leg["outputs_equal_bytes"] for leg in every)
    res["kernel_not_slower_at_any_shape"] = all(leg["kernel_not_slower_beyond_the_spread"] for leg in every)
    res["shapes_that_lose"] = [{k_: leg[k_] for k_ in ("nq", "n_pos", "max_terms") if k_ in leg} for leg in every
                               if not leg["kernel_not_slower_beyond_the_spread"]]
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
