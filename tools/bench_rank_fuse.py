#!/usr/bin/env python3
"""Rank fusion on the device, measured (scoring.rank_fuse over csrc/rank_fuse.hip).

  (a) sr_rank_fuse against the same fusion written in torch on the device - torch.unique over row * span + id, one scatter_add per
      list in list order, then rerank.rank_candidates (three stable sorts) - for both methods at 6 980 queries x (2 x 1000, k = 1000),
      (2 x 4096, k = 1000 and 4096), (4 x 1000, k = 1000) and 64 queries x (2 x 1000).  Ids, counts and score bits of the two routes are
      asserted identical before anything is timed.
  (b) sr_rank_fuse against sr_hybrid_union + sr_hybrid_rank (the weighted-sum route's two kernels, pair scorers not counted) on the same
      2 x 1000 lists.
  (c) the device work of a whole retrieve_rank_fused call (both searches, then fusion.fuse_hybrid_lists) against that of retrieve (both
      searches), k = 1000.

Lists: with --lists search (default) the two-list shapes are the top-4096 lists of real searches of the synthetic indexes tools/bench_hybrid.py
builds (BASELINE.json configs[1] / configs[2] shapes; independent Gaussian / Zipf scores: the two heads agree on next to nothing, so
nearly every entry is a document of its own - the most runs a shape can have); if the indexes do not fit, and for the four-list shape
always, random lists in which about 30 % of every later list's entries also stand in list 0.  The output names what each shape used.

HIP events around each call, the routes alternated in one process, median of --reps runs after 2 warm-up runs.  Writes one JSON document
(default profiles/rank_fuse.json) and prints it.

  python tools/bench_rank_fuse.py                    # full size, one MI355X
  python tools/bench_rank_fuse.py --scale 0.02 --nq 300
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_hybrid import alternated  # noqa: E402
from synth import build_index, build_queries, dense_queries, dense_rows  # noqa: E402


def random_lists(L, nq, depth, overlap, dev, seed):
    """ids int64 [L, nq, depth] without a repeat inside a row: every list draws from a pool of its own, then `overlap` of the slots of
    every list l >= 1 take entries of list 0 of the same query.  scores fp32: standard normal, each row descending."""
    g = torch.Generator(device=dev).manual_seed(seed)
    M, stride = L * depth, 1000
    perm = torch.rand((nq, M), device=dev, generator=g).argsort(1)
    ids = perm * stride + torch.randint(0, stride, (nq, M), device=dev, generator=g)
    ids = ids.view(nq, L, depth).permute(1, 0, 2).contiguous()
    n_shared = int(round(overlap * depth))
    for l in range(1, L):
        src = torch.rand((nq, depth), device=dev, generator=g).argsort(1)[:, :n_shared]
        dst = torch.rand((nq, depth), device=dev, generator=g).argsort(1)[:, :n_shared]
        ids[l].scatter_(1, dst, ids[0].gather(1, src))
    scores = torch.randn((L, nq, depth), device=dev, generator=g).sort(2, descending=True).values.contiguous()
    return ids, scores


def torch_fuse(ids, counts, scores, method, weights, c, k):
    """The same fusion in torch on the device -> (scores fp32 [kept], ids int64 [kept], counts int64 [nq]), rows in rank order."""
    from scaling_retriever_amd.rerank import rank_candidates
    L, nq, depth = ids.shape
    dev = ids.device
    valid = ids >= 0
    if counts is not None:
        valid = valid & (torch.arange(depth, device=dev)[None, None, :] < counts[:, :, None])
    span = int(ids.max()) + 1
    row = torch.arange(nq, device=dev)[None, :, None].expand_as(ids)
    uniq, inverse = torch.unique((row * span + ids)[valid], return_inverse=True)         # sorted: by query, then id; list-major input
    fused = torch.zeros(uniq.numel(), dtype=torch.float32, device=dev)
    at = 0
    for l in range(L):
        v = valid[l]
        n = int(v.sum())
        if method == "rrf":
            # the per-rank table in numpy float32 (one rounded add, one correctly rounded division), gathered on the device
            table = (np.float32(weights[l]) / (np.float32(c) + np.arange(1, depth + 1, dtype=np.float32))).astype(np.float32)
            contrib = torch.from_numpy(table).to(dev)[None, :].expand(nq, depth)[v]
        else:
            s = scores[l]
            mn = torch.where(v, s, torch.full_like(s, float("inf"))).amin(1, keepdim=True)
            mx = torch.where(v, s, torch.full_like(s, float("-inf"))).amax(1, keepdim=True)
            rng = mx - mn
            norm = torch.where(rng > 0, (s - mn) / rng, torch.ones_like(s))
            contrib = (norm * torch.tensor(float(weights[l]), dtype=torch.float32, device=dev))[v]
        fused.scatter_add_(0, inverse[at:at + n], contrib)                               # a document stands once in a list: one add per list
        at += n
    indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(torch.div(uniq, span, rounding_mode="floor"), minlength=nq), 0)
    doc = uniq % span
    order, kept = rank_candidates(fused, doc, indptr, k)
    return fused[order], doc[order], kept


def same_result(hip, ref, k):
    s, i, n = hip
    valid = torch.arange(k, device=s.device)[None, :] < n[:, None]
    return bool(torch.equal(n.to(torch.int64), ref[2]) and torch.equal(i[valid], ref[1])
                and torch.equal(s[valid].view(torch.int32), ref[0].view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (both indexes)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lists", type=str, default="search", choices=("search", "random"))
    ap.add_argument("--overlap", type=float, default=0.3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "rank_fuse.json"))
    a = ap.parse_args()
    from scaling_retriever_amd import fusion
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP, hybrid_rank, hybrid_union, rank_fuse
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    nq, deep = a.nq, 4096
    res = {"what": "rank fusion: sr_rank_fuse against the same fusion in torch, against sr_hybrid_union + sr_hybrid_rank, and inside a whole "
                   "retrieval (tools/bench_rank_fuse.py)", "device": torch.cuda.get_device_name(0), "n_gpus": 1, "data": "synthetic",
           "weights": "rrf: all 1, c = 60; minmax: 0.3, 1.7 (, 0.9, 1.1)",
           "timing": f"HIP events around each call, routes alternated in one process, median of {a.reps} runs after 2 warm-up runs"}

    # the lists of the two-list shapes
    searched = None
    if a.lists == "search":
        try:
            N = max(8 * (deep + 1024), int(a.n_docs * a.scale))
            dense = DenseIndexHIP(a.hidden, device=dev)
            dense.add_device_rows(dense_rows("gauss", N, a.hidden, dev, 1))
            dense.set_precision("fp32_filtered")
            Q = dense_queries("gauss", nq, a.hidden, dev, 2)
            indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
            q_indptr, q_cols, q_vals = build_queries(a.vocab, nq, a.l0_q, dev, 4)
            sparse = SparseIndexHIP(indptr, doc_ids, vals, N, device=dev)
            s2d = torch.randperm(N, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
            d2s = torch.empty_like(s2d)
            d2s[s2d] = torch.arange(N, device=dev)
            ds, dp = dense.search(Q, deep)
            ss, sp, sc = sparse.search(q_indptr, q_cols, q_vals, deep, threshold=0.0)
            searched = dict(ids=torch.stack([fusion.dense_to_tie(dp, d2s, N), fusion.sparse_to_tie(sp, sc, s2d)]),
                            scores=torch.stack([ds, ss]), counts=torch.stack([torch.full_like(sc, deep), sc]).to(torch.int32))
            res.update(scale=a.scale, n_docs=N, hidden=a.hidden, vocab=a.vocab, L0_d=a.l0_d, L0_q=a.l0_q)
        except (MemoryError, torch.cuda.OutOfMemoryError) as e:
            res["lists_fallback"] = f"the synthetic indexes did not fit ({type(e).__name__}): random lists everywhere"
            searched = None
            torch.cuda.empty_cache()

    def lists_of(L, n, depth):
        if searched is not None and L == 2:
            cut = lambda t: t[:, :n, :depth].contiguous()     # noqa: E731  (the top-depth list is the prefix of the top-4096 list)
            return cut(searched["ids"]), cut(searched["scores"]), torch.clamp(searched["counts"][:, :n], max=depth).contiguous(), "search"
        ids, scores = random_lists(L, n, depth, a.overlap, dev, 100 + L * depth)
        return ids, scores, None, f"random, {a.overlap:.0%} of a later list's entries also in list 0"

    # (a) the kernel against the torch route
    res["rank_fuse"] = []
    shapes = [(2, nq, 1000, 1000), (2, nq, deep, 1000), (2, nq, deep, deep), (4, nq, 1000, 1000), (2, min(64, nq), 1000, 1000)]
    for L, n, depth, k in shapes:
        ids, scores, counts, source = lists_of(L, n, depth)
        for method, w in (("rrf", (1.0,) * L), ("minmax", (0.3, 1.7, 0.9, 1.1)[:L])):
            sc_arg = scores if method == "minmax" else None
            hip = rank_fuse(ids, k, counts=counts, scores=sc_arg, method=method, weights=w)
            ref = torch_fuse(ids, counts, scores, method, w, 60.0, k)
            same = same_result(hip, ref, k)
            assert same, f"{L} x {depth}, k = {k}, {method}: the kernel and the torch route differ"
            t = alternated({"hip": lambda: rank_fuse(ids, k, counts=counts, scores=sc_arg, method=method, weights=w),
                            "torch": lambda: torch_fuse(ids, counts, scores, method, w, 60.0, k)}, a.reps)
            P = 1 << max(1, (L * depth - 1).bit_length())
            row = {"lists": L, "nq": n, "depth": depth, "k": k, "method": method, "source": source,
                   "mean_distinct_documents": round(float(torch.unique((torch.arange(n, device=dev)[None, :, None] * (int(ids.max()) + 1)
                                                                        + ids)[ids >= 0]).numel()) / n, 1),
                   "sort_slots": P, "lds_bytes": 16 * P, "hip": t["hip"], "torch": t["torch"],
                   "torch_over_hip": round(t["torch"]["median_ms"] / t["hip"]["median_ms"], 2), "same_ids_counts_score_bits": same}
            res["rank_fuse"].append(row)
            print("[rank_fuse]", json.dumps(row), file=sys.stderr, flush=True)
        del ids, scores, counts
        torch.cuda.empty_cache()

    # (b) against the two kernels of the weighted-sum route on the same 2 x 1000 lists, and (c) inside a whole retrieval
    if searched is not None:
        k = 1000
        dp_k, sp_k, sc_k = dp[:, :k].contiguous(), sp[:, :k].contiguous(), torch.clamp(sc, max=k)
        ip, dpos, spos, tie = hybrid_union(dp_k, sp_k, sc_k, s2d, d2s)
        dense_s = dense.score_pairs(Q, ip, dpos)
        sparse_s = sparse.score_pairs(q_indptr, q_cols, q_vals, ip, torch.clamp(spos, min=0))
        D, S = ds[:, k - 1].contiguous(), torch.where(sc_k == k, ss[:, k - 1], torch.zeros_like(ss[:, 0]))
        complete = torch.zeros(nq, dtype=torch.bool, device=dev)
        ids, scores, counts, _ = lists_of(2, nq, k)
        t = alternated({"rank_fuse_rrf": lambda: rank_fuse(ids, k, counts=counts),
                        "rank_fuse_minmax": lambda: rank_fuse(ids, k, counts=counts, scores=scores, method="minmax"),
                        "hybrid_union": lambda: hybrid_union(dp_k, sp_k, sc_k, s2d, d2s),
                        "hybrid_rank": lambda: hybrid_rank(ip, dpos, spos, tie, dense_s, sparse_s, (1.0, 1.0), k, D, S, complete, int(s2d.numel()),
                                                           dense.id_end)}, a.reps)
        two = t["hybrid_union"]["median_ms"] + t["hybrid_rank"]["median_ms"]
        res["against_union_plus_rank"] = {"nq": nq, "lists": "2 x 1000 (search)", **t, "union_plus_rank_ms": round(two, 3),
                                          "rank_fuse_rrf_over_union_plus_rank": round(t["rank_fuse_rrf"]["median_ms"] / two, 2),
                                          "note": "the weighted-sum route also runs both pair scorers over the union between its two kernels; "
                                                  "they are in neither figure"}
        print("[against_union_plus_rank]", json.dumps(res["against_union_plus_rank"]), file=sys.stderr, flush=True)
        del ip, dpos, spos, tie, dense_s, sparse_s

        def searches():
            d = dense.search(Q, k)
            s = sparse.search(q_indptr, q_cols, q_vals, k, threshold=0.0)
            return d, s

        def searches_and_fusion():
            (d_s, d_p), (s_s, s_p, s_c) = searches()
            return fusion.fuse_hybrid_lists(d_p, s_p, s_c, d2s, s2d, k, dense_scores=d_s, sparse_scores=s_s)
        t = alternated({"retrieve": searches, "retrieve_rank_fused": searches_and_fusion}, max(3, a.reps // 2), warmup=1)
        res["whole_call"] = {"nq": nq, "k": k, "what": "device work only: both searches, and both searches plus fusion.fuse_hybrid_lists (RRF); "
                                                      "query encoding and the run files are common to both and not in either figure", **t,
                             "fusion_share": round(1.0 - t["retrieve"]["median_ms"] / t["retrieve_rank_fused"]["median_ms"], 4)}
        print("[whole_call]", json.dumps(res["whole_call"]), file=sys.stderr, flush=True)
    res["not_measured"] = ["the overlap of real Lion runs (the synthetic heads agree on next to nothing)", "more than 4 lists at size",
                           "what RRF does to MRR / nDCG against the weighted sum (no checkpoint or qrels offline)"]
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
