#!/usr/bin/env python3
"""Hits inside the groups of a collapsed search (csrc/group_hits.hip + collapse.group_hits), measured (profiles/group_hits.json) on
the synthetic indexes of tools/bench_collapse.py: dense 8 841 823 x 2 048 fp32 rows (config 2, fp32_filtered), sparse V = 128 256,
Zipf(1.0), 128 postings per document (config 3); 6 980 and 64 queries, k = 1 000 groups, m = 3 hits per group.  Two key tables:
id // 8 (every group 8 consecutive documents) and random groups of mean size 8 with one planted group of 100 000 documents (a tenant).

Per head, key table and query count:
(a) the four steps on the slots the collapsed search returned, each on its own: sr_group_members_count, sr_group_members_fill, the
    head's score_pairs, sr_segment_topm (left out, and said so, where the pairs of the whole batch exceed --max-step-pairs: the driver
    then works in sub-batches);
(b) the whole search_collapsed(hits=3) call against the same call without hits;
(c) id // 8 only: the same hits computed in torch on the device - the members of every slot gathered into a padded [slots, 8] block,
    the same score_pairs, a stable descending sort (members are in id order, so ties keep the lower id first) - asserted identical to
    the driver's output before anything is timed.  The padded block of the planted table would be slots x 100 000: not built.

HIP events around each call, variants alternated in one process, median of --reps (7) runs after a warm-up (3 for the whole calls of
6 980 queries).  No target: the file records what the hardware says.  Reads nothing outside the repository.

  python tools/bench_group_hits.py                   # full size, one MI355X
  python tools/bench_group_hits.py --scale 0.02 --nq 300
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
from bench_collapse import alternated  # noqa: E402
from synth import build_index, build_queries, dense_queries, dense_rows  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


def torch_hits(score_pairs, slot_keys, members, m, threshold, pad):
    """The hits of every slot in torch ops on the device: padded member gather, score_pairs, stable sort."""
    uniq, mptr, mids = members
    nq, kg = slot_keys.shape
    dev = slot_keys.device
    g = torch.searchsorted(uniq, slot_keys.reshape(-1).clamp(min=0))
    g = g.clamp(max=uniq.numel() - 1)
    size = torch.where(slot_keys.reshape(-1) >= 0, mptr[g + 1] - mptr[g], torch.zeros_like(g))
    width = int(size.max())
    col = torch.arange(width, device=dev)[None, :]
    valid = col < size[:, None]
    ids = mids[(mptr[g][:, None] + col).clamp(max=mids.numel() - 1)]
    indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(size.view(nq, kg).sum(1), 0)
    scores = torch.full(ids.shape, float("-inf"), dtype=torch.float32, device=dev)
    scores[valid] = score_pairs(indptr, ids[valid])
    if threshold is not None:
        valid = valid & (scores > threshold)
        scores = scores.masked_fill(~valid, float("-inf"))
    s, at = torch.sort(scores, dim=1, descending=True, stable=True)
    keep = torch.gather(valid, 1, at)[:, :m]
    s, i = s[:, :m] + 0.0, torch.gather(ids, 1, at)[:, :m]
    return (torch.where(keep, s, torch.full_like(s, pad)).view(nq, kg, -1), torch.where(keep, i, torch.full_like(i, -1)).view(nq, kg, -1),
            valid.sum(1).to(torch.int32).view(nq, kg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (both indexes)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=128)
    ap.add_argument("--l0-q", type=int, default=32)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--planted", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-step-pairs", type=int, default=120_000_000, help="leg (a) materialises every pair of the batch: skipped beyond this")
    ap.add_argument("--heads", nargs="+", default=["dense", "sparse"])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "group_hits.json"))
    a = ap.parse_args()
    from scaling_retriever_amd.collapse import member_table
    from scaling_retriever_amd.scoring import (DenseIndexHIP, SparseIndexHIP, group_members_count, group_members_fill, segment_topm)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    k, m = a.k, a.m
    N = max(8 * (k + 1024), int(a.n_docs * a.scale))
    planted = min(a.planted, N // 4)
    gen = torch.Generator(device=dev).manual_seed(9)
    random_keys = torch.randint(0, max(1, N // 8), (N,), device=dev, generator=gen).to(torch.int32)
    random_keys[torch.randperm(N, device=dev, generator=gen)[:planted]] = N // 8
    key_tables = {"id_div_8": (torch.arange(N, device=dev) // 8).to(torch.int32), "random_mean_8_planted": random_keys}
    res = {"what": "hits inside the groups of a collapsed search: the four steps, the whole call with and without hits, and the same hits in "
                   "torch (tools/bench_group_hits.py)", "device": torch.cuda.get_device_name(0), "n_gpus": 1, "scale": a.scale,
           "data": "synthetic", "n_docs": N, "hidden": a.hidden, "vocab": a.vocab, "L0_d": a.l0_d, "L0_q": a.l0_q, "k": k, "m": m,
           "planted_group": planted,
           "timing": f"HIP events around each call, variants alternated in one process, median of {a.reps} runs after a warm-up run "
                     "(3 runs for the whole calls of more than 64 queries)",
           "not_measured": ["real group-size distributions (a chunked corpus)", "hits under filters at this size",
                            "several short segments packed into one wave (sr_segment_topm runs one wave per segment)",
                            "the torch route on the planted table (its padded block does not fit)", "m other than 3"]}
    def save():
        res["seconds"] = round(time.time() - t0, 1)
        text = json.dumps(res, indent=1)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        return text

    heads = {}
    if "dense" in a.heads:
        dense = DenseIndexHIP(a.hidden, device=dev)
        dense.add_device_rows(dense_rows("gauss", N, a.hidden, dev, 1))
        dense.set_precision("fp32_filtered")
        heads["dense"] = (dense, dense_queries("gauss", a.nq, a.hidden, dev, 2))
    if "sparse" in a.heads:
        indptr, doc_ids, vals, _ = build_index(a.vocab, N, a.l0_d, dev, 3)
        heads["sparse"] = (SparseIndexHIP(indptr, doc_ids, vals, N, device=dev), build_queries(a.vocab, a.nq, a.l0_q, dev, 4))

    for head_name, (head, queries) in heads.items():
        is_sparse = head_name == "sparse"
        threshold, pad = (0.0, 0.0) if is_sparse else (None, -FLT_MAX)
        res[head_name] = {}
        for table_name, keys in key_tables.items():
            members = member_table(keys)
            for n in sorted({min(64, a.nq), a.nq}, reverse=True):
                if is_sparse:
                    qp = queries[0][:n + 1].contiguous()
                    q = (qp, queries[1][:int(qp[-1])], queries[2][:int(qp[-1])])
                    collapsed = lambda **kw: head.search_collapsed(*q, k, keys, **kw)                       # noqa: E731
                    score_pairs = lambda ptr, ids: head.score_pairs(*q, ptr, ids)                           # noqa: E731
                else:
                    q = queries[:n].contiguous()
                    collapsed = lambda **kw: head.search_collapsed(q, k, keys, **kw)                        # noqa: E731
                    score_pairs = lambda ptr, ids: head.score_pairs(q, ptr, ids)                            # noqa: E731
                if not is_sparse:
                    head.set_batch_invariant(True)                # what the driver holds for the call: the steps are timed under it too
                found = collapsed(hits=m, members=members)
                slot_keys = found[2].contiguous()
                cell = {"nq": n, "mean_groups": round(float(found[3].float().mean()), 1), "mean_hits": round(found[4]["mean_hits"], 3)}
                seg_ptr, total = group_members_count(slot_keys, members)
                cell["pairs"] = int(total)
                cell["largest_slot"] = int((seg_ptr[1:] - seg_ptr[:-1]).max())
                if table_name == "id_div_8":
                    ref = torch_hits(score_pairs, slot_keys, members, m, threshold, pad)
                    same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                               for x, y in zip(found[5], ref))
                    assert same, ("the driver and the torch route differ", head_name, table_name, n)
                    cell["same_outputs_as_torch"] = same
                if total <= a.max_step_pairs:
                    cand_ptr = seg_ptr[::k].contiguous()
                    ids = group_members_fill(slot_keys, members, seg_ptr, total)
                    scores = score_pairs(cand_ptr, ids)
                    fns = {"count": lambda: group_members_count(slot_keys, members),
                           "fill": lambda: group_members_fill(slot_keys, members, seg_ptr, total),
                           "pair_score": lambda: score_pairs(cand_ptr, ids),
                           "select": lambda: segment_topm(scores, ids, seg_ptr, m, threshold=threshold, pad_score=pad)}
                    if table_name == "id_div_8":
                        fns["torch_hits"] = lambda: torch_hits(score_pairs, slot_keys, members, m, threshold, pad)
                    steps = alternated(fns, a.reps)
                    cell["steps"] = steps
                    cell["expand_plus_select_over_pair_score"] = round((steps["count"]["median_ms"] + steps["fill"]["median_ms"] +
                                                                        steps["select"]["median_ms"]) / steps["pair_score"]["median_ms"], 3)
                    # what the two new steps must move: the slot keys and offsets, the member ids out, ids and scores in, the hits out
                    cell["expand_select_min_bytes"] = int(slot_keys.numel() * (4 + 8 + 8 + m * 12 + 4) + total * (8 + 8 + 4))
                    del ids, scores
                else:
                    cell["steps"] = f"skipped: {int(total)} pairs exceed --max-step-pairs, the driver works in sub-batches"
                if not is_sparse:
                    head.set_batch_invariant(False)
                whole = alternated({"search_collapsed": lambda: collapsed(), "search_collapsed_hits": lambda: collapsed(hits=m, members=members),
                                    "search_collapsed_hits_table_per_call": lambda: collapsed(hits=m)}, a.reps if n <= 64 else 3)
                cell["whole_call"] = whole
                cell["hits_cost_ms"] = round(whole["search_collapsed_hits"]["median_ms"] - whole["search_collapsed"]["median_ms"], 3)
                res[head_name][f"{table_name}_nq_{n}"] = cell
                print(f"[{head_name} {table_name} nq={n}]", json.dumps(cell), file=sys.stderr, flush=True)
                del found, slot_keys, seg_ptr
                torch.cuda.empty_cache()
                save()                                            # cell by cell: a run that is cut short keeps what it measured
    print(save(), flush=True)


if __name__ == "__main__":
    main()
