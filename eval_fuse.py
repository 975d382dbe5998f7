#!/usr/bin/env python3
"""Rank fusion driver on MI355X: fuses the ranked lists of two or more run.json files on the device (scoring.rank_fuse, DESIGN.md
4.24).  It needs no model and no index - only the runs:

  python eval_fuse.py --run_paths a/run.json,b/run.json[,...] --output_dir DIR [--method rrf|minmax] [--c 60] [--weights 1,1] [--topk 1000]

The reference has no counterpart (its HybridRetriever dumps the two heads' runs and fuses nothing).  Query order is that of the
first run; a query that is missing from a later run has an empty list there.  Every run's entries are ordered by (score descending,
document id ascending), the score as the float32 the kernel reads.  Documents are numbered in ascending order of their id -
numerically when every id is a decimal integer, else by the string - so a tie at equal fused score breaks by document id.  Up to 8
runs; a query's list longer than sr_max_topk(), or lists that together exceed 2 * sr_max_topk() entries per query, are a ValueError.
"""
import argparse
import json
import os
import re

import numpy as np

METHODS = ("rrf", "minmax")
_DECIMAL = re.compile(r"-?[0-9]+\Z")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Fuse run.json files by rank (RRF) or by min-max normalised score on the device.")
    ap.add_argument("--run_paths", type=str, required=True, help="comma-separated run.json files; list l of the fusion is run l")
    ap.add_argument("--output_dir", type=str, required=True)
    ap.add_argument("--method", type=str, default="rrf", choices=METHODS)
    ap.add_argument("--c", type=float, default=60.0, help="rrf: the constant of w / (c + rank)")
    ap.add_argument("--weights", type=str, default=None, help="one weight per run, comma-separated (default: all 1)")
    ap.add_argument("--topk", type=int, default=1000, help="documents kept per query")
    args = ap.parse_args(argv)
    args.run_paths = [p for p in args.run_paths.split(",") if p]
    if not args.run_paths:
        ap.error("--run_paths names no file")
    if args.weights is None:
        args.weights = (1.0,) * len(args.run_paths)
    else:
        try:
            args.weights = tuple(float(x) for x in args.weights.split(","))
        except ValueError:
            ap.error("--weights takes numbers: one per run, comma-separated")
        if len(args.weights) != len(args.run_paths):
            ap.error(f"--weights takes one number per run ({len(args.run_paths)}), got {len(args.weights)}")
    if args.topk < 1:
        ap.error("--topk must be >= 1")
    return args


def number_documents(runs):
    """Every document id of the runs, once, in ascending order: numerically when every id is a decimal integer, else by the string.
    Returns (table: the ids in that order, number: id -> its place)."""
    docs = set()
    for run in runs:
        for hits in run.values():
            docs.update(hits)
    if all(_DECIMAL.match(d) for d in docs):
        table = sorted(docs, key=lambda d: (int(d), d))
    else:
        table = sorted(docs)
    return table, {d: i for i, d in enumerate(table)}


def build_lists(runs, number):
    """(qids of the first run in its order, ids int64 [L, nq, depth] padded with -1, scores fp32, counts int32 [L, nq]): every query's
    list of every run by (score descending, document number ascending)."""
    qids = list(runs[0])
    ordered = []
    for run in runs:
        rows = []
        for q in qids:
            hits = [(np.float32(s), number[d]) for d, s in run.get(q, {}).items()]
            rows.append(sorted(hits, key=lambda h: (-h[0], h[1])))
        ordered.append(rows)
    depth = max([1] + [len(row) for rows in ordered for row in rows])
    L, nq = len(runs), len(qids)
    ids = np.full((L, nq, depth), -1, np.int64)
    scores = np.zeros((L, nq, depth), np.float32)
    counts = np.zeros((L, nq), np.int32)
    for l, rows in enumerate(ordered):
        for q, row in enumerate(rows):
            counts[l, q] = len(row)
            if row:
                scores[l, q, :len(row)] = [h[0] for h in row]
                ids[l, q, :len(row)] = [h[1] for h in row]
    return qids, ids, scores, counts


def max_topk():
    from scaling_retriever_amd import _lib
    return int(_lib.load().sr_max_topk())


def check_limits(ids, counts, topk, limit):
    L, _, depth = ids.shape
    longest = int(counts.max(initial=0))
    if longest > limit:
        l, q = np.unravel_index(int(counts.argmax()), counts.shape)
        raise ValueError(f"eval_fuse: run {l} holds {longest} documents for query row {q}, at most sr_max_topk() = {limit} are fused")
    if L * depth > 2 * limit:
        raise ValueError(f"eval_fuse: {L} runs of up to {depth} documents per query are {L * depth} entries, at most {2 * limit} are fused")
    if topk > limit:
        raise ValueError(f"eval_fuse: --topk {topk}, at most sr_max_topk() = {limit} are returned")


def fuse_on_device(ids, counts, scores, k, method, weights, c):
    """numpy in, numpy out: the one library call of this driver."""
    import torch
    from scaling_retriever_amd import scoring
    from scaling_retriever_amd.utils.run_file import to_host
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    s, i, n = scoring.rank_fuse(torch.from_numpy(ids).to(dev), k, counts=torch.from_numpy(counts).to(dev),
                                scores=torch.from_numpy(scores).to(dev), method=method, weights=weights, c=c)
    return to_host(s), to_host(i), to_host(n)


def fuse(args):
    from scaling_retriever_amd import scoring
    from scaling_retriever_amd.utils.run_file import RunResult
    scoring.rank_fuse_arguments(len(args.run_paths), args.topk, args.method, args.weights, args.c)
    runs = []
    for path in args.run_paths:
        with open(path) as f:
            runs.append(json.load(f))
    table, number = number_documents(runs)
    qids, ids, scores, counts = build_lists(runs, number)
    check_limits(ids, counts, args.topk, max_topk())
    out_s, out_i, out_n = fuse_on_device(ids, counts, scores, args.topk, args.method, args.weights, args.c)
    res = RunResult(qids, out_s, out_i, table if table else ["-"], out_n)
    os.makedirs(args.output_dir, exist_ok=True)
    res.dump(os.path.join(args.output_dir, "run.json"))
    return res


def main(argv=None):
    return fuse(parse_args(argv))


if __name__ == "__main__":
    main()
