#!/usr/bin/env python3
"""Compare two runs on MI355X: the metrics of both from their run.json files and a two-sided paired randomization test of every
difference, on the device (scaling_retriever_amd/evaluation.py).  It needs no model and no index - only the
judgements and the runs:

  python eval_compare.py --qrel_path Q.json --run_paths a/run.json,b/run.json --metrics ndcg_cut_10,recip_rank \
      [--rr_depth 10] [--permutations 100000] [--seed 0] --output_dir DIR

Writes DIR/compare.json: per metric the two means, their difference, the number of paired queries, count_ge (the permutations whose
|T| reached the observed one) and p = (count_ge + 1) / (permutations + 1).  Query order is that of the first run; a query the second
run lacks has an empty list there and is not paired.  --rr_depth 10 makes recip_rank MRR@10 (the list is cut to its 10 best first).
The reference has no counterpart.
"""
import argparse
import json
import os


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Metrics of two run.json files and a paired randomization test of their differences.")
    ap.add_argument("--qrel_path", type=str, required=True, help="judgements {qid: {doc id: grade}} as JSON")
    ap.add_argument("--run_paths", type=str, required=True, help="two comma-separated run.json files: a,b")
    ap.add_argument("--metrics", type=str, default="ndcg_cut_10,recip_rank", help="comma-separated trec-style keys (recip_rank, recall_100, ...)")
    ap.add_argument("--rr_depth", type=int, default=0, help="cut every list to this many entries before recip_rank (0: no cut)")
    ap.add_argument("--permutations", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--output_dir", type=str, required=True)
    args = ap.parse_args(argv)
    args.run_paths = [p for p in args.run_paths.split(",") if p]
    if len(args.run_paths) != 2:
        ap.error(f"--run_paths takes two files, got {len(args.run_paths)}")
    args.metrics = [m for m in args.metrics.split(",") if m]
    if not args.metrics:
        ap.error("--metrics names no metric")
    from scaling_retriever_amd.evaluation import DEFAULT_CUTS, column_names
    known = column_names(DEFAULT_CUTS)
    for m in args.metrics:
        if m not in known:
            ap.error(f"--metrics: unknown metric {m!r}; one of recip_rank and recall_K, ndcg_cut_K, r_cap_K, map_cut_K for K in {DEFAULT_CUTS}")
    if args.rr_depth < 0:
        ap.error("--rr_depth must be >= 0")
    if not 1 <= args.permutations < (1 << 31):
        ap.error("--permutations must be in [1, 2^31)")
    return args


def load_pair(args):
    """-> (Qrels, [(qids, scores, positions, counts)] of the two runs over one document table, the second aligned with the first's
    query order)."""
    from scaling_retriever_amd import evaluation as E
    with open(args.qrel_path) as f:
        qrel = json.load(f)
    runs = []
    for path in args.run_paths:
        with open(path) as f:
            runs.append(json.load(f))
    table = sorted({str(d) for run in runs for docs in run.values() for d in docs}) or ["-"]
    runs[1] = {q: runs[1].get(q, {}) for q in runs[0]}
    return E.Qrels(qrel, table), [E.load_run_arrays(run, table)[:4] for run in runs]


def compare_runs(args):
    from scaling_retriever_amd import evaluation as E
    qrels, arrays = load_pair(args)
    results = [E.evaluate_arrays(s, p, c, qrels, qids, rr_depth=args.rr_depth) for qids, s, p, c in arrays]
    out = E.compare(results[0], results[1], args.metrics, n_perm=args.permutations, seed=args.seed)
    out = {"runs": args.run_paths, "permutations": args.permutations, "seed": args.seed, "rr_depth": args.rr_depth,
           "evaluated": [r.n_evaluated for r in results], "metrics": out}
    os.makedirs(args.output_dir, exist_ok=True)
    with open(os.path.join(args.output_dir, "compare.json"), "w") as f:
        json.dump(out, f, indent=4)
    return out


def main(argv=None):
    return compare_runs(parse_args(argv))


if __name__ == "__main__":
    main()
