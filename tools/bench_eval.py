#!/usr/bin/env python3
"""Evaluation on the device, measured (evaluation.py over csrc/eval_metrics.hip).

  (a) the metrics of a run from its arrays: evaluation.evaluate_arrays (sr_eval_ranked) against evaluation.evaluate_by_steps (the same
      bytes from torch operations) and against utils/metrics.py on the same RunResult (mrr_k at 10, evaluate "recall" and "ndcg_cut":
      what the evaluate_msmarco task runs today), at 6 980 x 1 000 with about 1.1 relevant documents per query, 6 980 x 4 096,
      54 x 1 000 with about 200 judged documents per query, and 64 x 1 000.  Per-query bytes, flags and means of the two device
      routes are asserted identical, and the means equal to utils/metrics.py where that route runs, before anything is timed.
  (b) the paired randomization test: evaluation.randomization_test (sr_eval_randomization) against the chunked numpy model of
      tests/eval_cases.py at 6 980 and 54 queries x 100 000 permutations x 4 columns; counts asserted identical.
  (c) the whole evaluate_msmarco task (run.json and qrels from disk to perf.json) with and without --device_eval; perf.json bytes
      asserted identical.

Data: synthetic, integer document ids.  Scores are fp32 normal draws sorted descending (a few rows tie by chance at the large shapes:
the output says whether keys were built); one extra row rounds them to two decimals so that every list ties.  Device routes: HIP events around each
call, the routes alternated in one process, median of --reps runs after 2 warm-up runs; a call includes its one wait for the stream.
The Python routes run once, on the host clock.  Writes one JSON document (default profiles/eval_device.json) and prints it.

  python tools/bench_eval.py                     # full size, one MI355X
  python tools/bench_eval.py --nq 300 --perms 2000
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_hybrid import alternated  # noqa: E402


def make_run(nq, depth, judged, rel_share, dev, seed, decimals=None):
    """-> (scores fp32 [nq, depth] descending, ids int64 [nq, depth] distinct inside a row, n_docs, qrels dict): every query judges
    about `judged` documents, 70 % of them from its list, a share `rel_share` of them with a grade in 1 .. 3 (the others 0)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    stride = 97
    ids = torch.rand((nq, depth), device=dev, generator=g).argsort(1) * stride + torch.randint(0, stride, (nq, depth), device=dev, generator=g)
    scores = torch.randn((nq, depth), device=dev, generator=g)
    if decimals is not None:
        scores = torch.round(scores * 10 ** decimals) / 10 ** decimals
    scores = scores.sort(1, descending=True).values.contiguous()
    n_docs = depth * stride
    rng = np.random.default_rng(seed)
    h_ids = ids.cpu().numpy()
    qrel = {}
    for q in range(nq):
        m = max(1, int(rng.poisson(judged - 1)) + 1) if judged < 10 else int(judged)
        inside = rng.random(m) < 0.7
        docs = np.where(inside, h_ids[q, rng.integers(0, depth, size=m)], rng.integers(0, n_docs, size=m))
        grades = np.where(rng.random(m) < rel_share, rng.integers(1, 4, size=m), 0)
        qrel[str(q)] = {str(int(d)): int(gr) for d, gr in zip(docs, grades)}
    return scores, ids.contiguous(), n_docs, qrel


def python_route(res, qrel):
    """What the evaluate_msmarco task computes today, on the RunResult (its dicts are built on access)."""
    from scaling_retriever_amd.utils import metrics as M
    t = time.perf_counter()
    out = {"mrr_10": M.mrr_k(res, qrel, 10), **M.evaluate(res, qrel, "recall"), **M.evaluate(res, qrel, "ndcg_cut")}
    return out, time.perf_counter() - t


def bits(t):
    return t.contiguous().view(torch.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--perms", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--python-deep", action="store_true", help="run utils/metrics.py at depth 4 096 too (minutes)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "eval_device.json"))
    a = ap.parse_args()
    import eval_cases as C
    import eval_dense
    from scaling_retriever_amd import evaluation as E
    from scaling_retriever_amd.utils.run_file import RunResult, to_host
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    t0 = time.time()
    res = {"what": "evaluation on the device: sr_eval_ranked against the torch composition and utils/metrics.py, sr_eval_randomization against "
                   "the numpy model, the evaluate_msmarco task both ways (tools/bench_eval.py)", "device": torch.cuda.get_device_name(0),
           "n_gpus": 1, "data": "synthetic", "cuts": list(E.DEFAULT_CUTS),
           "timing": f"device routes: HIP events around each call (its one stream wait included), routes alternated, median of {a.reps} runs after "
                     "2 warm-up runs; Python routes: once, host clock"}

    # (a) the metrics
    res["metrics"] = []
    keep = None
    shapes = [("dev_1000", a.nq, 1000, 1.1, 1.0, None, True), ("dev_4096", a.nq, 4096, 1.1, 1.0, None, a.python_deep),
              ("judged_200", min(54, a.nq), 1000, 200, 0.3, None, True), ("small_64", min(64, a.nq), 1000, 1.1, 1.0, None, True),
              ("dev_1000_tied_scores", a.nq, 1000, 1.1, 1.0, 2, False)]
    for name, nq, depth, judged, rel_share, decimals, with_python in shapes:
        scores, ids, n_docs, qrel = make_run(nq, depth, judged, rel_share, dev, 10 + depth + nq, decimals)
        qids = [str(q) for q in range(nq)]
        t = time.perf_counter()
        Q = E.Qrels(qrel, np.arange(n_docs, dtype=np.int64))
        rows = Q.rows_for(qids)
        build_s = time.perf_counter() - t
        tie = E.tie_keys(scores, ids, ids >= 0, Q.docs)
        tie_arg = False if tie is None else tie
        hip = E.evaluate_arrays(scores, ids, None, Q, rows, tie_key=tie_arg)
        ref = E.evaluate_by_steps(scores, ids, None, Q, rows, tie_key=tie_arg)
        same = bool(torch.equal(bits(hip.per_query), bits(ref.per_query)) and torch.equal(hip.flags, ref.flags)
                    and np.array_equal(hip.mean.view(np.int64), ref.mean.view(np.int64)) and hip.n_evaluated == ref.n_evaluated)
        assert same, f"{name}: the kernel and the torch composition differ"
        fns = {"hip_kernels": lambda: E.evaluate_arrays(scores, ids, None, Q, rows, tie_key=tie_arg),
               "hip_front_end": lambda: E.evaluate_arrays(scores, ids, None, Q, rows),
               "torch_steps": lambda: E.evaluate_by_steps(scores, ids, None, Q, rows, tie_key=tie_arg)}
        t = alternated(fns, a.reps)
        row = {"shape": name, "nq": nq, "depth": depth, "judged_per_query": round(len(rows.ids) / nq, 2),
               "relevant_per_query": round(float(rows.n_rel.mean()), 2), "evaluated": hip.n_evaluated, "tie_keys_built": tie is not None,
               "qrels_to_arrays_s": round(build_s, 3), **t, "torch_over_hip": round(t["torch_steps"]["median_ms"] / t["hip_kernels"]["median_ms"], 2),
               "same_bytes": same, "note": "hip_kernels: the tie keys given (or known to be unneeded); hip_front_end: the call a user makes - "
                                           "it sorts the scores to look for ties and builds keys for the rows that have them (integer ids: on the device)"}
        if with_python:
            run = RunResult(qids, to_host(scores), to_host(ids), Q.docs)
            want, sec = python_route(run, qrel)
            rr10 = E.evaluate_arrays(scores, ids, None, Q, rows, rr_depth=10)
            got = {"mrr_10": rr10.means["recip_rank"], **{k: hip.means[k] for k in want if k != "mrr_10"}}
            assert got == want, f"{name}: the device means differ from utils/metrics.py"
            row.update(python_metrics_s=round(sec, 2), same_means_as_metrics_py=True,
                       python_over_hip_front_end=round(sec * 1e3 / (2 * t["hip_front_end"]["median_ms"]), 1),
                       python_note="utils/metrics.py: mrr_k(10) + evaluate recall + evaluate ndcg_cut on the RunResult; the device needs two "
                                   "calls for the same figures (rr_depth 10 and 0): the ratio counts both")
            if name == "dev_1000":
                keep = (run, qrel)
        else:
            row["python_metrics_s"] = None
        res["metrics"].append(row)
        print("[metrics]", json.dumps(row), file=sys.stderr, flush=True)
        del scores, ids, hip, ref, tie
        torch.cuda.empty_cache()

    # (b) the randomization test
    res["randomization"] = []
    for n in (a.nq, min(54, a.nq)):
        diff = np.round(np.random.default_rng(n).standard_normal((4, n)) * 0.2, 4) + 0.004
        d_diff = torch.from_numpy(diff).to(dev)
        t_obs, count = E.randomization_test(d_diff, a.perms, seed=1)
        t = time.perf_counter()
        want_t, want_c = C.randomization(diff, a.perms, 1, chunk=max(1, min(4096, (1 << 25) // max(1, n))))
        sec = time.perf_counter() - t
        same = bool(np.array_equal(count, want_c) and np.array_equal(t_obs.view(np.int64), want_t.view(np.int64)))
        assert same, f"randomization n = {n}: the kernel and the numpy model differ"
        tt = alternated({"hip": lambda: E.randomization_test(d_diff, a.perms, seed=1)}, a.reps)
        row = {"n": n, "permutations": a.perms, "columns": 4, "count_ge": count.tolist(), "p": [(int(c) + 1) / (a.perms + 1) for c in count],
               **tt, "numpy_model_s": round(sec, 2), "numpy_over_hip": round(sec * 1e3 / tt["hip"]["median_ms"], 1), "same_counts": same,
               "signed_adds_per_s": round(4.0 * n * a.perms / (tt["hip"]["median_ms"] * 1e-3), 0)}
        res["randomization"].append(row)
        print("[randomization]", json.dumps(row), file=sys.stderr, flush=True)

    # (c) the whole task, files to perf.json
    if keep is not None:
        run, qrel = keep
        with tempfile.TemporaryDirectory() as tmp:
            run.dump(os.path.join(tmp, "run.json"))
            with open(os.path.join(tmp, "qrel.json"), "w") as f:
                json.dump(qrel, f)
            secs = {}
            for name, extra in (("python", []), ("device_eval", ["--device_eval"])):
                args = eval_dense.parse_args(["--task_name", "evaluate_msmarco", "--eval_run_path", os.path.join(tmp, "run.json"), "--eval_qrel_path",
                                              os.path.join(tmp, "qrel.json"), "--eval_metric", "['mrr_10', 'recall', 'ndcg_cut']", "--out_dir",
                                              os.path.join(tmp, name)] + extra)
                t = time.perf_counter()
                eval_dense.evaluate_msmarco(args)
                secs[name] = round(time.perf_counter() - t, 2)
            same = open(os.path.join(tmp, "python", "perf.json"), "rb").read() == open(os.path.join(tmp, "device_eval", "perf.json"), "rb").read()
            assert same, "evaluate_msmarco: the two perf.json differ"
            res["evaluate_msmarco_task"] = {"nq": run.scores.shape[0], "depth": run.scores.shape[1], "run_json_bytes": os.path.getsize(os.path.join(tmp, "run.json")),
                                            "seconds": secs, "same_perf_json_bytes": same,
                                            "note": "both read run.json with json.load; --device_eval then turns the dict into arrays on the host "
                                                    "(load_run_arrays), which is most of its time"}
            print("[task]", json.dumps(res["evaluate_msmarco_task"]), file=sys.stderr, flush=True)
    res["not_measured"] = ["real runs and real qrels (synthetic lists and judgements)", "ties in real scores (one synthetic row rounds the scores)",
                           "utils/metrics.py at 6 980 x 4 096 unless --python-deep is given", "lists longer than sr_max_topk()"]
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
