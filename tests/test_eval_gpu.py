"""GPU: evaluation on the device (evaluation.py over csrc/eval_metrics.hip, RunResult.evaluate, the drivers' --device_eval, eval_compare.py).
Every comparison is for equal bits (uint64 views of the doubles) against the Python model of tests/eval_cases.py, and against
evaluation.evaluate_by_steps, the torch composition."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import eval_cases as C

pytestmark = pytest.mark.gpu
CUTS = (1, 3, 5, 10, 20, 100, 1000)


def _rows(case, cuts, depth):
    from scaling_retriever_amd.evaluation import QrelRows
    indptr, ids, grades, n_rel, idcg, log2 = C.qrel_tables(case["rows"], cuts, depth)
    return QrelRows(indptr, ids, grades, n_rel, idcg, log2, tuple(cuts), np.diff(indptr) > 0)


def _check(case, cuts=CUTS, tie="str", order="score", rr_depth=0, exclude=None, steps=True):
    """The device result and the torch composition equal the model: every per-query byte, the flags, the means, the count.  Returns
    the model's (out, flags, mean, n)."""
    from scaling_retriever_amd import evaluation as E
    nq, depth = case["ids"].shape
    tk = C.str_tie_keys(case["scores"], case["ids"]) if isinstance(tie, str) else tie
    tables = C.qrel_tables(case["rows"], cuts, depth)
    want = C.eval_ranked(case["scores"], case["ids"], case.get("counts"), tk, exclude, *tables, cuts,
                         order=C.ORDER_SCORE if order == "score" else C.ORDER_LIST, rr_depth=rr_depth)
    rows = _rows(case, cuts, depth)
    for fn in (E.evaluate_arrays, E.evaluate_by_steps) if steps else (E.evaluate_arrays,):
        got = fn(case["scores"], case["ids"], case.get("counts"), rows, None, order=order, rr_depth=rr_depth, exclude=exclude,
                 tie_key=False if tk is None else tk)
        torch.cuda.synchronize()
        out, flags = got.per_query.cpu().numpy(), got.flags.cpu().numpy()
        assert out.dtype == np.float64 and out.shape == (nq, 1 + 4 * len(cuts)) and flags.dtype == np.int32, fn.__name__
        assert np.array_equal(flags, want[1]), (fn.__name__, flags, want[1])
        bad = np.argwhere(C.bits64(out) != C.bits64(want[0]))
        assert bad.size == 0, (fn.__name__, bad[:5], out[tuple(bad[0])], want[0][tuple(bad[0])])
        assert np.array_equal(C.bits64(got.mean), C.bits64(want[2])), (fn.__name__, got.mean, want[2])
        assert got.n_evaluated == want[3]
    return want


# ---------------------------------------------------------------------------------------------------------------- shapes ---
# depth 2, 256, 512: the ranking's sort (256 threads) over a single pair, fewer pairs than threads, one pair per thread
@pytest.mark.parametrize("nq,depth", [(3, 1), (3, 3), (1, 64), (3, 65), (257, 37), (3, 1000), (3, 4096), (3, 2), (3, 256), (3, 512)])
def test_shapes_with_heavy_ties(nq, depth):
    case = C.tied_case(np.random.default_rng(depth * 1000 + nq), nq, depth, max(8, 2 * depth), max_judged=min(12, depth), neg_zero=True)
    out, flags, mean, n = _check(case)
    if nq == 257:
        assert 0 < n < nq and (flags & 2).any() and not (flags & 2).all()          # means with non-evaluated queries in between
    _check(case, rr_depth=10)
    _check(case, tie=None)                                      # tie_key NULL: equal scores keep their list order


def test_no_query_and_no_cut():
    from scaling_retriever_amd import evaluation as E
    empty = dict(scores=np.zeros((0, 5), np.float32), ids=np.zeros((0, 5), np.int64), counts=np.zeros(0, np.int32), rows=[])
    out, flags, mean, n = _check(empty)
    assert n == 0 and (mean == 0).all()
    case = C.tied_case(np.random.default_rng(2), 5, 20, 40)
    out = _check(case, cuts=())[0]
    assert out.shape == (5, 1)
    _check(case, cuts=tuple(range(1, 17)))                      # 16 cuts, the limit
    _check(case, cuts=(25, 4096, 100000))                       # beyond the hits, beyond depth
    with pytest.raises(ValueError, match="cuts"):
        E.Qrels({}, ["a"], cuts=tuple(range(1, 18)))


def test_empty_lists_and_judgement_rows():
    rng = np.random.default_rng(3)
    case = C.tied_case(rng, 8, 30, 60, ragged=False)
    case["counts"] = np.array([30, 0, 30, 30, 30, 30, 30, 12], np.int32)
    case["ids"][2] = -1                                         # a row that is all padding
    case["rows"][3] = ([], [])                                  # no judgement
    hits = [int(x) for x in case["ids"][4][:6]]
    case["rows"][4] = (sorted(hits), [0, -1, 0, -1, 0, 0])      # judged, nothing relevant: flag bit 1
    case["rows"][5] = (sorted(set(int(x) for x in case["ids"][5]) | set(range(1000, 1050))), None)
    case["rows"][5] = (case["rows"][5][0], [1 + (i % 3) for i in range(len(case["rows"][5][0]))])      # more relevant than ranks
    case["rows"][6] = ([int(case["ids"][6][7])], [2])           # a row of one
    case["rows"][7] = (list(range(5000, 5003)), [1, 2, 3])      # only documents the index does not hold
    out, flags, mean, n = _check(case, cuts=(1, 5, 10, 30, 100))
    assert flags[1] & 1 == 0 and flags[2] & 1 == 0 and flags[3] == 2 and flags[4] == 3 and flags[5] == 1
    assert (out[[1, 2, 3, 4]] == 0).all() and out[5, 0] == 1.0 and out[6, 0] > 0 and (out[7] == 0).all() and flags[7] == 1


def test_a_long_judgement_row_and_the_full_lds():
    """2 000 judged documents against a list at the cap, half of them in the list: the judged sort and the ranking sort both run at
    their largest size."""
    rng = np.random.default_rng(4)
    case = C.tied_case(rng, 2, 4096, 9000, ragged=False, decimals=2)
    inside = [int(x) for x in rng.permutation(case["ids"][0])[:1000]]
    row = sorted(set(inside) | set(int(x) for x in rng.choice(np.arange(9000, 12000), size=1000, replace=False)))
    case["rows"][0] = (row, [int(g) for g in rng.integers(-1, 4, size=len(row))])
    case["rows"][1] = (sorted(int(x) for x in case["ids"][1]), [1] * 4096)      # every hit is relevant
    out, flags, _, _ = _check(case, cuts=(10, 1000, 4096))
    assert out[1, 0] == 1.0 and out[1, 3] == 1.0 and out[1, 6] == 1.0


def test_ties_across_a_cut_and_signed_zero():
    ids = np.arange(24, dtype=np.int64).reshape(2, 12)
    scores = np.array([[3, 2, 2, 2, 2, 1, 1, 1, 0.0, -0.0, 0.0, -0.0], [0.0, -0.0, -0.0, 0.0, -1, -1, -1, -1, -2, -2, -2, -2]], np.float32)
    case = dict(scores=scores, ids=ids, counts=np.array([12, 12], np.int32), rows=[([4, 7, 9, 11], [1, 2, 1, 3]), ([13, 14, 22], [1, 1, 2])])
    with_keys = _check(case, cuts=(2, 3, 6, 9, 10))[0]          # str(): "9" > "11" > "10": the run at 0.0 straddles the cuts 9 and 10
    without = _check(case, cuts=(2, 3, 6, 9, 10), tie=None)[0]
    assert not np.array_equal(with_keys, without)
    rev = np.zeros((2, 12), np.int32)
    rev[:] = np.arange(12)[::-1]
    _check(case, cuts=(2, 3, 6, 9, 10), tie=rev)                # the caller's own keys
    big = np.full((2, 12), 65535, np.int32)
    big[0, 3] = 0
    _check(case, cuts=(2, 3), tie=big)


def test_exclude_list_order_and_rr_depth():
    rng = np.random.default_rng(6)
    case = C.tied_case(rng, 6, 40, 80)
    case["scores"] = rng.permutation(case["scores"].ravel()).reshape(6, 40)     # a non-monotone list
    _check(case, order="list")
    _check(case, order="list", rr_depth=10)
    _check(case, rr_depth=10)
    _check(case, rr_depth=39)
    _check(case, rr_depth=5000)
    # exclude: the first relevant hit of every query that has one (and -1, and an id the list does not hold)
    exclude = np.full(6, -1, np.int64)
    for q in range(6):
        rel = {d for d, g in zip(*case["rows"][q]) if g > 0}
        first = [int(d) for r, d in enumerate(case["ids"][q]) if r < case["counts"][q] and int(d) in rel]
        if first:
            exclude[q] = first[0]
    assert (exclude >= 0).sum() >= 3
    exclude[np.nonzero(exclude < 0)[0][:1]] = 10 ** 6
    base = _check(case, order="list")[0]
    out = _check(case, order="list", exclude=exclude)[0]
    assert not np.array_equal(base, out)
    _check(case, exclude=exclude, rr_depth=10)


def test_device_found_errors_name_their_place():
    from scaling_retriever_amd import evaluation as E
    case = C.tied_case(np.random.default_rng(8), 5, 16, 40, ragged=False)
    case["rows"][2] = ([3, 9, 9, 12], [1, 1, 2, 0])             # not strictly ascending
    with pytest.raises(ValueError, match="judged ids of query 2 are not strictly ascending"):
        E.evaluate_arrays(case["scores"], case["ids"], None, _rows(case, (5,), 16), None, tie_key=False)
    with pytest.raises(C.EvalError, match="query 2"):
        C.eval_ranked(case["scores"], case["ids"], None, None, None, *C.qrel_tables(case["rows"], (5,), 16), (5,))
    case = C.tied_case(np.random.default_rng(9), 5, 16, 40, ragged=False)
    tie = np.zeros((5, 16), np.int32)
    tie[3, 7], tie[4, 1] = 65536, -1
    with pytest.raises(ValueError, match=r"tie_key 65536 \(query 3, entry 7\) is outside"):
        E.evaluate_arrays(case["scores"], case["ids"], None, _rows(case, (5,), 16), None, tie_key=tie)
    with pytest.raises(C.EvalError, match=r"\(query 3, entry 7\)"):
        C.eval_ranked(case["scores"], case["ids"], None, tie, None, *C.qrel_tables(case["rows"], (5,), 16), (5,))
    case["ids"][1] = np.arange(100, 116)
    case["ids"][1, 11] = 104                                    # a judged document twice; an unjudged one twice is no error
    case["ids"][1, 13] = 102
    case["rows"][1] = ([104, 200], [1, 1])
    with pytest.raises(ValueError, match=r"judged id 104 \(query 1, entry 11\) occurs twice"):
        E.evaluate_arrays(case["scores"], case["ids"], None, _rows(case, (5,), 16), None, tie_key=False)
    with pytest.raises(C.EvalError, match=r"judged id 104 \(query 1, entry 11\)"):
        C.eval_ranked(case["scores"], case["ids"], None, None, None, *C.qrel_tables(case["rows"], (5,), 16), (5,))
    counts = np.full(5, 16, np.int32)
    counts[1] = 11                                              # the repeat is beyond the valid prefix: no error
    case["counts"] = counts
    _check(case, cuts=(5,), tie=None)                           # and the library is usable afterwards


# ---------------------------------------------------------------------------------------------------- randomization test ---
@pytest.mark.parametrize("n,n_perm,n_cols", [(0, 255, 8), (1, 257, 1), (63, 1, 1), (64, 255, 8), (65, 257, 8), (1000, 10000, 1), (130, 10000, 8)])
def test_randomization_counts(n, n_perm, n_cols):
    from scaling_retriever_amd import evaluation as E
    rng = np.random.default_rng(n + n_perm)
    diff = np.round(rng.standard_normal((n_cols, n)) * 0.3, 2) + 0.02       # rounded: |T_b| == |T_obs| happens beyond the identity
    seed = 2 ** 64 - 3 if n == 65 else n_perm
    t_obs, count = E.randomization_test(diff, n_perm=n_perm, seed=seed)
    want_t, want_c = C.randomization(diff, n_perm, seed)
    assert t_obs.dtype == np.float64 and count.dtype == np.int64
    assert np.array_equal(C.bits64(t_obs), C.bits64(want_t)) and np.array_equal(count, want_c), (count, want_c)
    if n == 0:
        assert (count == n_perm).all()


def test_randomization_zero_differences_seeds_and_many_columns():
    from scaling_retriever_amd import evaluation as E
    assert E.randomization_test(np.zeros((3, 70)), n_perm=257, seed=5)[1].tolist() == [257] * 3
    diff = np.random.default_rng(1).standard_normal((11, 200)) + 0.1      # 11 columns: two calls, the same signs
    a = E.randomization_test(diff, n_perm=3000, seed=1)
    b = E.randomization_test(diff, n_perm=3000, seed=1)
    c = E.randomization_test(diff, n_perm=3000, seed=2)
    assert np.array_equal(a[1], b[1]) and np.array_equal(C.bits64(a[0]), C.bits64(b[0])) and not np.array_equal(a[1], c[1])
    assert np.array_equal(a[1], C.randomization(diff, 3000, 1)[1])


# ------------------------------------------------------------------------------------------------- front ends and drivers ---
@pytest.fixture(scope="module")
def searched():
    """A real dense search whose index holds every row twice: equal scores under different document ids, in every list."""
    from scaling_retriever_amd.scoring import DenseIndexHIP
    from scaling_retriever_amd.utils.run_file import RunResult, to_host
    rng = np.random.default_rng(11)
    D = rng.standard_normal((1500, 64), dtype=np.float32)
    D = np.concatenate([D, D])
    Q = rng.standard_normal((40, 64), dtype=np.float32)
    idx = DenseIndexHIP(64)
    idx.add_host_rows(D)
    s, i = idx.search(torch.from_numpy(Q).cuda(), 100)
    doc_ids = [f"doc{(7 * j) % 3000}" for j in range(3000)]
    res = RunResult([f"q{j}" for j in range(40)], to_host(s), to_host(i), doc_ids)
    h_i = res.positions
    qrel = {}
    for q in range(38):                                         # two queries without judgements
        picks = rng.choice(100, size=6, replace=False)
        qrel[f"q{q}"] = {doc_ids[int(h_i[q, r])]: int(g) for r, g in zip(picks, rng.integers(0, 4, size=6))}
        qrel[f"q{q}"][f"unknown{q}"] = 2
    return res, qrel


def test_run_result_evaluate_equals_metrics_py(searched):
    from scaling_retriever_amd import evaluation as E
    from scaling_retriever_amd.utils import metrics as M
    res, qrel = searched
    assert (res.scores[:, 0] == res.scores[:, 1]).all()         # the ties are there
    run = res.to_dict()
    got = res.evaluate(qrel)
    assert got.n_evaluated == 38
    want = {"recip_rank": M.mrr_k(run, qrel, 10 ** 9), **M.evaluate(run, qrel, "recall"), **M.evaluate(run, qrel, "ndcg_cut")}
    assert {k: got.means[k] for k in want} == want
    assert res.evaluate(qrel, rr_depth=10).means["recip_rank"] == M.mrr_k(run, qrel, 10)
    steps = E.evaluate_by_steps(res.scores, res.positions, None, E.Qrels(qrel, res.docs), res.qids)
    assert np.array_equal(C.bits64(steps.per_query.cpu().numpy()), C.bits64(got.per_query.cpu().numpy())) and steps.means == got.means
    # compare: a run against itself with its two best hits swapped
    other = res.positions.copy()
    other[:, [0, 5]] = other[:, [5, 0]]
    from scaling_retriever_amd.utils.run_file import RunResult
    res_b = RunResult(res.qids, res.scores, other, res.docs).evaluate(qrel, order="list")
    cmp = E.compare(got, res_b, ["ndcg_cut_10", "recip_rank"], n_perm=2000, seed=3)
    a, b = got.per_query.cpu().numpy(), res_b.per_query.cpu().numpy()
    both = (got.flags.cpu().numpy() & res_b.flags.cpu().numpy() & 1) != 0
    cols = [got.columns.index("ndcg_cut_10"), 0]
    want_c = C.randomization((a[both][:, cols] - b[both][:, cols]).T, 2000, 3)[1]
    assert [cmp[m]["count_ge"] for m in ("ndcg_cut_10", "recip_rank")] == want_c.tolist()
    assert cmp["recip_rank"]["p"] == (int(want_c[1]) + 1) / 2001 and cmp["recip_rank"]["n"] == 38
    assert cmp["ndcg_cut_10"]["diff"] == got.means["ndcg_cut_10"] - res_b.means["ndcg_cut_10"]


def test_device_eval_tasks_write_the_python_tasks_perf_json(searched, tmp_path):
    import eval_compare
    import eval_dense
    from scaling_retriever_amd import evaluation as E
    from scaling_retriever_amd.utils import metrics as M
    res, qrel = searched
    run = res.to_dict()
    run["q5"] = {}                                              # a judged query without hits still counts in the dict code
    own = res.docs.key(int(res.positions[3, 0]))
    run[own] = run.pop("q3")                                    # BEIR: a query whose id is a document's, its best hit
    qrel = dict(qrel)
    qrel[own] = qrel.pop("q3")
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    for d in ("a", "b"):
        with open(tmp_path / d / "run.json", "w") as f:
            json.dump(run, f)
    with open(tmp_path / "qrel.json", "w") as f:
        json.dump(qrel, f)
    common = ["--eval_qrel_path", str(tmp_path / "qrel.json"), "--eval_metric", "['mrr_10', 'recall', 'ndcg_cut', 'recip_rank']"]
    for d, extra in (("a", []), ("b", ["--device_eval"])):
        eval_dense.main(["--task_name", "evaluate_msmarco", "--eval_run_path", str(tmp_path / d / "run.json"), "--out_dir", str(tmp_path / d)]
                        + common + extra)
    assert (tmp_path / "a" / "perf.json").read_bytes() == (tmp_path / "b" / "perf.json").read_bytes()
    # BEIR: every run query needs a relevant document
    beir_qrel = {q: docs for q, docs in qrel.items()}
    beir_run = {q: docs for q, docs in run.items() if q in qrel and any(g > 0 for g in qrel[q].values())}
    for d in ("a", "b"):
        with open(tmp_path / d / "run.json", "w") as f:
            json.dump(beir_run, f)
    want = M.evaluate_beir(argparse.Namespace(out_dir=str(tmp_path / "a")), beir_qrel)
    got = E.device_eval_beir(argparse.Namespace(out_dir=str(tmp_path / "b")), beir_qrel)
    assert got == want and (tmp_path / "a" / "perf.json").read_bytes() == (tmp_path / "b" / "perf.json").read_bytes()
    with open(tmp_path / "b" / "run.json", "w") as f:
        json.dump(dict(beir_run, stranger={"doc1": 1.0}), f)
    with pytest.raises(KeyError):
        E.device_eval_beir(argparse.Namespace(out_dir=str(tmp_path / "b")), beir_qrel)
    # eval_compare.py: the two files hold one run: every difference is 0, every permutation reaches it
    with open(tmp_path / "b" / "run.json", "w") as f:
        json.dump(run, f)
    with open(tmp_path / "a" / "run.json", "w") as f:
        json.dump(run, f)
    out = eval_compare.main(["--qrel_path", str(tmp_path / "qrel.json"), "--run_paths", f"{tmp_path}/a/run.json,{tmp_path}/b/run.json",
                             "--metrics", "ndcg_cut_10,recip_rank,map_cut_100", "--rr_depth", "10", "--permutations", "500", "--output_dir",
                             str(tmp_path / "cmp")])
    assert json.load(open(tmp_path / "cmp" / "compare.json")) == out
    assert out["metrics"]["recip_rank"]["mean_a"] == M.mrr_k({q: d for q, d in run.items() if d}, qrel, 10)
    assert all(v["count_ge"] == 500 and v["p"] == 1.0 and v["diff"] == 0.0 for v in out["metrics"].values())
