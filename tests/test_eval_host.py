"""CPU: the model of sr_eval_ranked / sr_eval_randomization (tests/eval_cases.py) equals utils/metrics.py EXACTLY (== on floats) on runs
with heavy ties; the judgement tables of evaluation.Qrels equal the model's; run files load into the arrays truncate_run would rank; both
entry points and the drivers reject bad arguments before any device work."""
import ctypes
import json
import math

import numpy as np
import pytest

import eval_cases as C
from scaling_retriever_amd.utils import metrics as M

CUTS = (1, 3, 5, 10, 20, 100)


def model_of(case, cuts=CUTS, tie="str", rr_depth=0, order=C.ORDER_SCORE, exclude=None):
    nq, depth = case["ids"].shape
    tables = C.qrel_tables(case["rows"], cuts, depth)
    tk = C.str_tie_keys(case["scores"], case["ids"]) if tie == "str" else None
    return C.eval_ranked(case["scores"], case["ids"], case["counts"], tk, exclude, *tables, cuts, order=order, rr_depth=rr_depth)


@pytest.fixture(scope="module")
def tied():
    case = C.tied_case(np.random.default_rng(7), 40, 37, 90)
    return case, C.run_dict(case), C.qrel_dict(case)


def per_query(out, flags, col):
    return {f"q{q}": float(out[q, col]) for q in range(len(flags)) if flags[q] & 1}


def test_model_equals_metrics_py_on_heavy_ties(tied):
    case, run, qrel = tied
    ties = sum(int(a == b) for q in range(40) for a, b in zip(case["scores"][q, :case["counts"][q]], case["scores"][q, 1:case["counts"][q]]))
    assert ties > 100                                           # scores rounded to one decimal: the tie rule decides most ranks
    out, flags, mean, n = model_of(case)
    nc = len(CUTS)
    assert n == len([q for q in run if q in qrel]) and 0 < n < 40
    for j, k in enumerate(CUTS):
        assert per_query(out, flags, 1 + j) == M.recall_k(run, qrel, k, agg=False)
        assert per_query(out, flags, 1 + nc + j) == M.ndcg_k(run, qrel, k, agg=False)
        assert mean[1 + j] == M.recall_k(run, qrel, k) and mean[1 + nc + j] == M.ndcg_k(run, qrel, k)
    assert per_query(out, flags, 0) == {q: v["recip_rank"] for q, v in M.mrr_k(run, qrel, 10 ** 9, agg=False).items()}
    assert mean[0] == M.mrr_k(run, qrel, 10 ** 9)
    out10, flags10, mean10, _ = model_of(case, rr_depth=10)
    assert per_query(out10, flags10, 0) == {q: v["recip_rank"] for q, v in M.mrr_k(run, qrel, 10, agg=False).items()}
    assert mean10[0] == M.mrr_k(run, qrel, 10) and mean10[0] != mean[0]
    assert np.array_equal(C.bits64(out10[:, 1:]), C.bits64(out[:, 1:]))     # the cut touches recip_rank alone
    # the tie rule matters on these inputs: without the document-id keys some value differs
    plain = model_of(case, tie=None)[0]
    assert not np.array_equal(plain, out)


def test_r_cap_equals_recall_cap_k_under_its_own_tie_rule(tied):
    """recall_cap_k ranks by score alone with a stable sort: equal scores keep the run's order - the kernel's order without tie keys.  It
    counts every query of the run and divides by zero without a relevant document, so the run is cut to the queries it accepts."""
    case, run, qrel = tied
    out, flags, _, _ = model_of(case, tie=None)
    ok = [q for q in run if q in qrel and any(g > 0 for g in qrel[q].values())]
    sub = {q: run[q] for q in ok}
    nc = len(CUTS)
    for j, k in enumerate(CUTS):
        want = M.recall_cap_k(sub, qrel, k, agg=False)
        assert {q: float(out[int(q[1:]), 1 + 2 * nc + j]) for q in ok} == want
        s = 0.0
        for q in ok:
            s = s + float(out[int(q[1:]), 1 + 2 * nc + j])
        assert s / len(ok) == M.recall_cap_k(sub, qrel, k)
    with pytest.raises(KeyError):
        M.recall_cap_k({"nope": {"1": 1.0}}, qrel, 10)


def test_recip_rank_cuts_before_it_orders():
    """Twelve hits; entries 8 .. 11 tie, and the relevant document is entry 10 with the largest id string: ordering first puts it at rank
    9, inside a cut at 10; mrr_k cuts the list to its first 10 entries first and never sees it."""
    ids = np.array([[20, 21, 22, 23, 24, 25, 26, 27, 30, 31, 99, 32]], np.int64)
    scores = np.array([[9, 8, 7, 6, 5, 4, 3, 2, .5, .5, .5, .5]], np.float32)
    case = dict(ids=ids, scores=scores, counts=np.array([12], np.int32), rows=[([99], [1])])
    run, qrel = C.run_dict(case), C.qrel_dict(case)
    cut_first = model_of(case, rr_depth=10)[0][0, 0]
    order_first = model_of(case)[0][0, 0]
    assert cut_first == M.mrr_k(run, qrel, 10) == 0.0
    assert order_first == M.mrr_k(run, qrel, 10 ** 9) == 1.0 / 9        # rank 9 <= 10: cutting after ordering would report it


def test_list_order_exclude_and_map():
    ids = np.array([[5, 3, 9, 7, -1, 2]], np.int64)
    scores = np.array([[1, 5, 2, 4, 9, 3]], np.float32)         # not monotone: list order is not score order
    case = dict(ids=ids, scores=scores, counts=np.array([6], np.int32), rows=[([2, 3, 7, 50], [2, 1, 3, 1])])
    cuts = (2, 4, 10)
    as_list = model_of(case, cuts, tie=None, order=C.ORDER_LIST)[0][0]
    by_score = model_of(case, cuts, tie=None)[0][0]
    # list order: 5 3 9 7 2 -> relevant at ranks 2, 4, 5; score order: 3 7 2 9 5 -> ranks 1, 2, 3
    assert as_list[0] == 0.5 and by_score[0] == 1.0
    assert as_list[1:4].tolist() == [0.25, 0.5, 0.75] and by_score[1:4].tolist() == [0.5, 0.75, 0.75]
    assert as_list[10:].tolist() == [(1 / 2) / 4, (1 / 2 + 2 / 4) / 4, (1 / 2 + 2 / 4 + 3 / 5) / 4]
    assert by_score[7:10].tolist() == [1.0, 0.75, 0.75]         # r_cap: 2 / min(4, 2), 3 / min(4, 4), 3 / min(4, 10)
    dcg = 1 / math.log2(2) + 3 / math.log2(3) + 2 / math.log2(4)
    idcg = 3 / math.log2(2) + 2 / math.log2(3) + 1 / math.log2(4) + 1 / math.log2(5)
    assert by_score[6] == dcg / idcg
    without = model_of(case, cuts, tie=None, exclude=np.array([3], np.int64))[0][0]
    assert without[0] == 1.0 and without[1:4].tolist() == [0.5, 0.5, 0.5]      # the relevant hit 3 is dropped: 7 2 9 5


# ------------------------------------------------------------------------------------------------------------ Qrels, run files ---
def test_qrels_tables():
    from scaling_retriever_amd.evaluation import Qrels
    table = ["d0", "d1", "d2", "d3", "d4"]
    qrel = {"a": {"d3": 2, "zz": 1, "d0": 0, "d1": -1}, "b": {}, "c": {"yy": 3, "zz": 1, "d4": 3, "d2": 1}, "d": {"d1": 0}}
    Q = Qrels(qrel, table, cuts=(1, 2, 3, 10))
    assert Q.unknown == {"zz": 5, "yy": 6}                      # numbered from len(table) up, one number per document
    rows = Q.rows_for(["c", "nope", "a", "b", "d"])
    want = C.qrel_tables([([2, 4, 5, 6], [1, 3, 1, 3]), ([], []), ([0, 1, 3, 5], [0, -1, 2, 1]), ([], []), ([1], [0])], (1, 2, 3, 10), 4096)
    for got, w in zip((rows.indptr, rows.ids, rows.grades, rows.n_rel, rows.idcg, rows.log2), want):
        assert got.dtype == w.dtype and np.array_equal(got, w), (got, w)
    assert rows.present.tolist() == [True, False, True, True, True] and rows.n_rel.tolist() == [4, 0, 2, 0, 0]
    assert rows.idcg[0].tolist() == [3.0, 3.0 + 3 / math.log2(3), 3.0 + 3 / math.log2(3) + 1 / 2, 3.0 + 3 / math.log2(3) + 1 / 2 + 1 / math.log2(5)]
    assert Q.rows_for([]).indptr.tolist() == [0]
    for bad in [(0, 5), (5, 5), (10, 5), tuple(range(1, 18))]:
        with pytest.raises(ValueError, match="cuts"):
            Qrels(qrel, table, cuts=bad)


def test_load_run_arrays_orders_an_unsorted_file(tmp_path):
    from scaling_retriever_amd.evaluation import load_run_arrays
    run = {"q1": {"b": 0.5, "a": 2.0, "c": 0.5, "d": 1.25}, "q2": {}, "q3": {"d": -1.0, "a": -1.0}}
    path = tmp_path / "run.json"
    path.write_text(json.dumps(run))
    qids, scores, pos, counts, table = load_run_arrays(str(path))
    assert qids == ["q1", "q2", "q3"] and counts.tolist() == [4, 0, 2] and scores.dtype == np.float32 and pos.dtype == np.int64
    keys = table.keys_of(np.arange(table.n))
    assert keys == ["a", "b", "c", "d"]
    assert [keys[p] for p in pos[0]] == ["a", "d", "b", "c"] and scores[0].tolist() == [2.0, 1.25, 0.5, 0.5]     # stable: b before c
    assert [keys[p] for p in pos[2, :2]] == ["d", "a"] and (pos[1] == -1).all() and (pos[2, 2:] == -1).all()
    want = M.truncate_run(run, 4)
    assert [list(want[q]) for q in run] == [[keys[p] for p in pos[i, :counts[i]]] for i, q in enumerate(run)]
    with pytest.raises(KeyError):
        load_run_arrays(run, doc_table=["a", "b", "c"])
    with pytest.raises(ValueError, match="4097"):
        load_run_arrays({"q": {str(i): float(i) for i in range(4097)}})


def test_tie_keys_of_integer_and_string_tables_agree():
    """evaluation.tie_keys ranks str(doc id) among tied documents: with integer ids by an integer key (tensor code, here on the CPU),
    with any other table by sorting the strings.  Both equal the model's keys; "10" < "9", "1" < "10" < "100" < "11"."""
    import torch
    from scaling_retriever_amd.evaluation import tie_keys
    rng = np.random.default_rng(5)
    doc_ids = np.array([0, 1, 10, 100, 11, 9, 99, 100000, 19, 2, 20, 200, 12345678901234567, 5, 50, 55], np.int64)
    ids = np.stack([rng.permutation(16) for _ in range(6)]).astype(np.int64)
    scores = np.round(rng.standard_normal((6, 16)), 0).astype(np.float32)
    scores[0] = np.arange(16)                                   # a row without ties
    scores[1, :4] = [0.0, -0.0, 0.0, -0.0]
    ids[2, 3] = -1
    valid = torch.from_numpy(ids >= 0)
    want = C.str_tie_keys(scores, ids, doc_key=lambda p: str(int(doc_ids[p])))
    by_int = tie_keys(torch.from_numpy(scores), torch.from_numpy(ids), valid, doc_ids)
    by_str = tie_keys(torch.from_numpy(scores), torch.from_numpy(ids), valid, [str(int(d)) for d in doc_ids])
    assert by_int.dtype == torch.int32 and np.array_equal(by_int.numpy(), want) and np.array_equal(by_str.numpy(), want)
    assert want.max() >= 3 and (want[0] == 0).all()
    assert tie_keys(torch.from_numpy(scores[:1]), torch.from_numpy(ids[:1]), valid[:1], doc_ids) is None
    big = doc_ids.copy()
    big[3] = 10 ** 17                                           # beyond the integer key: the string route, the same keys
    want = C.str_tie_keys(scores, ids, doc_key=lambda p: str(int(big[p])))
    assert np.array_equal(tie_keys(torch.from_numpy(scores), torch.from_numpy(ids), valid, big).numpy(), want)


# ------------------------------------------------------------------------------------------------ the randomization model ---
def test_randomization_model_signs_and_counts():
    z = np.array([0, 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)

    def mix_int(v):
        v = (v + 0x9E3779B97F4A7C15) & C.MASK64
        v = ((v ^ (v >> 30)) * 0xBF58476D1CE4E5B9) & C.MASK64
        v = ((v ^ (v >> 27)) * 0x94D049BB133111EB) & C.MASK64
        return v ^ (v >> 31)
    with np.errstate(over="ignore"):
        assert C.mix(z).tolist() == [mix_int(int(v)) for v in z]
    f = C.flips(130, 3, 6, seed=2 ** 64 - 5)                    # the seed wraps
    for b in range(3):
        for q in (0, 63, 64, 129):
            word = mix_int((2 ** 64 - 5 + (3 + b) * 3 + (q >> 6)) & C.MASK64)
            assert bool(f[b, q]) == bool((word >> (q & 63)) & 1)
    diff = np.random.default_rng(0).standard_normal((2, 65))
    t_obs, count = C.randomization(diff, 257, seed=1, chunk=100)
    s = 0.0
    for x in diff[0]:
        s = s + float(x)
    assert t_obs[0] == s and (count >= 1).all() and (count <= 257).all()
    assert C.randomization(np.zeros((3, 10)), 99, seed=0)[1].tolist() == [99, 99, 99]
    assert C.randomization(np.zeros((2, 0)), 7, seed=0)[1].tolist() == [7, 7]


# ------------------------------------------------------------------------------------ argument checks before any device work ---
def test_eval_hooks_validate_before_they_launch():
    """sr_eval_ranked and sr_eval_randomization reject what they cannot run before anything touches a device: the device pointers below
    are never dereferenced (h_cuts is host memory and is read)."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.sr_eval_max_cuts() == 16

    def ranked(**kw):
        a = dict(dict(sc=p, ids=p, cnt=None, tie=None, ex=None, nq=3, depth=10, ip=p, qi=p, qg=p, nqr=5, nrel=p, idcg=p, log2=p, cuts=[5, 10],
                      order=0, rr=0, out=p, fl=p, mean=p, n=p), **kw)
        cuts = a["cuts"]
        h = None if cuts is None else (ctypes.c_int32 * max(1, len(cuts)))(*cuts)
        return lib.sr_eval_ranked(a["sc"], a["ids"], a["cnt"], a["tie"], a["ex"], a["nq"], a["depth"], a["ip"], a["qi"], a["qg"], a["nqr"],
                                  a["nrel"], a["idcg"], a["log2"], h, a.get("n_cuts", 0 if cuts is None else len(cuts)), a["order"], a["rr"],
                                  a["out"], a["fl"], a["mean"], a["n"], None)
    for change, text in [(dict(ids=None), b"null pointer"), (dict(ip=None), b"null pointer"), (dict(nrel=None), b"null pointer"),
                         (dict(log2=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(fl=None), b"null pointer"),
                         (dict(mean=None), b"null pointer"), (dict(n=None), b"null pointer"), (dict(qi=None), b"null pointer (judgements)"),
                         (dict(qg=None), b"null pointer (judgements)"), (dict(idcg=None), b"null pointer (idcg)"),
                         (dict(cuts=None, n_cuts=2), b"null pointer (cuts)"), (dict(sc=None), b"reads the scores"),
                         (dict(nq=-1), b"bad sizes"), (dict(nqr=-1), b"bad sizes"), (dict(depth=0), b"depth = 0"),
                         (dict(cuts=[5, 5]), b"strictly ascending (cut 1)"), (dict(cuts=[0, 5]), b"strictly ascending (cut 0)"),
                         (dict(cuts=[10, 5]), b"strictly ascending"), (dict(cuts=list(range(1, 18))), b"n_cuts = 17"),
                         (dict(n_cuts=-1), b"n_cuts = -1"), (dict(order=2), b"bad order 2"), (dict(order=-1), b"bad order -1"),
                         (dict(rr=-1), b"rr_depth = -1")]:
        rc = ranked(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    rc = ranked(depth=lib.sr_max_topk() + 1)
    assert rc == _lib.SR_ERR_UNSUPPORTED and b"depth = 4097" in lib.sr_last_error()

    def rand(**kw):
        a = dict(dict(diff=p, cols=2, n=10, perm=100, seed=0, t=p, c=p), **kw)
        return lib.sr_eval_randomization(a["diff"], a["cols"], a["n"], a["perm"], a["seed"], a["t"], a["c"], None)
    for change, text in [(dict(cols=0), b"n_cols = 0"), (dict(cols=9), b"n_cols = 9"), (dict(n=-1), b"bad n"), (dict(perm=0), b"n_perm = 0"),
                         (dict(perm=1 << 31), b"n_perm = 2147483648"), (dict(diff=None), b"null pointer"), (dict(t=None), b"null pointer"),
                         (dict(c=None), b"null pointer")]:
        rc = rand(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())


def test_python_front_ends_validate_before_a_device_is_asked_for():
    from scaling_retriever_amd import evaluation as E
    Q = E.Qrels({"a": {"d0": 1}}, ["d0", "d1"])
    ids, sc = np.zeros((1, 4), np.int64), np.zeros((1, 4), np.float32)
    for kw, text in [(dict(order="rank"), "order"), (dict(rr_depth=-1), "rr_depth"), (dict(counts=np.zeros(2, np.int32)), "counts"),
                     (dict(exclude=np.zeros(3, np.int64)), "exclude")]:
        a = dict(dict(counts=None, order="score", rr_depth=0, exclude=None), **kw)
        for fn in (E.evaluate_arrays, E.evaluate_by_steps):
            with pytest.raises(ValueError, match=text):
                fn(sc, ids, a["counts"], Q, ["a"], order=a["order"], rr_depth=a["rr_depth"], exclude=a["exclude"])
    with pytest.raises(ValueError, match="depth = 4097"):
        E.evaluate_arrays(np.zeros((1, 4097), np.float32), np.zeros((1, 4097), np.int64), None, Q, ["a"])
    with pytest.raises(ValueError, match="shaped like ids"):
        E.evaluate_arrays(None, ids, None, Q, ["a"])
    with pytest.raises(ValueError, match="1 lists, 2 queries"):
        E.evaluate_arrays(sc, ids, None, Q, ["a", "b"])
    for n_perm in (0, 1 << 31):
        with pytest.raises(ValueError, match="n_perm"):
            E.randomization_test(np.zeros((1, 4)), n_perm=n_perm)
    with pytest.raises(ValueError, match=r"\[n_cols, n\]"):
        E.randomization_test(np.zeros(4))
    with pytest.raises(ValueError, match="provide valid metric"):
        E.metric_dict({}, "map")
    assert E.column_names((5, 10))[:4] == ["recip_rank", "recall_5", "recall_10", "ndcg_cut_5"]


def test_driver_arguments(capsys):
    import eval_compare
    import eval_dense
    import eval_sparse
    a = eval_compare.parse_args(["--qrel_path", "q.json", "--run_paths", "a/run.json,b/run.json", "--output_dir", "out"])
    assert a.run_paths == ["a/run.json", "b/run.json"] and a.metrics == ["ndcg_cut_10", "recip_rank"]
    assert (a.rr_depth, a.permutations, a.seed) == (0, 100000, 0)
    a = eval_compare.parse_args(["--qrel_path", "q", "--run_paths", "a,b", "--output_dir", "o", "--metrics", "map_cut_100,r_cap_100", "--rr_depth",
                                 "10", "--permutations", "999", "--seed", "7"])
    assert a.metrics == ["map_cut_100", "r_cap_100"] and (a.rr_depth, a.permutations, a.seed) == (10, 999, 7)
    for bad in (["--run_paths", "a"], ["--run_paths", "a,b,c"], ["--run_paths", "a,b", "--metrics", "ndcg_cut_7"],
                ["--run_paths", "a,b", "--metrics", ","], ["--run_paths", "a,b", "--rr_depth", "-1"],
                ["--run_paths", "a,b", "--permutations", "0"]):
        with pytest.raises(SystemExit):
            eval_compare.parse_args(["--qrel_path", "q", "--output_dir", "o"] + bad)
    capsys.readouterr()
    for drv in (eval_dense, eval_sparse):
        assert drv.parse_args(["--task_name", "evaluate_msmarco"]).device_eval is False
        a = drv.parse_args(["--task_name", "evaluate_msmarco", "--device_eval", "--eval_metric", "['mrr_10', 'recall']"])
        assert a.device_eval is True and a.eval_metric == ["mrr_10", "recall"]
