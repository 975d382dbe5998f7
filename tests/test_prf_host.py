"""CPU: pseudo-relevance feedback without a device - the numpy model of tests/prf_cases.py against a plain per-term
Python loop and against float64 within the bound derived there, the argument rules of the Python layer and of the C entries, the
refusals of the classes that do not offer it, and the CLI flags."""
import ctypes
import os
import sys

import numpy as np
import pytest

import prf_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
V = 97
FB = np.array([[3, 4, 5, 7, 9, 11, 13, 15],
               [-1, 6, -1, 8, 10, -1, 12, 14],
               [20, 21, 22, 23, 24, 25, 26, 27],
               [30, 31, 32, 33, 34, 35, 36, 37],
               [40, 40, 41, 42, 41, 43, 44, 45],
               [46, 47, 48, 49, 0, 1, 2, 3]], dtype=np.int64)
COUNTS = np.array([8, 8, 8, 0, 8, 2], dtype=np.int32)
CASES = [dict(n_pos=3, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=0),
         dict(n_pos=3, n_neg=2, alpha=1.0, beta=0.75, gamma=0.5, max_terms=0),
         dict(n_pos=10, n_neg=4, alpha=0.5, beta=1.0, gamma=2.0, max_terms=6),
         dict(n_pos=2, n_neg=3, alpha=1.0, beta=0.5, gamma=8.0, max_terms=3)]


def _loop(q, d, fb_row, count, kw):
    """One query, term by term, with Python dicts and scalar fp32 operations: {term: w} of the kept terms."""
    (qi, qc, qv), (di, dc, dv) = q, d
    pos, neg = M.feedback_sets(fb_row, count, kw["n_pos"], kw["n_neg"])
    doc = lambda j: {int(t): F32(v) for t, v in zip(dc[di[j]:di[j + 1]], dv[di[j]:di[j + 1]])}      # noqa: E731
    query = {int(t): F32(v) for t, v in zip(qc, qv)}
    terms = set(query)
    for j in pos + neg:
        terms |= set(doc(j))
    cp, cn = M.coefficients(kw["beta"], kw["gamma"], len(pos), len(neg))
    w = {}
    for t in sorted(terms):
        P = N = F32(0.0)
        for j in pos:
            if t in doc(j):
                P = F32(P + doc(j)[t])
        for j in neg:
            if t in doc(j):
                N = F32(N + doc(j)[t])
        x = F32(F32(kw["alpha"]) * query[t]) if t in query else F32(0.0)
        if pos:
            x = F32(x + F32(cp * P))
        if neg:
            x = F32(x - F32(cn * N))
        if x > 0:
            w[t] = x
    if kw["max_terms"] and len(w) > kw["max_terms"]:
        best = sorted(w, key=lambda t: (-float(w[t]), t))[:kw["max_terms"]]
        w = {t: w[t] for t in sorted(best)}
    return w


@pytest.mark.parametrize("kw", CASES)
def test_model_equals_a_per_term_loop(kw):
    q, d = M.small_collection()
    indptr, cols, vals = M.rocchio_sparse(*q, *d, V, FB, COUNTS, **kw)
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == F32
    for r in range(len(FB)):
        a, b = q[0][r], q[0][r + 1]
        want = _loop((None, q[1][a:b], q[2][a:b]), d, FB[r], COUNTS[r], kw)
        got_c, got_v = cols[indptr[r]:indptr[r + 1]], vals[indptr[r]:indptr[r + 1]]
        assert got_c.tolist() == list(want) and np.array_equal(M.bits(got_v), M.bits(np.array(list(want.values()), F32))), (r, kw)


def test_model_sets_and_coefficients():
    assert M.feedback_sets([5, -1, 6, 7, 8], None, 2, 2) == ([5, 6], [7, 8])
    assert M.feedback_sets([5, -1, 6, 7, 8], 4, 2, 2) == ([5, 6], [7])           # the negative set never overlaps the positive one
    assert M.feedback_sets([5, -1, 6, 7, 8], 3, 3, 2) == ([5, 6], [])
    assert M.feedback_sets([5, 5, 5], None, 1, 5) == ([5], [5, 5])
    assert M.feedback_sets([5, 6], 0, 1, 1) == ([], [])
    from scaling_retriever_amd.prf import coefficient_tables
    cp, cn = coefficient_tables(0.75, 0.3)
    assert cp.dtype == F32 and cp.shape == (64,)
    for n in (1, 3, 7, 64):
        assert (cp[n - 1], cn[n - 1]) == M.coefficients(0.75, 0.3, n, n)
        assert cp[n - 1] == F32(F32(0.75) / F32(n))


@pytest.mark.parametrize("kw", CASES)
def test_model_against_float64_within_the_derived_bound(kw):
    """|w - exact| <= (p + g + 3) 2^-24 (alpha |q| + cp sum|d| + cn sum|d|) per term (tests/prf_cases.py), checked on the unpruned
    vector of every query, dense and sparse."""
    q, d = M.small_collection()
    (qi, qc, qv), (di, dc, dv) = q, d
    free = dict(kw, max_terms=0)
    indptr, cols, vals = M.rocchio_sparse(*q, *d, V, FB, COUNTS, **free)
    dense_rows = np.zeros((len(di) - 1, V), F32)
    for j in range(len(di) - 1):
        dense_rows[j, dc[di[j]:di[j + 1]]] = dv[di[j]:di[j + 1]]
    Q = np.zeros((len(qi) - 1, V), F32)
    for r in range(len(qi) - 1):
        Q[r, qc[qi[r]:qi[r + 1]]] = qv[qi[r]:qi[r + 1]]
    args = {k_: v for k_, v in free.items() if k_ != "max_terms"}
    dense = M.rocchio_dense(Q, lambda j: dense_rows[j], FB, COUNTS, **args)
    for r in range(len(FB)):
        pos, neg = M.feedback_sets(FB[r], COUNTS[r], kw["n_pos"], kw["n_neg"])
        cp, cn = (float(c) for c in M.coefficients(kw["beta"], kw["gamma"], len(pos), len(neg)))
        rows = dense_rows.astype(np.float64)
        P, N = rows[pos].sum(0) if pos else np.zeros(V), rows[neg].sum(0) if neg else np.zeros(V)
        aP, aN = np.abs(rows[pos]).sum(0) if pos else np.zeros(V), np.abs(rows[neg]).sum(0) if neg else np.zeros(V)
        alpha = float(F32(kw["alpha"]))
        exact = alpha * Q[r].astype(np.float64) + cp * P - cn * N
        bound = (len(pos) + len(neg) + 3) * 2.0 ** -24 * (alpha * np.abs(Q[r].astype(np.float64)) + cp * aP + cn * aN)
        assert (np.abs(dense[r].astype(np.float64) - exact) <= bound).all(), (r, kw)
        sparse = np.zeros(V)
        sparse[cols[indptr[r]:indptr[r + 1]]] = vals[indptr[r]:indptr[r + 1]]
        kept = dense[r] > 0
        assert np.array_equal(np.flatnonzero(kept), cols[indptr[r]:indptr[r + 1]])       # the two heads' models agree term for term
        assert (np.abs(sparse - exact)[kept] <= bound[kept]).all(), (r, kw)


def test_argument_rules_raise_before_a_device_is_touched():
    import torch
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.prf import prf_arguments
    cap = int(_lib.load().sr_max_topk())
    assert prf_arguments("search_prf", 10, 0, 1.0, 0.75, 0.0, 128, first_round=True) == 10
    assert prf_arguments("search_prf", 64, 64, 0.0, 0.0, 0.0, 0, first_round=True, fb_depth=128, subset=[1, 2]) == 128
    assert prf_arguments("feedback", 10, 3, 1.0, 0.75, 0.5, 0, depth=cap) is None
    ok = dict(n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=128)
    for change, text in [(dict(n_pos=0), "n_pos = 0"), (dict(n_pos=65), "n_pos = 65"), (dict(n_neg=-1), "n_neg = -1"), (dict(n_neg=65), "n_neg = 65"),
                         (dict(alpha=-0.5), "alpha"), (dict(beta=float("nan")), "beta"), (dict(gamma=float("inf")), "gamma"),
                         (dict(gamma=1e39), "gamma"), (dict(max_terms=-1), "max_terms = -1"), (dict(depth=cap + 1), f"sr_max_topk\\(\\) = {cap}"),
                         (dict(depth=0), "depth = 0"), (dict(n_neg=3, first_round=True), "fb_depth = 10 must be >= n_pos \\+ n_neg = 13"),
                         (dict(n_neg=3, first_round=True, fb_depth=12), "fb_depth = 12"), (dict(first_round=True, fb_depth=cap + 1), "fb_depth"),
                         (dict(subset=[1], mask=np.ones(4, bool)), "not both"),
                         (dict(allowed_masks=np.ones((1, 4), bool), query_group=None), "go together")]:
        with pytest.raises(ValueError, match=text):
            prf_arguments("search_prf", **dict(ok, **change))
    # the free function and the baselines check before they move anything: CPU tensors, no library call is reached
    from scaling_retriever_amd.prf import dense_feedback_by_steps, sparse_feedback_by_steps
    from scaling_retriever_amd.scoring import sparse_feedback
    q, d = M.small_collection()
    t = [torch.from_numpy(np.ascontiguousarray(x)) for x in (*q, *d)]
    for fn in (sparse_feedback, sparse_feedback_by_steps):
        with pytest.raises(ValueError, match="n_pos = 0"):
            fn(*t, V, torch.from_numpy(FB), n_pos=0)
        with pytest.raises(ValueError, match="gamma"):
            fn(*t, V, torch.from_numpy(FB), gamma=-1.0)
    with pytest.raises(ValueError, match="fb_ids int64 .nq, depth."):
        sparse_feedback(*t, V, torch.from_numpy(FB[0]))

    class NoIndex:
        device = torch.device("cpu")
    with pytest.raises(ValueError, match="n_neg = 70"):
        dense_feedback_by_steps(NoIndex(), None, torch.from_numpy(FB), n_neg=70)
    # the C entries check the same before any device work: the pointers below are never dereferenced
    lib, p, n = _lib.load(), ctypes.c_void_p(4096), ctypes.c_int64(-1)
    assert lib.sr_prf_max_entries() >= 8192

    def sparse(**kw):
        a = dict(dict(nq=2, n_docs=50, n_terms=97, depth=8, n_pos=3, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=0), **kw)
        return lib.sr_sparse_feedback(p, p, p, a["nq"], p, p, p, a["n_docs"], a["n_terms"], p, None, a["depth"], a["n_pos"], a["n_neg"],
                                      a["alpha"], a["beta"], a["gamma"], a["max_terms"], p, p, p, 100, ctypes.byref(n), None)

    def dense(**kw):
        a = dict(dict(idx=p, nq=2, depth=8, n_pos=3, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0), **kw)
        return lib.sr_dense_feedback(a["idx"], p, a["nq"], p, None, a["depth"], a["n_pos"], a["n_neg"], a["alpha"], a["beta"], a["gamma"], p, None)
    for change, text in [(dict(n_pos=0), b"n_pos = 0"), (dict(n_pos=65), b"n_pos = 65"), (dict(n_neg=65), b"n_neg = 65"), (dict(n_neg=-1), b"n_neg = -1"),
                         (dict(depth=0), b"depth = 0"), (dict(depth=cap + 1), b"sr_max_topk"), (dict(alpha=-1.0), b"finite and >= 0"),
                         (dict(beta=float("nan")), b"finite and >= 0"), (dict(gamma=float("inf")), b"finite and >= 0"), (dict(nq=-1), b"bad nq")]:
        for call in (sparse, dense):
            rc = call(**change)
            assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    for change, text in [(dict(max_terms=-1), b"max_terms -1"), (dict(n_terms=0), b"n_terms=0"), (dict(n_docs=-1), b"n_docs=-1")]:
        rc = sparse(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert n.value == -1
    assert dense(idx=None) == _lib.SR_ERR_INVALID and b"null index" in lib.sr_last_error()
    assert dense(nq=0) == _lib.SR_OK
    assert sparse(nq=0) == _lib.SR_OK and n.value == 0


def test_classes_without_feedback_refuse():
    from scaling_retriever_amd.distributed import ShardedDenseRetriever, ShardedSparseRetriever
    from scaling_retriever_amd.indexer import HybridRetriever, ShardedSparseRetrieval
    for cls, method, text in [(ShardedDenseRetriever, "search_prf", "doc-sharded"), (ShardedSparseRetriever, "search_prf", "doc-sharded"),
                              (ShardedSparseRetrieval, "retrieve_prf", "doc-sharded"), (HybridRetriever, "retrieve_prf", "per head")]:
        with pytest.raises(NotImplementedError, match=text):
            getattr(cls, method)(None)


def test_cli_flags_parse(capsys):
    sys.path.insert(0, ROOT)
    import eval_dense
    import eval_sparse
    base = ["--task_name", "retrieval", "--top_k", "10"]
    a = eval_sparse.parse_args(base + ["--prf_depth", "10", "--prf_alpha", "0.9", "--prf_beta", "0.6", "--prf_gamma", "0.1", "--prf_neg_depth", "5",
                                       "--prf_max_terms", "64"])
    assert (a.prf_depth, a.prf_alpha, a.prf_beta, a.prf_gamma, a.prf_neg_depth, a.prf_max_terms) == (10, 0.9, 0.6, 0.1, 5, 64)
    off = eval_sparse.parse_args(base)
    assert (off.prf_depth, off.prf_alpha, off.prf_beta, off.prf_gamma, off.prf_neg_depth, off.prf_max_terms) == (0, 1.0, 0.75, 0.0, 0, 128)
    b = eval_dense.parse_args(base + ["--prf_depth", "5", "--prf_beta", "0.5"])
    assert (b.prf_depth, b.prf_alpha, b.prf_beta, b.prf_gamma, b.prf_neg_depth) == (5, 1.0, 0.5, 0.0, 0)
    assert eval_dense.parse_args(base).prf_depth == 0 and not hasattr(b, "prf_max_terms")
    for driver in (eval_sparse, eval_dense):
        for extra, text in [(["--prf_depth", "65"], "[1, 64]"), (["--prf_depth", "5", "--prf_neg_depth", "65"], "[0, 64]"),
                            (["--prf_neg_depth", "3"], "need --prf_depth"), (["--prf_depth", "5", "--prf_beta", "-1"], ">= 0"),
                            (["--prf_depth", "5", "--collapse_file", "x.tsv"], "--collapse_file")]:
            with pytest.raises(SystemExit):
                driver.parse_args(base + extra)
            assert text in capsys.readouterr().err, (driver.__name__, extra)
    a.world_size = b.world_size = 2                               # the doc-sharded retrieval: refused before anything is loaded
    with pytest.raises(NotImplementedError, match="--prf_depth"):
        eval_sparse.sparse_retrieval(a)
    with pytest.raises(NotImplementedError, match="--prf_depth"):
        eval_dense.retrieval(b)
