"""CPU: the numpy model of sr_sparse_mmr against hand-worked values (tests/mmr_sparse_cases.py), the argument rules of the
sparse MMR entry points, the classes that refuse, and the eval driver's flag conflicts.  The GPU side is tests/test_mmr_sparse_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

import mmr_sparse_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _row(*pairs):
    return np.array([t for t, _ in pairs], np.int32), np.array([v for _, v in pairs], F32)


# d0 and d1 meet at term 0 with opposite signs, d2 is empty (its norm is zero), d3 meets d0 at term 1 alone
HAND = [_row((0, 2), (1, 1)), _row((0, -2)), _row(), _row((1, 3), (2, 4))]
HAND_REL = np.array([[1.0, 0.9, 0.5, 0.8]], F32)


def test_hand_worked_four_candidates_inner_product():
    """Small integers: every product and sum is exact.  ip(d1, d0) = -4, so d1's marginal value 0.5 * 0.9 + 0.5 * 4 lies ABOVE pick 0's
    0.5 * 1.0 - the one place the sequence may rise."""
    ip = M.ip_matrix(HAND, 8)
    assert ip.tolist() == [[5, -4, 0, 3], [-4, 4, 0, 0], [0, 0, 0, 0], [3, 0, 0, 25]]
    assert all(M.bits(ip[i, j]) == M.bits(M.ip_pair(HAND[i], HAND[j])) for i in range(4) for j in range(4))
    assert np.array_equal(M.bits(ip), M.bits(ip.T)) and not np.signbit(ip[2]).any()        # symmetric; +0.0f where nothing meets
    got = M.mmr(ip, lambda d: d, np.arange(4, dtype=np.int64)[None], HAND_REL, 4, 0.5)
    half = F32(0.5)
    lr = [F32(half * r) for r in HAND_REL[0]]
    # pick 0 by rel: d0.  m = (-4, 0, 3) -> v = (2.45, 0.25, -1.1): d1; nothing meets d1, the maxima stay: d2 (0.25), then d3 (-1.1)
    want_v = [lr[0], F32(lr[1] - F32(half * F32(-4))), F32(lr[2] - F32(half * F32(0))), F32(lr[3] - F32(half * F32(3)))]
    assert got[0][0].tolist() == [0, 1, 2, 3] and got[3][0].tolist() == [0, 1, 2, 3] and got[4].tolist() == [4]
    assert np.array_equal(M.bits(got[2][0]), M.bits(np.array(want_v, F32)))
    assert np.array_equal(M.bits(got[1][0]), M.bits(HAND_REL[0]))
    assert got[2][0, 1] > got[2][0, 0] and (np.diff(got[2][0, 1:]) <= 0).all()


def test_hand_worked_four_candidates_cosine():
    """The same rows under cosine: norms (sqrt 5, 2, 0, 5); the empty d2 has den = 0 with everything and similarity +0.0f, never a NaN.
    d3 now overtakes d2: 0.4 - 0.5 * 3 / (5 sqrt 5) = 0.266 against 0.25."""
    ip = M.ip_matrix(HAND, 8)
    cos = M.cosine_matrix(ip)
    r5 = np.sqrt(F32(5))
    assert np.isfinite(cos).all() and not cos[2].any() and not cos[:, 2].any() and not np.signbit(cos[2]).any()
    assert M.bits(cos[1, 0]) == M.bits(F32(F32(-4) / F32(F32(2) * r5))) and M.bits(cos[3, 0]) == M.bits(F32(F32(3) / F32(F32(5) * r5)))
    assert M.bits(cos[0, 1]) == M.bits(F32(F32(-4) / F32(r5 * F32(2))))          # den commutes: the matrix is symmetric
    assert cos[1, 1] == 1 and cos[3, 3] == 1 and cos[2, 2] == 0
    got = M.mmr(cos, lambda d: d, np.arange(4, dtype=np.int64)[None], HAND_REL, 4, 0.5)
    half = F32(0.5)
    lr = [F32(half * r) for r in HAND_REL[0]]
    want_v = [lr[0], F32(lr[1] - F32(half * cos[1, 0])), F32(lr[3] - F32(half * cos[3, 0])), F32(lr[2] - F32(half * F32(0)))]
    assert got[0][0].tolist() == [0, 1, 3, 2] and got[3][0].tolist() == [0, 1, 3, 2]
    assert np.array_equal(M.bits(got[2][0]), M.bits(np.array(want_v, F32)))
    assert got[2][0, 1] > got[2][0, 0] and (np.diff(got[2][0, 1:]) <= 0).all()
    # lambda = 1: the candidates by (rel, id), whatever the similarity
    for sim in (ip, cos):
        one = M.mmr(sim, lambda d: d, np.arange(4, dtype=np.int64)[None], HAND_REL, 3, 1.0)
        assert one[0][0].tolist() == [0, 1, 3] and np.array_equal(M.bits(one[2][0]), M.bits(HAND_REL[0, [0, 1, 3]]))


def test_the_collection_holds_the_rows_the_kernel_paths_need():
    rows = M.collection()
    lens = [len(t) for t, _ in rows]
    assert len(rows) == M.N_DOCS and {0, 1, 63, 64, 65, 130, 300} <= set(lens)
    assert all((np.diff(t) > 0).all() and t.min() >= 0 and t.max() < M.V for t, _ in rows if len(t))
    assert all(rows[50 + i][0] is rows[30 + i][0] for i in range(M.TWINS)) and lens[27] == 300 and lens[28] == 130
    ip = M.ip_matrix(rows[:70])
    assert all(M.bits(ip[i, j]) == M.bits(M.ip_pair(rows[i], rows[j])) for i, j in [(20, 24), (24, 27), (23, 28), (30, 50), (24, 24), (4, 4)])
    assert ip[60, 63] == 0 and ip[61, 65] == 0 and ip[3, 24] == 0                # disjoint rows, an empty row
    assert np.array_equal(M.bits(ip), M.bits(ip.T))
    # the order of the sum shows: the same products added in descending term order give other bits for a long pair
    t, v = rows[24]
    back = F32(0.0)
    for x in v[::-1]:
        back = F32(back + F32(x * x))
    assert M.bits(back) != M.bits(ip[24, 24])
    indptr, cols, vals = M.doc_major_csr(rows)
    t_indptr, docs, t_vals = M.term_major_csr(rows)
    assert indptr[-1] == t_indptr[-1] == cols.size == docs.size and indptr[600] == indptr[599]
    assert all((np.diff(docs[t_indptr[t]:t_indptr[t + 1]]) > 0).all() for t in range(M.V))


def test_argument_rules():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.mmr import SIM_MODES, mmr_arguments
    cap = _lib.load().sr_mmr_max_candidates()
    assert SIM_MODES == {"ip": _lib.SR_MMR_SIM_IP, "cosine": _lib.SR_MMR_SIM_COSINE}
    mmr_arguments("search_mmr", 10, 128, 0.5, sim="ip")
    mmr_arguments("search_mmr", cap, cap, 1.0, sim="cosine", subset=[1, 2])
    mmr_arguments("search_mmr", 10, 128, 0.5)                     # the dense head's calls carry no sim
    with pytest.raises(ValueError, match="k = 11 must lie in"):
        mmr_arguments("search_mmr", 11, 10, 0.5, sim="ip")
    with pytest.raises(ValueError, match="k = 0 must lie in"):
        mmr_arguments("search_mmr", 0, 10, 0.5, sim="ip")
    with pytest.raises(ValueError, match=f"sr_mmr_max_candidates\\(\\) = {cap}"):
        mmr_arguments("search_mmr", 10, cap + 1, 0.5, sim="ip")
    for lam in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="must lie in \\[0, 1\\]"):
            mmr_arguments("search_mmr", 10, 128, lam, sim="cosine")
    for sim in ("dot", "", 0):
        with pytest.raises(ValueError, match="must be one of"):
            mmr_arguments("search_mmr", 10, 128, 0.5, sim=sim)
    with pytest.raises(ValueError, match="not both"):
        mmr_arguments("search_mmr", 10, 128, 0.5, sim="ip", subset=[1], mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="not both"):
        mmr_arguments("search_mmr", 10, 128, 0.5, np.ones((1, 4), bool), [0], sim="ip", mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="go together"):
        mmr_arguments("search_mmr", 10, 128, 0.5, np.ones((1, 4), bool), None, sim="ip")


def test_the_entry_point_checks_before_any_device_work():
    """The symbol is in the built library, and a bad size, sim_mode, lambda or pointer is SR_ERR_INVALID without a device: the pointers
    below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib, p = _lib.load(), ctypes.c_void_p(4096)
    assert "sr_sparse_mmr" in _lib.SIGNATURES and lib.sr_sparse_mmr is not None
    cap = lib.sr_mmr_max_candidates()

    def call(nq=1, n=8, k=4, lam=0.5, sim=0, n_docs=10, ptr=p):
        return lib.sr_sparse_mmr(ptr, p, p, n_docs, p, p, None, nq, n, k, lam, sim, p, p, p, p, p, None)
    for kw, text in [(dict(n=cap + 1, k=1), b"sr_mmr_max_candidates"), (dict(n=0, k=1), b"candidates per query"), (dict(k=0), b"k = 0"),
                     (dict(k=9), b"k = 9"), (dict(lam=1.5), b"lambda"), (dict(lam=-0.5), b"lambda"), (dict(lam=float("nan")), b"lambda"),
                     (dict(sim=2), b"sim_mode = 2"), (dict(sim=-1), b"sim_mode"), (dict(n_docs=-1), b"n_docs"), (dict(nq=-1), b"nq"),
                     (dict(ptr=None), b"null pointer")]:
        assert call(**kw) == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (kw, lib.sr_last_error())
    assert call(nq=0) == _lib.SR_OK and call(nq=0, ptr=None) == _lib.SR_OK


def test_classes_without_a_diversified_search_refuse():
    from scaling_retriever_amd.distributed import ShardedSparseRetriever
    from scaling_retriever_amd.indexer import HybridRetriever, ShardedSparseRetrieval
    for cls, method, text in [(ShardedSparseRetriever, "search_mmr", "doc-sharded"), (ShardedSparseRetrieval, "retrieve_mmr", "doc-sharded"),
                              (HybridRetriever, "retrieve_mmr", "per head")]:
        with pytest.raises(NotImplementedError, match=text):
            getattr(cls, method)(None)


def test_eval_sparse_flag_conflicts(capsys):
    sys.path.insert(0, ROOT)
    import eval_sparse
    base = ["--task_name", "retrieval", "--top_k", "10"]
    a = eval_sparse.parse_args(base + ["--mmr_lambda", "0.5", "--mmr_fetch_k", "40"])
    assert (a.mmr_lambda, a.mmr_fetch_k, a.mmr_sim) == (0.5, 40, "cosine")
    assert eval_sparse.parse_args(base + ["--mmr_lambda", "0", "--mmr_fetch_k", "10", "--mmr_sim", "ip"]).mmr_sim == "ip"
    off = eval_sparse.parse_args(base)
    assert off.mmr_lambda is None and off.mmr_fetch_k == 0
    for extra, text in [(["--mmr_lambda", "0.5", "--mmr_fetch_k", "40", "--collapse_file", "x.tsv"], "--collapse_file"),
                        (["--mmr_lambda", "0.5", "--mmr_fetch_k", "40", "--prf_depth", "3"], "--prf_depth"),
                        (["--mmr_lambda", "1.5", "--mmr_fetch_k", "40"], "[0, 1]"),
                        (["--mmr_lambda", "0.5", "--mmr_fetch_k", "5"], "--mmr_fetch_k >= top_k"),
                        (["--mmr_lambda", "0.5"], "--mmr_fetch_k >= top_k"),
                        (["--mmr_lambda", "0.5", "--mmr_fetch_k", "40", "--mmr_sim", "dot"], "--mmr_sim"),
                        (["--mmr_fetch_k", "40"], "needs --mmr_lambda")]:
        with pytest.raises(SystemExit):
            eval_sparse.parse_args(base + extra)
        assert text in capsys.readouterr().err, extra
    a.world_size = 2                                              # the doc-sharded retrieval: refused before anything is loaded
    with pytest.raises(NotImplementedError, match="--mmr_lambda"):
        eval_sparse.sparse_retrieval(a)
