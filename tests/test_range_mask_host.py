"""CPU: the range searches and the exact hybrid search under a document bitmap - the new C-ABI symbols, the argument checks that come
before any device work, what is still refused, and the numpy route calculator of the masked hybrid test against the unmasked one."""
import ctypes
import os
import re

import numpy as np
import pytest

import hybrid_cases as H
import hybrid_mask_cases as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_dense_range_count_masked", "sr_dense_range_fill_masked", "sr_sparse_range_count_masked", "sr_sparse_range_fill_masked",
         "sr_doc_mask_remap")


def test_new_symbols_are_declared_exported_and_bound():
    from scaling_retriever_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the masked pairs take the unmasked arguments plus (d_mask_words, n_bits)
    for head in ("dense", "sparse"):
        for half in ("count", "fill"):
            assert len(_lib.SIGNATURES[f"sr_{head}_range_{half}_masked"][1]) == len(_lib.SIGNATURES[f"sr_{head}_range_{half}"][1]) + 2
    from scaling_retriever_amd import scoring
    assert callable(scoring.doc_mask_remap)


def test_entry_points_validate_before_they_touch_a_device():
    """The pointers below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    total = ctypes.c_int64(-1)
    rc = lib.sr_dense_range_count_masked(None, p, 4, p, p, 0, p, ctypes.byref(total), None)
    assert rc == _lib.SR_ERR_INVALID and b"sr_dense_range_count_masked: null index" in lib.sr_last_error()
    rc = lib.sr_dense_range_fill_masked(None, p, 4, p, p, 0, p, p, p, 10, None)
    assert rc == _lib.SR_ERR_INVALID and b"sr_dense_range_fill_masked: null index" in lib.sr_last_error()
    rc = lib.sr_sparse_range_count_masked(None, p, p, p, 4, p, p, 0, p, ctypes.byref(total), None)
    assert rc == _lib.SR_ERR_INVALID and b"sr_sparse_range_count_masked: null index" in lib.sr_last_error()
    rc = lib.sr_sparse_range_fill_masked(None, p, p, p, 4, p, p, 0, p, 0, 1, p, p, 10, None)
    assert rc == _lib.SR_ERR_INVALID and b"sr_sparse_range_fill_masked: null index" in lib.sr_last_error()
    # an empty dense index numbers its documents in [0, 0): any other n_bits is refused, and so is a null mask
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    rc = lib.sr_dense_range_count_masked(h, p, 4, p, p, 32, p, ctypes.byref(total), None)
    assert rc == _lib.SR_ERR_INVALID and b"n_bits=32" in lib.sr_last_error() and total.value == -1
    rc = lib.sr_dense_range_fill_masked(h, p, 4, p, p, 1, p, p, p, 10, None)
    assert rc == _lib.SR_ERR_INVALID and b"n_bits=1" in lib.sr_last_error()
    rc = lib.sr_dense_range_count_masked(h, p, 4, p, None, 0, p, ctypes.byref(total), None)
    assert rc == _lib.SR_ERR_INVALID and b"null mask" in lib.sr_last_error()
    rc = lib.sr_dense_range_fill_masked(h, p, 4, p, p, 0, p, p, p, 10, None)
    assert rc == _lib.SR_ERR_INVALID and b"count" in lib.sr_last_error()          # no count precedes it
    assert lib.sr_dense_index_destroy(h) == 0
    for change, text in [(dict(ns=-1), b"bad sizes"), (dict(nd=-1), b"bad sizes"), (dict(nd=(1 << 32) + 1), b"bad sizes"),
                         (dict(src=None), b"null pointer"), (dict(map=None), b"null pointer"), (dict(dst=None), b"null pointer")]:
        a = dict(dict(src=p, ns=10, map=p, nd=10, dst=p), **change)
        rc = lib.sr_doc_mask_remap(a["src"], a["ns"], a["map"], a["nd"], a["dst"], None)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert lib.sr_doc_mask_remap(None, 0, None, 0, None, None) == _lib.SR_OK


def test_mask_shape_and_not_both_errors_come_before_any_device_work(monkeypatch):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.indexer import DenseFlatIndexer, SparseRetrieval
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    dense = object.__new__(DenseIndexHIP)                 # no handle behind them: the checks come first
    sparse = object.__new__(SparseIndexHIP)
    sparse.n_docs = 100
    for bad in (np.ones((4, 4), bool), np.ones(10, np.float32), np.ones(10, np.int64), [[True, False]]):
        with pytest.raises(ValueError):
            dense.range_search(None, 0.0, mask=bad)
        with pytest.raises(ValueError):
            dense.range_count(None, 0.0, mask=bad)
        with pytest.raises(ValueError):
            dense.range_fill(None, None, None, 0, mask=bad)
        with pytest.raises(ValueError):
            sparse.range_search(None, None, None, 0.0, mask=bad)
    with pytest.raises(ValueError, match="4 words"):
        sparse.range_search(None, None, None, 0.0, mask=np.zeros(5, np.uint32))      # 100 documents: 4 words
    with pytest.raises(ValueError, match="not both"):
        DenseFlatIndexer.range_search(object.__new__(DenseFlatIndexer), None, 0.0, allowed_ids=["a"], allowed_mask=np.ones(3, bool))
    with pytest.raises(ValueError, match="not both"):
        SparseRetrieval.range_search(object.__new__(SparseRetrieval), None, allowed_ids=["a"], allowed_mask=np.ones(3, bool))


def test_what_is_still_refused(monkeypatch):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.indexer import HybridRetriever, ShardedSparseRetrieval

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    with pytest.raises(NotImplementedError):
        ShardedSparseRetrieval.range_search(object.__new__(ShardedSparseRetrieval), None, allowed_mask=np.ones(3, bool))
    with pytest.raises(NotImplementedError):
        ShardedSparseRetrieval.range_search(object.__new__(ShardedSparseRetrieval), None, allowed_ids=["a"])
    with pytest.raises(NotImplementedError):
        ShardedSparseRetrieval.search_fused(object.__new__(ShardedSparseRetrieval), None, None, 10, allowed_mask=np.ones(3, bool))
    ret = object.__new__(HybridRetriever)
    with pytest.raises(NotImplementedError, match=r"allowed_mask=ret\.allowed_mask\(ids\)"):
        ret.search_fused(None, None, 10, allowed_ids=["d1"])
    with pytest.raises(NotImplementedError, match=r"allowed_mask=ret\.allowed_mask\(ids\)"):
        ret.retrieve_fused_exact(None, 10, allowed_ids=["d1"])
    with pytest.raises(ValueError):                       # the weights come before the mask
        ret.search_fused(None, None, 10, weights=(-1.0, 1.0), allowed_mask=np.ones(3, bool))
    with pytest.raises(ValueError):
        ret.retrieve_fused_exact(None, 0, allowed_mask=np.ones(3, bool))
    header = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    assert "Not offered: a range search under a subset or mask" not in header
    from scaling_retriever_amd import hybrid
    assert "per-query masks" in hybrid.__doc__ and "allow-lists / masks" not in hybrid.__doc__


def _dense_sparse(case):
    """numpy float32 scores of every (query, document) of a hybrid case, as tests/test_hybrid_search_host.py computes them."""
    F32 = np.float32
    dense = (case["Q"].astype(np.float64) @ case["rows"].astype(np.float64).T).astype(F32)
    indptr, ids, vals = case["index"]
    d2s = case["d2s"]
    sp = np.zeros((len(case["Q"]), len(case["s2d"])), F32)
    for q, (c, v) in enumerate(case["queries"]):
        for t, x in zip(c, v):
            d = ids[indptr[t]:indptr[t + 1]]
            sp[q, d] = sp[q, d] + F32(x) * vals[indptr[t]:indptr[t + 1]]
    return dense, np.where(d2s >= 0, sp[:, np.clip(d2s, 0, None)], F32(0)).astype(F32)


def test_masked_route_calculator_against_the_unmasked_one_and_brute_force():
    case = H.integer_case()
    dense, sparse = _dense_sparse(case)
    N, d2s, n_s2d, w, k = case["N"], case["d2s"], len(case["s2d"]), (1.0, 1.0), 10
    tie = H.tie_of(d2s, n_s2d)
    everything = np.ones(N, bool)
    for depths in ((10,), (20, 80), (40, 160, 640)):
        a = H.expected_routes(dense, sparse, d2s, n_s2d, w, k, depths)
        b = HM.expected_routes(dense, sparse, d2s, n_s2d, w, k, depths, everything)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), depths
    fused = H.fuse(w, dense, sparse)
    assert all(np.array_equal(x, y) for x, y in zip(H.rank_rows(fused, tie, k), HM.rank_rows(fused, tie, k, everything)))
    # a subset: the rows are the allowed documents' own ranking, and both kinds of route occur
    rng = np.random.default_rng(5)
    allowed = rng.random(N) < 0.5
    pool = np.flatnonzero(allowed)
    route, union, hits = HM.expected_routes(dense, sparse, d2s, n_s2d, w, k, (10,), allowed)
    ids, sc, n = HM.rank_rows(fused, tie, k, allowed)
    assert allowed[ids].all() and (n == k).all() and (route == -1).any() and (hits[route == -1] > 0).all() and (hits[route >= 0] == 0).all()
    for q in range(len(fused)):
        o = pool[np.lexsort((tie[pool], -fused[q][pool].astype(np.float64)))[:k]]
        assert np.array_equal(ids[q], o)
    # 7 documents: complete at any depth >= 7, D = -FLT_MAX; no document: nothing to rank
    seven = np.zeros(N, bool)
    seven[pool[:7]] = True
    route, union, hits = HM.expected_routes(dense, sparse, d2s, n_s2d, w, k, (10,), seven)
    assert route.tolist() == [0] * len(fused) and (union == 7).all() and (hits == 0).all()
    assert HM.rank_rows(fused, tie, k, seven)[2].tolist() == [7] * len(fused)
    route, union, hits = HM.expected_routes(dense, sparse, d2s, n_s2d, w, k, (10,), np.zeros(N, bool))
    assert route.tolist() == [0] * len(fused) and not union.any() and not hits.any()
    ids, sc, n = HM.rank_rows(fused, tie, k, np.zeros(N, bool))
    assert (ids == -1).all() and (sc == -H.FLT_MAX).all() and not n.any()
