"""CPU: the exact hybrid search's new C-ABI symbols, the argument checks that must come before any device work, and the numpy restatement
of the certificate and of the d* bisection (tests/hybrid_cases.py: the expected-route calculator of tests/test_hybrid_search_gpu.py)
against a brute-force scan over every float of a window."""
import ctypes
import os
import re

import numpy as np
import pytest

import hybrid_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_new_symbols_are_declared_exported_and_bound():
    from scaling_retriever_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("sr_hybrid_union", "sr_hybrid_rank"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    from scaling_retriever_amd import hybrid, scoring
    from scaling_retriever_amd.indexer import HybridRetriever
    assert callable(scoring.hybrid_union) and callable(scoring.hybrid_rank) and callable(hybrid.search_fused)
    assert callable(HybridRetriever.search_fused) and callable(HybridRetriever.retrieve_fused_exact)


def test_entry_points_validate_before_they_touch_a_device():
    """The pointers below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    total = ctypes.c_int64(-1)

    def union(**kw):
        a = dict(dict(a=p, ai=None, kd=8, b=p, bc=p, ks=8, s2d=p, ns=10, d2s=p, nd=10, nq=1, oi=p, od=p, os=p, ot=p, cap=16), **kw)
        return lib.sr_hybrid_union(a["a"], a["ai"], a["kd"], a["b"], a["bc"], a["ks"], a["s2d"], a["ns"], a["d2s"], a["nd"], a["nq"], a["oi"],
                                   a["od"], a["os"], a["ot"], a["cap"], ctypes.byref(total), None)
    for change, text in [(dict(nq=-1), b"bad nq"), (dict(oi=None), b"null pointer"), (dict(ks=4097), b"list B"), (dict(kd=4097), b"list A"),
                         (dict(ns=1 << 31, nd=1 << 31), b"32-bit tie"), (dict(cap=-1), b"bad capacity"), (dict(b=None), b"null pointer"),
                         (dict(d2s=None), b"null pointer")]:
        rc = union(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())

    def rank(**kw):
        a = dict(dict(ip=p, nq=1, wd=1.0, ws=1.0, k=10, ns=10, ie=10, D=p), **kw)
        return lib.sr_hybrid_rank(a["ip"], p, p, p, p, p, a["nq"], a["wd"], a["ws"], a["k"], a["D"], p, p, a["ns"], a["ie"], p, p, p, p, p, None)
    for change, text in [(dict(nq=-1), b"bad nq"), (dict(k=0), b"bad k"), (dict(wd=-1.0), b"weights"), (dict(ws=float("inf")), b"weights"),
                         (dict(wd=float("nan")), b"weights"), (dict(ns=1 << 31, ie=1 << 31), b"32-bit tie"), (dict(D=None), b"null pointer")]:
        rc = rank(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert rank(k=lib.sr_max_topk() + 1) == _lib.SR_ERR_UNSUPPORTED and b"sr_hybrid_rank" in lib.sr_last_error()
    assert rank(nq=0) == _lib.SR_OK


def test_weights_and_topk_are_checked_before_the_library_is_asked_for_a_device(monkeypatch):
    from scaling_retriever_amd import _lib, hybrid
    from scaling_retriever_amd.indexer import HybridRetriever

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    ret = object.__new__(HybridRetriever)               # no index behind it: the checks come first
    bad = [dict(topk=0), dict(topk=-3), dict(topk=2.5), dict(topk="ten"), dict(weights=(-1.0, 1.0)), dict(weights=(1.0, float("nan"))),
           dict(weights=(float("inf"), 1.0)), dict(weights=(1e39, 1.0)), dict(weights=("a", 1.0)), dict(weights=(None, 1.0)),
           dict(weights=(1.0,)), dict(weights=3.0)]
    for change in bad:
        a = dict(dict(topk=10, weights=(1.0, 1.0)), **change)
        with pytest.raises(ValueError):
            hybrid.check_arguments(a["topk"], a["weights"])
        with pytest.raises(ValueError):
            ret.search_fused(None, None, a["topk"], weights=a["weights"])
        with pytest.raises(ValueError):
            ret.retrieve_fused_exact(None, a["topk"], weights=a["weights"])
    assert hybrid.check_arguments(np.int64(7), (0, 2)) == (7, (0.0, 2.0))
    with pytest.raises(NotImplementedError):
        ret.search_fused(None, None, 10, allowed_ids=["d1"])
    with pytest.raises(NotImplementedError):
        ret.retrieve_fused_exact(None, 10, allowed_ids=["d1"])
    assert hybrid.default_depths(10, 4096) == (40, 160, 640, 2560) and hybrid.default_depths(1000, 4096) == (4000,)
    assert hybrid.default_depths(2000, 4096) == (2000,)


def test_sharded_classes_refuse_the_fused_search():
    from scaling_retriever_amd.distributed import ShardedDenseRetriever, ShardedSparseRetriever
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval
    for cls in (ShardedDenseRetriever, ShardedSparseRetriever, ShardedSparseRetrieval):
        with pytest.raises(NotImplementedError):
            cls.search_fused(object.__new__(cls), None, None, 10)


def test_ordered_image_of_the_floats():
    x = np.array([-np.inf, -H.FLT_MAX, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, H.FLT_MAX, np.inf], F32)
    o = H.f2ord(x)
    assert (np.diff(o.astype(np.int64)) > 0).all()
    assert np.array_equal(H.ord2f(o).view(np.uint32), x.view(np.uint32))
    assert int(o[5]) - int(o[4]) == 1 and int(o[3]) + 1 == int(o[4])            # neighbours in the image are neighbours among the floats


@pytest.mark.parametrize("w", [(1.0, 1.0), (0.3, 2.0), (2.5, 0.7), (1.0, 0.0), (0.0, 1.0)])
def test_bisection_and_certificate_agree_with_a_scan_over_every_float_of_a_window(w):
    """g(d) = fuse(w, d, S) over EVERY float32 of a window of 2^16 consecutive values around a centre: the bisection's d* must be the
    smallest float of the whole line with g(d*) >= F_k - inside the window where the scan finds the step there, and consistent with
    the window's ends where it does not - and the certificate must equal 'no float d <= D has g(d) >= F_k ... or F_k > g(D)'."""
    rng = np.random.default_rng(int(1000 * w[0] + 10 * w[1]))
    for centre, S in [(0.0, 0.0), (0.0, 1.25), (1.0, 3.0), (-2.5, 0.5), (37.0, 11.0), (1e-40, 2.0), (-1e-41, 0.0), (3e38, 1e37)]:
        lo = int(H.f2ord(F32(centre))) - (1 << 15)
        window = H.ord2f(np.arange(lo, lo + (1 << 16), dtype=np.uint64))
        assert (np.diff(window.astype(np.float64)) >= 0).all()
        g = H.fuse(w, window, F32(S))
        assert (g[1:] >= g[:-1]).all()                                          # monotone under round-to-nearest
        for Fk in np.unique(np.concatenate([g[rng.integers(0, len(g), 6)], [g[0], g[-1], np.nextafter(g[len(g) // 2], F32(np.inf))]])):
            thr = H.range_threshold(w, Fk, S)
            reach = np.flatnonzero(g >= Fk)
            if len(reach) == 0:                                                 # the step lies above the window
                assert thr >= window[-1]
            elif reach[0] == 0:                                                 # at or below its first float
                assert thr < window[0]
            else:
                assert thr.view(np.uint32) == window[reach[0] - 1].view(np.uint32), (w, centre, S, Fk)
            if np.isfinite(thr):
                assert H.fuse(w, np.nextafter(thr, F32(np.inf)), S) >= Fk > H.fuse(w, thr, S)
            # the certificate for every D of a sample of the window: F_k > g(D), strictly
            for i in rng.integers(0, len(window), 8):
                assert H.certified(w, Fk, window[i], S) == bool(Fk > g[i])
    assert H.certified(w, None, 0.0, 0.0) is False and H.certified(w, None, 0.0, 0.0, complete=True) is True
    assert H.range_threshold(w, None, 1.0) == -np.inf


def test_the_equality_row_does_not_certify():
    w = (1.0, 1.0)
    B = H.fuse(w, 2.0, 3.0)
    assert not H.certified(w, B, 2.0, 3.0) and H.certified(w, np.nextafter(B, F32(np.inf)), 2.0, 3.0)


def test_expected_routes_of_the_family_case_cover_all_three():
    """A condition on the inputs of the end-to-end GPU test, here from numpy's own float32 scores (the GPU test recomputes it from the
    pair scorers' bits): with weights (1, 1) the three families are served by depth 0, depth 1 and the range route."""
    case = H.family_case()
    dense = (case["Q"].astype(np.float64) @ case["rows"].astype(np.float64).T).astype(F32)
    indptr, ids, vals = case["index"]
    sp = np.zeros((len(case["Q"]), case["N"]), F32)
    for q, (c, v) in enumerate(case["queries"]):
        for t, x in zip(c, v):
            d = ids[indptr[t]:indptr[t + 1]]
            sp[q, d] = sp[q, d] + F32(x) * vals[indptr[t]:indptr[t + 1]]
    route, union, hits = H.expected_routes(dense, sp[:, case["d2s"]], case["d2s"], case["N"], (1.0, 1.0), 10, (40, 160, 640))
    assert route.tolist() == [0] * 8 + [1] * 8 + [-1] * 8
    assert (hits[route == -1] > 0).all() and (hits[route >= 0] == 0).all()
