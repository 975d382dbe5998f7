"""GPU: the exact hybrid search (scaling_retriever_amd/hybrid.py over csrc/hybrid_fuse.hip).  Every comparison is for equal bits:
sr_hybrid_union against np.union1d, sr_hybrid_rank against np.lexsort over numpy float32 fused scores, and hybrid.search_fused against
the brute-force ranking of both heads' pair scores over ALL documents (existing entry points, pinned elsewhere to the CPU oracle), with
the route of every query as tests/hybrid_cases.py calculates it."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import hybrid_cases as H

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------- union ---
def _maps(rng, N, n_sparse):
    """d2s / s2d of N dense documents of which n_sparse (a random choice, in random order) have a sparse position."""
    s2d = rng.permutation(N)[:n_sparse].astype(np.int64)
    d2s = np.full(N, -1, np.int64)
    d2s[s2d] = np.arange(n_sparse)
    return d2s, s2d


def _check_union(got, A_rows, B_rows, d2s, s2d):
    indptr, dpos, spos, tie = (t.cpu().numpy() for t in got)
    assert indptr[0] == 0 and len(indptr) == len(A_rows) + 1 and indptr[-1] == len(dpos) == len(spos) == len(tie)
    for q, (a, b) in enumerate(zip(A_rows, B_rows)):
        want = np.union1d(a[a >= 0], s2d[b])
        assert np.array_equal(dpos[indptr[q]:indptr[q + 1]], want), q
    assert np.array_equal(spos, d2s[dpos])
    assert np.array_equal(tie, np.where(spos >= 0, spos, len(s2d) + dpos))


def test_union_of_small_rectangular_lists():
    from scaling_retriever_amd.scoring import hybrid_union
    rng = np.random.default_rng(1)
    N, n_sparse, nq, kd, ks = 60, 50, 5, 8, 8
    d2s, s2d = _maps(rng, N, n_sparse)
    B = np.stack([rng.choice(n_sparse, ks, replace=False) for _ in range(nq)]).astype(np.int64)
    counts = np.array([8, 8, 0, 8, 3], np.int32)                       # row 2: an empty sparse row; row 4: counts < ks
    A = np.empty((nq, kd), np.int64)
    A[0] = rng.permutation(s2d[B[0]])                                  # full overlap
    A[1] = rng.choice(np.setdiff1d(np.arange(N), s2d[B[1]]), kd, replace=False)      # disjoint (with documents that have no posting)
    A[2] = rng.choice(N, kd, replace=False)
    A[3] = np.concatenate([rng.choice(N, 5, replace=False), [-1, -1, -1]])           # -1 padding in A
    A[4] = np.concatenate([s2d[B[4][:2]], rng.choice(N, 6, replace=False)])          # may repeat a document: the union keeps it once
    got = hybrid_union(_cuda(A), _cuda(B), _cuda(counts), _cuda(s2d), _cuda(d2s))
    _check_union(got, list(A), [B[q][:counts[q]] for q in range(nq)], d2s, s2d)
    assert (d2s[A[1]] < 0).any()                                       # the tie rule of a document without a posting was exercised
    # nq = 0 is legal
    e = hybrid_union(torch.zeros((0, kd), dtype=torch.int64, device="cuda"), torch.zeros((0, ks), dtype=torch.int64, device="cuda"),
                     torch.zeros((0,), dtype=torch.int32, device="cuda"), _cuda(s2d), _cuda(d2s))
    assert e[0].cpu().tolist() == [0] and e[1].numel() == 0


def test_union_at_the_lds_limit():
    from scaling_retriever_amd.scoring import hybrid_union
    rng = np.random.default_rng(2)
    N, n_sparse, nq = 12000, 9000, 3
    d2s, s2d = _maps(rng, N, n_sparse)
    # the limit, then the other sizes of the two in-LDS sorts (256 threads): a single pair, fewer pairs than threads, one and two a thread
    for kd, ks in ((4096, 4096), (2, 2), (256, 512), (512, 1024), (1024, 256)):
        A = np.stack([rng.choice(N, kd, replace=False) for _ in range(nq)]).astype(np.int64)
        A[1, rng.choice(kd, min(100, kd // 2), replace=False)] = -1
        B = np.stack([rng.choice(n_sparse, ks, replace=False) for _ in range(nq)]).astype(np.int64)
        counts = np.array([ks, ks - 1, ks], np.int32)
        got = hybrid_union(_cuda(A), _cuda(B), _cuda(counts), _cuda(s2d), _cuda(d2s))
        _check_union(got, list(A), [B[q][:counts[q]] for q in range(nq)], d2s, s2d)
    with pytest.raises(ValueError, match="4097"):                      # one more does not fit the in-LDS sort
        hybrid_union(torch.zeros((1, 4097), dtype=torch.int64, device="cuda"), _cuda(B[:1]), _cuda(counts[:1]), _cuda(s2d), _cuda(d2s))


def test_union_with_an_ascending_csr_list():
    from scaling_retriever_amd.scoring import hybrid_union
    rng = np.random.default_rng(3)
    N, n_sparse, ks = 50000, 30000, 40
    d2s, s2d = _maps(rng, N, n_sparse)
    lens = [0, 1, 20000, 300]
    A_rows = [np.sort(rng.choice(N, n, replace=False)).astype(np.int64) for n in lens]
    a_indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    B = np.stack([rng.choice(n_sparse, ks, replace=False) for _ in lens]).astype(np.int64)
    B[2, :15] = d2s[A_rows[2][d2s[A_rows[2]] >= 0][:15]]               # entries of B that are in A
    counts = np.array([40, 40, 40, 0], np.int32)
    got = hybrid_union(_cuda(np.concatenate(A_rows)), _cuda(B), _cuda(counts), _cuda(s2d), _cuda(d2s), a_indptr=_cuda(a_indptr))
    _check_union(got, A_rows, [B[q][:counts[q]] for q in range(len(lens))], d2s, s2d)


def test_union_names_a_sparse_position_without_a_dense_document():
    from scaling_retriever_amd.scoring import hybrid_union
    rng = np.random.default_rng(4)
    N, n_sparse, nq, kd, ks = 60, 50, 3, 8, 8
    d2s, s2d = _maps(rng, N, n_sparse)
    s2d_hole = s2d.copy()
    s2d_hole[37] = -1                                                  # the inverted index holds a document the dense index does not
    A = np.stack([rng.choice(N, kd, replace=False) for _ in range(nq)]).astype(np.int64)
    B = np.stack([rng.choice(np.setdiff1d(np.arange(n_sparse), [37]), ks, replace=False) for _ in range(nq)]).astype(np.int64)
    counts = np.full(nq, ks, np.int32)
    bad = B.copy()
    bad[1, 5] = 37
    with pytest.raises(ValueError, match=r"sparse position 37 \(query 1, entry 5"):
        hybrid_union(_cuda(A), _cuda(bad), _cuda(counts), _cuda(s2d_hole), _cuda(d2s))
    bad[1, 5] = n_sparse + 3                                           # outside s2d
    with pytest.raises(ValueError, match=f"sparse position {n_sparse + 3}"):
        hybrid_union(_cuda(A), _cuda(bad), _cuda(counts), _cuda(s2d_hole), _cuda(d2s))
    # beyond the row's count it is not read, and the library stays usable
    bad[1, 5] = 37
    counts[1] = 5
    got = hybrid_union(_cuda(A), _cuda(bad), _cuda(counts), _cuda(s2d_hole), _cuda(d2s))
    _check_union(got, list(A), [bad[q][:counts[q]] for q in range(nq)], d2s, s2d)


# -------------------------------------------------------------------------------------------------------- rank ---
@pytest.mark.parametrize("w", [(1.0, 1.0), (0.3, 2.0)])
@pytest.mark.parametrize("k", [1, 10, 4096, 256, 512, 1024])   # the kept keys' sort (256 threads): k = 1 is a single pair, 4096 the limit
def test_rank_equals_lexsort_with_certificate_and_threshold(k, w):
    from scaling_retriever_amd.scoring import hybrid_rank
    rng = np.random.default_rng(10 * k + int(10 * w[0]))
    id_end, n_sparse = 60000, 40000
    d2s, s2d = _maps(rng, id_end, n_sparse)
    lens = sorted({n for n in (0, 1, k - 1, k, k + 1, 8192, 50000) if n >= 0})
    lens = lens + [max(k, 64), max(k, 64), max(k, 64)]                 # three more rows for the certificate: equality, just below, complete
    nq = len(lens)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dpos = np.concatenate([np.sort(rng.choice(id_end, n, replace=False)) for n in lens]).astype(np.int64)
    spos = d2s[dpos]
    tie = np.where(spos >= 0, spos, n_sparse + dpos)
    dense = (np.round(rng.standard_normal(len(dpos)) * 8) / 4 + 0.0).astype(F32)      # multiples of 0.25: ties decide most ranks
    sparse = (np.round(np.abs(rng.standard_normal(len(dpos))) * 8) / 4).astype(F32)
    sparse_in = sparse.copy()
    sparse_in[spos < 0] = 77.0                                          # must be ignored: no posting means 0.0
    fused = H.fuse(w, dense, np.where(spos >= 0, sparse, F32(0)))
    want_ids, want_sc, want_n, Fk = [], [], [], []
    for q in range(nq):
        sl = slice(indptr[q], indptr[q + 1])
        o = np.lexsort((tie[sl], -fused[sl].astype(np.float64)))[:k]
        want_ids.append(dpos[sl][o]); want_sc.append(fused[sl][o]); want_n.append(len(o))
        Fk.append(fused[sl][o[k - 1]] if len(o) >= k else None)
    D = (np.round(rng.standard_normal(nq) * 8) / 4).astype(F32)
    S = (np.round(np.abs(rng.standard_normal(nq)) * 8) / 4).astype(F32)
    complete = np.zeros(nq, bool)
    eq, below, comp = nq - 3, nq - 2, nq - 1
    # B == F_k exactly must not certify; one float less does
    S[eq] = S[below] = 0
    if w == (1.0, 1.0):
        D[eq] = Fk[eq]
        D[below] = np.nextafter(F32(Fk[below]), F32(-np.inf))
        assert H.fuse(w, D[eq], S[eq]) == Fk[eq]
    D[comp], S[comp], complete[comp] = 100.0, 100.0, True               # B far above F_k, yet certified: the dense list was complete
    out = hybrid_rank(_cuda(indptr), _cuda(dpos), _cuda(spos), _cuda(tie), _cuda(dense), _cuda(sparse_in), w, k, _cuda(D), _cuda(S),
                      _cuda(complete), n_sparse, id_end)
    got_s, got_i, got_n, got_c, got_t = (t.cpu().numpy() for t in out)
    assert got_s.shape == got_i.shape == (nq, k)
    for q in range(nq):
        n = want_n[q]
        assert got_n[q] == n, (q, lens[q])
        assert np.array_equal(got_i[q, :n], want_ids[q]), (q, lens[q])
        assert np.array_equal(_bits(got_s[q, :n]), _bits(want_sc[q])), (q, lens[q])
        assert (got_i[q, n:] == -1).all() and (got_s[q, n:] == -H.FLT_MAX).all()
        assert bool(got_c[q]) == H.certified(w, Fk[q], D[q], S[q], complete[q]), (q, lens[q])
        thr = got_t[q]
        if Fk[q] is None:
            assert thr == -np.inf
        else:
            print(f"k={k} w={w} q={q} len={lens[q]} Fk={Fk[q]} S={S[q]} thr={thr}")
            assert thr == -np.inf or H.fuse(w, np.nextafter(F32(thr), F32(np.inf)), S[q]) >= Fk[q] > H.fuse(w, thr, S[q]), (q, thr)
            if thr == -np.inf:
                assert H.fuse(w, -H.FLT_MAX, S[q]) >= Fk[q]
        assert _bits(thr) == _bits(H.range_threshold(w, Fk[q], S[q])), (q, thr)
    if w == (1.0, 1.0):
        assert not got_c[eq] and got_c[below]
    assert got_c[comp]


def test_rank_limits():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import hybrid_rank
    z64, zf = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.float32, device="cuda")
    indptr = _cuda(np.array([0, 4], np.int64))
    one = torch.zeros(1, dtype=torch.float32, device="cuda")
    args = lambda tie, k: (indptr, z64, z64, tie, zf, zf, (1.0, 1.0), k, one, one, one.bool(), 10, 10)      # noqa: E731
    with pytest.raises(_lib.SrHipError, match="4097"):
        hybrid_rank(*args(_cuda(np.arange(4, dtype=np.int64)), 4097))
    with pytest.raises(ValueError, match="tie 20"):                     # outside [0, n_s2d + id_end)
        hybrid_rank(*args(_cuda(np.array([0, 1, 20, 3], np.int64)), 2))
    s, i, n, c, t = hybrid_rank(*args(_cuda(np.array([3, 2, 1, 0], np.int64)), 2))       # all fused scores equal: the ties decide
    assert n.cpu().tolist() == [2] and s.cpu().tolist() == [[0.0, 0.0]]
    e = hybrid_rank(_cuda(np.zeros(1, np.int64)), z64[:0], z64[:0], z64[:0], zf[:0], zf[:0], (1.0, 1.0), 5, zf[:0], zf[:0], zf[:0].bool(), 10, 10)
    assert e[0].shape == (0, 5)


# -------------------------------------------------------------------------------------------------- end to end ---
class _Indexes:
    """Both resident indexes of a hybrid_cases case, and the brute-force pair scores of every (query, document)."""

    def __init__(self, case, precision="fp32"):
        from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP
        self.case = case
        self.dense = DenseIndexHIP(case["rows"].shape[1])
        self.dense.add_host_rows(case["rows"])
        if precision != "fp32":
            self.dense.set_precision(precision)
        indptr, ids, vals = case["index"]
        self.n_sparse = len(case["s2d"])
        self.sparse = SparseIndexHIP(indptr, ids, vals, self.n_sparse)
        self.d2s, self.s2d = _cuda(case["d2s"]), _cuda(case["s2d"])
        self.Q = _cuda(case["Q"])
        self.csr = tuple(_cuda(a) for a in H.query_csr(case["queries"]))
        nq, N = case["Q"].shape[0], case["N"]
        every = np.arange(nq + 1, dtype=np.int64) * N
        self.dense_all = self.dense.score_pairs(self.Q, every, np.tile(np.arange(N, dtype=np.int64), nq)).cpu().numpy().reshape(nq, N)
        d2s = case["d2s"]
        sp = self.sparse.score_pairs(*self.csr, every, np.tile(np.clip(d2s, 0, None), nq)).cpu().numpy().reshape(nq, N)
        self.sparse_all = np.where(d2s >= 0, sp, F32(0)).astype(F32)
        self.tie = H.tie_of(d2s, self.n_sparse)

    def search(self, rows, k, w, depths, **kw):
        from scaling_retriever_amd import hybrid
        rows = np.asarray(rows)
        sub = H.query_csr([self.case["queries"][r] for r in rows])
        return hybrid.search_fused(self.dense, self.sparse, self.d2s, self.s2d, self.Q[_cuda(rows)], *(_cuda(a) for a in sub), k, weights=w,
                                   depths=depths, **kw)

    def check(self, rows, k, w, depths, **kw):
        """search_fused over the given queries equals brute force - ids, score bits, counts - and reports the calculated routes."""
        rows = np.asarray(rows)
        got_s, got_i, got_n, stats = self.search(rows, k, w, depths, **kw)
        want_i, want_s, want_n = H.rank_rows(H.fuse(w, self.dense_all[rows], self.sparse_all[rows]), self.tie, k)
        assert np.array_equal(got_n, want_n)
        assert np.array_equal(got_i, want_i), np.flatnonzero((got_i != want_i).any(1))
        assert np.array_equal(_bits(got_s), _bits(want_s))
        route, union, hits = H.expected_routes(self.dense_all[rows], self.sparse_all[rows], self.case["d2s"], self.n_sparse, w, k, depths)
        assert np.array_equal(stats["depth"], route), (stats["depth"], route)
        assert np.array_equal(stats["union"], union) and np.array_equal(stats["range_hits"], hits)
        return got_s, got_i, got_n, stats


@functools.lru_cache(maxsize=None)
def _family():
    return _Indexes(H.family_case())


@pytest.mark.parametrize("w", [(1.0, 1.0), (0.3, 2.0), (1.0, 0.0), (0.0, 1.0)])
def test_search_fused_equals_brute_force_on_every_route(w):
    ix = _family()
    k, depths = 10, (40, 160, 640)
    before = ix.dense.batch_invariant
    a = ix.check(np.arange(24), k, w, depths)
    if w == (1.0, 1.0):                                                 # a condition on the inputs: each route serves a query
        assert {0, 1, -1} <= set(a[3]["depth"].tolist()), a[3]["depth"]
        assert a[3]["depth"].tolist() == [0] * 8 + [1] * 8 + [-1] * 8
    rows70 = np.arange(70) % 24                                         # more than 64 queries: the other dense accumulation path
    b = ix.check(rows70, k, w, depths)
    assert np.array_equal(b[1], a[1][rows70]) and np.array_equal(_bits(b[0]), _bits(a[0][rows70])) and np.array_equal(b[2], a[2][rows70])
    assert np.array_equal(b[3]["depth"], a[3]["depth"][rows70])
    assert ix.dense.batch_invariant == before


def test_search_fused_range_route_in_sub_batches_and_its_memory_error():
    ix = _family()
    k, depths, w = 10, (40,), (1.0, 1.0)
    whole = ix.check(np.arange(24), k, w, depths)
    hits = whole[3]["range_hits"]
    assert (whole[3]["depth"] == -1).sum() >= 8
    budget = int((hits.max() + 40) * 64 * 2)                            # two of the longest lists at most: several sub-batches
    parts = ix.check(np.arange(24), k, w, depths, fallback_bytes=budget)
    assert np.array_equal(parts[1], whole[1]) and np.array_equal(_bits(parts[0]), _bits(whole[0]))
    q_big = int(np.argmax(hits))
    with pytest.raises(MemoryError, match=f"query {q_big} "):
        ix.search(np.arange(24), k, w, depths, fallback_bytes=int((hits.max() + 40) * 64 - 1))


def test_search_fused_small_batch_of_a_dim_256_index_restores_batch_invariance():
    rng = np.random.default_rng(21)
    case = H.integer_case(seed=9, N=900, dim=256, nq=8)
    case["rows"] = (case["rows"] * rng.uniform(0.5, 1.5, case["rows"].shape)).astype(F32)       # real-valued: the accumulation order shows
    ix = _Indexes(case)
    for start in (False, True):
        ix.dense.set_batch_invariant(start)
        ix.check(np.arange(8), 10, (1.0, 0.5), (20, 80))
        assert ix.dense.batch_invariant == start


@pytest.mark.parametrize("precision", ["fp32", "fp32_filtered"])
def test_search_fused_on_an_integer_valued_index(precision):
    ix = _Indexes(H.integer_case(), precision)
    for w, depths in [((1.0, 1.0), (10,)), ((1.0, 1.0), (20, 80)), ((1.0, 2.0), (10, 40)), ((2.0, 1.0), None)]:
        got = ix.check(np.arange(16), 10, w, depths if depths is not None else (40, 160, 640, 2560))
        if depths is None:                                              # the default schedule is the same call
            dflt = ix.search(np.arange(16), 10, w, None)
            assert dflt[3]["depths"] == (40, 160, 640, 2560) and np.array_equal(dflt[1], got[1])
    routes = ix.check(np.arange(16), 10, (1.0, 1.0), (10,))[3]["depth"]
    assert (routes == -1).any()
    # 70 queries (the large-batch dense path) return the same rows
    rows70 = np.arange(70) % 16
    a, b = ix.check(np.arange(16), 10, (1.0, 1.0), (20, 80)), ix.check(rows70, 10, (1.0, 1.0), (20, 80))
    assert np.array_equal(b[1], a[1][rows70]) and np.array_equal(_bits(b[0]), _bits(a[0][rows70]))


def test_search_fused_edge_cases():
    rng = np.random.default_rng(31)
    N, dim, V = 7, 64, 12
    d2s = np.array([2, -1, 0, 4, -1, 1, 3], np.int64)                   # documents 1 and 4 have no posting
    s2d = np.array([2, 5, 0, 6, 3], np.int64)
    postings = {t: (np.sort(rng.choice(5, 3, replace=False)).astype(np.int32), rng.uniform(0.5, 2.0, 3).astype(F32)) for t in range(V)}
    queries = [(np.array([1, 4, 7], np.int32), np.array([1.0, 0.5, 2.0], F32)),
               (np.zeros(0, np.int32), np.zeros(0, F32)),               # an empty sparse row
               (np.array([0], np.int32), np.array([1.0], F32))]
    case = dict(rows=rng.standard_normal((N, dim), dtype=F32), Q=rng.standard_normal((3, dim), dtype=F32), index=H.sparse_csr(postings, V),
                queries=queries, d2s=d2s, s2d=s2d, N=N, V=V)
    ix = _Indexes(case)
    s, i, n, stats = ix.check(np.arange(3), 10, (1.0, 1.0), (10, 40))    # N = 7 < k: every document, then padding
    assert n.tolist() == [7, 7, 7] and (i[:, 7:] == -1).all() and (s[:, 7:] == -H.FLT_MAX).all()
    assert all(sorted(r[:7].tolist()) == list(range(7)) for r in i)
    assert stats["depth"].tolist() == [0, 0, 0]                         # certified: the dense list is complete
    ix.check(np.arange(3), 3, (1.0, 1.0), (3,))
    ix.check(np.arange(3), 3, (0.5, 3.0), (3, 5))
    ix.dense.set_precision("bf16x3")
    with pytest.raises(ValueError, match="bf16x3"):
        ix.search(np.arange(3), 3, (1.0, 1.0), (3,))
    ix.dense.set_precision("fp32")
    for bad in ((2,), (5000,), ()):                                     # below k, beyond sr_max_topk(), empty
        with pytest.raises(ValueError, match="depth"):
            ix.search(np.arange(3), 3, (1.0, 1.0), bad)
    with pytest.raises(ValueError, match="sr_max_topk"):
        ix.search(np.arange(3), 5000, (1.0, 1.0), None)
    e = ix.search(np.arange(0), 3, (1.0, 1.0), (3,))
    assert e[0].shape == (0, 3) and e[2].shape == (0,)


def test_rows_certified_at_depth_k_equal_the_torch_route_of_retrieve_fused():
    """depths = (k,): the candidates are exactly the union retrieve_fused ranks.  Both heads are given the SAME top-k set in different
    orders (the dedicated term's k largest values are those of the dense top-k, reversed), so F_k = min over the set of dense + sparse
    > D_k + S_k and every query is certified at depth 0 by the strict inequality; the rows must be those of retrieve_fused's torch
    route (torch.unique, drop_repeats, rank_candidates - restated by tools/bench_hybrid.py) on the same lists."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from bench_hybrid import torch_rank, torch_union
    rng = np.random.default_rng(41)
    N, dim, V, nq, k, w = 500, 64, 16, 6, 10, (1.0, 1.0)
    rows, Q = rng.standard_normal((N, dim), dtype=F32), rng.standard_normal((nq, dim), dtype=F32)
    a = Q.astype(np.float64) @ rows.astype(np.float64).T
    a = (a - a.mean(1, keepdims=True)) / a.std(1, keepdims=True)
    s2d = rng.permutation(N).astype(np.int64)
    d2s = np.empty(N, np.int64)
    d2s[s2d] = np.arange(N)
    postings, queries = {}, []
    for q in range(nq):
        order = np.argsort(-a[q])
        v = np.empty(N)
        v[order] = 0.01 + 3.0 * (N - np.arange(N)) / N                  # strictly decreasing in the dense rank: the same top-k set ...
        top = order[:k]
        v[top] = v[top][::-1].copy()                                    # ... in the opposite order
        postings[q] = (np.arange(N, dtype=np.int32), v.astype(F32)[s2d])
        queries.append((np.array([q], np.int32), np.array([1.0], F32)))
    ix = _Indexes(dict(rows=rows, Q=Q, index=H.sparse_csr(postings, V), queries=queries, d2s=d2s, s2d=s2d, N=N, V=V))
    got_s, got_i, got_n, stats = ix.check(np.arange(nq), k, w, (k,))
    assert stats["depth"].tolist() == [0] * nq and stats["union"].tolist() == [k] * nq
    ds, dp = ix.dense.search(ix.Q, k)
    ss, sp, sc = ix.sparse.search(*ix.csr, k, threshold=0.0)
    indptr, dpos, spos, tie = torch_union(sp, sc, dp, ix.s2d, ix.d2s, N)
    dense_s = ix.dense.score_pairs(ix.Q, indptr, dpos)
    sparse_s = ix.sparse.score_pairs(*ix.csr, indptr, torch.clamp(spos, min=0))
    t_s, t_i, t_n = torch_rank(dense_s, sparse_s, dpos, spos, tie, indptr, w, k)
    assert t_n.cpu().tolist() == got_n.tolist()
    assert np.array_equal(t_i.cpu().numpy().reshape(nq, k), got_i) and np.array_equal(_bits(t_s.cpu().numpy().reshape(nq, k)), _bits(got_s))


# ------------------------------------------------------------------------------------- through the toy hybrid model ---
@pytest.fixture(scope="module")
def toy(golden_dir, tmp_path_factory):
    """The fixtures of tests/test_pair_scores_gpu.py's retrieve_fused test: a tiny LlamaBiHybrid, 90 documents, 8 queries."""
    from fake_tokenizer import FakeTokenizer
    from golden_weights import make_weights
    from torch.utils.data import DataLoader
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    from scaling_retriever_amd.indexer import HybridIndexer
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiHybrid
    from test_pipeline import ListDataset, _corpus
    tmp = tmp_path_factory.mktemp("hybrid_toy")
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    tok = FakeTokenizer(vocab_size=cfg["vocab_size"], padding_side="left")
    docs = ListDataset(_corpus(90, seed=1, max_words=20))
    queries = ListDataset([(f"q{i}", t) for i, (_, t) in enumerate(_corpus(8, seed=2, max_words=6))])
    collate_d, collate_q = LlamaSparseCollectionCollator(tok, 24), LlamaSparseCollectionCollator(tok, 8)
    hyb = LlamaBiHybrid.from_weights(cfg, w).to("cuda").eval()
    sp_dir, de_dir = str(tmp / "sp"), str(tmp / "de")
    HybridIndexer(hyb, sp_dir, de_dir, device="cuda", chunk_size=40, compute_stats=True,
                  dim_voc=hyb.vocab_size).index(DataLoader(docs, batch_size=16, shuffle=False, collate_fn=collate_d))
    q_loader = lambda: DataLoader(queries, batch_size=4, shuffle=False, collate_fn=collate_q)      # noqa: E731
    return hyb, sp_dir, de_dir, q_loader, tmp


def _retriever(toy, name):
    from scaling_retriever_amd.indexer import HybridRetriever
    hyb, sp_dir, de_dir, q_loader, tmp = toy
    return HybridRetriever(hyb, sp_dir, de_dir, str(tmp / name), dim_voc=hyb.vocab_size, device="cuda"), str(tmp / name)


def _brute_force_run(ret, sparse_q, dense_q, qids, w, k):
    """The exact fused top-k from both heads' score_candidates over ALL documents (existing entry points)."""
    all_ids = list(ret.dense_index.index_id_to_db_id)
    by_dense = ret.dense_index.score_candidates(dense_q, [all_ids] * len(qids), qids)
    in_sparse = [d for d in all_ids if ret.inverse_id_map().get(d) >= 0]
    by_sparse = ret.score_candidates(sparse_q, qids, [in_sparse] * len(qids))
    spos, n_s2d = ret.inverse_id_map(), int(ret._position_maps()[1].numel())
    out = {}
    for q in qids:
        rd, rs = by_dense[str(q)], (by_sparse[str(q)] if str(q) in by_sparse else {})
        d = np.array([rd[str(i)] for i in all_ids], F32)
        s = np.array([rs.get(str(i), 0.0) for i in all_ids], F32)
        f = H.fuse(w, d, s)
        tie = np.array([spos.get(i) if spos.get(i) >= 0 else n_s2d + p for p, i in enumerate(all_ids)])
        o = np.lexsort((tie, -f.astype(np.float64)))[:k]
        out[q] = ([str(all_ids[j]) for j in o], f[o])
    return out


def test_retrieve_fused_exact_through_the_toy_model(toy):
    w, k = (0.7, 1.3), 10
    ret_a, out_a = _retriever(toy, "a")
    ret_a.retrieve_fused(toy[3](), topk=k, weights=w)
    ret_b, out_b = _retriever(toy, "b")
    res, stats = ret_b.retrieve_fused_exact(toy[3](), k, weights=w)
    run = json.load(open(os.path.join(out_b, "fused_exact", "run.json")))
    assert run == {q: dict(r) for q, r in res.items()} and len(run) == 8
    sparse_q, dense_q, qids = ret_b._generate_query_vecs(toy[3]())
    want = _brute_force_run(ret_b, sparse_q, dense_q, qids, w, k)
    for q in qids:
        assert list(run[q].keys()) == want[q][0], q
        assert np.array_equal(np.array(list(run[q].values()), F32), want[q][1]), q
    assert stats["depths"] == (40, 160, 640, 2560) and (stats["depth"] >= 0).all()            # depth 160 holds all 90 documents: complete
    # retrieve_fused in the directory the exact run was written to: the three existing outputs are the bytes of the first directory
    ret_b.retrieve_fused(toy[3](), topk=k, weights=w)
    for head, name in (("sparse", "run.json"), ("sparse", "q_stats.json"), ("dense", "run.json"), ("fused", "run.json")):
        assert open(os.path.join(out_a, head, name), "rb").read() == open(os.path.join(out_b, head, name), "rb").read(), (head, name)
    assert json.load(open(os.path.join(out_b, "fused_exact", "run.json"))) == run


def test_certified_rows_equal_the_existing_fused_route(toy):
    """With depths = (k,) the candidates are retrieve_fused's union: every query the certificate covers has the same row there.  At
    k = 10 the certificate is rare (F_k > D_k + S_k at the lists' own depth; none of the 8 toy queries had it when this was written);
    at k = 90 = every document the dense list is complete and all 8 are certified."""
    w = (1.0, 1.0)
    ret, out = _retriever(toy, "c")
    sparse_q, dense_q, qids = ret._generate_query_vecs(toy[3]())
    for k in (10, 90):
        _, _, fused_res = ret.retrieve_fused(toy[3](), topk=k, weights=w)
        res, stats = ret.search_fused(sparse_q, dense_q, k, weights=w, depths=(k,), qids=qids)
        want = _brute_force_run(ret, sparse_q, dense_q, qids, w, k)
        n_certified = 0
        for r, q in enumerate(qids):
            assert list(res[q].keys()) == want[q][0], q                  # exact for every query, whatever the route
            if stats["depth"][r] == 0:
                n_certified += 1
                assert list(res[q].keys()) == list(fused_res[q].keys()), q
                assert np.array_equal(np.array(list(res[q].values()), F32), np.array(list(fused_res[q].values()), F32)), q
        print("k =", k, "certified at depth 0:", n_certified, "of", len(qids), stats["depth"].tolist())
    assert n_certified == len(qids)                                      # k = 90: the dense list holds every document
