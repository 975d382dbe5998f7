"""GPU: search within a document subset (csrc/subset_search.hip: sr_dense_search_subset / sr_sparse_search_subset).  Every comparison
is for equal ids and equal score BITS.  Expected = the unrestricted search of the same handle with k = every document, filtered on the
host (_filter_full: keep the subset's documents in the order the search returned them, cut to k, pad); the dense test and the tiled
sparse test also rebuild it with tests/test_subset_host.py::subset_topk_spec from the documents' scores and require the two to agree.  Dense scores must also be the bits sr_dense_score_pairs returns for the pair.

The issue asks for a sparse index of 300 documents and 64 terms with one document of more than 1 024 postings.  A document has at most
one posting per term, so the two cannot hold in one index: the 300 x 64 index is tested as stated (with the forward index of the
certified scorer, so the pair route takes both of its ways), and a second index of 300 documents and 1 100 terms carries the document
with 1 030 postings, which keeps an index from having a forward index."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FMIN = np.float32(-3.402823466e38)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _filter_full(full_s, full_i, subset, k, pad_score, counts=None):
    """The unrestricted search's rows (k = every document) -> the subset's rows: the kept entries in the order they came, cut to k."""
    nq = full_s.shape[0]
    out_s = np.full((nq, k), pad_score, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    out_c = np.zeros(nq, np.int32)
    allowed = set(int(x) for x in subset)
    for q in range(nq):
        n = full_s.shape[1] if counts is None else int(counts[q])
        keep = [j for j in range(n) if int(full_i[q, j]) in allowed][:k]
        out_c[q] = len(keep)
        out_s[q, :len(keep)] = full_s[q, keep]
        out_i[q, :len(keep)] = full_i[q, keep]
    return out_s, out_i, out_c


# ------------------------------------------------------------------------------------------------------- dense ---
SEG = [(70, 0, 1), (129, 100, 3), (1, 1000, 1)]        # (rows, id_base, id_stride): 200 documents, ids 0..69, 100, 103, .., 484, 1000
GID = np.concatenate([b + s * np.arange(n, dtype=np.int64) for n, b, s in SEG])


def _dense_index(H, storage, batch_invariant):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    rng = np.random.default_rng(H)
    D = rng.standard_normal((200, H), dtype=np.float32)
    # duplicate rows: equal scores inside a subset, across the subset boundary and across segments
    D[80] = D[5]
    D[150] = D[5]
    D[199] = D[5]
    D[11] = D[10]
    D[69] = D[70]
    D[131] = D[130]
    if storage == "fp16":
        D = D.astype(np.float16).astype(np.float32)
    idx = DenseIndexHIP(H, row_dtype=storage)
    r0 = 0
    for n, b, s in SEG:
        idx.add_host_rows(D[r0:r0 + n], id_base=b, id_stride=s)
        r0 += n
    assert idx.ntotal == 200 and idx.stored_dtype() == storage
    if batch_invariant:
        idx.set_batch_invariant(True)
    return idx, D


def _dense_subsets():
    rng = np.random.default_rng(3)
    subs = {"empty": np.zeros(0, np.int64), "single": GID[150:151].copy(), "all": GID.copy()}
    for m in (63, 64, 65):                           # straddle the three segments; 5 and 80 in, 150 and 199 in or out by chance
        rows = np.sort(np.concatenate([[5, 10, 69, 70, 80, 130], rng.choice(np.setdiff1d(np.arange(200), [5, 10, 69, 70, 80, 130, 199]),
                                                                             m - 7, replace=False), [199]]))
        assert len(rows) == m and len(set(rows.tolist())) == m and rows[-1] == 199
        subs[f"m{m}"] = GID[rows]
    return subs


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("H,batch_invariant", [(320, False), (256, True)])
def test_dense_subset_equals_the_filtered_full_search(monkeypatch, H, batch_invariant, storage):
    from test_subset_host import subset_topk_spec
    idx, D = _dense_index(H, storage, batch_invariant)
    subs = _dense_subsets()
    rng = np.random.default_rng(17)
    for nq in (1, 17, 70):                           # below one query block, one partial block, more than 64
        Q = torch.from_numpy(rng.standard_normal((nq, H), dtype=np.float32)).cuda()
        fs, fi = idx.search(Q, 200)
        fs, fi = fs.cpu().numpy(), fi.cpu().numpy()
        assert (fi >= 0).all() and len(set((fs[0, :]).tolist())) < 200          # the planted duplicates tie
        by_doc = np.empty((nq, 200), np.float32)         # score of every document, in GID's order
        for q in range(nq):
            by_doc[q, np.searchsorted(GID, fi[q])] = fs[q]
        for name, sub in subs.items():
            m = len(sub)
            for k in sorted({1, 10, max(1, m), m + 5}):
                s, i = idx.search(Q, k, subset=sub)
                s, i = s.cpu().numpy(), i.cpu().numpy()
                es, ei, _ = _filter_full(fs, fi, sub, k, FMIN)
                ss, si, _ = subset_topk_spec(by_doc, GID, sub, k, FMIN)       # the specification of tests/test_subset_host.py
                assert np.array_equal(si, ei) and np.array_equal(_bits(ss), _bits(es)), (H, storage, nq, name, k)
                assert np.array_equal(i, ei), (H, storage, nq, name, k)
                assert np.array_equal(_bits(s), _bits(es)), (H, storage, nq, name, k)
            if m:
                # the bits of sr_dense_score_pairs for every returned pair (s, i: the k = m + 5 result)
                valid = i >= 0
                assert valid.sum() == nq * m
                indptr = np.concatenate([[0], np.cumsum(valid.sum(1))]).astype(np.int64)
                pairs = idx.score_pairs(Q, indptr, i[valid]).cpu().numpy()
                assert np.array_equal(_bits(pairs), _bits(s[valid])), (H, storage, nq, name)
    # Several slabs and several query sub-batches give the bits of one slab and one batch.  The smallest limit the handle accepts is
    # 1 MiB.  (a) 700 queries, k = 10: 8 bytes per (query, slab entry) leave 187 -> 128 entries per slab: two slabs for the 200 rows.
    # (b) 70 queries, k = m + 4096 (the largest k, through the large select): its 20 k bytes per query leave room for 11 queries per
    # batch - seven sub-batches -, and the dev switch SR_SUBSET_MAX_SLAB=64 cuts every batch's subset into slabs of 64 as well.
    Qa = torch.from_numpy(rng.standard_normal((700, H), dtype=np.float32)).cuda()
    Qb = Qa[:70].contiguous()
    cases = [(Qa, "all", 10, None), (Qa, "m65", 10, "64"), (Qb, "all", 200 + 4096, "64"), (Qb, "m65", 70, "64")]
    want = [idx.search(Q, k, subset=subs[name]) for Q, name, k, _ in cases]
    fs, fi = idx.search(Qb, 200)
    es, ei, _ = _filter_full(fs.cpu().numpy(), fi.cpu().numpy(), subs["all"], 200 + 4096, FMIN)
    assert np.array_equal(want[2][1].cpu().numpy(), ei) and np.array_equal(_bits(want[2][0].cpu().numpy()), _bits(es))
    idx.set_workspace_limit(1 << 20)
    try:
        for (Q, name, k, max_slab), (ws, wi) in zip(cases, want):
            if max_slab:
                monkeypatch.setenv("SR_SUBSET_MAX_SLAB", max_slab)
            else:
                monkeypatch.delenv("SR_SUBSET_MAX_SLAB", raising=False)
            s, i = idx.search(Q, k, subset=subs[name])
            assert torch.equal(i, wi) and torch.equal(s.view(torch.int32), ws.view(torch.int32)), (name, k)
    finally:
        idx.set_workspace_limit(4 << 30)
        monkeypatch.delenv("SR_SUBSET_MAX_SLAB", raising=False)
    s, i = idx.search(Qb, 70, subset=subs["m65"])
    assert torch.equal(i, want[3][1])


def test_dense_subset_rejects_bad_lists_and_stays_usable():
    idx, D = _dense_index(256, "fp32", True)
    Q = torch.from_numpy(np.random.default_rng(5).standard_normal((3, 256), dtype=np.float32)).cuda()
    good = np.array([3, 69, 100, 103, 484, 1000], np.int64)
    want_s, want_i = idx.search(Q, 4, subset=good)
    for bad, pos in [(np.array([3, 69, 103, 100, 484], np.int64), 3),          # a descending pair
                     (np.array([3, 69, 69, 100], np.int64), 2),                  # a repeated id
                     (np.array([3, 69, 100, 101, 484], np.int64), 3),            # between two strided ids: in no segment
                     (np.array([3, 70, 100], np.int64), 1),                      # in the gap between two segments
                     (np.array([-1, 3], np.int64), 0),
                     (np.array([3, 1000, 1001], np.int64), 2)]:                  # past the last segment
        with pytest.raises(ValueError, match=f"position {pos}\\b"):
            idx.search(Q, 4, subset=bad)
        # one valid call gives the right answer
        s, i = idx.search(Q, 4, subset=good)
        assert torch.equal(i, want_i) and torch.equal(s, want_s)
    fs, fi = idx.search(Q, 200)
    es, ei, _ = _filter_full(fs.cpu().numpy(), fi.cpu().numpy(), good, 4, FMIN)
    assert np.array_equal(want_i.cpu().numpy(), ei) and np.array_equal(_bits(want_s.cpu().numpy()), _bits(es))


# ------------------------------------------------------------------------------------------------------ sparse ---
N_DOCS = 300


def _sparse_index(V, long_doc, n_docs=N_DOCS):
    """CSR by term over n_docs (300) documents; term V - 1 has no posting; long_doc: document 17 has a posting in 1 030 terms."""
    rng = np.random.default_rng(V)
    lists_i, lists_v = [], []
    for t in range(V):
        n = 0 if t == V - 1 else int(rng.integers(3, (120 if V <= 64 else 12) * n_docs // N_DOCS))
        di = np.sort(rng.choice(n_docs, n, replace=False)).astype(np.int32)
        if long_doc and t < 1030 and 17 not in di:
            di = np.sort(np.append(di, np.int32(17)))
        lists_i.append(di)
        # a coarse grid of values: equal scores (ties) between documents are common
        lists_v.append((rng.integers(1, 5, len(di)) * 0.5).astype(np.float32))
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in lists_i])]).astype(np.int64)
    ids, vals = np.concatenate(lists_i).astype(np.int32), np.concatenate(lists_v).astype(np.float32)
    if long_doc:
        assert int((ids == 17).sum()) > 1024
    return indptr, ids, vals


def _sparse_queries(V):
    rng = np.random.default_rng(V + 1)
    qs = []
    for n in (1, 5, 20, 40, 3, 12):                  # ascending, distinct terms
        c = np.sort(rng.choice(V - 1, min(n, V - 1), replace=False)).astype(np.int32)
        qs.append((c, (rng.integers(1, 7, len(c)) * 0.25).astype(np.float32)))
    c = rng.choice(V - 1, 10, replace=False).astype(np.int32)
    c = np.concatenate([c, c[:4], [-1, V + 5], c[2:3]]).astype(np.int32)        # unordered, repeated and out-of-range term ids
    qs.append((c, (rng.integers(1, 7, len(c)) * 0.25).astype(np.float32)))
    qs.append((np.array([V - 1], np.int32), np.array([1.0], np.float32)))       # no match: the term has no posting
    qs.append((np.zeros(0, np.int32), np.zeros(0, np.float32)))                 # no term at all
    assert len(qs) == 9
    return qs


def _csr(queries):
    qi = np.concatenate([[0], np.cumsum([len(c) for c, _ in queries])]).astype(np.int64)
    return qi, np.concatenate([c for c, _ in queries]), np.concatenate([v for _, v in queries])


def _sparse_subsets():
    rng = np.random.default_rng(4)
    subs = {"empty": np.zeros(0, np.int64), "single": np.array([17], np.int64), "all": np.arange(N_DOCS, dtype=np.int64)}
    for m in (63, 64, 65):
        subs[f"m{m}"] = np.sort(np.concatenate([[0, 17, N_DOCS - 1], rng.choice(np.arange(1, N_DOCS - 1)[np.arange(1, N_DOCS - 1) != 17],
                                                                              m - 3, replace=False)])).astype(np.int64)
    return subs


@pytest.mark.parametrize("V,long_doc", [(64, False), (1100, True)])
def test_sparse_subset_equals_the_filtered_full_search_on_both_routes(monkeypatch, V, long_doc):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    monkeypatch.setenv("SR_SPARSE_CERT", "1")        # the certified scorer's forward index at this size as well (where the index qualifies)
    indptr, ids, vals = _sparse_index(V, long_doc)
    idx = SparseIndexHIP(indptr, ids, vals, N_DOCS)
    # V = 64: the index has the forward index, so the pair route takes its forward way for the queries with ascending valid terms and the
    # posting lists for the others; a document of more than 1 024 postings: no forward index, posting lists only
    assert idx.cert_stats()["present"] == (0 if long_doc else 1)
    subs = _sparse_subsets()
    queries = _sparse_queries(V)
    for nq in (1, 9):
        qi, qc, qv = _csr(queries[:nq] if nq > 1 else queries[2:3])
        monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE", raising=False)
        s0 = idx.search(qi, qc, qv, N_DOCS)[0].cpu().numpy()
        mid = float(np.median(s0[0][s0[0] > 0]))     # a threshold that cuts the first query's list in the middle
        for thr in (0.0, mid):
            fs, fi, fc = [x.cpu().numpy() for x in idx.search(qi, qc, qv, N_DOCS, threshold=thr)]
            assert 0 < fc[0] <= N_DOCS
            for name, sub in subs.items():
                m = len(sub)
                for k in sorted({1, 10, max(1, m), m + 5}):
                    es, ei, ec = _filter_full(fs, fi, sub, k, np.float32(0), counts=fc)
                    for route, pair_way in (("pairs", None), ("pairs", "postings"), ("array", None)):
                        monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", route)
                        if pair_way:                 # the pair route through the posting lists for every query
                            monkeypatch.setenv("SR_PAIR_SPARSE_ROUTE", pair_way)
                        try:
                            s, i, c = [x.cpu().numpy() for x in idx.search(qi, qc, qv, k, threshold=thr, subset=sub)]
                        finally:
                            monkeypatch.delenv("SR_PAIR_SPARSE_ROUTE", raising=False)
                        assert np.array_equal(c, ec), (V, nq, thr, name, k, route, pair_way)
                        assert np.array_equal(i, ei), (V, nq, thr, name, k, route, pair_way)
                        assert np.array_equal(_bits(s), _bits(es)), (V, nq, thr, name, k, route, pair_way)
    # the rule's own choice, global ids (id_base / id_stride), and - k = 8 000 under the smallest limit the handle accepts, 1 MiB: the
    # large select's 20 k bytes per query leave room for 6 of the 9 queries per batch; SR_SUBSET_MAX_SLAB=64 cuts the pair route's subset
    # into slabs as well - the same rows
    monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE", raising=False)
    qi, qc, qv = _csr(queries)
    fs, fi, fc = [x.cpu().numpy() for x in idx.search(qi, qc, qv, N_DOCS, id_base=7, id_stride=3)]
    for name in ("m65", "all"):
        for k in (20, 8000):
            es, ei, ec = _filter_full(fs, fi, 7 + 3 * subs[name], k, np.float32(0), counts=fc)
            for limit, max_slab in ((4 << 30, None), (1 << 20, "64")):
                idx.set_workspace_limit(limit)
                if max_slab:
                    monkeypatch.setenv("SR_SUBSET_MAX_SLAB", max_slab)
                try:
                    s, i, c = [x.cpu().numpy() for x in idx.search(qi, qc, qv, k, id_base=7, id_stride=3, subset=subs[name])]
                finally:
                    idx.set_workspace_limit(4 << 30)
                    monkeypatch.delenv("SR_SUBSET_MAX_SLAB", raising=False)
                assert np.array_equal(c, ec) and np.array_equal(i, ei) and np.array_equal(_bits(s), _bits(es)), (name, k, limit)
    # one query's buffers beyond the limit: SR_ERR_NOMEM before anything runs
    idx.set_workspace_limit(1 << 20)
    try:
        with pytest.raises(MemoryError, match="workspace"):
            idx.search(qi, qc, qv, 100000, subset=subs["all"])
    finally:
        idx.set_workspace_limit(4 << 30)


def test_sparse_subset_over_several_doc_tiles(monkeypatch):
    """The array route works per tile of 8 192 documents.  20 000 documents are three tiles (the last one partial): subsets with entries
    in tiles 0 and 2 and none in tile 1 (that tile's workgroups leave early), with entries on both sides of both tile edges, and one of
    more than 8 192 entries, so that a slab smaller than the subset makes the host launch the tiles one at a time, each launch followed by
    a compaction that raises tau.  Both routes against the filtered full search: ids, score bits, counts."""
    from test_subset_host import subset_topk_spec
    from scaling_retriever_amd.scoring import SparseIndexHIP
    monkeypatch.setenv("SR_SPARSE_CERT", "1")
    N, V, T = 20000, 64, 8192
    indptr, ids, vals = _sparse_index(V, False, n_docs=N)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    assert idx.cert_stats()["present"] == 1
    rng = np.random.default_rng(6)
    t0, t1, t2 = np.arange(0, T), np.arange(T, 2 * T), np.arange(2 * T, N)
    subs = {
        "tiles_0_and_2": np.sort(np.concatenate([[0, T - 1, 2 * T, N - 1], rng.choice(t0[1:-1], 900, replace=False),
                                                 rng.choice(t2[1:-1], 700, replace=False)])),
        "edges": np.sort(np.concatenate([[T - 1, T, 2 * T - 1, 2 * T], rng.choice(t0[:-1], 500, replace=False),
                                         rng.choice(t1[1:-1], 500, replace=False), rng.choice(t2[1:], 500, replace=False)])),
        "tile_1_only": np.sort(rng.choice(t1, 1300, replace=False)),
        "large": np.sort(np.concatenate([[T - 1, T, 2 * T - 1, 2 * T], rng.choice(np.setdiff1d(np.arange(N), [T - 1, T, 2 * T - 1, 2 * T]),
                                                                                  15000, replace=False)])),
    }
    for name, sub in subs.items():
        subs[name] = sub.astype(np.int64)
        assert len(set(sub.tolist())) == len(sub)
    assert not ((subs["tiles_0_and_2"] >= T) & (subs["tiles_0_and_2"] < 2 * T)).any() and len(subs["large"]) > T
    qi, qc, qv = _csr(_sparse_queries(V))
    monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE", raising=False)
    s0 = idx.search(qi, qc, qv, N)[0].cpu().numpy()
    mid = float(np.median(s0[0][s0[0] > 0]))
    for thr in (0.0, mid):
        fs, fi, fc = [x.cpu().numpy() for x in idx.search(qi, qc, qv, N, threshold=thr)]
        # the documents' scores as an array (those the search did not return score <= thr: any such value serves), for the specification
        dense_scores = np.full((9, N), np.float32(thr), np.float32)
        for q in range(9):
            dense_scores[q, fi[q, :fc[q]]] = fs[q, :fc[q]]
        for name, sub in subs.items():
            for k in (20, 8000):
                es, ei, ec = _filter_full(fs, fi, sub, k, np.float32(0), counts=fc)
                ss, si, sc = subset_topk_spec(dense_scores, np.arange(N), sub, k, np.float32(0), threshold=thr)
                assert np.array_equal(si, ei) and np.array_equal(_bits(ss), _bits(es)) and np.array_equal(sc, ec), (thr, name, k)
                # unlimited; a slab of 8 192 entries (one tile per launch for the large subset); the same under the smallest workspace limit
                for route, limit, max_slab in (("pairs", 4 << 30, None), ("array", 4 << 30, None), ("array", 4 << 30, "8192"),
                                               ("array", 1 << 20, "8192"), (None, 4 << 30, None)):
                    if route:
                        monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", route)
                    else:                            # the rule's own choice: every one of these subsets holds at least n_docs / 16 entries
                        monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE", raising=False)
                    if max_slab:
                        monkeypatch.setenv("SR_SUBSET_MAX_SLAB", max_slab)
                    idx.set_workspace_limit(limit)
                    try:
                        s, i, c = [x.cpu().numpy() for x in idx.search(qi, qc, qv, k, threshold=thr, subset=sub)]
                    finally:
                        idx.set_workspace_limit(4 << 30)
                        monkeypatch.delenv("SR_SUBSET_MAX_SLAB", raising=False)
                    assert np.array_equal(c, ec), (thr, name, k, route, limit, max_slab)
                    assert np.array_equal(i, ei), (thr, name, k, route, limit, max_slab)
                    assert np.array_equal(_bits(s), _bits(es)), (thr, name, k, route, limit, max_slab)


def test_sparse_subset_rejects_bad_lists_and_stays_usable(monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    indptr, ids, vals = _sparse_index(64, False)
    idx = SparseIndexHIP(indptr, ids, vals, N_DOCS)
    qi, qc, qv = _csr(_sparse_queries(64))
    good = np.array([0, 17, 40, 299], np.int64)
    for route in ("pairs", "array"):
        monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", route)
        want = [x.cpu().numpy() for x in idx.search(qi, qc, qv, 3, subset=good)]
        for bad, pos in [(np.array([0, 40, 17, 299], np.int64), 2),         # a descending pair
                         (np.array([0, 17, 17], np.int64), 2),               # a repeated position
                         (np.array([0, 17, 300], np.int64), 2),              # a position >= n_docs
                         (np.array([-1, 17], np.int64), 0)]:
            with pytest.raises(ValueError, match=f"position {pos}\\b"):
                idx.search(qi, qc, qv, 3, subset=bad)
            got = [x.cpu().numpy() for x in idx.search(qi, qc, qv, 3, subset=good)]
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
    fs, fi, fc = [x.cpu().numpy() for x in idx.search(qi, qc, qv, N_DOCS)]
    es, ei, ec = _filter_full(fs, fi, good, 3, np.float32(0), counts=fc)
    assert np.array_equal(want[1], ei) and np.array_equal(_bits(want[0]), _bits(es)) and np.array_equal(want[2], ec)


# ------------------------------------------------------------------------------------------------ Python layer ---
def test_search_knn_with_allowed_ids():
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    rng = np.random.default_rng(21)
    H, n = 64, 90
    embs = rng.standard_normal((n, H), dtype=np.float32)
    embs[40] = embs[3]
    pids = [f"p{7 * i}" for i in range(n)]
    index = DenseFlatIndexer()
    index.init_index(H)
    index.index_data(embs[:50], pids[:50])
    index.index_data(embs[50:], pids[50:])
    q = rng.standard_normal((5, H), dtype=np.float32)
    full_ids, full_scores = index.search_knn(q, n)
    allowed = [pids[j] for j in (40, 3, 77, 3, 12, 55, 89, 0)]               # any order, with a duplicate
    ids, scores = index.search_knn(q, 10, allowed_ids=allowed)
    for r in range(5):
        keep = [j for j in range(n) if full_ids[r][j] in set(allowed)][:10]
        assert ids[r] == [full_ids[r][j] for j in keep] + [None] * (10 - len(keep))
        assert np.array_equal(_bits(scores[r, :len(keep)]), _bits(full_scores[r, keep]))
        assert (scores[r, len(keep):] == FMIN).all()
    s2, p2 = index.search_arrays(q, 10, allowed_ids=allowed)
    assert np.array_equal(_bits(s2), _bits(scores)) and p2[0, 0] in (0, 3, 12, 40, 55, 77, 89)
    assert index.search_knn(q, 3, allowed_ids=[])[0] == [[None] * 3] * 5
    with pytest.raises(ValueError, match="p5"):
        index.search_knn(q, 10, allowed_ids=["p7", "p5"])
    # the default is unchanged
    again_ids, again_scores = index.search_knn(q, n)
    assert again_ids == full_ids and np.array_equal(again_scores, full_scores)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from golden_weights import make_weights
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    return cfg, make_weights(cfg, int(z["weight_seed"]))


def test_sparse_retrieve_with_allowed_ids(tiny, tmp_path):
    from test_indexer_gpu import FakeLoader, _corpus
    from scaling_retriever_amd.indexer import SparseIndexer, SparseRetrieval
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    cfg, w = tiny
    V = cfg["vocab_size"]
    rng = np.random.default_rng(1)
    docs, queries = _corpus(rng, 50, V, 1, 6), _corpus(rng, 7, V, 1, 3)
    pids, qids = [f"p{i}" for i in range(len(docs))], [f"q{i}" for i in range(len(queries))]
    model = LlamaBiSparse.from_weights(cfg, w, precision="bf16").to("cuda").eval()
    index_dir = str(tmp_path / "index")
    SparseIndexer(model, index_dir=index_dir, compute_stats=True, dim_voc=model.vocab_size, device="cuda").index(
        FakeLoader(docs, pids, batch_size=8, pad_id=V - 1))

    def retriever(name):
        return SparseRetrieval(config={"index_dir": index_dir, "out_dir": str(tmp_path / name)}, model=model, compute_stats=True,
                               dim_voc=model.vocab_size, device="cuda")
    loader = lambda: FakeLoader(queries, qids, batch_size=4, pad_id=V - 1)      # noqa: E731
    full = retriever("full").retrieve(loader(), topk=50, threshold=0.0).to_dict()
    allowed = [f"p{j}" for j in (49, 3, 8, 3, 21, 30, 31, 44, 0, 17, 26)]
    res = retriever("sub").retrieve(loader(), topk=5, threshold=0.0, allowed_ids=allowed)
    want = {}
    for qid, row in full.items():
        kept = [(d, s) for d, s in row.items() if d in set(allowed)][:5]
        if kept:                                      # a query without a hit has no entry, as in the unrestricted run
            want[qid] = dict(kept)
    assert len(want) >= 3
    got = res.to_dict()
    assert got == want and all(list(got[q]) == list(want[q]) for q in want)
    assert (tmp_path / "sub" / "run.json").read_text() == json.dumps(want)
    assert "L0_q" in json.load(open(tmp_path / "sub" / "q_stats.json"))
    with pytest.raises(ValueError, match="p999"):
        retriever("bad").retrieve(loader(), topk=5, allowed_ids=["p1", "p999"])
