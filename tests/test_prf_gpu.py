"""GPU: pseudo-relevance feedback (csrc/prf.hip) against the numpy model of tests/prf_cases.py - equal bits (uint32) of
every value, equal columns and row pointers - and the Python layers over the two kernels.  The sparse collection holds 50 documents
over 97 terms (128 256 where said), the dense index 300 rows."""
import numpy as np
import pytest
import torch

import prf_cases as M

pytestmark = pytest.mark.gpu
F32 = np.float32
V, N_DOCS, NQ, DEPTH = 97, 50, 6, 8

# query 0: an empty document (3), a one-posting document (4), a -0.0 value (5); 1: padding in mid-list; 2: a query without terms;
# 3: counts of 0; 4: the same document twice; 5: two valid entries only (n_pos above the valid count, g = 0 under a negative set)
FB = np.array([[3, 4, 5, 7, 9, 11, 13, 15],
               [-1, 6, -1, 8, 10, -1, 12, 14],
               [20, 21, 22, 23, 24, 25, 26, 27],
               [30, 31, 32, 33, 34, 35, 36, 37],
               [40, 40, 41, 42, 41, 43, 44, 45],
               [46, 47, 48, 49, 0, 1, 2, 3]], dtype=np.int64)
COUNTS = np.array([8, 8, 8, 0, 8, 2], dtype=np.int32)


def _cuda(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _feedback(q, d, fb, counts, n_terms=V, **kw):
    from scaling_retriever_amd.scoring import sparse_feedback
    got = sparse_feedback(*_cuda(q), *_cuda(d), n_terms, torch.from_numpy(fb).cuda(), None if counts is None else torch.from_numpy(counts).cuda(),
                          **kw)
    return [t.cpu().numpy() for t in got]


def _model(q, d, fb, counts, n_terms=V, n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=128):
    return M.rocchio_sparse(*q, *d, n_terms, fb, counts, n_pos, n_neg, alpha, beta, gamma, max_terms)


def _same_csr(got, want, what=""):
    for name, g, w in zip(("indptr", "cols", "vals"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if name == "vals":
            g, w = M.bits(g), M.bits(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, g[:12].tolist(), w[:12].tolist())


# --------------------------------------------------------------------------------------------------------- 1. the sparse kernel
@pytest.mark.parametrize("kw", [
    dict(n_pos=3, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=0),
    dict(n_pos=3, n_neg=2, alpha=1.0, beta=0.75, gamma=0.5, max_terms=0),
    dict(n_pos=10, n_neg=0, alpha=0.5, beta=1.0, gamma=0.0, max_terms=0),          # n_pos above every valid count
    dict(n_pos=3, n_neg=5, alpha=1.0, beta=0.75, gamma=0.25, max_terms=0),         # query 5: two valid entries, g = 0
    dict(n_pos=2, n_neg=3, alpha=1.0, beta=0.5, gamma=8.0, max_terms=0),           # gamma drives terms to w <= 0: dropped
    dict(n_pos=4, n_neg=0, alpha=0.0, beta=1.0, gamma=0.0, max_terms=0),
    dict(n_pos=3, n_neg=2, alpha=1.0, beta=0.75, gamma=0.5, max_terms=1),
    dict(n_pos=3, n_neg=2, alpha=1.0, beta=0.75, gamma=0.5, max_terms=5),
    dict(n_pos=8, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=1000),
])
def test_sparse_kernel_equals_the_model(kw):
    q, d = M.small_collection()
    want = _model(q, d, FB, COUNTS, **kw)
    _same_csr(_feedback(q, d, FB, COUNTS, **kw), want, kw)
    if kw["max_terms"] == 0 and kw["gamma"] == 8.0:
        free = _model(q, d, FB, COUNTS, **dict(kw, gamma=0.0))
        assert want[0][-1] < free[0][-1]                        # the negative set did drop terms
    if kw["max_terms"] == 0:                                    # counts of 0: alpha q alone
        assert want[0][4] - want[0][3] == (q[0][4] - q[0][3] if kw["alpha"] > 0 else 0)


def test_sparse_kernel_without_counts_and_budget_at_the_kept_count():
    q, d = M.small_collection()
    kw = dict(n_pos=3, n_neg=2, alpha=1.0, beta=0.75, gamma=0.5)
    free = _model(q, d, FB, None, max_terms=0, **kw)
    _same_csr(_feedback(q, d, FB, None, max_terms=0, **kw), free)
    kept = int(np.diff(free[0]).max())
    for m in (kept, kept + 1, kept - 1):
        _same_csr(_feedback(q, d, FB, None, max_terms=m, **kw), _model(q, d, FB, None, max_terms=m, **kw), m)
    _same_csr(_feedback(q, d, FB, None, max_terms=kept, **kw), free)


def test_sparse_budget_ties_go_to_the_lower_term():
    """Power-of-two values: w = 0.5 (A + B) is exact, three terms tie at 1.0 around the cut."""
    d = (np.array([0, 6, 10], dtype=np.int64), np.array([1, 5, 9, 20, 40, 60, 5, 9, 33, 60], dtype=np.int32),
         np.array([1, 2, 1, 2, 1, 1, 2, 1, 4, 1], dtype=F32))
    q = (np.array([0, 0], dtype=np.int64), np.zeros(0, np.int32), np.zeros(0, F32))
    fb = np.array([[0, 1]], dtype=np.int64)
    kw = dict(n_pos=2, n_neg=0, alpha=1.0, beta=1.0, gamma=0.0)
    got = _feedback(q, d, fb, None, max_terms=4, **kw)
    _same_csr(got, _model(q, d, fb, None, max_terms=4, **kw))
    assert got[1].tolist() == [5, 9, 20, 33] and got[2].tolist() == [2.0, 1.0, 1.0, 2.0]
    got = _feedback(q, d, fb, None, max_terms=3, **kw)
    assert got[1].tolist() == [5, 9, 33] and got[2].tolist() == [2.0, 1.0, 2.0]


def test_sparse_kernel_rejects_what_it_finds_on_the_device():
    q, d = M.small_collection()
    bad = (q[0], q[1].copy(), q[2])
    qi = int(np.flatnonzero(np.diff(q[0]) >= 2)[-1])
    a = int(q[0][qi])
    bad[1][a], bad[1][a + 1] = bad[1][a + 1], bad[1][a]         # two columns of one query swapped
    with pytest.raises(ValueError, match=f"query {qi} "):
        _feedback(bad, d, FB, COUNTS, n_pos=3)
    fb = FB.copy()
    fb[4, 2] = N_DOCS
    with pytest.raises(ValueError, match=f"id {N_DOCS} .query 4, entry 2"):
        _feedback(q, d, fb, COUNTS, n_pos=3)
    fb[4, 2] = 1 << 40
    with pytest.raises(ValueError, match="query 4, entry 2"):
        _feedback(q, d, fb, COUNTS, n_pos=1)                    # found although the entry is not used


def test_sparse_kernel_on_the_full_vocabulary():
    """Terms at and above 2^16 and up to V = 128 256."""
    big = 128256
    rng = np.random.default_rng(5)
    marks = np.array([0, 65535, 65536, 65537, 131071 % big, big - 1], dtype=np.int32)
    di, dc, dv = [0], [], []
    for r in range(N_DOCS):
        c = np.unique(np.concatenate([rng.choice(big, size=9, replace=False), rng.choice(marks, size=2, replace=False)])).astype(np.int32)
        dc.append(c)
        dv.append((np.round(rng.uniform(0.1, 2.0, size=c.size) * 64) / 64).astype(F32))
        di.append(di[-1] + c.size)
    d = (np.asarray(di, dtype=np.int64), np.concatenate(dc), np.concatenate(dv))
    qc = [np.unique(np.concatenate([rng.choice(big, size=4, replace=False), marks[i:i + 2]])).astype(np.int32) for i in range(4)]
    q = (np.concatenate([[0], np.cumsum([c.size for c in qc])]).astype(np.int64), np.concatenate(qc),
         rng.uniform(0.1, 2.0, size=sum(c.size for c in qc)).astype(F32))
    fb = rng.integers(0, N_DOCS, size=(4, DEPTH)).astype(np.int64)
    for kw in (dict(n_pos=5, n_neg=3, beta=0.75, gamma=0.25, max_terms=0), dict(n_pos=8, n_neg=0, max_terms=16)):
        got = _feedback(q, d, fb, None, n_terms=big, **kw)
        _same_csr(got, _model(q, d, fb, None, n_terms=big, **kw), kw)
    assert got[1].max() >= 65536


def test_sparse_kernel_with_the_largest_sets():
    """Also the sizes of the entry sort (sr_block_sort over the next power of two >= a query's entries, 256 threads): fewer pairs than
    threads (256), one pair per thread (512), two (1024), and the LDS cap of 8192 entries with documents of up to 97 terms."""
    rng = np.random.default_rng(9)
    fb = rng.integers(0, N_DOCS, size=(NQ, 128)).astype(np.int64)
    fb[1, 5::7] = -1
    counts = np.array([128, 128, 128, 127, 100, 64], dtype=np.int32)
    for doc_terms, n_set, slots in ((12, 64, {512, 1024}), (12, 20, {256, 512}), (97, 64, {8192})):
        q, d = M.small_collection(doc_terms=doc_terms)
        ent = M.entries(q[0], d[0], fb, counts, n_set, n_set)
        assert slots <= {1 << max(1, (e - 1).bit_length()) for e in ent} and max(ent) <= 8192, ent      # the inputs reach these sizes
        for m in (0, 32):
            kw = dict(n_pos=n_set, n_neg=n_set, alpha=1.0, beta=0.75, gamma=0.5, max_terms=m)
            _same_csr(_feedback(q, d, fb, counts, **kw), _model(q, d, fb, counts, **kw), (doc_terms, n_set, m))


def test_queries_at_and_above_the_entry_cap_take_the_other_route(monkeypatch):
    """SR_PRF_MAX_ENTRIES=64: a query of exactly 64 entries stays in LDS, one of 65 runs on the global workspace - the same rows as
    the uncapped call, whatever the route."""
    from scaling_retriever_amd import _lib
    q, d = M.small_collection()
    lens = np.diff(d[0])
    docs, total = [], 0
    for doc in range(6, N_DOCS):
        if total + lens[doc] <= 56:
            docs.append(doc)
            total += int(lens[doc])
    rng = np.random.default_rng(3)
    qc = [np.sort(rng.choice(V, size=n - total, replace=False)).astype(np.int32) for n in (64, 65, total + 5)]
    q2 = (np.concatenate([[0], np.cumsum([c.size for c in qc])]).astype(np.int64), np.concatenate(qc),
          rng.uniform(0.1, 2.0, size=sum(c.size for c in qc)).astype(F32))
    fb = np.tile(np.array(docs, dtype=np.int64), (3, 1))
    fb[2, 3:] = -1
    kw = dict(n_pos=len(docs), n_neg=0, alpha=1.0, beta=0.75, gamma=0.0)
    assert M.entries(q2[0], d[0], fb, None, len(docs), 0)[:2] == [64, 65]
    assert _lib.load().sr_prf_max_entries() >= 8192
    free = [_feedback(q2, d, fb, None, max_terms=m, **kw) for m in (0, 7)]
    base = [_feedback(q, d, FB, COUNTS, n_pos=3, n_neg=2, gamma=0.5, max_terms=m) for m in (0, 5)]
    monkeypatch.setenv("SR_PRF_MAX_ENTRIES", "64")
    assert _lib.load().sr_prf_max_entries() == 64
    for m, want in zip((0, 7), free):
        _same_csr(_feedback(q2, d, fb, None, max_terms=m, **kw), want, m)
        _same_csr(want, _model(q2, d, fb, None, max_terms=m, **kw), m)
    monkeypatch.setenv("SR_PRF_MAX_ENTRIES", "16")              # most queries of the base case on the workspace, the small ones in LDS
    for m, want in zip((0, 5), base):
        _same_csr(_feedback(q, d, FB, COUNTS, n_pos=3, n_neg=2, gamma=0.5, max_terms=m), want, m)


@pytest.mark.parametrize("fallback_bytes", [1 << 30, 3 * 4 * V * 2])
def test_sparse_kernel_equals_the_composition(fallback_bytes):
    from scaling_retriever_amd.prf import sparse_feedback_by_steps
    q, d = M.small_collection()
    for kw in (dict(n_pos=3, n_neg=2, alpha=1.0, beta=0.75, gamma=0.5, max_terms=0), dict(n_pos=10, n_neg=4, alpha=0.5, beta=1.0, gamma=2.0, max_terms=6)):
        got = sparse_feedback_by_steps(*_cuda(q), *_cuda(d), V, torch.from_numpy(FB).cuda(), torch.from_numpy(COUNTS).cuda(),
                                       fallback_bytes=fallback_bytes, **kw)
        _same_csr([t.cpu().numpy() for t in got], _feedback(q, d, FB, COUNTS, **kw), kw)


# ------------------------------------------------------------------------------------------------------- 2. the sparse index
_sparse = {}


def _sparse_index():
    """(SparseIndexHIP over the collection, its queries (none empty), the doc-major CSR)."""
    if not _sparse:
        from scaling_retriever_amd.scoring import SparseIndexHIP
        _, d = M.small_collection()
        q, _ = M.small_collection(seed=11, edge=False)
        t_indptr, t_docs, t_vals = M.transpose_csr(d[0], d[1], d[2], V)         # the doc-major CSR transposed: rows are terms
        _sparse["x"] = (SparseIndexHIP(t_indptr, t_docs, t_vals, N_DOCS), q, d, (t_indptr, t_docs, t_vals))
    return _sparse["x"]


def test_forward_rows_equal_the_numpy_transpose():
    idx, _, d, t = _sparse_index()
    want = M.transpose_csr(*t, N_DOCS)
    for _ in range(2):                                          # built, dropped, built again
        got = [x.cpu().numpy() for x in idx.forward_rows()]
        assert idx.forward_rows()[1] is idx.forward_rows()[1]
        _same_csr(got, want)
        _same_csr(got, d)
        idx.drop_forward_rows()


def test_sparse_search_prf_without_feedback_weight_is_the_plain_search():
    idx, q, _, _ = _sparse_index()
    want = idx.search(*q, 10)
    got = idx.search_prf(*q, 10, n_pos=5, alpha=1.0, beta=0.0, gamma=0.0, max_terms=0)
    for g, w in zip(got[:3], want):
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
    _same_csr([t.cpu().numpy() for t in got[3]], q)


def test_sparse_search_prf_is_search_feedback_search():
    idx, q, d, _ = _sparse_index()
    kw = dict(n_pos=4, n_neg=2, alpha=1.0, beta=0.75, gamma=0.25, max_terms=12)
    mask = np.ones(N_DOCS, dtype=bool)
    mask[::3] = False
    for filt in (dict(), dict(mask=mask), dict(subset=np.flatnonzero(mask).astype(np.int64))):
        got = idx.search_prf(*q, 7, fb_depth=9, threshold=0.0, **kw, **filt)
        s1, i1, c1 = idx.search(*q, 9, **filt)
        new = idx.feedback(*q, i1, c1, **kw)
        _same_csr([t.cpu().numpy() for t in new], _model(q, d, i1.cpu().numpy(), c1.cpu().numpy(), **kw), filt.keys())
        want = idx.search(*new, 7, **filt)
        for g, w in zip(got[:3], want):
            assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w)
        _same_csr([t.cpu().numpy() for t in got[3]], [t.cpu().numpy() for t in new])
        if filt:
            for ids, cnt in ((i1, c1), (got[1], got[2])):       # the feedback set and the result hold allowed documents only
                ids, cnt = ids.cpu().numpy(), cnt.cpu().numpy()
                assert all(mask[ids[r, :cnt[r]]].all() for r in range(ids.shape[0])) and cnt.max() > 0
    # per-query filters: every group's rows are those of its own mask
    masks = np.stack([mask, ~mask])
    group = np.arange(len(q[0]) - 1) % 2
    got = idx.search_prf(*q, 7, fb_depth=9, masks=masks, query_group=group, **kw)
    ids, cnt = got[1].cpu().numpy(), got[2].cpu().numpy()
    assert all(masks[group[r]][ids[r, :cnt[r]]].all() for r in range(ids.shape[0]))
    # id_base / id_stride map the final ids alone
    plain = idx.search_prf(*q, 7, fb_depth=9, **kw)
    moved = idx.search_prf(*q, 7, fb_depth=9, id_base=1000, id_stride=3, **kw)
    assert torch.equal(moved[0].view(torch.int32), plain[0].view(torch.int32)) and torch.equal(moved[2], plain[2])
    a, b, cnt = plain[1].cpu().numpy(), moved[1].cpu().numpy(), plain[2].cpu().numpy()
    assert all(np.array_equal(b[r, :cnt[r]], 1000 + 3 * a[r, :cnt[r]]) for r in range(a.shape[0])) and cnt.max() > 0
    _same_csr([t.cpu().numpy() for t in moved[3]], [t.cpu().numpy() for t in plain[3]])


# ------------------------------------------------------------------------------------------------------------- 3. the dense head
N1, N2, BASE2, STRIDE2 = 150, 150, 1000, 2
_dense = {}


def _dense_index(H, row_dtype):
    """(DenseIndexHIP of two segments, the second with strided ids; the global ids; {id: stored row as fp32}; queries)."""
    key = (H, row_dtype)
    if key not in _dense:
        from scaling_retriever_amd.scoring import DenseIndexHIP
        rng = np.random.default_rng(H + (7 if row_dtype == "fp16" else 0))
        D = rng.standard_normal((N1 + N2, H)).astype(F32)
        idx = DenseIndexHIP(H, row_dtype=row_dtype)
        idx.add_host_rows(D[:N1])
        idx.add_host_rows(D[N1:], id_base=BASE2, id_stride=STRIDE2)
        gid = np.concatenate([np.arange(N1, dtype=np.int64), BASE2 + STRIDE2 * np.arange(N2, dtype=np.int64)])
        stored = D.astype(np.float16).astype(F32) if row_dtype == "fp16" else D
        _dense[key] = (idx, gid, {int(g): stored[r] for r, g in enumerate(gid)}, rng.standard_normal((5, H)).astype(F32))
    return _dense[key]


@pytest.mark.parametrize("H,row_dtype", [(128, "fp32"), (128, "fp16"), (80, "fp32"), (80, "fp16"), (1040, "fp32"), (2064, "fp16")])
def test_dense_kernel_equals_the_model_and_the_composition(H, row_dtype):
    from scaling_retriever_amd.prf import dense_feedback_by_steps
    idx, gid, row_of, Q = _dense_index(H, row_dtype)
    rng = np.random.default_rng(H)
    fb = rng.choice(gid, size=(5, 12)).astype(np.int64)
    fb[1, [0, 4, 5]] = -1
    fb[2, 3] = fb[2, 1]                                         # the same document twice
    counts = np.array([12, 12, 12, 0, 2], dtype=np.int32)
    Qd, fbd, cd = torch.from_numpy(Q).cuda(), torch.from_numpy(fb).cuda(), torch.from_numpy(counts).cuda()
    for kw in (dict(n_pos=3, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0), dict(n_pos=4, n_neg=3, alpha=0.5, beta=0.75, gamma=0.25),
               dict(n_pos=64, n_neg=64, alpha=1.0, beta=1.0, gamma=1.0)):
        for c, cdev in ((counts, cd), (None, None)):
            want = M.rocchio_dense(Q, row_of.__getitem__, fb, c, **kw)
            got = idx.feedback(Qd, fbd, cdev, **kw)
            assert np.array_equal(M.bits(got.cpu().numpy()), M.bits(want)), (kw, c is None)
            steps = dense_feedback_by_steps(idx, Qd, fbd, cdev, **kw)
            assert torch.equal(steps.view(torch.int32), got.view(torch.int32)), (kw, c is None)
    bad = fb.copy()
    bad[2, 7] = BASE2 + 1                                       # between two strided ids: in no segment
    with pytest.raises(ValueError, match=f"id {BASE2 + 1} .query 2, entry 7"):
        idx.feedback(Qd, torch.from_numpy(bad).cuda(), None, n_pos=3)


@pytest.mark.parametrize("row_dtype", ["fp32", "fp16"])
def test_dense_search_prf(row_dtype):
    idx, gid, _, Q = _dense_index(128, row_dtype)
    Qd = torch.from_numpy(Q).cuda()
    want = idx.search(Qd, 10)
    got = idx.search_prf(Qd, 10, n_pos=5, alpha=1.0, beta=0.0, gamma=0.0)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
    assert torch.equal(got[2].view(torch.int32), Qd.view(torch.int32))
    kw = dict(n_pos=4, n_neg=2, alpha=1.0, beta=0.75, gamma=0.25)
    mask = np.zeros(int(gid.max()) + 1, dtype=bool)
    mask[gid[::2]] = True
    for filt in (dict(), dict(mask=mask)):
        got = idx.search_prf(Qd, 7, fb_depth=9, **kw, **filt)
        _, fb = idx.search(Qd, 9, **filt)
        new = idx.feedback(Qd, fb, None, **kw)
        want = idx.search(new, 7, **filt)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], want[1])
        assert torch.equal(got[2].view(torch.int32), new.view(torch.int32))
        if filt:
            assert mask[fb.cpu().numpy()].all() and mask[got[1].cpu().numpy()].all()


# ------------------------------------------------------------------------------------------------- 4. retrieval classes and CLI
def test_dense_flat_indexer_search_prf_maps_the_ids_back():
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    rng = np.random.default_rng(4)
    D = rng.standard_normal((90, 64)).astype(F32)
    ix = DenseFlatIndexer()
    ix.init_index(64)
    db_ids = [f"doc-{i}" for i in range(90)]
    ix.index_data(D[:50], db_ids[:50])
    ix.index_data(D[50:], db_ids[50:])
    q = rng.standard_normal((5, 64)).astype(F32)
    kw = dict(n_pos=4, n_neg=2, alpha=1.0, beta=0.75, gamma=0.25)
    allowed = [f"doc-{i}" for i in range(0, 90, 2)]
    for filt in (dict(), dict(allowed_ids=allowed)):
        _, pos = ix.search_arrays(q, 6, **filt)
        new = M.rocchio_dense(q, lambda d: D[d], pos, None, **kw)
        want_scores, want_pos = ix.search_arrays(new, 8, **filt)
        lists, scores, got_new = ix.search_prf(q, 8, fb_depth=6, **kw, **filt)
        assert np.array_equal(M.bits(got_new), M.bits(new)) and np.array_equal(M.bits(scores), M.bits(want_scores))
        assert lists == [[db_ids[p] for p in row] for row in want_pos]
    assert all(d in allowed for row in lists for d in row)
    with pytest.raises(ValueError, match="not both"):
        ix.search_prf(q, 8, allowed_ids=allowed, allowed_mask=np.ones(90, bool))
    with pytest.raises(ValueError, match="fb_depth = 4"):
        ix.search_prf(q, 8, **kw)


from test_hybrid_search_gpu import toy  # noqa: E402,F401  (the module-scoped fixture: a tiny LlamaBiHybrid, 90 documents, 8 queries)


class _SparseHead:
    """The sparse head of the toy hybrid model, as the model SparseRetrieval drives."""

    def __init__(self, hyb):
        self.hyb = hyb
        self.vocab_size = hyb.vocab_size

    def eval(self):
        return self

    def to(self, device):
        return self

    def encode(self, **inputs):
        return self.hyb.encode(**inputs)[0]


def test_retrieve_prf_through_the_toy_model(toy):  # noqa: F811
    import json
    import os
    from scaling_retriever_amd.indexer import HybridRetriever, SparseRetrieval
    hyb, sp_dir, de_dir, q_loader, tmp = toy
    out = str(tmp / "prf_sparse")
    ret = SparseRetrieval(_SparseHead(hyb), {"index_dir": sp_dir, "out_dir": out}, hyb.vocab_size, "cuda", compute_stats=True)
    ret.retrieve(q_loader(), topk=10)
    before = {n: open(os.path.join(out, n), "rb").read() for n in ("run.json", "q_stats.json")}
    kw = dict(n_pos=3, n_neg=2, alpha=1.0, beta=0.75, gamma=0.25, max_terms=16, fb_depth=6)
    res = ret.retrieve_prf(q_loader(), 10, **kw)
    assert {n: open(os.path.join(out, n), "rb").read() for n in before} == before
    run = json.load(open(os.path.join(out, "prf", "run.json")))
    assert run == {q: dict(r) for q, r in res.items()} and len(run) == 8
    q, qids = ret._generate_query_vecs(q_loader())
    s, i, c, new = ret.hip_index.search_prf(q.row_ptr, q.cols, q.vals, 10, **kw)
    s, i, c = s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()
    for r, qid in enumerate(qids):
        hits = run[str(qid)]
        assert list(hits) == [str(ret.doc_ids[int(p)]) for p in i[r, :c[r]]], qid
        assert np.array_equal(np.array(list(hits.values()), F32), s[r, :c[r]]), qid
    l0 = json.load(open(os.path.join(out, "prf", "q_stats.json")))["L0_q"]
    lens = np.diff(new[0].cpu().numpy())
    assert l0 == float(lens.mean()) and 0 < lens.max() <= 16
    assert json.load(open(os.path.join(out, "run.json"))) != run            # the feedback moved something
    hybrid = HybridRetriever(hyb, sp_dir, de_dir, str(tmp / "prf_hybrid"), dim_voc=hyb.vocab_size, device="cuda")
    with pytest.raises(NotImplementedError, match="per head"):
        hybrid.retrieve_prf(q_loader(), 10)


def test_eval_drivers_write_the_feedback_run_beside_the_plain_one(golden_dir, tmp_path):
    import json
    import os
    import sys
    from golden_weights import make_weights
    from test_eval_drivers import ROOT, _texts, _write_model
    sys.path.insert(0, ROOT)
    import eval_dense
    import eval_sparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    rng = np.random.default_rng(3)
    models = _write_model(str(tmp_path), cfg, w, rng)
    docs, queries = _texts(rng, 60, 3, 20), _texts(rng, 6, 2, 6)
    (tmp_path / "corpus.tsv").write_text("".join(f"d{i}\t{t}\n" for i, t in enumerate(docs)))
    (tmp_path / "queries.tsv").write_text("".join(f"q{i}\t{t}\n" for i, t in enumerate(queries)))
    corpus, query_path = str(tmp_path / "corpus.tsv"), str(tmp_path / "queries.tsv")

    def both(run_driver, names):
        plain, prf = str(tmp_path / (run_driver.__name__ + "_plain")), str(tmp_path / (run_driver.__name__ + "_prf"))
        run_driver(plain, [])
        run_driver(prf, ["--prf_depth", "3", "--prf_neg_depth", "2", "--prf_gamma", "0.25"])
        for n in names:
            assert open(os.path.join(prf, n), "rb").read() == open(os.path.join(plain, n), "rb").read(), n
        assert not os.path.exists(os.path.join(plain, "prf"))
        run, first = json.load(open(os.path.join(prf, "prf", "run.json"))), json.load(open(os.path.join(prf, "run.json")))
        assert list(run) == list(first) and all(0 < len(hits) <= 10 for hits in run.values())
        assert all(list(h.values()) == sorted(h.values(), reverse=True) for h in run.values())
        return prf

    lora = models["dense"][0]
    emb_dir = str(tmp_path / "embs")
    eval_dense.main(["--task_name", "write_doc_embeds", "--model_name_or_path", lora, "--corpus_path", corpus, "--doc_embed_dir", emb_dir,
                     "--eval_batch_size", "16", "--doc_max_length", "16", "--chunk_size", "32", "--token_budget", "0"])

    def dense(out, extra):
        eval_dense.main(["--task_name", "retrieval", "--model_name_or_path", lora, "--query_path", query_path, "--doc_embed_dir", emb_dir,
                         "--top_k", "10", "--query_max_length", "8", "--out_dir", out] + extra)
    both(dense, ["run.json"])

    lora_s = models["sparse"][0]
    index_dir = str(tmp_path / "sp_index")
    eval_sparse.main(["--task_name", "indexing", "--model_name_or_path", lora_s, "--corpus_path", corpus, "--index_dir", index_dir,
                      "--eval_batch_size", "8", "--doc_max_length", "16", "--token_budget", "0"])

    def sparse(out, extra):
        eval_sparse.main(["--task_name", "retrieval", "--model_name_or_path", lora_s, "--query_path", query_path, "--index_dir", index_dir,
                          "--top_k", "10", "--query_max_length", "8", "--out_dir", out] + extra + (["--prf_max_terms", "16"] if extra else []))
    prf = both(sparse, ["run.json", "q_stats.json"])
    assert 0 < json.load(open(os.path.join(prf, "prf", "q_stats.json")))["L0_q"] <= 16
