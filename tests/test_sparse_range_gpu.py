"""Sparse range search (sr_sparse_range_count / _fill, SparseIndexHIP.range_search, SparseRetrieval.range_search): every document
with score > thr[q], as CSR in document order.

Oracle: oracle.scoring.numba_score_float per (query, threshold) on the CPU, unknown terms dropped before the call.  lims, ids and
score bits are compared for EQUALITY, there is no tolerance anywhere and no case is left out.

Index shapes: V = 300 terms over n_docs = 100 (one partial tile), 8 192 (exactly one tile) and 32 805 (five tiles, the last partial).
Terms 0-9 are empty, 10-59 hold 1 to 10 postings, 60-62 have density 0.5 / 0.6 / 0.7 (a run inside one tile exceeds 1 024 postings:
several load groups) with values from a grid of sixteenths, so that many documents tie, term 63 has a posting in the very last
document, the rest are random lists of density 0.2 % - 5 % with random fp32 values.

Queries: 70, of 32, 0, 1, 70, 130 terms in turn (the last two cross a 64-term batch) in random (non-ascending) order; query 3 repeats
a term, query 4 carries the unknown ids -1, V and V + 5; weights are random, some negative, some zero.  nq = 1, 5 and 70 take the
first queries of that list.

Thresholds, one kind per query, rotated so that every nq meets every kind: 0.0; -1.0 (every document, zero scores included); the
query's exact 10th and 3 000th best score (the last document's where the index is smaller) - the 3 000th sits on a tie for the queries
whose matching documents are fewer, and among the grid-valued documents; a value above the maximum; +inf; -inf; NaN."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 300
SHAPES = (100, 8192, 32805)
NQ_ALL = 70
TERM_COUNTS = (32, 0, 1, 70, 130)
KINDS = 8
SENTINEL_S, SENTINEL_I = -12345.0, -777
_CACHE = {}


def _collection(n_docs):
    """(indptr int64 [V + 1], doc ids int32, vals fp32) by term, doc ids ascending inside a term; read-only."""
    key = ("coll", n_docs)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + n_docs)
        lists = []
        for t in range(V):
            if t < 10:
                n = 0
            elif t < 60:
                n = int(rng.integers(1, 11))
            elif t < 63:
                n = int(n_docs * (0.5, 0.6, 0.7)[t - 60])
            else:
                n = max(1, int(n_docs * rng.uniform(0.002, 0.05)))
            docs = np.sort(rng.choice(n_docs, size=min(n, n_docs), replace=False)).astype(np.int32)
            if t == 63 and docs[-1] != n_docs - 1:
                docs[-1] = n_docs - 1
            if 60 <= t < 63:
                vals = (rng.integers(1, 17, size=len(docs)) / 16.0).astype(np.float32)
            else:
                vals = rng.uniform(0.05, 3.0, size=len(docs)).astype(np.float32)
            lists.append((docs, vals))
        indptr = np.concatenate([[0], np.cumsum([len(d) for d, _ in lists])]).astype(np.int64)
        ids = np.concatenate([d for d, _ in lists]).astype(np.int32)
        vals = np.concatenate([v for _, v in lists]).astype(np.float32)
        for a in (indptr, ids, vals):
            a.setflags(write=False)
        per_tile = np.bincount(ids[indptr[60]:indptr[61]] // 8192)
        assert n_docs < 8192 or per_tile.max() > 1024
        assert ids[indptr[64] - 1] == n_docs - 1 and indptr[10] == 0
        _CACHE[key] = (indptr, ids, vals)
    return _CACHE[key]


def _queries():
    """[(cols int32, vals fp32)] * 70; read-only."""
    if "queries" not in _CACHE:
        rng = np.random.default_rng(77)
        out = []
        for q in range(NQ_ALL):
            n = TERM_COUNTS[q % len(TERM_COUNTS)]
            cols = rng.permutation(V)[:n].astype(np.int32)
            if n >= 32:                                   # the heavy terms take part: runs of several load groups
                for j, t in enumerate((60, 61)):
                    if t not in cols:
                        cols[(7 * q + 3 + 11 * j) % n] = t
            w = rng.normal(0.6, 1.0, size=n).astype(np.float32)
            w[rng.random(n) < 0.1] = 0.0
            if n == 1:
                cols[0] = (60, 61, 62, 63, 100, 5)[(q // 5) % 6]           # a heavy, a last-document, a random and an empty term
                w[0] = np.float32(1.5 if q % 2 == 0 else -0.75)
            if q == 3:
                cols[5] = cols[2]                         # the same term twice: counts each time
            if q == 4:
                cols[[1, 64, 100]] = (-1, V, V + 5)       # unknown ids: empty lists
            if n > 1:
                assert (np.diff(cols) < 0).any() and (w < 0).any()
            cols.setflags(write=False)
            w.setflags(write=False)
            out.append((cols, w))
        assert any((w == 0).any() for _, w in out)
        _CACHE["queries"] = out
    return _CACHE["queries"]


def _oracle(n_docs, q, thr):
    """(doc positions int64 ascending, scores fp32) of query q under threshold thr: numba_score_float, unknown terms dropped."""
    key = ("hits", n_docs, q, np.float32(thr).tobytes())
    if key not in _CACHE:
        from oracle import scoring as SC
        indptr, ids, vals = _collection(n_docs)
        cols, w = _queries()[q]
        known = (cols >= 0) & (cols < V)
        with np.errstate(invalid="ignore"):
            fi, neg = SC.numba_score_float(indptr, ids, vals, cols[known], w[known], np.float32(thr), n_docs)
        _CACHE[key] = (fi.astype(np.int64), (-neg).astype(np.float32))
    return _CACHE[key]


def _all_scores(n_docs, q):
    pos, s = _oracle(n_docs, q, -np.inf)
    assert len(pos) == n_docs
    return s


def _kth_best(n_docs, q, k):
    return np.sort(_all_scores(n_docs, q))[::-1][min(k, n_docs) - 1]


def _thresholds(n_docs, nq, rot=0):
    thr = np.empty(nq, np.float32)
    for q in range(nq):
        kind = (q + rot) % KINDS
        mx = _all_scores(n_docs, q).max()
        thr[q] = (0.0, -1.0, _kth_best(n_docs, q, 10), _kth_best(n_docs, q, 3000), np.nextafter(mx, np.float32(np.inf)),
                  np.inf, -np.inf, np.nan)[kind]
    return thr


def _expected(n_docs, thr, id_base=0, id_stride=1):
    lims = np.zeros(len(thr) + 1, np.int64)
    scores, ids = [], []
    for q, t in enumerate(thr):
        pos, s = _oracle(n_docs, q, t)
        lims[q + 1] = lims[q] + len(pos)
        scores.append(s)
        ids.append(id_base + pos * id_stride)
    return lims, np.concatenate(scores).astype(np.float32), np.concatenate(ids).astype(np.int64)


def _csr(nq):
    qs = _queries()[:nq]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in qs])]).astype(np.int64)
    cols = np.concatenate([c for c, _ in qs]).astype(np.int32)
    vals = np.concatenate([w for _, w in qs]).astype(np.float32)
    return indptr, cols, vals


def _index(n_docs):
    """One device index per shape, shared by the tests that do not change its settings."""
    key = ("index", n_docs)
    if key not in _CACHE:
        from scaling_retriever_amd.scoring import SparseIndexHIP
        _CACHE[key] = SparseIndexHIP(*(a.copy() for a in _collection(n_docs)), n_docs)
    return _CACHE[key]


def _assert_equal(got, want, what=""):
    lims, scores, ids = (t.cpu().numpy() for t in got)
    elims, escores, eids = want
    print(what, "total", int(lims[-1]), "expected", int(elims[-1]))
    assert np.array_equal(lims, elims), "lims differ"
    assert np.array_equal(ids, eids), "ids differ"
    assert np.array_equal(scores.view(np.int32), escores.view(np.int32)), "score bits differ"


@pytest.fixture
def chunk_tiles(monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("SR_SPARSE_RANGE_CHUNK_TILES", raising=False)
        else:
            monkeypatch.setenv("SR_SPARSE_RANGE_CHUNK_TILES", str(v))
    return set_


@pytest.mark.parametrize("chunk", [None, 2, 3])
@pytest.mark.parametrize("nq", [1, 5, NQ_ALL])
@pytest.mark.parametrize("n_docs", SHAPES)
def test_range_equals_oracle(n_docs, nq, chunk, chunk_tiles):
    chunk_tiles(chunk)
    idx = _index(n_docs)
    for rot in (range(KINDS) if nq < KINDS else (0,)):
        thr = _thresholds(n_docs, nq, rot)
        got = idx.range_search(*_csr(nq), thr)
        _assert_equal(got, _expected(n_docs, thr), f"n_docs={n_docs} nq={nq} chunk={chunk} rot={rot}")


@pytest.mark.parametrize("n_docs", [8192, 32805])
def test_scores_equal_score_pairs_and_two_calls_give_the_same_bytes(n_docs):
    idx = _index(n_docs)
    nq = NQ_ALL
    thr = _thresholds(n_docs, nq)
    got = idx.range_search(*_csr(nq), thr)
    assert int(got[0][-1]) > n_docs
    pairs = idx.score_pairs(*_csr(nq), got[0], got[2])
    assert torch.equal(pairs.view(torch.int32), got[1].view(torch.int32))
    again = idx.range_search(*_csr(nq), torch.from_numpy(thr))
    assert torch.equal(got[0], again[0]) and torch.equal(got[2], again[2])
    assert torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))


@pytest.mark.parametrize("thr", [0.0, -1.0])
def test_the_set_equals_a_search_with_k_of_the_collection(thr):
    n_docs, nq = 8192, 5
    idx = _index(n_docs)
    lims, scores, ids = (t.cpu().numpy() for t in idx.range_search(*_csr(nq), thr))
    fs, fi, fc = (t.cpu().numpy() for t in idx.search(*_csr(nq), n_docs, threshold=thr))
    assert lims[-1] > n_docs
    for q in range(nq):
        a = set(zip(ids[lims[q]:lims[q + 1]].tolist(), scores[lims[q]:lims[q + 1]].view(np.int32).tolist()))
        b = set(zip(fi[q, :fc[q]].tolist(), fs[q, :fc[q]].view(np.int32).tolist()))
        assert a == b and len(a) == fc[q] == lims[q + 1] - lims[q], q


def test_sorted_lists_are_prefixes_of_the_full_ranking():
    """sort=True: score descending, ties by ascending id = the first lims[q + 1] - lims[q] entries of search(k = n_docs) without a threshold."""
    n_docs, nq = 8192, 16
    idx = _index(n_docs)
    thr = _thresholds(n_docs, nq)
    thr[np.isneginf(thr)] = -1.0
    lims, scores, ids = (t.cpu().numpy() for t in idx.range_search(*_csr(nq), thr, sort=True))
    fs, fi, fc = (t.cpu().numpy() for t in idx.search(*_csr(nq), n_docs, threshold=float("-inf")))
    assert lims[-1] > n_docs and (fc == n_docs).all()
    for q in range(nq):
        c = lims[q + 1] - lims[q]
        assert np.array_equal(ids[lims[q]:lims[q + 1]], fi[q, :c]), q
        assert np.array_equal(scores[lims[q]:lims[q + 1]].view(np.int32), fs[q, :c].view(np.int32)), q


@pytest.mark.parametrize("id_base,id_stride", [(7, 3), ((1 << 32) + 5, 1), ((1 << 40), 1 << 12)])
def test_id_base_and_stride(id_base, id_stride):
    n_docs, nq = 32805, 5
    thr = _thresholds(n_docs, nq)
    got = _index(n_docs).range_search(*_csr(nq), thr, id_base=id_base, id_stride=id_stride)
    _assert_equal(got, _expected(n_docs, thr, id_base, id_stride), f"id_base={id_base} id_stride={id_stride}")
    with pytest.raises(ValueError):
        _index(n_docs).range_search(*_csr(nq), thr, id_base=-1)
    with pytest.raises(ValueError):
        _index(n_docs).range_search(*_csr(nq), thr, id_stride=0)


def test_workspace_limit_changes_the_chunking_not_the_result():
    """60 000 queries x 5 tiles x 4 bytes exceed the smallest limit (1 MiB): two tiles per chunk; the default limit keeps one.  The
    queries are the 70 of the list over and over, each under its 10th best score, and the first 70 lists are the oracle's.  Then
    270 000 queries, whose table does not fit even as one chunk: MemoryError naming the bytes."""
    from scaling_retriever_amd.scoring import SparseIndexHIP
    n_docs, reps = 32805, 858
    nq = NQ_ALL * reps
    indptr, cols, vals = _csr(NQ_ALL)
    big_indptr = np.concatenate([[0], np.cumsum(np.tile(np.diff(indptr), reps))]).astype(np.int64)
    big = (big_indptr, np.tile(cols, reps), np.tile(vals, reps))
    thr70 = np.array([_kth_best(n_docs, q, 10) for q in range(NQ_ALL)], np.float32)
    thr = np.tile(thr70, reps)
    assert 4 * nq * 5 > (1 << 20) >= 4 * nq * 3
    idx = SparseIndexHIP(*(a.copy() for a in _collection(n_docs)), n_docs)
    want = idx.range_search(*big, thr)
    elims, escores, eids = _expected(n_docs, thr70)
    assert elims[-1] > 200                               # up to 9 each, fewer where the 10th best score is tied
    _assert_equal((want[0][:NQ_ALL + 1], want[1][:elims[-1]], want[2][:elims[-1]]), (elims, escores, eids), "first 70")
    idx.set_workspace_limit(1 << 20)
    got = idx.range_search(*big, thr)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    n_big = 270000
    with pytest.raises(MemoryError, match=str(4 * n_big) + " bytes"):
        idx.range_search(np.zeros(n_big + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 0.0)
    idx.close()


def _raw(idx, nq, thr, capacity=None, pad=16, fill_thr=None, count=True, fill_nq=None):
    """count + fill through the C ABI with sentinel-filled outputs: (rc_count, rc_fill, total, lims, scores, ids)."""
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr
    dev = idx.device
    qp, qc, qv = (torch.from_numpy(a).to(dev) for a in _csr(max(nq, fill_nq or 0)))
    lims = torch.zeros(max(nq, fill_nq or 0) + 1, dtype=torch.int64, device=dev)
    total = ctypes.c_int64(-1)
    rc_count = idx.lib.sr_sparse_range_count(idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(thr), _ptr(lims), ctypes.byref(total),
                                             _lib.stream_ptr()) if count else None
    n = max(total.value, 0)
    scores = torch.full((n + pad,), SENTINEL_S, dtype=torch.float32, device=dev)
    ids = torch.full((n + pad,), SENTINEL_I, dtype=torch.int64, device=dev)
    rc_fill = idx.lib.sr_sparse_range_fill(idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq if fill_nq is None else fill_nq,
                                           _ptr(thr if fill_thr is None else fill_thr), _ptr(lims), 0, 1, _ptr(scores), _ptr(ids),
                                           n if capacity is None else capacity(n), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc_count, rc_fill, total.value, lims, scores, ids


def test_raw_abi_errors_and_edges():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import SparseIndexHIP
    n_docs, nq = 32805, 16
    idx = SparseIndexHIP(*(a.copy() for a in _collection(n_docs)), n_docs)          # a fresh handle: no count yet
    thr_np = _thresholds(n_docs, NQ_ALL)
    thr = torch.from_numpy(thr_np).to(idx.device)
    untouched = lambda s, i: bool((s == SENTINEL_S).all()) and bool((i == SENTINEL_I).all())

    # fill without a count
    rc_c, rc_f, _, _, s, i = _raw(idx, nq, thr, count=False)
    assert rc_f == _lib.SR_ERR_INVALID and b"count" in idx.lib.sr_last_error() and untouched(s, i)
    # the padding behind the result is never written
    rc_c, rc_f, total, lims, s, i = _raw(idx, nq, thr)
    assert rc_c == 0 and rc_f == 0 and total == int(lims[nq]) > n_docs and untouched(s[total:], i[total:])
    _assert_equal((lims[:nq + 1], s[:total], i[:total]), _expected(n_docs, thr_np[:nq]), "raw")
    # a fill with another nq
    rc_c, rc_f, total, _, s, i = _raw(idx, nq, thr, fill_nq=nq + 1)
    assert rc_c == 0 and rc_f == _lib.SR_ERR_INVALID and b"preceding count" in idx.lib.sr_last_error() and untouched(s, i)
    # capacity = total - 1
    rc_c, rc_f, total, _, s, i = _raw(idx, nq, thr, capacity=lambda n: n - 1)
    assert rc_c == 0 and rc_f == _lib.SR_ERR_INVALID and b"capacity" in idx.lib.sr_last_error() and untouched(s, i)
    # a fill with LOWER thresholds than the count's (every document a hit, the chunks of a query overrun into each other's slots):
    # whatever lands in query q's segment is a document of the index and a score of query q (two workgroups may write one slot, so
    # the two halves of a slot are checked separately); nothing lands outside the segments
    rc_c, rc_f, total, lims, s, i = _raw(idx, nq, thr, fill_thr=torch.full((nq,), -np.inf, device=idx.device))
    assert rc_c == 0 and rc_f == 0 and untouched(s[total:], i[total:])
    lims_h, s_h, i_h = lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy()
    for q in range(nq):
        seg_s, seg_i = s_h[lims_h[q]:lims_h[q + 1]], i_h[lims_h[q]:lims_h[q + 1]]
        wrote = seg_i != SENTINEL_I
        assert ((seg_i[wrote] >= 0) & (seg_i[wrote] < n_docs)).all(), q
        assert np.isin(seg_s.view(np.int32), np.append(_all_scores(n_docs, q), np.float32(SENTINEL_S)).view(np.int32)).all(), q
        assert ((seg_s == SENTINEL_S) == ~wrote).all(), q
    # ... and with HIGHER ones (+inf: nothing is a hit): nothing is written at all
    rc_c, rc_f, total, lims, s, i = _raw(idx, nq, thr, fill_thr=torch.full((nq,), np.inf, device=idx.device))
    assert rc_c == 0 and rc_f == 0 and total > 0 and untouched(s, i)
    # nq beyond one launch's grid: rejected before any device work, the count's state is gone
    from scaling_retriever_amd.scoring import _ptr
    total = ctypes.c_int64(-5)
    rc = idx.lib.sr_sparse_range_count(idx._h, _ptr(lims), _ptr(lims), _ptr(lims), 1 << 24, _ptr(thr), _ptr(lims), ctypes.byref(total), None)
    assert rc == _lib.SR_ERR_INVALID and b"2^24" in idx.lib.sr_last_error() and total.value == -5
    # nq = 0
    lims, s, i = idx.range_search(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), 0.0)
    assert lims.tolist() == [0] and s.numel() == 0 and i.numel() == 0
    # queries without any term: zero scores, hits exactly under a negative threshold
    lims, s, i = idx.range_search(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.array([0.0, -0.5, np.nan], np.float32))
    assert lims.tolist() == [0, 0, n_docs, n_docs] and torch.equal(i.cpu(), torch.arange(n_docs)) and bool((s == 0).all())
    idx.close()


def test_trailing_documents_without_postings_are_returned_under_a_negative_threshold():
    from scaling_retriever_amd.scoring import SparseIndexHIP
    n_post, n_docs = 8192, 8192 + 700                    # the second tile holds no posting at all
    indptr, ids, vals = _collection(n_post)
    idx = SparseIndexHIP(indptr.copy(), ids.copy(), vals.copy(), n_docs)
    nq = 5
    thr = np.array([-1.0, 0.0, -1.0, -1.0, -0.001], np.float32)
    lims, s, i = (t.cpu().numpy() for t in idx.range_search(*_csr(nq), thr))
    for q in range(nq):
        full = np.concatenate([_all_scores(n_post, q), np.zeros(700, np.float32)])
        hit = np.nonzero(full > thr[q])[0]
        assert np.array_equal(i[lims[q]:lims[q + 1]], hit), q
        assert np.array_equal(s[lims[q]:lims[q + 1]].view(np.int32), full[hit].view(np.int32)), q
    assert lims[1] - lims[0] >= 700 and i[lims[1] - 1] == n_docs - 1
    idx.close()


def test_static_numba_score_float_is_one_range_search():
    """n_docs = 20 000, more than 4 096 passing documents: indexes and negated scores are the oracle's."""
    from oracle import scoring as SC
    from scaling_retriever_amd.indexer import SparseRetrieval
    rng = np.random.default_rng(23)
    Vs, N = 60, 20000
    lists = []
    for t in range(Vs):
        docs = np.sort(rng.choice(N, size=int(rng.integers(1, 4000)), replace=False)).astype(np.int32)
        lists.append((docs, rng.uniform(0.1, 2.0, size=len(docs)).astype(np.float32)))
    indptr = np.concatenate([[0], np.cumsum([len(d) for d, _ in lists])]).astype(np.int64)
    ids, vals = np.concatenate([d for d, _ in lists]), np.concatenate([v for _, v in lists])
    d_ids, d_vals = {t: lists[t][0] for t in range(Vs)}, {t: lists[t][1] for t in range(Vs)}
    cols = np.array([41, 2, 30, 9, 17, 5, 55, 23], np.int32)
    qv = np.array([0.5, 1.25, -0.75, 2.0, 0.3, 1.0, 0.0, 0.8], np.float32)
    for thr, least in ((0.0, 4097), (1.0, 1), (-1.0, 4097)):
        fi, neg = SparseRetrieval.numba_score_float(d_ids, d_vals, cols, qv, threshold=thr, size_collection=N)
        ei, en = SC.numba_score_float(indptr, ids, vals, cols, qv, thr, N)
        assert len(ei) >= least
        assert fi.dtype == np.int64 and neg.dtype == np.float32 and np.array_equal(fi, ei)
        assert np.array_equal(neg.view(np.int32), en.view(np.int32))


def test_retrieval_range_search_returns_collection_ids(golden_dir, tmp_path):
    """SparseIndexer -> SparseRetrieval on the tiny model, as tests/test_indexer_gpu.py builds them; ids go through doc_id_table."""
    import json

    from golden_weights import make_weights
    from oracle import scoring as SC
    from test_indexer_gpu import FakeLoader, _corpus
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval, SparseIndexer, SparseRetrieval
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    Vm = cfg["vocab_size"]
    rng = np.random.default_rng(1)
    docs, queries = _corpus(rng, 50, Vm, 1, 6), _corpus(rng, 7, Vm, 1, 3)
    pids, qids = [f"p{i}" for i in range(len(docs))], [f"q{i}" for i in range(len(queries))]
    model = LlamaBiSparse.from_weights(cfg, w, precision="bf16").to("cuda").eval()
    index_dir = str(tmp_path / "index")
    SparseIndexer(model, index_dir=index_dir, compute_stats=False, dim_voc=model.vocab_size, device="cuda").index(
        FakeLoader(docs, pids, batch_size=8, pad_id=Vm - 1))
    retr = SparseRetrieval(config={"index_dir": index_dir, "out_dir": str(tmp_path / "out")}, model=model, dim_voc=model.vocab_size, device="cuda")
    indptr, ids, vals = retr.sparse_index.csr(Vm)
    qvecs, _ = retr._generate_query_vecs(FakeLoader(queries, qids, batch_size=4, pad_id=Vm - 1))
    full = [-SC.numba_score_float(indptr, ids, vals, c, v, -np.inf, 50)[1] for c, v in qvecs]
    thr = np.array([np.sort(s)[-5] for s in full], np.float32)          # the 5th best: at most 4 hits each
    for vecs in (qvecs, [qvecs[i] for i in range(len(qvecs))]):          # the device CSR and the reference's list of pairs
        for sort in (True, False):
            id_lists, score_lists = retr.range_search(vecs, thr, sort=sort)
            assert len(id_lists) == len(score_lists) == len(queries)
            for qi, (c, v) in enumerate(qvecs):
                fi, neg = SC.numba_score_float(indptr, ids, vals, c, v, thr[qi], 50)
                if sort:
                    order = np.lexsort((fi, neg))
                    fi, neg = fi[order], neg[order]
                assert id_lists[qi] == [pids[j] for j in fi], (qi, sort)
                assert score_lists[qi].dtype == np.float32 and np.array_equal(score_lists[qi].view(np.int32), (-neg).view(np.int32))
    id_lists, _ = retr.range_search(qvecs)                              # the reference's default threshold 0
    for qi, (c, v) in enumerate(qvecs):
        assert sorted(id_lists[qi]) == sorted(pids[j] for j in SC.numba_score_float(indptr, ids, vals, c, v, 0.0, 50)[0])
    # under a negative threshold every document that has a collection id comes back, and only those: a document without a posting has
    # none (doc_ids.pkl), its placeholder in doc_id_table is never returned
    with_id = sorted(retr.doc_ids)
    retr.doc_ids.pop(with_id[-1])                                       # make one: the last document loses its id
    retr._doc_table = None
    id_lists, score_lists = retr.range_search(qvecs, -1.0, sort=False)
    for qi in range(len(queries)):
        assert id_lists[qi] == [pids[j] for j in with_id[:-1]] and len(score_lists[qi]) == len(with_id) - 1
    with pytest.raises(NotImplementedError):
        ShardedSparseRetrieval.range_search(retr, qvecs)
