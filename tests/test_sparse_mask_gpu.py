"""GPU: sparse search under a document bitmap (sr_sparse_search_masked; the mask route of csrc/subset_search.hip: the certified
scorer's pass, cert_score_kernel<KS, true>, with one bit test where a document would become a stage-1 key).  Every comparison is for
equal counts, equal ids and equal score BITS: against the oracle's term-serial fp32 sums over the collection, filtered to the allowed
positions and cut to k, and between the three routes (pairs, array, mask) through both forms of the filter.  The cert_stats() deltas
keep a comparison from passing on the hand-back route alone.

Inputs are the generators of tests/test_sparse_cert_gpu.py at the shapes, seeds and k of its test_certified_search_is_bit_exact."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import scoring as O
from test_sparse_cert_gpu import _zipf_index, _zipf_queries

pytestmark = pytest.mark.gpu

SHAPES = [
    (3000, 66000, 48, 70, 32, 1000, 0.0),
    (800, 40000, 30, 33, 16, 100, 0.0),
    (2000, 50001, 40, 40, 24, 500, 3.0),         # a partial last tile, N % 32 == 17
]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("SR_SPARSE_CERT", "1")        # build + use the certified scorer below its size threshold as well


@functools.lru_cache(maxsize=None)
def _shape(n):
    """Index, queries and the oracle's full ranking (k = N) of shape n, computed once and never changed."""
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[n]
    rng = np.random.default_rng(V + N + k)
    indptr, ids, vals = _zipf_index(rng, V, N, L0_d)
    qi, qc, qv = _zipf_queries(rng, V, nq, L0_q)
    full_i, full_s, full_c = O.sparse_retrieve_c(indptr, ids, vals, qi, qc, qv, N, thr, N, q_threads=4)
    return indptr, ids, vals, qi, qc, qv, full_i, full_s, full_c


def _masks(N):
    mrng = np.random.default_rng(5)
    i = np.arange(N)
    out = {"half": mrng.random(N) < 0.5, "sixteenth": mrng.random(N) < 1 / 16}
    out["odd_blocks"] = (i // 32) % 2 == 1
    out["tile1_and_tail"] = ((i >= 1024) & (i < 2048)) | (i >= N - 700)
    out["all_but_few"] = i % 97 != 0
    out["diag"] = i % 32 == (i // 32) % 32
    out["anti_diag"] = ~out["diag"]
    out["all"] = np.ones(N, bool)
    return out


def _expected(full_i, full_s, full_c, flags, k):
    """The full ranking filtered to the allowed positions, in the order it came, cut to k, padded with (0, -1)."""
    nq = full_i.shape[0]
    es, ei, ec = np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
    for q in range(nq):
        row = full_i[q, :int(full_c[q])]
        keep = np.flatnonzero(flags[row])[:k]
        ec[q] = len(keep)
        ei[q, :len(keep)] = row[keep]
        es[q, :len(keep)] = full_s[q, keep]
    return es, ei, ec


def _np(res):
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in res]


def _same(got, want, what):
    assert np.array_equal(got[2], want[2]), (what, "counts")
    bad = [q for q in range(len(want[2])) if not (np.array_equal(got[1][q], want[1][q]) and np.array_equal(_bits(got[0][q]), _bits(want[0][q])))]
    assert not bad, f"{what}: queries with different rows: {bad[:10]} ({len(bad)} of {len(want[2])})"


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_masked_equals_the_oracle_over_the_allowed_documents(forced, monkeypatch, n):
    """redone_exact delta <= nq // 8 per call is the cap test_certified_search_is_bit_exact holds unmasked: the mask route itself must
    carry the call."""
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[n]
    indptr, ids, vals, qi, qc, qv, full_i, full_s, full_c = _shape(n)
    monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", "mask")
    idx = SparseIndexHIP(indptr, ids, vals, N)
    assert idx.cert_stats()["present"] == 1
    for name, flags in _masks(N).items():
        before = idx.cert_stats()
        got = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=flags))
        after = idx.cert_stats()
        redone = after["redone_exact"] - before["redone_exact"]
        print(f"shape {n} mask {name}: allowed {int(flags.sum())}, handed back {redone} of {nq}")
        _same((got[0], got[1], got[2]), _expected(full_i, full_s, full_c, flags, k), f"shape {n} mask {name}")
        assert after["searches"] - before["searches"] == 1 and after["queries"] - before["queries"] == nq, (name, before, after)
        assert redone <= nq // 8, (name, redone, nq)


@pytest.mark.parametrize("n", [0, 1])
def test_three_routes_return_the_same_bits(forced, monkeypatch, n):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[n]
    indptr, ids, vals, qi, qc, qv, full_i, full_s, full_c = _shape(n)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    masks = _masks(N)
    masks["empty"] = np.zeros(N, bool)
    masks["single"] = np.arange(N) == 17
    for name, flags in masks.items():
        want = _expected(full_i, full_s, full_c, flags, k)
        subset = np.flatnonzero(flags).astype(np.int64)
        for route in ("pairs", "array", "mask"):
            monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", route)
            before = idx.cert_stats()["redone_exact"]
            _same(_np(idx.search(qi, qc, qv, k, threshold=thr, mask=flags)), want, f"shape {n} mask {name} route {route} (mask=)")
            _same(_np(idx.search(qi, qc, qv, k, threshold=thr, subset=subset)), want, f"shape {n} mask {name} route {route} (subset=)")
            if name == "single" and route == "mask":          # k exceeds the allowed count: every query is handed back, twice
                assert idx.cert_stats()["redone_exact"] - before == 2 * nq
        if name == "empty":
            assert (want[1] == -1).all() and (want[0] == 0).all() and (want[2] == 0).all()
        if name == "half":
            shifted = (want[0], np.where(want[1] >= 0, 7 + 3 * want[1], -1), want[2])
            for route in ("pairs", "array", "mask"):
                monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", route)
                _same(_np(idx.search(qi, qc, qv, k, threshold=thr, id_base=7, id_stride=3, mask=flags)), shifted, f"ids 7 + 3 d, route {route} (mask=)")
                _same(_np(idx.search(qi, qc, qv, k, threshold=thr, id_base=7, id_stride=3, subset=subset)), shifted, f"ids 7 + 3 d, route {route} (subset=)")


def test_mask_tail_bits_and_partial_last_tile(forced, monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[2]
    indptr, ids, vals, qi, qc, qv, full_i, full_s, full_c = _shape(2)
    assert N % 1024 != 0 and N % 32 == 17                        # a partial last tile, a partial last mask word
    idx = SparseIndexHIP(indptr, ids, vals, N)
    plain = _np(idx.search(qi, qc, qv, k, threshold=thr))
    n_words = (N + 31) // 32
    ones = np.full(n_words, 0xffffffff, np.uint32)               # the 15 bits beyond n_bits set as well
    last = np.zeros(N, bool)
    last[N - 1] = True
    scores_it = np.array([(full_i[q, :int(full_c[q])] == N - 1).any() for q in range(nq)])
    assert scores_it.any()
    for route in ("mask", "array", "pairs", None):
        if route is None:
            monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE")
        else:
            monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", route)
        got = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=ones))
        _same(got, plain, f"every bit set, route {route}")
        assert got[1].max() < N
        got = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=torch.from_numpy(ones.view(np.int32)).cuda()))
        _same(got, plain, f"every bit set, int32 cuda words, route {route}")
        s, i, c = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=last))
        assert np.array_equal(c, scores_it.astype(np.int32)), route
        assert (i[scores_it, 0] == N - 1).all() and (i[:, 1:] == -1).all() and (i[~scores_it, 0] == -1).all(), route
        for q in np.flatnonzero(scores_it):
            at = int(np.flatnonzero(full_i[q, :int(full_c[q])] == N - 1)[0])
            assert _bits(s[q, :1])[0] == _bits(full_s[q, at:at + 1])[0] and s[q, 0] > thr
        for bad in (ones[:-1], np.concatenate([ones, ones[:1]])):
            with pytest.raises(ValueError, match=f"holds {n_words} words"):
                idx.search(qi, qc, qv, k, threshold=thr, mask=bad)
        _same(_np(idx.search(qi, qc, qv, k, threshold=thr, mask=ones)), plain, f"after a refused mask, route {route}")
    # a bool mask of the wrong length reaches the library, which refuses it before any device work
    with pytest.raises(ValueError, match="n_bits"):
        idx.search(qi, qc, qv, k, threshold=thr, mask=np.ones(N + 1, bool))
    _same(_np(idx.search(qi, qc, qv, k, threshold=thr)), plain, "after a refused length")


def test_queries_outside_the_fast_path_under_a_mask(forced, monkeypatch):
    """The query set of test_queries_outside_the_fast_path_come_back_identical (negative weights, descending / shuffled order, a
    duplicate term, empty, unknown terms, zero weights, 90 rare terms, 300 terms, an inf weight), rebuilt from the generators, under
    `half`: what the plan kernel flags is re-done UNDER THE SAME FILTER, next to certified queries."""
    from scaling_retriever_amd.scoring import SparseIndexHIP
    rng = np.random.default_rng(11)
    V, N = 2500, 33000
    indptr, ids, vals = _zipf_index(rng, V, N, 40)
    qi, qc, qv = _zipf_queries(rng, V, 24, 20)
    qc, qv, qi = list(np.split(qc, qi[1:-1])), list(np.split(qv, qi[1:-1])), None
    qv[1] = -qv[1]
    qv[2][::3] *= -1
    qc[3], qv[3] = qc[3][::-1].copy(), qv[3][::-1].copy()
    p = rng.permutation(len(qc[4])); qc[4], qv[4] = qc[4][p], qv[4][p]
    qc[5] = np.concatenate([qc[5], qc[5][-1:]]); qv[5] = np.concatenate([qv[5], qv[5][-1:]])
    qc[6], qv[6] = np.zeros(0, np.int32), np.zeros(0, np.float32)
    qc[7], qv[7] = np.array([V, V + 3], np.int32), np.array([1.0, 2.0], np.float32)
    qc[8] = np.concatenate([qc[8], [V + 1]]).astype(np.int32); qv[8] = np.concatenate([qv[8], [2.0]]).astype(np.float32)
    qv[9][::2] = 0.0
    qc[10] = np.sort(rng.choice(np.arange(200, V), size=90, replace=False)).astype(np.int32)
    qv[10] = np.log1p(rng.uniform(0, 20, size=90)).astype(np.float32)
    qc[11] = np.sort(rng.choice(V, size=300, replace=False)).astype(np.int32)
    qv[11] = np.log1p(rng.uniform(0, 20, size=300)).astype(np.float32)
    qv[12][0] = np.float32(np.inf)
    qi = np.concatenate([[0], np.cumsum([len(c) for c in qc])]).astype(np.int64)
    qc, qv = np.concatenate(qc), np.concatenate(qv)
    flags = np.random.default_rng(5).random(N) < 0.5
    monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", "mask")
    idx = SparseIndexHIP(indptr, ids, vals, N)
    s, i, c = _np(idx.search(qi, qc, qv, 50, mask=flags))
    st = idx.cert_stats()
    assert st["searches"] == 1 and st["queries"] == 24 and 9 <= st["redone_exact"] <= 14, st
    for q in range(len(qi) - 1):
        if q == 12:
            continue                  # the chain holds inf / nan: the order of equal keys is not pinned by the oracle
        cols, v = qc[qi[q]:qi[q + 1]], qv[qi[q]:qi[q + 1]]
        known = (cols >= 0) & (cols < V)
        fi, neg = O.numba_score_float(indptr, ids, vals, cols[known], v[known], 0.0, N)
        ei, es = O.select_topk(fi[flags[fi]], neg[flags[fi]], 50)
        assert c[q] == len(ei), (q, c[q], len(ei))
        assert np.array_equal(i[q, :c[q]], ei) and np.array_equal(_bits(s[q, :c[q]]), _bits(es)), q
        assert (i[q, c[q]:] == -1).all() and (s[q, c[q]:] == 0).all()


def test_masked_search_in_several_query_batches(forced, monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[0]
    indptr, ids, vals, qi, qc, qv, full_i, full_s, full_c = _shape(0)
    flags = _masks(N)["half"]
    monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", "mask")
    idx = SparseIndexHIP(indptr, ids, vals, N)
    one = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=flags))
    assert idx.cert_stats()["searches"] == 1
    monkeypatch.setenv("SR_SPARSE_CERT_BATCH", "32")
    several = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=flags))
    assert idx.cert_stats()["searches"] == 1 + (nq + 31) // 32
    _same(several, one, "batches of 32 queries")
    _same(one, _expected(full_i, full_s, full_c, flags, k), "one batch")


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from golden_weights import make_weights
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    return cfg, make_weights(cfg, int(z["weight_seed"]))


def test_retrieve_with_allowed_mask(tiny, tmp_path):
    from test_indexer_gpu import FakeLoader, _corpus
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval, SparseIndexer, SparseRetrieval
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
    allowed = [f"p{j}" for j in (49, 3, 8, 3, 21, 30, 31, 44, 0, 17, 26)]
    by_ids = retriever("ids")
    by_ids.retrieve(loader(), topk=5, threshold=0.0, allowed_ids=allowed)
    flags = np.zeros(by_ids.hip_index.n_docs, bool)
    flags[by_ids.allowed_subset(allowed).cpu().numpy()] = True
    assert flags.sum() == 10
    by_mask = retriever("mask")
    res = by_mask.retrieve(loader(), topk=5, threshold=0.0, allowed_mask=flags)
    run = (tmp_path / "mask" / "run.json").read_bytes()
    assert run == (tmp_path / "ids" / "run.json").read_bytes() and len(json.loads(run)) >= 3
    assert res.to_dict() == json.loads(run)
    assert by_mask.retrieve(loader(), topk=5, threshold=0.0, allowed_mask=torch.from_numpy(flags)).to_dict() == json.loads(run)
    with pytest.raises(ValueError, match="not both"):
        by_mask.retrieve(loader(), topk=5, allowed_ids=allowed, allowed_mask=flags)
    with pytest.raises(ValueError, match="one flag per document position"):
        by_mask.retrieve(loader(), topk=5, allowed_mask=flags[:-1])
    with pytest.raises(NotImplementedError, match="allowed_mask"):
        ShardedSparseRetrieval.retrieve(object.__new__(ShardedSparseRetrieval), loader(), 5, allowed_mask=flags)


def test_default_rule_takes_the_mask_route_from_the_measured_product_on(forced, monkeypatch):
    """Without a forced route a call goes to the mask route where the scorer applies and nq x m >= 64 x 1 000 000 (csrc/subset_search.hip,
    SR_SUBSET_SPARSE_MASK_CROSSOVER), through both entry points; below the product the list routes serve it and the scorer sees no query.
    The rows are the forced array route's either way."""
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, _, L0_q, k, thr = SHAPES[1]
    indptr, ids, vals = _shape(1)[:3]
    nq = 1700
    qi, qc, qv = _zipf_queries(np.random.default_rng(9), V, nq, L0_q)
    masks = _masks(N)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE", raising=False)
    for name, through_the_scorer in (("all", True), ("half", False)):
        flags = masks[name]
        assert (nq * int(flags.sum()) >= 64 * 1000000) == through_the_scorer
        before = idx.cert_stats()["queries"]
        by_mask = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=flags))
        by_list = _np(idx.search(qi, qc, qv, k, threshold=thr, subset=np.flatnonzero(flags)))
        assert idx.cert_stats()["queries"] - before == (2 * nq if through_the_scorer else 0), name
        monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", "array")
        want = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=flags))
        monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE")
        _same(by_mask, want, f"default rule, mask= ({name})")
        _same(by_list, want, f"default rule, subset= ({name})")
