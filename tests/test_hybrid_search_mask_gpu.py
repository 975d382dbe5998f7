"""GPU: the exact hybrid search under a document bitmap (hybrid.search_fused(mask=), HybridRetriever.search_fused(allowed_mask=)).

Every comparison is for equal bits, as in tests/test_hybrid_search_gpu.py whose indexes and brute-force pair scores are shared: ids,
score bits and counts against hybrid_cases.rank_rows over the fused pair scores of the ALLOWED documents only, and the route of every
query (stats depth / union / range_hits) against tests/hybrid_mask_cases.py.  Masks over dense positions: every bit (must equal the
unmasked search, stats included), random 50 % and 5 %, the band [N/4, 3N/4), 7 documents (fewer than k), none, and on the
integer-valued case every document with a posting cleared."""
import json
import os

import numpy as np
import pytest
import torch

import hybrid_cases as H
import hybrid_mask_cases as HM
import test_hybrid_search_gpu as T

pytestmark = pytest.mark.gpu
F32 = np.float32
_bits = T._bits


def _masks(N, d2s):
    rng = np.random.default_rng(77 + N)
    r = np.arange(N)
    seven = np.zeros(N, bool)
    seven[rng.choice(N, 7, replace=False)] = True
    return {"all": np.ones(N, bool), "r50": rng.random(N) < 0.5, "band": (r >= N // 4) & (r < 3 * N // 4), "r05": rng.random(N) < 0.05,
            "seven": seven, "none": np.zeros(N, bool), "no_posting": np.asarray(d2s) < 0}


def _search(ix, rows, k, w, depths, allowed, **kw):
    from scaling_retriever_amd.scoring import pack_doc_mask
    return ix.search(rows, k, w, depths, mask=pack_doc_mask(allowed), **kw)


def _check(ix, rows, k, w, depths, allowed, **kw):
    """search_fused under the mask equals brute force over the allowed documents - ids, score bits, counts - and reports the calculated
    routes."""
    rows = np.asarray(rows)
    got_s, got_i, got_n, stats = _search(ix, rows, k, w, depths, allowed, **kw)
    want_i, want_s, want_n = HM.rank_rows(H.fuse(w, ix.dense_all[rows], ix.sparse_all[rows]), ix.tie, k, allowed)
    print("allowed", int(allowed.sum()), "depth", stats["depth"].tolist(), "range_hits", stats["range_hits"].tolist())
    assert np.array_equal(got_n, want_n), (got_n, want_n)
    assert np.array_equal(got_i, want_i), np.flatnonzero((got_i != want_i).any(1))
    assert np.array_equal(_bits(got_s), _bits(want_s))
    assert (got_i[got_i >= 0] < len(allowed)).all() and allowed[got_i[got_i >= 0]].all()
    route, union, hits = HM.expected_routes(ix.dense_all[rows], ix.sparse_all[rows], ix.case["d2s"], ix.n_sparse, w, k, depths, allowed)
    assert np.array_equal(stats["depth"], route), (stats["depth"], route)
    assert np.array_equal(stats["union"], union) and np.array_equal(stats["range_hits"], hits)
    return got_s, got_i, got_n, stats


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("case", ["family", "integer"])
def test_every_bit_set_equals_the_unmasked_search(case):
    ix = T._family() if case == "family" else T._Indexes(H.integer_case())
    nq, N = ix.case["Q"].shape[0], ix.case["N"]
    for depths in ((40, 160, 640), (10,)):
        a = ix.search(np.arange(nq), 10, (1.0, 1.0), depths)
        b = _check(ix, np.arange(nq), 10, (1.0, 1.0), depths, np.ones(N, bool))
        assert _same(a, b)
        for key in ("depth", "union", "range_hits"):
            assert np.array_equal(a[3][key], b[3][key]), key
        assert a[3]["depths"] == b[3]["depths"]


@pytest.mark.parametrize("name", ["r50", "band", "r05", "seven", "none"])
def test_family_case_under_a_mask(name):
    ix = T._family()
    N, k, w = ix.case["N"], 10, (1.0, 1.0)
    allowed = _masks(N, ix.case["d2s"])[name]
    before = ix.dense.batch_invariant
    got = _check(ix, np.arange(24), k, w, (40, 160, 640), allowed)
    depth = got[3]["depth"]
    if name == "r50":                                    # a condition on the inputs: every route, the masked range kernel with them, is exercised
        assert {0, 1, -1} <= set(depth.tolist()), depth
    if name == "seven":                                  # fewer than k allowed documents: the count says so, the rest is padding
        assert got[2].tolist() == [7] * 24 and (got[1][:, 7:] == -1).all() and (got[0][:, 7:] == -H.FLT_MAX).all()
        assert depth.tolist() == [0] * 24                # the dense list holds every allowed document: complete
    if name == "none":
        assert got[2].tolist() == [0] * 24 and (got[1] == -1).all() and (got[0] == -H.FLT_MAX).all()
    assert ix.dense.batch_invariant == before
    if name in ("r50", "band"):
        # the first depth alone: most queries take the range route
        short = _check(ix, np.arange(24), k, w, (10,), allowed)
        assert (short[3]["depth"] == -1).sum() >= 8 and (short[3]["range_hits"][short[3]["depth"] == -1] > 0).all()
        assert _same(short, got)
        # 70 queries: the large-batch dense path returns the same rows
        rows70 = np.arange(70) % 24
        big = _check(ix, rows70, k, w, (40, 160, 640), allowed)
        assert np.array_equal(big[1], got[1][rows70]) and np.array_equal(_bits(big[0]), _bits(got[0][rows70]))
        assert np.array_equal(big[3]["depth"], depth[rows70])


def test_other_weights_under_a_mask():
    ix = T._family()
    allowed = _masks(ix.case["N"], ix.case["d2s"])["r50"]
    for w in ((0.3, 2.0), (1.0, 0.0), (0.0, 1.0)):
        _check(ix, np.arange(24), 10, w, (40, 160), allowed)


def test_range_route_in_sub_batches_under_a_mask():
    ix = T._family()
    k, depths, w = 10, (40,), (1.0, 1.0)
    allowed = _masks(ix.case["N"], ix.case["d2s"])["r50"]
    whole = _check(ix, np.arange(24), k, w, depths, allowed)
    hits = whole[3]["range_hits"]
    assert (whole[3]["depth"] == -1).sum() >= 8
    budget = int((hits.max() + 40) * 64 * 2)             # two of the longest lists at most: several sub-batches
    parts = _check(ix, np.arange(24), k, w, depths, allowed, fallback_bytes=budget)
    assert _same(parts, whole)


@pytest.mark.parametrize("precision", ["fp32", "fp32_filtered"])
def test_integer_case_under_a_mask(precision):
    ix = T._Indexes(H.integer_case(), precision)
    masks = _masks(ix.case["N"], ix.case["d2s"])
    routes = _check(ix, np.arange(16), 10, (1.0, 1.0), (10,), masks["r50"])[3]["depth"]
    assert (routes == -1).any()
    for name in ("r50", "band", "no_posting", "seven"):
        for w, depths in [((1.0, 1.0), (20, 80)), ((1.0, 2.0), (10, 40))]:
            _check(ix, np.arange(16), 10, w, depths, masks[name])
    assert masks["no_posting"].sum() > 50
    rows70 = np.arange(70) % 16
    a, b = _check(ix, np.arange(16), 10, (1.0, 1.0), (20, 80), masks["r50"]), _check(ix, rows70, 10, (1.0, 1.0), (20, 80), masks["r50"])
    assert np.array_equal(b[1], a[1][rows70]) and np.array_equal(_bits(b[0]), _bits(a[0][rows70]))


def test_mask_errors():
    ix = T._family()
    N = ix.case["N"]
    with pytest.raises(ValueError, match="words"):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), mask=np.zeros(N // 32 + 1, np.uint32))
    with pytest.raises(ValueError):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), mask=np.ones(N, bool))          # not packed words


# ------------------------------------------------------------------------------------- through the toy hybrid model ---
toy = T.toy


def test_allowed_mask_through_the_toy_model(toy):
    w, k = (0.7, 1.3), 10
    ret, out = T._retriever(toy, "masked")
    sparse_q, dense_q, qids = ret._generate_query_vecs(toy[3]())
    all_ids = [str(d) for d in ret.dense_index.index_id_to_db_id]
    allowed_ids = all_ids[3::2]
    flags = ret.allowed_mask(allowed_ids + allowed_ids[:2])
    assert flags.dtype == bool and flags.shape == (len(all_ids),) and int(flags.sum()) == len(allowed_ids)
    assert [all_ids[p] for p in np.flatnonzero(flags)] == allowed_ids
    full = T._brute_force_run(ret, sparse_q, dense_q, qids, w, len(all_ids))          # the whole ranking: filtered, then cut to k
    keep = set(allowed_ids)
    res, stats = ret.search_fused(sparse_q, dense_q, k, weights=w, qids=qids, allowed_mask=flags)
    res2, stats2 = ret.retrieve_fused_exact(toy[3](), k, weights=w, allowed_mask=flags)
    run = json.load(open(os.path.join(out, "fused_exact", "run.json")))
    assert run == {q: dict(r) for q, r in res2.items()} and len(run) == len(qids)
    for q in qids:
        sel = [j for j, d in enumerate(full[q][0]) if d in keep][:k]
        assert list(res[q].keys()) == [full[q][0][j] for j in sel] == list(run[q].keys()), q
        assert np.array_equal(np.array(list(res[q].values()), F32), full[q][1][sel]), q
        assert np.array_equal(np.array(list(run[q].values()), F32), full[q][1][sel]), q
    assert (stats["depth"] >= 0).all()                   # depth 160 holds every allowed document: complete
    with pytest.raises(NotImplementedError, match="allowed_mask"):
        ret.search_fused(sparse_q, dense_q, k, allowed_ids=allowed_ids)
    with pytest.raises(ValueError, match="one flag per index position"):
        ret.search_fused(sparse_q, dense_q, k, allowed_mask=flags[:-1])
    with pytest.raises(ValueError, match="unknown"):
        ret.allowed_mask(["no-such-document"])
