"""GPU: the exact hybrid search under a document bitmap per query (hybrid.search_fused(masks=, query_group=),
HybridRetriever.search_fused / retrieve_fused_exact(allowed_masks=, query_group=)), and the range searches of the three indexer classes
under groups.

Every comparison is for equal bits.  Indexes and brute-force pair scores are those of tests/test_hybrid_search_gpu.py, masks those of
tests/test_hybrid_search_mask_gpu.py.  The expected rows and routes of query q come from tests/hybrid_mask_cases.py (numpy only) called
with allowed = masks[group[q]]; in addition the result must equal one search_fused(mask=masks[g]) per group over that group's queries
alone.  Groups: random 50 %, the band [N/4, 3N/4), random 5 %, 7 documents (fewer than k) and none, dealt round-robin over the queries."""
import json
import os

import numpy as np
import pytest
import torch

import hybrid_cases as H
import hybrid_mask_cases as HM
import test_hybrid_search_gpu as T
import test_hybrid_search_mask_gpu as TM

pytestmark = pytest.mark.gpu
F32 = np.float32
_bits = T._bits
GROUPS = ("r50", "band", "r05", "seven", "none")


def _groups(ix, n_rows):
    m = TM._masks(ix.case["N"], ix.case["d2s"])
    return np.stack([m[name] for name in GROUPS]), np.arange(n_rows) % len(GROUPS)


def _search(ix, rows, k, w, depths, allowed, group, **kw):
    from scaling_retriever_amd.scoring import pack_doc_masks
    return ix.search(rows, k, w, depths, masks=pack_doc_masks(torch.from_numpy(allowed)), query_group=group, **kw)


def _check(ix, rows, k, w, depths, allowed, group, **kw):
    """search_fused under groups equals, query by query, brute force over the allowed documents of the query's group - ids, score bits,
    counts, and the calculated routes - and group by group the masked search of that group's queries alone."""
    rows = np.asarray(rows)
    got_s, got_i, got_n, stats = _search(ix, rows, k, w, depths, allowed, group, **kw)
    print("depth", stats["depth"].tolist(), "range_hits", stats["range_hits"].tolist())
    for g in np.unique(group):
        sel = np.flatnonzero(group == g)
        r = rows[sel]
        want_i, want_s, want_n = HM.rank_rows(H.fuse(w, ix.dense_all[r], ix.sparse_all[r]), ix.tie, k, allowed[g])
        assert np.array_equal(got_n[sel], want_n), (g, got_n[sel], want_n)
        assert np.array_equal(got_i[sel], want_i), g
        assert np.array_equal(_bits(got_s[sel]), _bits(want_s)), g
        ids = got_i[sel]
        assert allowed[g][ids[ids >= 0]].all()
        route, union, hits = HM.expected_routes(ix.dense_all[r], ix.sparse_all[r], ix.case["d2s"], ix.n_sparse, w, k, depths, allowed[g])
        assert np.array_equal(stats["depth"][sel], route), (g, stats["depth"][sel], route)
        assert np.array_equal(stats["union"][sel], union) and np.array_equal(stats["range_hits"][sel], hits), g
        one = TM._search(ix, r, k, w, depths, allowed[g], **kw)
        assert np.array_equal(one[1], got_i[sel]) and np.array_equal(_bits(one[0]), _bits(got_s[sel])) and np.array_equal(one[2], got_n[sel]), g
        for key in ("depth", "union", "range_hits"):
            assert np.array_equal(one[3][key], stats[key][sel]), (g, key)
    return got_s, got_i, got_n, stats


def test_family_case_under_groups_takes_every_route_in_one_call():
    ix = T._family()
    k, w = 10, (1.0, 1.0)
    allowed, group = _groups(ix, 24)
    before = ix.dense.batch_invariant
    got = _check(ix, np.arange(24), k, w, (40, 160, 640), allowed, group)
    depth = got[3]["depth"]
    assert {0, 1, -1} <= set(depth.tolist()), depth                     # a condition on the inputs: all three routes in this one call
    seven, none = group == GROUPS.index("seven"), group == GROUPS.index("none")
    assert got[2][seven].tolist() == [7] * int(seven.sum()) and (got[1][seven][:, 7:] == -1).all() and (depth[seven] == 0).all()
    assert not got[2][none].any() and (got[1][none] == -1).all() and (got[0][none] == -H.FLT_MAX).all() and (depth[none] == 0).all()
    assert ix.dense.batch_invariant == before
    # the first depth alone: most queries of the large groups take the range route (the grouped dense range search)
    short = _check(ix, np.arange(24), k, w, (10,), allowed, group)
    assert (short[3]["depth"] == -1).sum() >= 6 and (short[3]["range_hits"][short[3]["depth"] == -1] > 0).all()
    assert TM._same(short, got)
    # 70 queries: the large-batch paths return the same rows
    rows70 = np.arange(70) % 24
    big = _check(ix, rows70, k, w, (40, 160, 640), allowed, np.arange(70) % 24 % len(GROUPS))
    assert np.array_equal(big[1], got[1][rows70]) and np.array_equal(_bits(big[0]), _bits(got[0][rows70]))
    assert np.array_equal(big[3]["depth"], depth[rows70])


def test_other_weights_and_one_group():
    ix = T._family()
    allowed, group = _groups(ix, 24)
    for w in ((0.3, 2.0), (1.0, 0.0), (0.0, 1.0)):
        _check(ix, np.arange(24), 10, w, (40, 160), allowed, group)
    # one group is the masked search, stats included (checked inside _check against search_fused(mask=))
    _check(ix, np.arange(24), 10, (1.0, 1.0), (40, 160), allowed[:1], np.zeros(24, np.int64))


def test_range_route_in_sub_batches_under_groups():
    ix = T._family()
    k, depths, w = 10, (40,), (1.0, 1.0)
    allowed, group = _groups(ix, 24)
    whole = _search(ix, np.arange(24), k, w, depths, allowed, group)
    hits = whole[3]["range_hits"]
    assert (whole[3]["depth"] == -1).sum() >= 6
    budget = int((hits.max() + 40) * 64 * 2)             # two of the longest lists at most: several sub-batches
    parts = _check(ix, np.arange(24), k, w, depths, allowed, group, fallback_bytes=budget)
    assert TM._same(parts, whole)
    for key in ("depth", "union", "range_hits"):
        assert np.array_equal(parts[3][key], whole[3][key]), key


@pytest.mark.parametrize("precision", ["fp32", "fp32_filtered"])
def test_integer_case_under_groups(precision):
    ix = T._Indexes(H.integer_case(), precision)
    m = TM._masks(ix.case["N"], ix.case["d2s"])
    allowed = np.stack([m["r50"], m["band"], m["no_posting"], m["seven"]])
    group = np.arange(16) % 4
    routes = _check(ix, np.arange(16), 10, (1.0, 1.0), (10,), allowed, group)[3]["depth"]
    assert (routes == -1).any()
    for w, depths in [((1.0, 1.0), (20, 80)), ((1.0, 2.0), (10, 40))]:
        _check(ix, np.arange(16), 10, w, depths, allowed, group)


def test_argument_errors():
    from scaling_retriever_amd.scoring import pack_doc_masks
    ix = T._family()
    N = ix.case["N"]
    allowed, group = _groups(ix, 3)
    words = pack_doc_masks(torch.from_numpy(allowed))
    with pytest.raises(ValueError, match="words"):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), masks=np.zeros((2, N // 32 + 2), np.uint32), query_group=group)
    with pytest.raises(ValueError, match="packed"):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), masks=allowed, query_group=group)          # not packed words
    with pytest.raises(ValueError, match="not both"):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), mask=words[0], masks=words, query_group=group)
    with pytest.raises(ValueError, match="go together"):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), masks=words)
    with pytest.raises(ValueError, match="one group id per query"):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), masks=words, query_group=group[:2])
    with pytest.raises(ValueError, match="query 1 is in group 5"):
        ix.search(np.arange(3), 10, (1.0, 1.0), (40,), masks=words, query_group=np.array([0, 5, 1]))


# ------------------------------------------------------------------------------------- through the toy hybrid model ---
toy = T.toy


def test_allowed_masks_through_the_toy_model(toy):
    w, k = (0.7, 1.3), 10
    ret, out = T._retriever(toy, "grouped")
    sparse_q, dense_q, qids = ret._generate_query_vecs(toy[3]())
    all_ids = [str(d) for d in ret.dense_index.index_id_to_db_id]
    flags = np.stack([ret.allowed_mask(all_ids[3::2]), ret.allowed_mask(all_ids[::3]), ret.allowed_mask(all_ids[:4]),
                      np.zeros(len(all_ids), bool)])
    group = np.arange(len(qids)) % len(flags)
    res, stats = ret.search_fused(sparse_q, dense_q, k, weights=w, qids=qids, allowed_masks=flags, query_group=group)
    res2, stats2 = ret.retrieve_fused_exact(toy[3](), k, weights=w, allowed_masks=flags, query_group=group)
    run = json.load(open(os.path.join(out, "fused_exact", "run.json")))
    assert run == {q: dict(r) for q, r in res2.items()}
    full = T._brute_force_run(ret, sparse_q, dense_q, qids, w, len(all_ids))          # the whole ranking: filtered, then cut to k
    for j, q in enumerate(qids):
        keep = {all_ids[p] for p in np.flatnonzero(flags[group[j]])}
        sel = [i for i, d in enumerate(full[q][0]) if d in keep][:k]
        got = res.get(q, {})                                    # a query without a hit has no entry
        assert list(got.keys()) == [full[q][0][i] for i in sel] == list(run.get(q, {}).keys()), q
        assert np.array_equal(np.array(list(got.values()), F32), full[q][1][sel]), q
    # group by group: the masked search of its queries alone
    for g in range(len(flags)):
        sel = np.flatnonzero(group == g)
        one, _ = ret.search_fused([sparse_q[int(i)] for i in sel], dense_q[torch.from_numpy(sel).to(dense_q.device)], k, weights=w,
                                  qids=[qids[i] for i in sel], allowed_mask=flags[g])
        for i in sel:
            assert list(one.get(qids[i], {}).items()) == list(res.get(qids[i], {}).items()), qids[i]
    with pytest.raises(ValueError, match="not both"):
        ret.search_fused(sparse_q, dense_q, k, allowed_mask=flags[0], allowed_masks=flags, query_group=group)
    with pytest.raises(ValueError, match="go together"):
        ret.retrieve_fused_exact(toy[3](), k, allowed_masks=flags)
    with pytest.raises(ValueError, match="one row of flags per group"):
        ret.search_fused(sparse_q, dense_q, k, allowed_masks=flags[:, :-1], query_group=group)

    # the range searches of the three indexer classes under groups: each query's lists are those under its own group's mask
    dq = dense_q.float()
    d_thr = float(np.median(np.concatenate(ret.dense_index.range_search(dq, -1e30)[1])))      # half of all pairs pass
    d_ids, d_scores = ret.dense_index.range_search(dq, d_thr, allowed_masks=flags, query_group=group)
    h_ids, h_scores = ret.range_search(sparse_q, -1.0, allowed_masks=flags, query_group=group)          # masks over DENSE positions
    d2s, _ = ret._position_maps()
    d2s = d2s.cpu().numpy()
    n_sparse = ret.hip_index.n_docs
    s_flags = np.zeros((len(flags), n_sparse), bool)
    for g in range(len(flags)):
        s_flags[g, d2s[flags[g] & (d2s >= 0)]] = True
    from scaling_retriever_amd.indexer import SparseRetrieval
    s_ids, s_scores = SparseRetrieval.range_search(ret, sparse_q, -1.0, allowed_masks=s_flags, query_group=group)
    assert sum(len(x) for x in d_ids) > 0 and sum(len(x) for x in s_ids) > 0
    for g in range(len(flags)):
        one_d = ret.dense_index.range_search(dq, d_thr, allowed_mask=flags[g])
        one_s = SparseRetrieval.range_search(ret, sparse_q, -1.0, allowed_mask=s_flags[g])
        for j in np.flatnonzero(group == g):
            assert d_ids[j] == one_d[0][j] and np.array_equal(_bits(d_scores[j]), _bits(one_d[1][j])), (g, j)
            assert s_ids[j] == one_s[0][j] == h_ids[j], (g, j)
            assert np.array_equal(_bits(s_scores[j]), _bits(one_s[1][j])) and np.array_equal(_bits(h_scores[j]), _bits(one_s[1][j])), (g, j)
    with pytest.raises(ValueError, match="not both"):
        ret.dense_index.range_search(dq, 0.0, allowed_mask=flags[0], allowed_masks=flags, query_group=group)
    with pytest.raises(ValueError, match="one group id per query"):
        ret.dense_index.range_search(dq, 0.0, allowed_masks=flags, query_group=group[:-1])
