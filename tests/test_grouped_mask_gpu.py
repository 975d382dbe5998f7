"""GPU: dense search under per-query document filters (sr_dense_search_grouped: filter groups; dense_split_kernel<true, true, true> in
csrc/dense_split_grouped.hip).  Every comparison is for equal ids and equal score BITS: the grouped pass and the group loop against one
masked search per group on the gather route (the capability the grouped search replaces) and, for the first queries, against the
oracle's fmaf chain over the allowed rows.  filter_stats() is what shows that the grouped pass ran: without it the loop alone could
pass everything."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import scoring as O

pytestmark = pytest.mark.gpu

FMIN = np.float32(-3.402823466e38)
_CACHE = {}


def _grouped_route(monkeypatch, route):
    monkeypatch.setenv("SR_DEV_SWITCHES", "1")
    monkeypatch.setenv("SR_GROUPED_DENSE_ROUTE", route)


def _same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def _per_group_masked(monkeypatch, idx, q, k, flags, groups):
    """The reference: one masked search per group over exactly that group's queries, in their order, on the gather route."""
    monkeypatch.setenv("SR_DEV_SWITCHES", "1")
    monkeypatch.setenv("SR_SUBSET_DENSE_ROUTE", "gather")
    scores = torch.full((q.shape[0], k), 7.0, device="cuda")
    ids = torch.full((q.shape[0], k), 7, dtype=torch.int64, device="cuda")
    before = idx.filter_stats()
    for g in np.unique(groups):
        sel = torch.from_numpy(np.flatnonzero(groups == g)).cuda()
        s, i = idx.search(q[sel].contiguous(), k, mask=flags[g])
        scores[sel], ids[sel] = s, i
    assert idx.filter_stats() == before
    return scores, ids


def _stats_delta(idx, before):
    after = idx.filter_stats()
    return after[0] - before[0], after[1] - before[1]


def _corpus(H, N):
    key = ("D", H, N)
    if key not in _CACHE:
        rng = np.random.default_rng(H + N)
        D = (rng.standard_normal((N, H), dtype=np.float32) * (0.5 / np.sqrt(H))).astype(np.float32)
        D[7000 % N] = D[300]              # exact twins; at N = 12 000 in different segments of either layout
        _CACHE[key] = D
    return _CACHE[key]


def _index(H, N, layout, storage):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    key = ("idx", H, N, layout, storage)
    if key not in _CACHE:
        D = _corpus(H, N)
        Ds = D.astype(np.float16).astype(np.float32) if storage == "fp16" else D
        idx = DenseIndexHIP(H, row_dtype=storage)
        idx.set_precision("fp32_filtered")
        if layout == "contiguous":        # three segments with a tile tail each; the later id_base values are no multiples of 32
            third = N // 3
            for s0 in range(3):
                idx.add_host_rows(D[s0 * third:(s0 + 1) * third if s0 < 2 else N], id_base=s0 * third)
        else:
            idx.add_host_rows(D[0::2], id_base=0, id_stride=2)
            idx.add_host_rows(D[1::2], id_base=1, id_stride=2)
        assert idx.ntotal == N and idx.id_end == N and idx.stored_dtype() == storage
        _CACHE[key] = (idx, Ds)
    return _CACHE[key]


def _six_masks(N):
    """empty, all, single bit, random 1 %, random 50 %, one range that starts and ends mid-word and mid-tile"""
    rng = np.random.default_rng(N)
    flags = np.zeros((6, N), bool)
    flags[1] = True
    flags[2, 5000 % N] = True
    flags[3] = rng.random(N) < 0.01
    flags[4] = rng.random(N) < 0.5
    flags[5, 1003:N - 2445] = True
    return flags


# --------------------------------------------------------------------- grouped = per-group masked = oracle, both routes ---
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("k", [1, 100, 1000])
@pytest.mark.parametrize("nq", [70, 300])
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_grouped_equals_per_group_masked_equals_oracle(monkeypatch, layout, nq, k, storage):
    from scaling_retriever_amd.scoring import pack_doc_masks
    H, N = 256, 12000
    idx, Ds = _index(H, N, layout, storage)
    flags = _six_masks(N)
    rng = np.random.default_rng(nq + H)
    Q = (rng.standard_normal((nq, H), dtype=np.float32) * (0.5 / np.sqrt(H))).astype(np.float32)
    q = torch.from_numpy(Q).cuda()
    words = pack_doc_masks(torch.from_numpy(flags).cuda())
    assert words.shape == (6, (N + 31) // 32) and words.dtype == torch.int32
    # q % 6: every 16-lane row group and every query tile mixes groups; q % 5: group 5 has no query; all in one group
    assignments = {"mixed": np.arange(nq) % 6, "a group without queries": np.arange(nq) % 5, "one group": np.full(nq, 4)}
    for name, groups in assignments.items():
        ref = _per_group_masked(monkeypatch, idx, q, k, flags, groups)
        for route in ("pass", "loop"):
            _grouped_route(monkeypatch, route)
            before = idx.filter_stats()
            got = idx.search_grouped(q, k, torch.from_numpy(flags).cuda(), groups)
            delta = _stats_delta(idx, before)
            print(f"{layout} {storage} nq {nq} k {k} assignment '{name}' route {route}: filter_stats advanced by {delta}")
            assert delta == ((1, 0) if route == "pass" else (0, 0)), (name, route, delta)
            assert _same(got, ref), (name, route)
            assert _same(idx.search_grouped(q, k, words, torch.from_numpy(groups).cuda()), ref), (name, route, "packed")
        ids = ref[1].cpu().numpy()
        for qi in range(nq):                                 # no returned id is masked out for its query; the padding is the group's
            row = ids[qi]
            assert flags[groups[qi]][row[row >= 0]].all() and (row >= 0).sum() == min(k, flags[groups[qi]].sum()), (name, qi)
        if name == "one group":                              # one group is the masked search
            monkeypatch.setenv("SR_SUBSET_DENSE_ROUTE", "gather")
            assert _same(idx.search(q, k, mask=flags[4]), ref)
    # the oracle, first 8 queries of the mixed assignment
    key = ("oracle", H, N, storage, nq)
    if key not in _CACHE:
        _CACHE[key] = O.dense_scores_fma(Q[:8], Ds, O.mfma_korder(H))
    full = _CACHE[key]
    _grouped_route(monkeypatch, "pass")
    got = idx.search_grouped(q, k, words, np.arange(nq) % 6)
    for qi in range(8):
        allowed = np.flatnonzero(flags[qi % 6]).astype(np.int64)
        os_, oi = O.topk_rows(full[qi:qi + 1, allowed], k)
        want_i = np.where(oi >= 0, allowed[np.maximum(oi, 0)] if len(allowed) else -1, -1)
        assert np.array_equal(got[1][qi:qi + 1].cpu().numpy(), want_i), qi
        assert np.array_equal(got[0][qi:qi + 1].cpu().numpy().view(np.uint32), os_.view(np.uint32)), qi


# ------------------------------------------------------------------------------------------ the mask is the query's own ---
@pytest.mark.parametrize("route", ["pass", "loop"])
def test_the_mask_is_the_querys_own(monkeypatch, route):
    H, N, nq, k = 256, 12000, 70, 10
    idx, Ds = _index(H, N, "contiguous", "fp32")
    aimed = (100, 6001, 11990)            # first tile, mid-corpus, the last partial tile
    flags = np.ones((2, N), bool)
    flags[0, list(aimed)] = False         # group 0 excludes the documents the queries are aimed at, and one of the twins (300, 7000)
    flags[0, 7000] = False
    rng = np.random.default_rng(5)
    Q = (rng.standard_normal((nq, H), dtype=np.float32) * (0.5 / np.sqrt(H))).astype(np.float32)
    groups = rng.integers(0, 2, nq)
    for i, j in enumerate(aimed):         # two identical queries, one per group
        Q[2 * i] = Q[2 * i + 1] = Ds[j] * np.float32(3.0)
        groups[2 * i], groups[2 * i + 1] = 0, 1
    Q[6] = Q[7] = Ds[300] * np.float32(2.0)
    groups[6], groups[7] = 0, 1
    q = torch.from_numpy(Q).cuda()
    _grouped_route(monkeypatch, route)
    scores, ids = idx.search_grouped(q, k, flags, groups)
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    for i, j in enumerate(aimed):
        assert j not in ids[2 * i] and ids[2 * i + 1, 0] == j, (j, ids[2 * i], ids[2 * i + 1])
    assert ids[6, 0] == 300 and 7000 not in ids[6]                       # one twin allowed
    assert ids[7, 0] == 300 and ids[7, 1] == 7000 and scores[7, 0].view(np.uint32) == scores[7, 1].view(np.uint32)   # both: ascending doc index
    assert _same((torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda()), _per_group_masked(monkeypatch, idx, q, k, flags, groups))


# ------------------------------------------------------------------------------------------------- re-do under groups ---
def test_redo_under_groups(monkeypatch):
    """The twin blocks of test_redo_under_a_mask: three blocks of 3 000 exact twins, a query aimed at each.  Groups 0 and 1 allow all of
    blocks 1 and 2 and 50 twins of block 3: the queries aimed at blocks 1 and 2 - one in each of these groups - cannot be certified (more
    than kp - k allowed ties at the cut) and are re-done under their own group's list; the third is certified.  Group 2 allows no twin
    block; its zero query (every score 0) is re-done as well."""
    from scaling_retriever_amd.scoring import DenseIndexHIP
    rng = np.random.default_rng(17)
    H, k, nq, N = 256, 100, 300, 40000
    D = rng.standard_normal((N, H), dtype=np.float32)
    twins = rng.standard_normal((3, H), dtype=np.float32)
    for t in range(3):
        D[5000 + 3000 * t:8000 + 3000 * t] = twins[t]
    Q = rng.standard_normal((nq, H), dtype=np.float32)
    for t, q_ in enumerate((4, 150, 299)):
        Q[q_] = twins[t] * 3.0
    Q[5] = 0
    flags = np.ones((3, N), bool)
    flags[0, 11050:14000] = False
    flags[1, 11050:14000] = False
    flags[1, 20000:20100] = False          # group 1 is another set than group 0
    flags[2, 5000:14000] = False
    groups = np.arange(nq) % 3
    groups[4], groups[150], groups[299], groups[5] = 0, 1, 0, 2
    idx = DenseIndexHIP(H)
    idx.set_precision("fp32_filtered")
    idx.add_host_rows(D[:20000])
    idx.add_host_rows(D[20000:])
    q = torch.from_numpy(Q).cuda()
    _grouped_route(monkeypatch, "loop")
    ref = idx.search_grouped(q, k, flags, groups)
    assert idx.filter_stats() == (0, 0)
    _grouped_route(monkeypatch, "pass")
    got = idx.search_grouped(q, k, flags, groups)
    cert, redone = idx.filter_query_stats()
    print(f"redo under groups: certified {cert}, redone {redone}")
    assert idx.filter_stats() == (0, 1) and cert + redone == nq and 3 <= redone <= 16, (cert, redone)
    assert _same(got, ref)
    assert _same(got, _per_group_masked(monkeypatch, idx, q, k, flags, groups))
    ids = got[1].cpu().numpy()
    assert set(ids[299, :50].tolist()) == set(range(11000, 11050))       # the 50 allowed twins lead query 299
    assert np.array_equal(ids[5], np.flatnonzero(flags[2])[:k])          # all ties: ascending doc index
    idx.close()


# ------------------------------------------------------------------------------------------------ inapplicable pass ---
def test_inapplicable_pass_is_served_by_the_loop(monkeypatch):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    rng = np.random.default_rng(23)
    H, N = 256, 12000
    D = rng.standard_normal((N, H), dtype=np.float32)
    flags = rng.random((3, N)) < 0.5
    Dn = D.copy()
    Dn[17, 3] = np.inf
    flags_n = flags.copy()
    flags_n[:, 17] = False
    cases = [("nq 17", D, "fp32_filtered", 17, 100, flags), ("fp32 precision", D, "fp32", 100, 100, flags),
             ("k 3000", D, "fp32_filtered", 100, 3000, flags), ("non-finite row, masked out", Dn, "fp32_filtered", 100, 100, flags_n)]
    for name, rows, precision, nq, k, fl in cases:
        idx = DenseIndexHIP(H)
        idx.set_precision(precision)
        idx.add_host_rows(rows[:7000])
        idx.add_host_rows(rows[7000:])
        q = torch.from_numpy(rng.standard_normal((nq, H), dtype=np.float32)).cuda()
        groups = np.arange(nq) % 3
        ref = _per_group_masked(monkeypatch, idx, q, k, fl, groups)
        _grouped_route(monkeypatch, "pass")
        assert _same(idx.search_grouped(q, k, fl, groups), ref), name
        assert idx.filter_stats() == (0, 0) and idx.filter_query_stats() == (0, 0), (name, idx.filter_stats())
        idx.close()


# --------------------------------------------------------------------------------------------------------------- errors ---
def test_grouped_errors_leave_the_index_usable(monkeypatch):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import DenseIndexHIP, pack_doc_masks
    rng = np.random.default_rng(29)
    H, nq = 256, 100
    D = rng.standard_normal((5000, H), dtype=np.float32)
    idx = DenseIndexHIP(H)
    idx.set_precision("fp32_filtered")
    idx.add_host_rows(D[:3000], id_base=0, id_stride=2)      # ids 0, 2, .., 5998
    idx.add_host_rows(D[3000:], id_base=1, id_stride=2)      # ids 1, 3, .., 3999: the odd ids from 4001 on name no document
    assert idx.ntotal == 5000 and idx.id_end == 5999
    q = torch.from_numpy(rng.standard_normal((nq, H), dtype=np.float32)).cuda()
    valid = np.zeros(5999, bool)
    valid[0::2] = True
    valid[1:4000:2] = True
    flags = valid[None, :] & (rng.random((3, 5999)) < 0.5)
    groups = np.arange(nq) % 3
    ref = _per_group_masked(monkeypatch, idx, q, 10, flags, groups)
    for route in ("pass", "loop"):
        _grouped_route(monkeypatch, route)
        bad_groups = groups.copy()
        bad_groups[7], bad_groups[11] = 3, -1
        with pytest.raises(ValueError, match="query 7 "):
            idx.search_grouped(q, 10, flags, bad_groups)
        bad_groups[7] = 0
        with pytest.raises(ValueError, match="query 11 "):
            idx.search_grouped(q, 10, flags, bad_groups)
        with pytest.raises(ValueError, match="n_bits=5998"):
            idx.search_grouped(q, 10, flags[:, :5998], groups)
        with pytest.raises(ValueError, match="words"):
            idx.search_grouped(q, 10, np.zeros((3, 190), np.uint32), groups)
        bad = flags.copy()
        bad[2, 4001] = True                                  # a gap bit, in group 2 only
        bad[2, 4411] = True
        with pytest.raises(ValueError, match="group 2: mask bit 4001 "):
            idx.search_grouped(q, 10, bad, groups)
        assert _same(idx.search_grouped(q, 10, flags, groups), ref)          # a following valid call returns the right answer
    assert idx.filter_stats() == (1, 0)                      # the valid call on the pass route; an invalid one never reaches the pass
    # an invalid call leaves every output row as padding
    words = pack_doc_masks(torch.from_numpy(bad).cuda())
    bad_groups = groups.copy()
    bad_groups[42] = 3
    for gr, needle in ((groups, b"4001"), (bad_groups, b"query 42 ")):
        g32 = torch.from_numpy(gr.astype(np.int32)).cuda()
        w = words if needle == b"4001" else pack_doc_masks(torch.from_numpy(flags).cuda())
        out_s = torch.full((nq, 10), 7.0, device="cuda")
        out_i = torch.full((nq, 10), 7, dtype=torch.int64, device="cuda")
        rc = idx.lib.sr_dense_search_grouped(idx._h, ctypes.c_void_p(q.data_ptr()), nq, 10, ctypes.c_void_p(w.data_ptr()), 3, 5999,
                                             ctypes.c_void_p(g32.data_ptr()), ctypes.c_void_p(out_s.data_ptr()),
                                             ctypes.c_void_p(out_i.data_ptr()), _lib.stream_ptr())
        assert rc == _lib.SR_ERR_INVALID and needle in idx.lib.sr_last_error(), idx.lib.sr_last_error()
        assert bool((out_i == -1).all()) and bool((out_s == float(FMIN)).all()), needle
    assert _same(idx.search_grouped(q, 10, flags, groups), ref)
    idx.close()


# ------------------------------------------------------------------------------------------------------------ wide rows ---
def test_grouped_pass_wide_rows(monkeypatch):
    H, N, nq, k = 2048, 9000, 130, 100
    idx, Ds = _index(H, N, "contiguous", "fp32")
    rng = np.random.default_rng(41)
    flags = np.stack([rng.random(N) < 0.5, rng.random(N) < 0.1, np.ones(N, bool), np.arange(N) % 7 == 3])
    Q = (rng.standard_normal((nq, H), dtype=np.float32) * (0.5 / np.sqrt(H))).astype(np.float32)
    q = torch.from_numpy(Q).cuda()
    groups = np.arange(nq) % 4
    ref = _per_group_masked(monkeypatch, idx, q, k, flags, groups)
    _grouped_route(monkeypatch, "pass")
    before = idx.filter_stats()
    got = idx.search_grouped(q, k, flags, groups)
    assert _stats_delta(idx, before) == (1, 0)
    assert _same(got, ref)


# --------------------------------------------------------------------------------------------------------- upper layers ---
def test_search_knn_under_groups(monkeypatch):
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    rng = np.random.default_rng(31)
    H, N, nq, k = 256, 6000, 80, 20
    D = rng.standard_normal((N, H), dtype=np.float32)
    ix = DenseFlatIndexer()
    ix.init_index(H)
    ix.index_data(D[:2500], [f"p{i}" for i in range(2500)])
    ix.index_data(D[2500:], [f"p{i}" for i in range(2500, N)])
    Q = rng.standard_normal((nq, H), dtype=np.float32)
    flags = rng.random((3, N)) < 0.3
    groups = np.arange(nq) % 3
    monkeypatch.setenv("SR_DEV_SWITCHES", "1")
    monkeypatch.setenv("SR_SUBSET_DENSE_ROUTE", "gather")
    ref_lists, ref_scores = [None] * nq, np.zeros((nq, k), np.float32)
    for g in range(3):
        sel = np.flatnonzero(groups == g)
        lists, scores = ix.search_knn(Q[sel], k, allowed_mask=flags[g])
        for n, qi in enumerate(sel):
            ref_lists[qi] = lists[n]
        ref_scores[sel] = np.asarray(scores)
    for route in ("pass", "loop"):
        _grouped_route(monkeypatch, route)
        before = ix.index.filter_stats()
        lists, scores = ix.search_knn(Q, k, allowed_masks=flags, query_group=groups)
        assert _stats_delta(ix.index, before) == ((1, 0) if route == "pass" else (0, 0))
        assert lists == ref_lists and np.array_equal(np.asarray(scores).view(np.uint32), ref_scores.view(np.uint32)), route
        s2, i2 = ix.search_arrays(Q, k, allowed_masks=torch.from_numpy(flags), query_group=torch.from_numpy(groups))
        assert np.array_equal(np.asarray(s2).view(np.uint32), ref_scores.view(np.uint32)) and i2.shape == (nq, k)
    with pytest.raises(ValueError, match="not both"):
        ix.search_knn(Q, k, allowed_mask=flags[0], allowed_masks=flags, query_group=groups)
    with pytest.raises(ValueError, match="not both"):
        ix.search_knn(Q, k, allowed_ids=["p1"], allowed_masks=flags, query_group=groups)
    with pytest.raises(ValueError, match="go together"):
        ix.search_knn(Q, k, allowed_masks=flags)
    with pytest.raises(ValueError, match="go together"):
        ix.search_knn(Q, k, query_group=groups)
    with pytest.raises(ValueError, match="one flag per index position"):
        ix.search_knn(Q, k, allowed_masks=flags[:, :-1], query_group=groups)
    with pytest.raises(ValueError, match="one group id per query"):
        ix.search_knn(Q, k, allowed_masks=flags, query_group=groups[:-1])
