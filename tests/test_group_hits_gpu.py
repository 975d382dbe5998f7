"""GPU: the hits inside a collapsed search's groups (collapse.group_hits, csrc/group_hits.hip).  The two device steps against the plain
models of tests/group_hits_cases.py and the drivers of both heads against the definition applied to the exact score matrix -
torch.equal / array_equal on every output, scores compared as bits.  All scores are small integers (plus a few special values that
are only compared), so numpy's result is the device's bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import collapse_cases as C
import group_hits_cases as H

pytestmark = pytest.mark.gpu

FLT_MAX = H.FLT_MAX


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------- select
def _select_case(m):
    """Segments of every length at which the kernel takes another path - empty, below / at / above m, around one and two tiles of 64,
    many tiles - plus hand-made ones.  Scores run in blocks of 50 equal values (by position, so a block crosses tile boundaries) whose
    values do not descend along the segment: the best entries of a long segment lie in many tiles; ids are shuffled inside a segment."""
    rng = np.random.default_rng(100 + m)
    lens = [0, 1, 2, m - 1, m, m + 1, 63, 64, 65, 127, 128, 129, 1000, 5000]
    scores, ids, indptr, base = [], [], [0], 0
    for L in lens:
        pos = np.arange(L)
        s = (((pos // 50) * 7) % 11).astype(np.float32)
        if L == 129:
            s[128], s[0], s[64] = FLT_MAX, -FLT_MAX, 3.0
        if L == 5000:
            s[4999], s[77], s[4000] = FLT_MAX, -FLT_MAX, -FLT_MAX
        scores.append(s)
        ids.append(base + rng.permutation(L))
        base += L + 3
        indptr.append(indptr[-1] + L)
    # -0.0 and +0.0 are one score: the lower id comes first and both read back as +0.0; everything else in the segment is negative
    hand = [([-0.0, 0.0, -1.0, -2.0], [base + 5, base + 1, base + 3, base + 2]),
            ([0.0, -0.0, -0.0], [base + 19, base + 11, base + 17]),
            ([3.0, 3.0, 4.0, 3.0], [base + 23, base + 21, base + 29, base + 22])]      # three entries equal to the threshold 3.0
    for s, i in hand:
        scores.append(np.array(s, np.float32))
        ids.append(np.array(i))
        indptr.append(indptr[-1] + len(s))
    return np.concatenate(scores).astype(np.float32), np.concatenate(ids).astype(np.int64), np.array(indptr, np.int64)


def _topm(scores, ids, indptr, m, **kw):
    from scaling_retriever_amd.scoring import segment_topm
    out = segment_topm(_cuda(scores), _cuda(ids), _cuda(indptr), m, **kw)
    torch.cuda.synchronize()
    return out


def _same(got, want, what):
    for name, g, w in zip(("scores", "ids", "counts"), got, want):
        g = g.cpu()
        assert g.dtype == torch.from_numpy(w).dtype, (what, name)
        if name == "scores":
            assert np.array_equal(_bits(g.numpy()), _bits(w)), (what, name)            # -0.0 must read back as +0.0: bits, not values
        else:
            assert torch.equal(g, torch.from_numpy(w)), (what, name)


@pytest.mark.parametrize("m", [1, 2, 3, 8, 63, 64])
def test_select_equals_the_model(m):
    scores, ids, indptr = _select_case(m)
    assert np.signbit(scores).any() and (scores == 3.0).sum() > 50
    _same(_topm(scores, ids, indptr, m), H.segment_topm_model(scores, ids, indptr, m), (m, "no threshold"))
    for threshold, pad in ((3.0, 0.0), (-1.0, 0.0), (0.0, -FLT_MAX)):
        _same(_topm(scores, ids, indptr, m, threshold=threshold, pad_score=pad),
              H.segment_topm_model(scores, ids, indptr, m, threshold=threshold, pad_score=pad), (m, threshold))
    # the tie rule reads the id, not the position: the same entries in another order inside every segment give the same bytes
    rng = np.random.default_rng(m)
    perm = np.concatenate([a + rng.permutation(b - a) for a, b in zip(indptr[:-1], indptr[1:])]).astype(np.int64)
    _same(_topm(scores[perm], ids[perm], indptr, m), H.segment_topm_model(scores, ids, indptr, m), (m, "permuted"))


def test_select_empty_shapes_and_two_runs_give_the_same_bytes():
    got = _topm(np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(4, np.int64), 3)
    assert got[0].shape == (3, 3) and (got[1] == -1).all() and (got[2] == 0).all() and (got[0] == -FLT_MAX).all()
    got = _topm(np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(1, np.int64), 3)
    assert got[0].shape == (0, 3) and got[2].shape == (0,)
    scores, ids, indptr = _select_case(8)
    a, b = _topm(scores, ids, indptr, 8), _topm(scores, ids, indptr, 8)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_select_names_a_bad_indptr_on_the_device_and_the_library_stays_usable():
    scores, ids, indptr = _select_case(3)
    good = H.segment_topm_model(scores, ids, indptr, 3)
    n = len(scores)
    start = indptr.copy()
    start[0] = 1
    with pytest.raises(ValueError, match="must start at 0"):
        _topm(scores, ids, start, 3)
    _same(_topm(scores, ids, indptr, 3), good, "after a bad start")
    down = indptr.copy()
    down[5] = down[4] - 1                            # the last offset still names the arrays' length
    assert down[-1] == n
    with pytest.raises(ValueError, match="decreases behind segment 4"):
        _topm(scores, ids, down, 3)
    _same(_topm(scores, ids, indptr, 3), good, "after a decreasing indptr")


# ---------------------------------------------------------------------------------------------------------------------- expand
def _expand_case(n):
    """n documents in a 500-member group (key 7) that holds ids 31, 32, 33 and n - 1, a 40-member group (key 2^20), a single-member
    group with the table's first key (0), a pair with its last (2^31 - 1), the rest in groups of a few; slot rows with padding, a key
    twice in a row, the first and the last key; three masks: one with bits 31 and 33 and n - 1 set and 32 clear, its complement, none."""
    rng = np.random.default_rng(n)
    keys = (1000 + 17 * rng.integers(0, 13, n)).astype(np.int32)
    rest = np.setdiff1d(np.arange(n), [31, 32, 33, n - 1])
    pick = rng.permutation(rest)
    keys[np.concatenate([[31, 32, 33, n - 1], pick[:496]])] = 7
    keys[pick[496:536]] = 1 << 20
    keys[pick[536]] = 0
    keys[pick[537:539]] = (1 << 31) - 1
    small = int(keys[pick[540]])
    slot_keys = np.array([[7, 1 << 20, 0, -1, -1],
                          [(1 << 31) - 1, 7, 7, small, 0],
                          [-1, -1, -1, -1, -1],
                          [small, -1, 1 << 20, (1 << 31) - 1, 7],
                          [0, 0, 0, 0, 0],
                          [1 << 20, small, 7, -1, (1 << 31) - 1]], np.int32)
    flags = np.zeros((3, n), bool)
    flags[0] = rng.random(n) < 0.5
    flags[0, [31, 33, n - 1]], flags[0, 32] = True, False
    flags[1] = ~flags[0]
    return keys, slot_keys, flags


@pytest.mark.parametrize("n", [640, 641, 671])       # n_bits % 32 in {0, 1, 31}
def test_expand_equals_the_model(n):
    from scaling_retriever_amd.collapse import member_table
    from scaling_retriever_amd.scoring import group_members, pack_doc_masks
    keys, slot_keys, flags = _expand_case(n)
    table = H.member_table_model(keys)
    assert sorted(np.diff(table[1]).tolist())[-2:] == [40, 500] and 1 in np.diff(table[1]) and table[0][0] == 0 and table[0][-1] == (1 << 31) - 1
    members = member_table(_cuda(keys))
    for got, want in zip(members, table):
        assert torch.equal(got.cpu(), torch.from_numpy(want))
    words = pack_doc_masks(torch.from_numpy(flags), "cuda")
    query_group = np.array([0, 1, 2, 0, 1, 2])
    sk = _cuda(slot_keys)
    cases = {"no mask": (None, None), "one mask": ((words[0], n), flags[0]), "one stacked mask": ((words[:1], n), flags[0]),
             "the complement": ((words[1], n), flags[1]), "three masks": ((words, n, _cuda(query_group)), flags[query_group])}
    for name, (filt, keep) in cases.items():
        want = H.members_model(slot_keys, table, keep)
        a = group_members(sk, members, filt)
        b = group_members(sk, members, filt)
        torch.cuda.synchronize()
        assert torch.equal(a[0].cpu(), torch.from_numpy(want[0])), (n, name, "indptr")
        assert torch.equal(a[1].cpu(), torch.from_numpy(want[1])), (n, name, "ids")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (n, name, "two runs")
    # under three masks query 2 (all padding) and every slot of the all-denied mask are empty, the 500-member group included
    want = H.members_model(slot_keys, table, flags[query_group])
    sizes = np.diff(want[0]).reshape(slot_keys.shape)
    assert (sizes[2] == 0).all() and (sizes[5] == 0).all() and sizes[0, 0] > 100 and sizes[1, 1] == sizes[1, 2] > 100
    # more slots than one workgroup owns (256), so the scan crosses workgroups
    many = np.tile(slot_keys, (40, 1))
    want = H.members_model(many, table, flags[0])
    got = group_members(_cuda(many), members, (words[0], n))
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0])) and torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    empty = group_members(torch.zeros((0, 5), dtype=torch.int32, device="cuda"), members, None)
    assert empty[0].tolist() == [0] and empty[1].numel() == 0


def test_expand_names_what_is_wrong_and_the_library_stays_usable():
    from scaling_retriever_amd.collapse import member_table
    from scaling_retriever_amd.scoring import group_members, group_members_count, group_members_fill, pack_doc_masks
    n = 640
    keys, slot_keys, flags = _expand_case(n)
    table = H.member_table_model(keys)
    members = member_table(_cuda(keys))
    words = pack_doc_masks(torch.from_numpy(flags), "cuda")
    good = H.members_model(slot_keys, table, flags[0])

    def check_good(what):
        got = group_members(_cuda(slot_keys), members, (words[0], n))
        assert torch.equal(got[0].cpu(), torch.from_numpy(good[0])) and torch.equal(got[1].cpu(), torch.from_numpy(good[1])), what
    absent = slot_keys.copy()
    absent[3, 2], absent[4, 0] = 8, 9                # 8 and 9 are keys of no document
    with pytest.raises(ValueError, match="sr_group_members_count: query 3, slot 2: key 8 is not in the member table"):
        group_members(_cuda(absent), members, None)
    check_good("after an absent key")
    indptr, total = group_members_count(_cuda(slot_keys), members, None)
    with pytest.raises(ValueError, match="sr_group_members_fill: query 3, slot 2: key 8"):
        group_members_fill(_cuda(absent), members, indptr, total, None)
    check_good("after an absent key in fill")
    for bad_group in (3, -1, 1 << 40):
        groups = np.array([0, 1, 2, 0, bad_group, 7], np.int64)
        with pytest.raises(ValueError, match=r"query 4 is in group -?\d+, outside \[0, 3\)"):
            group_members(_cuda(slot_keys), members, (words, n, _cuda(groups)))
        check_good("after a bad group")
    # a mask over fewer bits than the table's ids: the first member at or beyond n_bits is named - query 0's first slot is the
    # 500-member group, whose members from 600 on are outside
    short = 600
    first = int(table[2][table[1][1]:table[1][2]][table[2][table[1][1]:table[1][2]] >= short][0])
    assert table[0][1] == 7
    with pytest.raises(ValueError, match=r"query 0, slot 0: member id %d \(entry \d+ of the member table\) is outside the mask's \[0, 600\)" % first):
        group_members(_cuda(slot_keys), members, (words[0, :(short + 31) // 32].contiguous(), short))
    check_good("after a member outside the mask")


# --------------------------------------------------------------------------------------------------------------------- drivers
def _dense_index(rows, row_dtype, precision, strided=False):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    idx = DenseIndexHIP(rows.shape[1], row_dtype=row_dtype)
    if strided:                                      # two interleaved segments: the documents keep their numbers
        for base in (0, 1):
            idx.add_device_rows(_cuda(rows[base::2]), id_base=base, id_stride=2)
    else:
        idx.add_host_rows(rows)
    idx.set_precision(precision)
    return idx


def _filters():
    rng = np.random.default_rng(11)
    flags = rng.random(C.N_DOCS) < 0.5
    group_flags = np.stack([rng.random(C.N_DOCS) < 0.6, rng.random(C.N_DOCS) < 0.1, np.zeros(C.N_DOCS, bool)])
    group_flags[2, :30] = True
    return flags, group_flags


def _check_hits(got, want, what):
    for name, g, w in zip(("scores", "ids", "counts"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(_bits(g), _bits(w)) if name == "scores" else np.array_equal(g, w), (what, name)


def _check_invariant(found, m, what):
    """hits[.., 0] is the slot's representative, id and score bits; stats carries the mean number of hits returned."""
    s, i, g, c, stats, (hs, hi, hc) = found
    valid = g >= 0
    assert torch.equal(hi[..., 0], i) and torch.equal(hs[..., 0][valid].view(torch.int32), s[valid].view(torch.int32)), what
    assert bool((hc[valid] >= 1).all()) and bool((hc[~valid] == 0).all()), what
    n = int(valid.sum())
    assert stats["mean_hits"] == pytest.approx(float(hc.clamp(max=m)[valid].sum()) / n if n else 0.0), what


NQ, K = 48, 50


@pytest.mark.parametrize("row_dtype,precision", [("fp32", "fp32"), ("fp32", "fp32_filtered"), ("fp16", "fp32"), ("fp16", "fp32_filtered")])
def test_dense_search_collapsed_hits(row_dtype, precision):
    from scaling_retriever_amd.collapse import member_table
    D, Q, keys, S = C.dense_case()
    idx = _dense_index(D, row_dtype, precision)
    flags, group_flags = _filters()
    q = _cuda(Q[:NQ])
    query_group = (np.arange(NQ) % 3).astype(np.int64)
    members = member_table(_cuda(keys))
    cases = {"all": ({}, None), "subset": (dict(subset=np.flatnonzero(flags)), flags), "mask": (dict(mask=flags), flags),
             "groups": (dict(masks=group_flags, query_group=query_group), group_flags[query_group])}
    for name, (kw, keep) in cases.items():
        collapsed = C.collapsed_ranking(C.full_ranking(S[:NQ], keep=keep), keys, K)
        plain = idx.search_collapsed(q, K, keys, **kw)
        assert len(plain) == 5 and "mean_hits" not in plain[4]                       # without hits=: today's tuple
        for m in (1, 3):
            found = idx.search_collapsed(q, K, keys, hits=m, members=members if m == 3 else None, **kw)
            assert len(found) == 6 and idx.batch_invariant is False
            for a, b in zip(found[:4], plain[:4]):
                assert torch.equal(a, b), (name, m)
            assert np.array_equal(found[2].cpu().numpy(), collapsed[2]), (name, m)
            _check_hits(found[5], H.hits_model(S[:NQ], keys, collapsed[2], keep, None, m), (name, m))
            _check_invariant(found, m, (name, m))
            hs, hi, hc = found[5]                                                      # every hit's score is the pair scorer's
            valid = hi >= 0
            indptr = torch.zeros(NQ + 1, dtype=torch.int64, device="cuda")
            indptr[1:] = torch.cumsum(valid.reshape(NQ, -1).sum(1), 0)
            pair = idx.score_pairs(q, indptr, hi[valid])
            assert torch.equal(pair.view(torch.int32), hs[valid].view(torch.int32)), (name, m)
            assert torch.equal(valid.sum(2).to(torch.int32), hc.clamp(max=m)), (name, m)
    idx.close()


def test_dense_hits_on_two_strided_segments_in_sub_batches_and_the_memory_error():
    D, Q, keys, S = C.dense_case()
    idx = _dense_index(D, "fp32", "fp32", strided=True)
    q = _cuda(Q[:NQ])
    collapsed = C.collapsed_ranking(C.full_ranking(S[:NQ]), keys, K)
    want = H.hits_model(S[:NQ], keys, collapsed[2], None, None, 3)
    whole = idx.search_collapsed(q, K, keys, hits=3)
    _check_hits(whole[5], want, "strided")
    _check_invariant(whole, 3, "strided")
    pairs = want[2].sum(1)                                                             # (query, member) pairs of every query
    assert pairs[0] > 500 and pairs.sum() > 3 * pairs.max()
    # at most max(pairs) pairs at a time: at least three sub-batches, the same bytes
    from scaling_retriever_amd.collapse import PAIR_BYTES
    small = idx.search_collapsed(q, K, keys, hits=3, fallback_bytes=int(pairs.max()) * PAIR_BYTES)
    for a, b in zip(small[5], whole[5]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    one = idx.search_collapsed(q[:1], K, keys, hits=3)
    for a, b in zip(one[5], whole[5]):
        assert torch.equal(a, b[:1])
    with pytest.raises(MemoryError, match=r"query 0 alone needs %d bytes for its %d" % (int(pairs[0]) * PAIR_BYTES, int(pairs[0]))):
        idx.search_collapsed(q, K, keys, hits=3, fallback_bytes=500 * PAIR_BYTES)      # query 0 holds the 500-member group
    for m in (0, 65):
        with pytest.raises(ValueError, match=r"integer in \[1, 64\]"):
            idx.search_collapsed(q, K, keys, hits=m)
    assert idx.batch_invariant is False
    idx.close()


@pytest.mark.parametrize("threshold", [0.0, -1.0])
def test_sparse_search_collapsed_hits(threshold):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    indptr, doc_ids, vals, qi, qc, qv, keys, S = C.sparse_case()
    idx = SparseIndexHIP(indptr, doc_ids, vals, C.S_DOCS)
    nq, k, m = len(qi) - 1, 50, 3
    above = S > threshold
    flags, group_flags = _filters()
    query_group = (np.arange(nq) % 3).astype(np.int64)
    cases = {"all": ({}, None), "subset": (dict(subset=np.flatnonzero(flags)), flags), "mask": (dict(mask=flags), flags),
             "groups": (dict(masks=group_flags, query_group=query_group), group_flags[query_group])}
    for name, (kw, keep) in cases.items():
        collapsed = C.collapsed_ranking(C.full_ranking(S, keep=above if keep is None else (keep if keep.ndim == 2 else keep[None]) & above), keys, k)
        found = idx.search_collapsed(qi, qc, qv, k, keys, threshold=threshold, hits=m, **kw)
        assert np.array_equal(found[2].cpu().numpy(), collapsed[2]), name
        want = H.hits_model(S, keys, collapsed[2], keep, np.float32(threshold), m, pad_score=np.float32(0.0))
        _check_hits(found[5], want, (threshold, name))
        _check_invariant(found, m, (threshold, name))
        if name == "all":
            assert (want[2] > m).any() and (threshold >= 0 or (want[0][want[1] >= 0] == 0).any())      # -1.0 admits zero-score members
            hs, hi, hc = found[5]
            valid = hi >= 0
            cand = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
            cand[1:] = torch.cumsum(valid.reshape(nq, -1).sum(1), 0)
            pair = idx.score_pairs(qi, qc, qv, cand, hi[valid])
            assert torch.equal(pair.view(torch.int32), hs[valid].view(torch.int32))
            # ids = 1 + 2 * position: keys are indexed by those, every other entry is a key nothing may read
            ext = np.full(1 + (C.S_DOCS - 1) * 2 + 1, -1, np.int32)
            ext[1 + 2 * np.arange(C.S_DOCS)] = keys
            moved = idx.search_collapsed(qi, qc, qv, k, ext, threshold=threshold, id_base=1, id_stride=2, hits=m)
            _check_hits(moved[5], (want[0], np.where(want[1] >= 0, 1 + 2 * want[1], -1), want[2]), (threshold, "id_base / id_stride"))
            _check_invariant(moved, m, (threshold, "id_base / id_stride"))
            small = idx.search_collapsed(qi, qc, qv, k, keys, threshold=threshold, hits=m, fallback_bytes=250_000)
            for a, b in zip(small[5], found[5]):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    idx.close()


# ---------------------------------------------------------------------------------------------------------------- indexer level
def test_dense_flat_indexer_search_collapsed_hits():
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    D, Q, keys, S = C.dense_case()
    db_ids = [f"p{i}" for i in range(C.N_DOCS)]
    labels = [f"g{g}" for g in keys.tolist()]
    ix = DenseFlatIndexer()
    ix.init_index(C.DIM)
    ix.index_data(D, db_ids)
    nq, k, m = 30, 10, 2
    flags, _ = _filters()
    for kw, keep in (({}, None), (dict(allowed_mask=flags), flags)):
        collapsed = C.collapsed_ranking(C.full_ranking(S[:nq], keep=keep), keys, k)
        hs, hi, hc = H.hits_model(S[:nq], keys, collapsed[2], keep, None, m)
        plain = ix.search_collapsed(Q[:nq], k, labels, **kw)
        got = ix.search_collapsed(Q[:nq], k, labels, hits=m, **kw)
        assert len(got) == nq
        for qn, (row, old) in enumerate(zip(got, plain)):
            assert len(row) == 4 and row[0] == old[0] and row[2] == old[2] and np.array_equal(_bits(row[1]), _bits(old[1])), qn
            assert len(row[3]) == len(row[0]) == int(collapsed[3][qn])
            for j, (passages, scores) in enumerate(row[3]):
                n = min(int(hc[qn, j]), m)
                assert passages == [f"p{i}" for i in hi[qn, j, :n]] and np.array_equal(_bits(scores), _bits(hs[qn, j, :n])), (qn, j)
                assert passages[0] == row[2][j]


def _runs_from_full(full, group_of, topk, m):
    """(group-keyed run, passage-level hits run) of the definition applied to a full ranking as run.json holds it (best first)."""
    groups, hits = {}, {}
    for qid, row in full.items():
        top, per_group = {}, {}
        for pid, score in row.items():
            g = group_of[pid]
            if g not in top and len(top) < topk:
                top[g] = score
            per_group.setdefault(g, [])
            if len(per_group[g]) < m:
                per_group[g].append((pid, score))
        groups[qid] = top
        hits[qid] = {pid: score for g in top for pid, score in per_group[g]}
    return groups, hits


def _same_run(got, want, what):
    assert got == want and list(got) == list(want) and [list(r) for r in got.values()] == [list(r) for r in want.values()], what


def test_sparse_retrieval_writes_the_hits_run(golden_dir, tmp_path):
    """SparseRetrieval.retrieve(collapse=, hits=2): hits/run.json is the definition applied to the full ranking the plain retrieve
    writes, key order included; run.json is byte for byte the file of the same call without hits; q_stats.json gains mean_hits."""
    from golden_weights import make_weights
    from test_indexer_gpu import FakeLoader, _corpus
    from scaling_retriever_amd.indexer import SparseIndexer, SparseRetrieval
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
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
    retriever("full").retrieve(loader(), topk=len(docs), threshold=0.0)
    full = json.loads((tmp_path / "full" / "run.json").read_text())
    group_of = {p: f"doc{i // 4}" for i, p in enumerate(pids)}
    want_groups, want_hits = _runs_from_full(full, group_of, 5, 2)
    assert any(len(r) > len(want_groups[q]) for q, r in want_hits.items())            # some group has a second hit
    retriever("plain").retrieve(loader(), topk=5, threshold=0.0, collapse=group_of)
    res, hits_res = retriever("hits").retrieve(loader(), topk=5, threshold=0.0, collapse=group_of, hits=2)
    assert (tmp_path / "hits" / "run.json").read_bytes() == (tmp_path / "plain" / "run.json").read_bytes()
    assert not (tmp_path / "plain" / "hits").exists()
    _same_run(json.loads((tmp_path / "hits" / "hits" / "run.json").read_text()), want_hits, "hits/run.json")
    assert res.to_dict() == want_groups and hits_res.to_dict() == want_hits
    stats = json.loads((tmp_path / "hits" / "q_stats.json").read_text())
    n_groups = sum(len(r) for r in want_groups.values())
    assert stats["collapse"]["mean_hits"] == pytest.approx(sum(len(r) for r in want_hits.values()) / n_groups)
    assert "mean_hits" not in json.loads((tmp_path / "plain" / "q_stats.json").read_text())["collapse"]
    with pytest.raises(ValueError, match="pass collapse= as well"):
        retriever("bad").retrieve(loader(), topk=5, hits=2)


from test_hybrid_search_gpu import toy  # noqa: E402,F401  (the module-scoped fixture: a tiny LlamaBiHybrid, 90 documents, 8 queries)


def test_hybrid_retriever_writes_both_hits_runs(toy):  # noqa: F811
    """HybridRetriever.retrieve(collapse=, hits=2): sparse/hits/run.json and dense/hits/run.json equal the definition applied to the
    full rankings the plain retrieve writes; both run.json files are byte for byte those of the call without hits."""
    from test_hybrid_search_gpu import _retriever
    full_ret, full_dir = _retriever(toy, "hits_full")
    n_docs = len(full_ret.dense_index.index_id_to_db_id)
    full_ret.retrieve(toy[3](), topk=n_docs)
    db_ids = list(full_ret.dense_index.index_id_to_db_id)
    group_of = {d: f"doc{i // 3}" for i, d in enumerate(db_ids)}
    plain_ret, plain_dir = _retriever(toy, "hits_plain")
    plain_ret.retrieve(toy[3](), topk=5, collapse=group_of)
    ret, out_dir = _retriever(toy, "hits_run")
    out = ret.retrieve(toy[3](), topk=5, collapse=group_of, hits=2)
    assert len(out) == 4
    for n, head in enumerate(("sparse", "dense")):
        full = json.load(open(os.path.join(full_dir, head, "run.json")))
        want_groups, want_hits = _runs_from_full(full, group_of, 5, 2)
        assert open(os.path.join(out_dir, head, "run.json"), "rb").read() == open(os.path.join(plain_dir, head, "run.json"), "rb").read(), head
        _same_run(json.load(open(os.path.join(out_dir, head, "hits", "run.json"))), want_hits, head)
        assert out[n].to_dict() == want_groups and out[2 + n].to_dict() == want_hits, head
    stats = json.load(open(os.path.join(out_dir, "sparse", "q_stats.json")))
    assert stats["collapse"]["mean_hits"] >= 1.0 and stats["collapse_dense"]["mean_hits"] >= 1.0
    with pytest.raises(ValueError, match="pass collapse= as well"):
        ret.retrieve(toy[3](), topk=5, hits=2)
