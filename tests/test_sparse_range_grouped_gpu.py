"""Sparse range search under a document bitmap per query (sr_sparse_range_count_grouped / _fill_grouped,
SparseIndexHIP.range_search(masks=, query_group=)).

Collections, queries, thresholds and the cached oracle lists are those of tests/test_sparse_range_gpu.py (numba_score_float per query
and threshold), the named masks those of tests/test_sparse_range_mask_gpu.py; the expected list of query q is the oracle's with the
documents whose bit is clear in masks[group[q]] removed.  In addition the result must equal one range_search(mask=) per group.  Lims,
ids and score bits are compared for EQUALITY.

Group patterns: one group over each named mask (the masked call byte for byte); three groups dealt round-robin; one group per query;
a list with an unused group and an all-clear group.  The thresholds of tests/test_sparse_range_gpu.py include -1.0 and -inf, under which
the zero-score documents of the query's own allowed set are hits."""
import ctypes

import numpy as np
import pytest
import torch

import test_sparse_range_gpu as B
import test_sparse_range_mask_gpu as M

pytestmark = pytest.mark.gpu


def _expected(n_docs, thr, allowed, group, id_base=0, id_stride=1):
    lims = np.zeros(len(thr) + 1, np.int64)
    scores, ids = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
    for q, t in enumerate(thr):
        pos, s = B._oracle(n_docs, q, t)
        keep = allowed[group[q]][pos]
        lims[q + 1] = lims[q] + int(keep.sum())
        scores.append(s[keep])
        ids.append(id_base + pos[keep] * id_stride)
    return lims, np.concatenate(scores).astype(np.float32), np.concatenate(ids).astype(np.int64)


def _patterns(n_docs, nq):
    m = M._masks(n_docs)
    rng = np.random.default_rng(900 + n_docs + nq)
    three = np.stack([m["r50"], m.get("tiles", m["r03"]), m["last"]])
    out = {
        "round_robin": (three, np.arange(nq) % 3),
        "per_query": (rng.random((nq, n_docs)) < rng.random((nq, 1)), np.arange(nq)),
        # group 2 has no query, group 1 allows nothing
        "unused_and_clear": (np.stack([m["r50"], m["none"], m["all"], m["r03"]]), np.array([0, 1, 3])[np.arange(nq) % 3]),
    }
    return {k: (a, g.astype(np.int64)) for k, (a, g) in out.items()}


def _per_group(idx, nq, thr, allowed, group, **kw):
    indptr, cols, vals = B._csr(nq)
    lists = [None] * nq
    for g in np.unique(group):
        sel = np.nonzero(group == g)[0]
        sub_ptr = np.concatenate([[0], np.cumsum(indptr[sel + 1] - indptr[sel])]).astype(np.int64)
        take = np.concatenate([np.arange(indptr[j], indptr[j + 1]) for j in sel] + [np.zeros(0, np.int64)]).astype(np.int64)
        lims, s, i = (t.cpu().numpy() for t in idx.range_search(sub_ptr, cols[take], vals[take], thr[sel], mask=allowed[g], **kw))
        for j, qi in enumerate(sel):
            lists[qi] = (s[lims[j]:lims[j + 1]], i[lims[j]:lims[j + 1]])
    lims = np.concatenate([[0], np.cumsum([len(x[0]) for x in lists])]).astype(np.int64)
    return lims, np.concatenate([x[0] for x in lists]).astype(np.float32), np.concatenate([x[1] for x in lists]).astype(np.int64)


@pytest.mark.parametrize("nq", [1, 5, B.NQ_ALL])
@pytest.mark.parametrize("n_docs", B.SHAPES)
def test_grouped_range_equals_filtered_oracle(n_docs, nq):
    idx = B._index(n_docs)
    for rot in ((0, 1, 3, 6) if nq < B.KINDS else (0,)):          # nq = 1: the thresholds 0.0, -1.0, the 3 000th best and -inf in turn
        thr = B._thresholds(n_docs, nq, rot)
        what = f"n_docs={n_docs} nq={nq} rot={rot}"
        zeros = np.zeros(nq, np.int64)
        for name, allowed in M._masks(n_docs).items():
            got = idx.range_search(*B._csr(nq), thr, masks=allowed[None], query_group=zeros)
            B._assert_equal(got, _expected(n_docs, thr, allowed[None], zeros), f"{what} G=1 {name}")
            assert M._same(got, idx.range_search(*B._csr(nq), thr, mask=allowed)), name      # one group: the masked call
        for name, (allowed, group) in _patterns(n_docs, nq).items():
            got = idx.range_search(*B._csr(nq), thr, masks=allowed, query_group=group)
            B._assert_equal(got, _expected(n_docs, thr, allowed, group), f"{what} {name}")
            if name != "per_query":
                B._assert_equal(got, _per_group(idx, nq, thr, allowed, group), f"{what} {name} per group")
            if name == "unused_and_clear":
                assert not np.diff(got[0].cpu().numpy())[group == 1].any()


def test_zero_score_documents_follow_their_own_groups_bits():
    """Queries without any term: every score is +0.0, so under a negative threshold the hits are exactly the set bits of the query's group."""
    n_docs = 32805
    idx = B._index(n_docs)
    m = M._masks(n_docs)
    allowed = np.stack([m["tiles"], m["r03"], m["none"]])
    group = np.array([0, 0, 1, 2, 1, 0])
    thr = np.array([0.0, -0.5, -0.5, -0.5, np.nan, -np.inf], np.float32)
    lims, s, i = idx.range_search(np.zeros(7, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), thr, masks=allowed, query_group=group)
    m0, m1 = int(allowed[0].sum()), int(allowed[1].sum())
    assert np.diff(lims.cpu().numpy()).tolist() == [0, m0, m1, 0, 0, m0] and bool((s == 0).all())
    want = np.concatenate([np.nonzero(allowed[0])[0], np.nonzero(allowed[1])[0], np.nonzero(allowed[0])[0]])
    assert np.array_equal(i.cpu().numpy(), want)


def test_ids_chunks_scores_forms_and_repeatability(monkeypatch):
    from scaling_retriever_amd.scoring import pack_doc_masks
    n_docs, nq = 32805, B.NQ_ALL
    idx = B._index(n_docs)
    thr = B._thresholds(n_docs, nq)
    allowed, group = _patterns(n_docs, nq)["round_robin"]
    want = _expected(n_docs, thr, allowed, group, 7, 3)
    got = idx.range_search(*B._csr(nq), thr, id_base=7, id_stride=3, masks=allowed, query_group=group)
    B._assert_equal(got, want, "default chunking")
    B._assert_equal(got, _per_group(idx, nq, thr, allowed, group, id_base=7, id_stride=3), "per group")
    monkeypatch.setenv("SR_SPARSE_RANGE_CHUNK_TILES", "2")
    again = idx.range_search(*B._csr(nq), thr, id_base=7, id_stride=3, masks=allowed, query_group=group)
    B._assert_equal(again, want, "two tiles per chunk")
    monkeypatch.delenv("SR_SPARSE_RANGE_CHUNK_TILES")
    plain = idx.range_search(*B._csr(nq), thr, masks=allowed, query_group=group)
    assert int(plain[0][-1]) > 1000
    assert M._same(idx.range_search(*B._csr(nq), thr, masks=allowed, query_group=group), plain)      # two calls, the same bytes
    pairs = idx.score_pairs(*B._csr(nq), plain[0], plain[2])
    assert torch.equal(pairs.view(torch.int32), plain[1].view(torch.int32))
    # packed words whose last word has every bit at or beyond n_docs set: those bits are ignored
    words = pack_doc_masks(torch.from_numpy(allowed)).numpy().view(np.uint32).copy()
    words[:, -1] |= np.uint32((0xFFFFFFFF << (n_docs % 32)) & 0xFFFFFFFF)
    for form in (words, torch.from_numpy(words.view(np.int32)).cuda(), torch.from_numpy(allowed).cuda()):
        assert M._same(idx.range_search(*B._csr(nq), thr, masks=form, query_group=torch.from_numpy(group).cuda()), plain)


def test_errors():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr
    n_docs, nq, G = 8192, 5, 3
    idx = B._index(n_docs)
    thr = B._thresholds(n_docs, nq)
    group = np.arange(nq) % G
    flags = np.ones((G, n_docs), bool)
    with pytest.raises(ValueError, match="words"):
        idx.range_search(*B._csr(nq), thr, masks=np.zeros((G, n_docs // 32 + 1), np.uint32), query_group=group)
    with pytest.raises(ValueError):
        idx.range_search(*B._csr(nq), thr, masks=np.ones((G, n_docs - 1), bool), query_group=group)
    with pytest.raises(ValueError, match="not both"):
        idx.range_search(*B._csr(nq), thr, mask=flags[0], masks=flags, query_group=group)
    with pytest.raises(ValueError, match="go together"):
        idx.range_search(*B._csr(nq), thr, masks=flags)
    with pytest.raises(ValueError, match="query 2 is in group 3"):
        idx.range_search(*B._csr(nq), thr, masks=flags, query_group=np.array([0, 1, 3, 0, 1]))
    with pytest.raises(ValueError, match="query 1 is in group -1"):
        idx.range_search(*B._csr(nq), thr, masks=flags, query_group=np.array([0, -1, 3, 0, 1]))
    # the raw ABI, with sentinels in the outputs
    qp, qc, qv = (torch.from_numpy(a).cuda() for a in B._csr(nq))
    t = torch.from_numpy(thr).cuda()
    words = torch.full((G, n_docs // 32), -1, dtype=torch.int32, device="cuda")
    g = torch.from_numpy(group.astype(np.int32)).cuda()
    st = _lib.stream_ptr()
    err = idx.lib.sr_last_error

    def count(kind, lims, total, n_groups=G, n_bits=n_docs, groups=g):
        head = (idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(t))
        if kind == "plain":
            return idx.lib.sr_sparse_range_count(*head, _ptr(lims), ctypes.byref(total), st)
        if kind == "masked":
            return idx.lib.sr_sparse_range_count_masked(*head, _ptr(words[0]), n_docs, _ptr(lims), ctypes.byref(total), st)
        return idx.lib.sr_sparse_range_count_grouped(*head, _ptr(words), n_groups, n_bits, _ptr(groups), _ptr(lims), ctypes.byref(total), st)

    def fill(kind, lims, s, i, cap, n_groups=G, n_bits=n_docs):
        head = (idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(t))
        if kind == "plain":
            rc = idx.lib.sr_sparse_range_fill(*head, _ptr(lims), 0, 1, _ptr(s), _ptr(i), cap, st)
        elif kind == "masked":
            rc = idx.lib.sr_sparse_range_fill_masked(*head, _ptr(words[0]), n_docs, _ptr(lims), 0, 1, _ptr(s), _ptr(i), cap, st)
        else:
            rc = idx.lib.sr_sparse_range_fill_grouped(*head, _ptr(words), n_groups, n_bits, _ptr(g), _ptr(lims), 0, 1, _ptr(s), _ptr(i), cap, st)
        torch.cuda.synchronize()
        return rc

    def outputs(n):
        return (torch.full((n + 16,), B.SENTINEL_S, dtype=torch.float32, device="cuda"), torch.full((n + 16,), B.SENTINEL_I, dtype=torch.int64, device="cuda"))
    untouched = lambda s, i: bool((s == B.SENTINEL_S).all()) and bool((i == B.SENTINEL_I).all())      # noqa: E731
    # wrong n_bits, n_groups = 0: before any device work, lims and total untouched
    for kw, text in ((dict(n_bits=n_docs - 1), b"n_bits"), (dict(n_bits=n_docs + 1), b"n_bits"), (dict(n_groups=0), b"n_groups=0")):
        lims, total = torch.full((nq + 1,), 99, dtype=torch.int64, device="cuda"), ctypes.c_int64(-1)
        assert count("grouped", lims, total, **kw) == _lib.SR_ERR_INVALID and text in err()
        torch.cuda.synchronize()
        assert total.value == -1 and bool((lims == 99).all())
        s, i = outputs(0)
        assert fill("grouped", lims, s, i, 16, **kw) == _lib.SR_ERR_INVALID and text in err() and untouched(s, i)
    # a group id of -1 and of G: lims zero, total 0, no fill can follow
    for bad in (-1, G):
        gb = g.clone()
        gb[3] = bad
        lims, total = torch.full((nq + 1,), 99, dtype=torch.int64, device="cuda"), ctypes.c_int64(-1)
        assert count("grouped", lims, total, groups=gb) == _lib.SR_ERR_INVALID and f"query 3 is in group {bad}".encode() in err()
        assert total.value == 0 and not bool(lims.any())
        s, i = outputs(0)
        assert fill("grouped", lims, s, i, 16) == _lib.SR_ERR_INVALID and untouched(s, i)
    # fills after counts of every kind: only the own kind is served
    for ck in ("plain", "masked", "grouped"):
        for fk in ("plain", "masked", "grouped"):
            lims, total = torch.zeros(nq + 1, dtype=torch.int64, device="cuda"), ctypes.c_int64(-1)
            assert count(ck, lims, total) == 0 and total.value > 0
            s, i = outputs(total.value)
            rc = fill(fk, lims, s, i, total.value)
            if ck == fk:
                assert rc == 0 and not bool((i[:total.value] == B.SENTINEL_I).any()) and untouched(s[total.value:], i[total.value:]), (ck, fk)
            else:
                assert rc == _lib.SR_ERR_INVALID and b"preceding count ran" in err() and untouched(s, i), (ck, fk)
    # capacity below the total
    lims, total = torch.zeros(nq + 1, dtype=torch.int64, device="cuda"), ctypes.c_int64(-1)
    assert count("grouped", lims, total) == 0
    s, i = outputs(total.value)
    assert fill("grouped", lims, s, i, total.value - 1) == _lib.SR_ERR_INVALID and b"capacity" in err() and untouched(s, i)
