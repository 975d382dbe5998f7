"""Dense range search under a document bitmap per query (sr_dense_range_count_grouped / _fill_grouped,
DenseIndexHIP.range_search(masks=, query_group=)).

Oracle, layouts, queries and thresholds are those of tests/test_dense_range_gpu.py (its cached score matrices are shared, not
recomputed): the expected list of query q is np.nonzero((S[q] > thr[q]) & allowed[group[q]]) in index order with those score bits -
numpy only, independent of the code under test.  On top of that the result must equal one range_search(mask=) per group.  Lims, ids and
score bits are compared for EQUALITY, there is no tolerance anywhere.

N = 863 = 3 * 256 + 95 rows make four 256-row tiles.  The named row masks are those of tests/test_dense_range_mask_gpu.py.  Group
patterns: one group over each named mask (must be the masked call byte for byte); three groups dealt round-robin over {r50, hole, tail}
(neighbouring query columns of one 32-column block differ, and the union is non-empty where single groups are empty); three groups in
contiguous runs of queries; one group per query with a random mask each; a list with an unused group and an all-clear group; two groups
whose union is clear on rows 256-511 (a skipped tile between tiles that run).  Layout "two" puts a stride-1 segment at id_base = 300 (a
32-row block spans two mask words), "strided" has strides 2 and 3 (the per-row gather) and is also run with every gap bit set."""
import ctypes

import numpy as np
import pytest
import torch

import test_dense_range_gpu as B
import test_dense_range_mask_gpu as M

pytestmark = pytest.mark.gpu

SENTINEL_S, SENTINEL_I = B.SENTINEL_S, B.SENTINEL_I
chunk_rows = B.chunk_rows


def _expected(S, thr, ids_of_row, allowed_rows, group):
    """allowed_rows bool [G, N] over rows, group int [nq]."""
    nq = len(thr)
    lims = np.zeros(nq + 1, np.int64)
    scores, ids = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
    with np.errstate(invalid="ignore"):
        for q in range(nq):
            hit = np.nonzero((S[q] > thr[q]) & allowed_rows[group[q]])[0]
            lims[q + 1] = lims[q] + len(hit)
            scores.append(S[q, hit])
            ids.append(ids_of_row[hit])
    return lims, np.concatenate(scores).astype(np.float32), np.concatenate(ids).astype(np.int64)


def _bits2(allowed_rows, ids_of_row, id_end, gaps=False):
    return np.stack([M._bits(a, ids_of_row, id_end, gaps) for a in allowed_rows])


def _patterns(N, nq):
    """name -> (allowed bool [G, N] over rows, group int64 [nq]); the same for every test of a shape."""
    m = M._row_masks(N)
    rng = np.random.default_rng(77 * N + nq)
    three = np.stack([m["r50"], m["hole"], m["tail"]])
    runs = np.minimum(np.arange(nq) * 3 // max(nq, 1), 2)
    hole2 = rng.random(N) < 0.3
    hole2[256:512] = False
    out = {
        "round_robin": (three, np.arange(nq) % 3),
        "runs": (three, runs),
        "per_query": (rng.random((nq, N)) < rng.random((nq, 1)), np.arange(nq)),
        # group 2 has no query, group 1 allows nothing
        "unused_and_clear": (np.stack([m["r50"], m["none"], m["all"], m["r03"]]), np.array([0, 1, 3])[np.arange(nq) % 3]),
        "union_hole": (np.stack([m["hole"], hole2]), (np.arange(nq) // 2) % 2),
    }
    return {k: (a, g.astype(np.int64)) for k, (a, g) in out.items()}


def _per_group(idx, q, thr, bits, group):
    """One range_search(mask=) per group that has a query, its lists put back in query order: (lims, scores, ids) on the host."""
    nq = len(group)
    lists = [None] * nq
    for g in np.unique(group):
        sel = np.nonzero(group == g)[0]
        lims, s, i = idx.range_search(q[torch.from_numpy(sel).cuda()], thr[sel], mask=bits[g])
        lims, s, i = lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy()
        for j, qi in enumerate(sel):
            lists[qi] = (s[lims[j]:lims[j + 1]], i[lims[j]:lims[j + 1]])
    lims = np.concatenate([[0], np.cumsum([len(x[0]) for x in lists])]).astype(np.int64)
    return lims, np.concatenate([x[0] for x in lists]).astype(np.float32), np.concatenate([x[1] for x in lists]).astype(np.int64)


@pytest.mark.parametrize("chunk", [None, 512])
@pytest.mark.parametrize("nq", [1, 33, 130, 300])
@pytest.mark.parametrize("H", [48, 320])
@pytest.mark.parametrize("layout", list(B.LAYOUTS))
def test_grouped_range_search_equals_filtered_oracle(layout, H, nq, chunk, chunk_rows):
    chunk_rows(chunk)
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    idx, ids_of_row = B._index(layout, H, rows)
    id_end = idx.id_end
    thr = B._thresholds(S, nq)
    what = f"{layout} H={H} nq={nq} chunk={chunk}"
    # one group: the masked call, byte for byte
    zeros = np.zeros(nq, np.int64)
    for name, allowed in M._row_masks(N).items():
        bits = M._bits(allowed, ids_of_row, id_end)
        got = idx.range_search(q[:nq], thr, masks=bits[None], query_group=zeros)
        B._assert_equal(got, _expected(S, thr, ids_of_row, allowed[None], zeros), f"{what} G=1 {name}")
        assert M._same(got, idx.range_search(q[:nq], thr, mask=bits)), name
    for name, (allowed, group) in _patterns(N, nq).items():
        bits = _bits2(allowed, ids_of_row, id_end)
        got = idx.range_search(q[:nq], thr, masks=bits, query_group=group)
        B._assert_equal(got, _expected(S, thr, ids_of_row, allowed, group), f"{what} {name}")
        if name in ("round_robin", "unused_and_clear"):
            B._assert_equal(got, _per_group(idx, q, thr, bits, group), f"{what} {name} per group")
        if name == "unused_and_clear":
            counts = np.diff(got[0].cpu().numpy())
            assert not counts[group == 1].any()                           # the all-clear group's queries get empty lists
        if layout == "strided":                                          # set bits in the gaps of the strided segments are ignored
            gaps = _bits2(allowed, ids_of_row, id_end, gaps=True)
            assert M._same(idx.range_search(q[:nq], thr, masks=gaps, query_group=group), got), name
    idx.close()


@pytest.mark.parametrize("nq", [33, 130])
def test_fp16_rows_under_groups(nq):
    layout, H = "strided", 320
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    rows16 = rows.half()
    f16, ids_of_row = B._index(layout, H, rows16, row_dtype="fp16")
    twin, _ = B._index(layout, H, rows16.float())
    assert f16.stored_dtype() == "fp16"
    thr = B._thresholds(S, nq)
    for name in ("round_robin", "per_query", "union_hole"):
        allowed, group = _patterns(N, nq)[name]
        bits = _bits2(allowed, ids_of_row, f16.id_end)
        a = f16.range_search(q[:nq], thr, masks=bits, query_group=group)
        b = twin.range_search(q[:nq], thr, masks=bits, query_group=group)
        assert M._same(a, b), name
        full = twin.range_search(q[:nq], thr)                           # the twin's unrestricted lists, filtered on the host
        fl, fs, fi = (t.cpu().numpy() for t in full)
        qq = np.repeat(np.arange(nq), np.diff(fl))
        keep = bits[group[qq], fi]
        assert np.array_equal(a[2].cpu().numpy(), fi[keep]) and np.array_equal(a[1].cpu().numpy().view(np.int32), fs[keep].view(np.int32)), name
        assert np.array_equal(np.diff(a[0].cpu().numpy()), np.bincount(qq[keep], minlength=nq)), name
    f16.close()
    twin.close()


def test_mask_forms_scores_and_repeatability():
    """Bool arrays / tensors and packed words (numpy / device) are one filter, group ids of any integer type too; every returned score
    is score_pairs' bit for bit; two calls return the same bytes; the two halves on their own, as the hybrid search calls them."""
    from scaling_retriever_amd.scoring import pack_doc_masks
    layout, H, nq = "two", 320, 130
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    idx, ids_of_row = B._index(layout, H, rows)
    thr = B._thresholds(S, nq)
    allowed, group = _patterns(N, nq)["round_robin"]
    bits = _bits2(allowed, ids_of_row, idx.id_end)
    got = idx.range_search(q[:nq], thr, masks=bits, query_group=group)
    B._assert_equal(got, _expected(S, thr, ids_of_row, allowed, group), "bool array")
    assert int(got[0][-1]) > N // 4
    pairs = idx.score_pairs(q[:nq], got[0], got[2])
    assert torch.equal(pairs.view(torch.int32), got[1].view(torch.int32))
    assert M._same(idx.range_search(q[:nq], thr, masks=bits, query_group=group), got)      # two calls, the same bytes
    words = pack_doc_masks(torch.from_numpy(bits))
    for form in (torch.from_numpy(bits), torch.from_numpy(bits).cuda(), words.numpy().view(np.uint32), words.cuda()):
        for gform in (group, group.astype(np.int32), torch.from_numpy(group).cuda(), group.tolist()):
            assert M._same(idx.range_search(q[:nq], thr, masks=form, query_group=gform), got)
    w_dev, g_dev = words.cuda(), torch.from_numpy(group).cuda()
    qq, t, lims, total = idx.range_count(q[:nq], thr, masks=w_dev, query_group=g_dev)
    idx.search_grouped(q[:nq], 5, w_dev, g_dev)                 # a grouped search between the halves leaves the count's state alone
    s, i = idx.range_fill(qq, t, lims, total, masks=w_dev, query_group=g_dev)
    assert M._same((lims, s, i), got)
    # sort=True under groups: the prefix of each query's own masked ranking
    ls, ss, si = (x.cpu().numpy() for x in idx.range_search(q[:nq], thr, sort=True, masks=bits, query_group=group))
    fs, fi = (x.cpu().numpy() for x in idx.search_grouped(q[:nq], int(allowed.sum(1).max()), bits, group))
    for j in range(nq):
        c = ls[j + 1] - ls[j]
        assert np.array_equal(si[ls[j]:ls[j + 1]], fi[j, :c]) and np.array_equal(ss[ls[j]:ls[j + 1]].view(np.int32), fs[j, :c].view(np.int32)), j
    idx.close()


def _raw(idx, q, thr, words, n_groups, n_bits, groups, count_nq=None, pad=16, cap_less=0):
    """count + fill through the C ABI with sentinel-filled outputs: (rc_count, rc_fill, total, lims, scores, ids)."""
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr
    nq = q.shape[0]
    cq = nq if count_nq is None else count_nq
    lims = torch.full((nq + 1,), 99, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    rc_count = idx.lib.sr_dense_range_count_grouped(idx._h, _ptr(q), cq, _ptr(thr), _ptr(words), n_groups, n_bits, _ptr(groups), _ptr(lims),
                                                    ctypes.byref(total), _lib.stream_ptr())
    n = max(total.value, 0)
    scores = torch.full((n + pad,), SENTINEL_S, dtype=torch.float32, device="cuda")
    ids = torch.full((n + pad,), SENTINEL_I, dtype=torch.int64, device="cuda")
    rc_fill = idx.lib.sr_dense_range_fill_grouped(idx._h, _ptr(q), nq, _ptr(thr), _ptr(words), n_groups, n_bits, _ptr(groups), _ptr(lims),
                                                  _ptr(scores), _ptr(ids), n - cap_less, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc_count, rc_fill, total.value, lims, scores, ids


def test_raw_abi_errors_and_sentinels():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr, pack_doc_masks
    layout, H, nq = "two", 48, 33
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    q = q[:nq].contiguous()
    idx, ids_of_row = B._index(layout, H, rows)
    thr_np = B._thresholds(S, nq)
    thr = torch.from_numpy(thr_np).cuda()
    untouched = lambda s, i: bool((s == SENTINEL_S).all()) and bool((i == SENTINEL_I).all())      # noqa: E731
    allowed, group = _patterns(N, nq)["round_robin"]
    G = len(allowed)
    w = pack_doc_masks(torch.from_numpy(_bits2(allowed, ids_of_row, idx.id_end))).cuda()
    g = torch.from_numpy(group.astype(np.int32)).cuda()
    err = idx.lib.sr_last_error

    # the plain case: the padding behind the result is never written
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, G, idx.id_end, g)
    assert rc_c == 0 and rc_f == 0 and total == int(lims[-1]) > 0 and untouched(s[total:], i[total:])
    B._assert_equal((lims, s[:total], i[:total]), _expected(S, thr_np, ids_of_row, allowed, group), "raw")
    # capacity below the total: refused, nothing written
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, G, idx.id_end, g, cap_less=1)
    assert rc_c == 0 and rc_f == _lib.SR_ERR_INVALID and b"capacity" in err() and untouched(s, i)
    # wrong n_bits, n_groups = 0: refused by both halves before any device work, lims and total untouched
    for bad in (idx.id_end - 1, idx.id_end + 1, 0):
        rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, G, bad, g)
        assert rc_c == _lib.SR_ERR_INVALID and rc_f == _lib.SR_ERR_INVALID and b"n_bits" in err() and untouched(s, i), bad
        assert total == -1 and bool((lims == 99).all())
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, 0, idx.id_end, g)
    assert rc_c == _lib.SR_ERR_INVALID and rc_f == _lib.SR_ERR_INVALID and b"n_groups=0" in err() and untouched(s, i)
    assert total == -1 and bool((lims == 99).all())
    # a group id of -1 and of G: named, lims zero, total 0, and no fill can follow
    for bad_id, at in ((-1, 7), (G, 20)):
        gb = g.clone()
        gb[at] = bad_id
        gb[at + 3] = bad_id
        rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, G, idx.id_end, gb)
        assert rc_c == _lib.SR_ERR_INVALID and total == 0 and not bool(lims.any())
        assert rc_f == _lib.SR_ERR_INVALID and untouched(s, i)
        rc = idx.lib.sr_dense_range_count_grouped(idx._h, _ptr(q), nq, _ptr(thr), _ptr(w), G, idx.id_end, _ptr(gb), _ptr(lims), ctypes.byref(ctypes.c_int64(0)),
                                                  _lib.stream_ptr())
        assert rc == _lib.SR_ERR_INVALID and f"query {at} is in group {bad_id}".encode() in err()
    # a fill after a count of another nq
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, G, idx.id_end, g, count_nq=nq - 1)
    assert rc_c == 0 and rc_f == _lib.SR_ERR_INVALID and b"preceding count" in err() and untouched(s, i)
    # a fill after a count of another kind, in all directions
    one = w[0].contiguous()
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(0)
    st = _lib.stream_ptr()
    counts = {
        "plain": lambda: idx.lib.sr_dense_range_count(idx._h, _ptr(q), nq, _ptr(thr), _ptr(lims), ctypes.byref(total), st),
        "masked": lambda: idx.lib.sr_dense_range_count_masked(idx._h, _ptr(q), nq, _ptr(thr), _ptr(one), idx.id_end, _ptr(lims), ctypes.byref(total), st),
        "grouped": lambda: idx.lib.sr_dense_range_count_grouped(idx._h, _ptr(q), nq, _ptr(thr), _ptr(w), G, idx.id_end, _ptr(g), _ptr(lims),
                                                                ctypes.byref(total), st),
    }
    fills = {
        "plain": lambda s, i, n: idx.lib.sr_dense_range_fill(idx._h, _ptr(q), nq, _ptr(thr), _ptr(lims), _ptr(s), _ptr(i), n, st),
        "masked": lambda s, i, n: idx.lib.sr_dense_range_fill_masked(idx._h, _ptr(q), nq, _ptr(thr), _ptr(one), idx.id_end, _ptr(lims), _ptr(s), _ptr(i), n, st),
        "grouped": lambda s, i, n: idx.lib.sr_dense_range_fill_grouped(idx._h, _ptr(q), nq, _ptr(thr), _ptr(w), G, idx.id_end, _ptr(g), _ptr(lims), _ptr(s),
                                                                      _ptr(i), n, st),
    }
    for ck in counts:
        for fk in fills:
            assert counts[ck]() == 0 and total.value > 0
            s = torch.full((total.value,), SENTINEL_S, dtype=torch.float32, device="cuda")
            i = torch.full((total.value,), SENTINEL_I, dtype=torch.int64, device="cuda")
            rc = fills[fk](s, i, total.value)
            torch.cuda.synchronize()
            if ck == fk:
                assert rc == 0 and not bool((i == SENTINEL_I).any()), (ck, fk)
            else:
                assert rc == _lib.SR_ERR_INVALID and b"preceding count ran" in err() and untouched(s, i), (ck, fk)
    # a grouped fill with another number of groups than its count
    assert counts["grouped"]() == 0
    s = torch.full((total.value,), SENTINEL_S, dtype=torch.float32, device="cuda")
    i = torch.full((total.value,), SENTINEL_I, dtype=torch.int64, device="cuda")
    rc = idx.lib.sr_dense_range_fill_grouped(idx._h, _ptr(q), nq, _ptr(thr), _ptr(w), G - 1, idx.id_end, _ptr(g), _ptr(lims), _ptr(s), _ptr(i), total.value, st)
    torch.cuda.synchronize()
    assert rc == _lib.SR_ERR_INVALID and b"n_groups" in err() and untouched(s, i)
    # Python: a group id outside the groups, nq = 0, an empty index
    with pytest.raises(ValueError, match="query 4 is in group 3"):
        idx.range_search(q, thr, masks=w, query_group=np.where(np.arange(nq) == 4, 3, 0))
    with pytest.raises(ValueError, match="is in group"):
        idx.range_search(q, thr, masks=w, query_group=np.where(np.arange(nq) == 4, 2 ** 40, 0))
    lims, s, i = idx.range_search(q[:0], 0.0, masks=w, query_group=np.zeros(0, np.int64))
    assert lims.tolist() == [0] and s.numel() == 0
    idx.close()
    from scaling_retriever_amd.scoring import DenseIndexHIP
    empty = DenseIndexHIP(H)
    lims, s, i = empty.range_search(q, -np.inf, masks=np.zeros((2, 0), bool), query_group=np.arange(nq) % 2)
    assert lims.tolist() == [0] * (nq + 1) and s.numel() == 0
    empty.close()
