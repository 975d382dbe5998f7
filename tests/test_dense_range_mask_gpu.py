"""Dense range search under a document bitmap (sr_dense_range_count_masked / _fill_masked, DenseIndexHIP.range_search(mask=)).

Oracle, layouts, queries and thresholds are those of tests/test_dense_range_gpu.py (its cached score matrices are shared, not
recomputed): the expected list of query q is np.nonzero((S[q] > thr[q]) & allowed) in index order with those score bits.  Lims, ids
and score bits are compared for EQUALITY.

Masks are given over rows and carried to bits over [0, id_end) through the layout's ids.  N = 863 = 3 * 256 + 95 rows make four
256-row tiles, so the masks place whole skipped tiles before, between and after tiles that run: every bit, no bit, the last row alone,
random 50 % and 3 %, rows 256-511 clear between two random tiles, only the partial last tile (rows 768-862; with
SR_RANGE_CHUNK_ROWS=512 the whole first chunk is skipped), and on the strided layout every gap bit set on top."""
import ctypes

import numpy as np
import pytest
import torch

import test_dense_range_gpu as B

pytestmark = pytest.mark.gpu

SENTINEL_S, SENTINEL_I = B.SENTINEL_S, B.SENTINEL_I


def _row_masks(N):
    """name -> bool [N] over rows, the same for every test of a layout size."""
    rng = np.random.default_rng(1000 + N)
    r = np.arange(N)
    hole = rng.random(N) < 0.5
    hole[256:512] = False
    last = np.zeros(N, bool)
    last[-1] = True
    return {"all": np.ones(N, bool), "none": np.zeros(N, bool), "last": last, "r50": rng.random(N) < 0.5, "r03": rng.random(N) < 0.03,
            "hole": hole, "tail": r >= 768}


def _bits(allowed_rows, ids_of_row, id_end, gaps=False):
    """bool [id_end] over global document indices: the rows' flags at their ids; gaps=True sets every bit that names no document."""
    bits = np.ones(id_end, bool) if gaps else np.zeros(id_end, bool)
    bits[ids_of_row] = allowed_rows
    return bits


def _expected(S, thr, ids_of_row, allowed_rows):
    nq = len(thr)
    lims = np.zeros(nq + 1, np.int64)
    scores, ids = [], []
    with np.errstate(invalid="ignore"):
        for q in range(nq):
            hit = np.nonzero((S[q] > thr[q]) & allowed_rows)[0]
            lims[q + 1] = lims[q] + len(hit)
            scores.append(S[q, hit])
            ids.append(ids_of_row[hit])
    return lims, np.concatenate(scores).astype(np.float32), np.concatenate(ids).astype(np.int64)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("chunk", [None, 512])
@pytest.mark.parametrize("nq", [1, 33, 130, 300])
@pytest.mark.parametrize("H", [48, 320])
@pytest.mark.parametrize("layout", list(B.LAYOUTS))
def test_masked_range_search_equals_filtered_oracle(layout, H, nq, chunk, chunk_rows):
    chunk_rows(chunk)
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    idx, ids_of_row = B._index(layout, H, rows)
    id_end = idx.id_end
    assert id_end == ids_of_row.max() + 1
    thr = B._thresholds(S, nq)
    unmasked = idx.range_search(q[:nq], thr)
    for name, allowed in _row_masks(N).items():
        want = _expected(S, thr, ids_of_row, allowed)
        bits = _bits(allowed, ids_of_row, id_end)
        got = idx.range_search(q[:nq], thr, mask=bits)
        B._assert_equal(got, want, f"{layout} H={H} nq={nq} chunk={chunk} mask={name}")
        if name == "all":
            assert _same(got, unmasked)                                  # every bit set: the unrestricted result, byte for byte
        if name == "none":
            assert int(got[0][-1]) == 0 and not bool(got[0].any())
        if layout == "strided":                                          # set bits in the gaps of the strided segments are ignored
            assert _same(idx.range_search(q[:nq], thr, mask=_bits(allowed, ids_of_row, id_end, gaps=True)), got), name
    idx.close()


@pytest.fixture
def chunk_rows(monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("SR_RANGE_CHUNK_ROWS", raising=False)
        else:
            monkeypatch.setenv("SR_RANGE_CHUNK_ROWS", str(v))
    return set_


def test_mask_forms_scores_and_repeatability():
    """A bool tensor, a bool array and packed words (numpy / device) are one mask; every returned score is score_pairs' bit for bit;
    two calls return the same bytes."""
    from scaling_retriever_amd.scoring import pack_doc_mask
    layout, H, nq = "strided", 320, 130
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    idx, ids_of_row = B._index(layout, H, rows)
    thr = B._thresholds(S, nq)
    allowed = _row_masks(N)["r50"]
    bits = _bits(allowed, ids_of_row, idx.id_end)
    got = idx.range_search(q[:nq], thr, mask=bits)
    B._assert_equal(got, _expected(S, thr, ids_of_row, allowed), "bool array")
    assert int(got[0][-1]) > N // 2
    pairs = idx.score_pairs(q[:nq], got[0], got[2])
    assert torch.equal(pairs.view(torch.int32), got[1].view(torch.int32))
    words = pack_doc_mask(bits)
    for form in (torch.from_numpy(bits), torch.from_numpy(bits).cuda(), words, torch.from_numpy(words.view(np.int32)).cuda()):
        assert _same(idx.range_search(q[:nq], thr, mask=form), got)
    # the two halves on their own, as the hybrid search calls them
    w_dev = torch.from_numpy(words.view(np.int32)).cuda()
    qq, t, lims, total = idx.range_count(q[:nq], thr, mask=w_dev)
    s, i = idx.range_fill(qq, t, lims, total, mask=w_dev)
    assert _same((lims, s, i), got)
    # sort=True under a mask: the prefix of the masked ranking
    ls, ss, si = idx.range_search(q[:nq], thr, sort=True, mask=bits)
    fs, fi = idx.search(q[:nq], int(allowed.sum()), mask=bits)
    ls, ss, si, fs, fi = ls.cpu().numpy(), ss.cpu().numpy(), si.cpu().numpy(), fs.cpu().numpy(), fi.cpu().numpy()
    for j in range(nq):
        c = ls[j + 1] - ls[j]
        assert np.array_equal(si[ls[j]:ls[j + 1]], fi[j, :c]) and np.array_equal(ss[ls[j]:ls[j + 1]].view(np.int32), fs[j, :c].view(np.int32)), j
    idx.close()


@pytest.mark.parametrize("nq", [33, 130])
def test_fp16_rows_under_a_mask(nq):
    layout, H = "strided", 320
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    rows16 = rows.half()
    f16, ids_of_row = B._index(layout, H, rows16, row_dtype="fp16")
    twin, _ = B._index(layout, H, rows16.float())
    assert f16.stored_dtype() == "fp16"
    thr = B._thresholds(S, nq)
    for name in ("hole", "r03", "tail"):
        bits = _bits(_row_masks(N)[name], ids_of_row, f16.id_end)
        a, b = f16.range_search(q[:nq], thr, mask=bits), twin.range_search(q[:nq], thr, mask=bits)
        assert _same(a, b), name
        full = twin.range_search(q[:nq], thr)                           # the twin's unrestricted lists, filtered on the host
        keep = torch.from_numpy(bits).cuda()[full[2]]
        assert torch.equal(a[2], full[2][keep]) and torch.equal(a[1].view(torch.int32), full[1][keep].view(torch.int32)), name
    f16.close()
    twin.close()


def _raw(idx, q, thr, words, n_bits, count_nq=None, pad=16):
    """count + fill through the C ABI with sentinel-filled outputs: (rc_count, rc_fill, total, lims, scores, ids)."""
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr
    nq = q.shape[0]
    cq = nq if count_nq is None else count_nq
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    rc_count = idx.lib.sr_dense_range_count_masked(idx._h, _ptr(q), cq, _ptr(thr), _ptr(words), n_bits, _ptr(lims), ctypes.byref(total),
                                                   _lib.stream_ptr())
    n = max(total.value, 0)
    scores = torch.full((n + pad,), SENTINEL_S, dtype=torch.float32, device="cuda")
    ids = torch.full((n + pad,), SENTINEL_I, dtype=torch.int64, device="cuda")
    rc_fill = idx.lib.sr_dense_range_fill_masked(idx._h, _ptr(q), nq, _ptr(thr), _ptr(words), n_bits, _ptr(lims), _ptr(scores), _ptr(ids), n,
                                                 _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc_count, rc_fill, total.value, lims, scores, ids


def test_raw_abi_errors_and_sentinels():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr, pack_doc_mask
    layout, H, nq = "two", 48, 33
    N = B.LAYOUTS[layout][0]
    rows, q, S = B._data(N, H)
    q = q[:nq].contiguous()
    idx, ids_of_row = B._index(layout, H, rows)
    thr_np = B._thresholds(S, nq)
    thr = torch.from_numpy(thr_np).cuda()
    untouched = lambda s, i: bool((s == SENTINEL_S).all()) and bool((i == SENTINEL_I).all())      # noqa: E731
    masks = _row_masks(N)
    dev_words = lambda a: torch.from_numpy(pack_doc_mask(_bits(a, ids_of_row, idx.id_end)).view(np.int32)).cuda()      # noqa: E731

    # no bit set: all lims zero, the fill writes nothing
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, dev_words(masks["none"]), idx.id_end)
    assert rc_c == 0 and rc_f == 0 and total == 0 and not bool(lims.any()) and untouched(s, i)
    # a mask with hits: the padding behind the result is never written
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, dev_words(masks["r50"]), idx.id_end)
    assert rc_c == 0 and rc_f == 0 and total == int(lims[-1]) > 0 and untouched(s[total:], i[total:])
    B._assert_equal((lims, s[:total], i[:total]), _expected(S, thr_np, ids_of_row, masks["r50"]), "raw")
    # wrong n_bits: refused by both halves, nothing written
    w = dev_words(masks["all"])
    for bad in (idx.id_end - 1, idx.id_end + 1, 0):
        rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, bad)
        assert rc_c == _lib.SR_ERR_INVALID and rc_f == _lib.SR_ERR_INVALID and b"n_bits" in idx.lib.sr_last_error() and untouched(s, i), bad
    # a fill after a count of another nq
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, w, idx.id_end, count_nq=nq - 1)
    assert rc_c == 0 and rc_f == _lib.SR_ERR_INVALID and b"preceding count" in idx.lib.sr_last_error() and untouched(s, i)
    # a masked fill after an unmasked count, and the reverse
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(0)
    assert idx.lib.sr_dense_range_count(idx._h, _ptr(q), nq, _ptr(thr), _ptr(lims), ctypes.byref(total), _lib.stream_ptr()) == 0
    s = torch.full((total.value,), SENTINEL_S, dtype=torch.float32, device="cuda")
    i = torch.full((total.value,), SENTINEL_I, dtype=torch.int64, device="cuda")
    rc = idx.lib.sr_dense_range_fill_masked(idx._h, _ptr(q), nq, _ptr(thr), _ptr(w), idx.id_end, _ptr(lims), _ptr(s), _ptr(i), total.value,
                                            _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.SR_ERR_INVALID and b"without a mask" in idx.lib.sr_last_error() and untouched(s, i)
    assert idx.lib.sr_dense_range_count_masked(idx._h, _ptr(q), nq, _ptr(thr), _ptr(w), idx.id_end, _ptr(lims), ctypes.byref(total),
                                               _lib.stream_ptr()) == 0
    rc = idx.lib.sr_dense_range_fill(idx._h, _ptr(q), nq, _ptr(thr), _ptr(lims), _ptr(s), _ptr(i), total.value, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.SR_ERR_INVALID and b"under a mask" in idx.lib.sr_last_error() and untouched(s, i)
    # Python: a packed mask of the wrong length, a bool mask of the wrong length
    with pytest.raises(ValueError, match="words"):
        idx.range_search(q, thr, mask=np.zeros((idx.id_end + 31) // 32 + 1, np.uint32))
    with pytest.raises(ValueError):
        idx.range_search(q, thr, mask=np.ones(idx.id_end - 1, bool))
    with pytest.raises(ValueError):
        idx.range_count(q, thr, mask=np.ones(idx.id_end + 40, bool))
    # nq = 0 and an empty index
    lims, s, i = idx.range_search(q[:0], 0.0, mask=np.ones(idx.id_end, bool))
    assert lims.tolist() == [0] and s.numel() == 0
    idx.close()
    from scaling_retriever_amd.scoring import DenseIndexHIP
    empty = DenseIndexHIP(H)
    lims, s, i = empty.range_search(q, -np.inf, mask=np.zeros(0, bool))
    assert lims.tolist() == [0] * (nq + 1) and s.numel() == 0
    empty.close()


def test_indexer_allowed_ids_equal_allowed_mask_equal_filtered_lists():
    import math
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    H, N, nq = 64, 600, 5
    g = torch.Generator(device="cpu").manual_seed(5)
    rows = (torch.randn((N, H), generator=g) * (0.5 / math.sqrt(H))).numpy()
    q = (torch.randn((nq, H), generator=g) / math.sqrt(H)).numpy()
    ix = DenseFlatIndexer()
    ix.init_index(H)
    ix.index_data(rows[:320], [f"doc-{j}" for j in range(320)])
    ix.index_data(rows[320:], [f"doc-{j}" for j in range(320, N)])
    allowed = np.random.default_rng(3).random(N) < 0.3
    allowed[256:512] = False
    names = [f"doc-{j}" for j in np.nonzero(allowed)[0]]
    for sort in (True, False):
        full_ids, full_scores = ix.range_search(q, -0.05, sort=sort)
        by_ids = ix.range_search(q, -0.05, sort=sort, allowed_ids=names[::-1] + names[:3])
        by_mask = ix.range_search(q, -0.05, sort=sort, allowed_mask=allowed)
        keep_set = set(names)
        for i in range(nq):
            keep = np.array([d in keep_set for d in full_ids[i]], bool)
            want_ids = [d for d in full_ids[i] if d in keep_set]
            assert len(want_ids) > 20
            for got in (by_ids, by_mask):
                assert got[0][i] == want_ids
                assert np.array_equal(got[1][i].view(np.int32), full_scores[i][keep].view(np.int32))
    with pytest.raises(ValueError, match="not both"):
        ix.range_search(q, 0.0, allowed_ids=names, allowed_mask=allowed)
    with pytest.raises(ValueError, match="unknown"):
        ix.range_search(q, 0.0, allowed_ids=["no-such-doc"])
