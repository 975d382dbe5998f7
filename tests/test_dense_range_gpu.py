"""Dense range search (sr_dense_range_count / _fill, DenseIndexHIP.range_search): every document with score > thr[q], as CSR.

Oracle: the CPU score matrix oracle.scoring.dense_scores_fma(Q, D, mfma_korder(H)) - the exact kernel's fmaf chain.  The expected
list of query q is np.nonzero(S[q] > thr[q]) in index order with those score bits; ids, score bits and lims are compared for
EQUALITY, there is no tolerance anywhere.

Shapes are the smallest that reach every path: N = 863 = 3 * 256 + 95 as one segment and as two (300 + 563, with plain and with
strided ids) and N = 129; H = 48 (3 k-steps: the pipeline's prologue covers the whole loop) and 320; nq = 1 and 33 (128-wide query
tile, partial), 130 (256-wide tile, partial) and 300 (two query tiles); the default chunking (one 256-row tile per chunk here)
and SR_RANGE_CHUNK_ROWS=256 / 512 (several tiles per chunk, last chunk partial)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NQ_MAX = 300
SENTINEL_S, SENTINEL_I = -12345.0, -777
_CACHE = {}

# name -> (N, [(rows, id_base, id_stride)])
LAYOUTS = {
    "one": (863, [(863, 0, 1)]),
    "two": (863, [(300, 0, 1), (563, 300, 1)]),
    "strided": (863, [(300, 7, 2), (563, 2000, 3)]),
    "small": (129, [(129, 0, 1)]),
}


def _data(N, H):
    """(rows cuda, queries cuda, S = oracle scores [NQ_MAX, N]) made once per shape and never modified."""
    key = (N, H)
    if key not in _CACHE:
        from oracle import scoring as SC
        g = torch.Generator(device="cpu").manual_seed(7000 * N + H)
        rows = torch.randn((N, H), generator=g) * (0.5 / math.sqrt(H))
        q = torch.randn((NQ_MAX, H), generator=g) / math.sqrt(H)
        S = SC.dense_scores_fma(q.numpy(), rows.numpy(), SC.mfma_korder(H))
        S.setflags(write=False)
        _CACHE[key] = (rows.cuda(), q.cuda(), S)
    return _CACHE[key]


def _index(layout, H, rows, row_dtype="fp32"):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    idx = DenseIndexHIP(H, row_dtype=row_dtype)
    r0, ids = 0, []
    for n, base, stride in LAYOUTS[layout][1]:
        idx.add_device_rows(rows[r0:r0 + n], id_base=base, id_stride=stride)
        ids.append(base + stride * np.arange(n, dtype=np.int64))
        r0 += n
    return idx, np.concatenate(ids)


def _thresholds(S, nq):
    """One kind per query, neighbours differ: (q + 3) % 8 = 0 above the row maximum (0 hits), 1 the maximum itself (0 hits:
    strict), 2 the second largest score (1 hit), 3 the 5 % quantile from the top, 4 one document's exact score (that document out,
    every larger one in), 5 -inf (all), 6 +inf, 7 NaN (0 hits)."""
    N = S.shape[1]
    thr = np.empty(nq, np.float32)
    for q in range(nq):
        row = np.sort(S[q])[::-1]
        kind = (q + 3) % 8
        thr[q] = [np.nextafter(row[0], np.float32(np.inf)), row[0], row[1], row[int(0.05 * N)], S[q, (7 * q + 11) % N],
                  -np.inf, np.inf, np.nan][kind]
    return thr


def _expected(S, thr, ids_of_row):
    nq = len(thr)
    lims = np.zeros(nq + 1, np.int64)
    scores, ids = [], []
    with np.errstate(invalid="ignore"):
        for q in range(nq):
            hit = np.nonzero(S[q] > thr[q])[0]
            lims[q + 1] = lims[q] + len(hit)
            scores.append(S[q, hit])
            ids.append(ids_of_row[hit])
    return lims, np.concatenate(scores).astype(np.float32), np.concatenate(ids).astype(np.int64)


def _assert_equal(got, want, what=""):
    lims, scores, ids = (t.cpu().numpy() for t in got)
    elims, escores, eids = want
    print(what, "total", int(lims[-1]), "expected", int(elims[-1]))
    assert np.array_equal(lims, elims), "lims differ"
    assert np.array_equal(ids, eids), "ids differ"
    assert np.array_equal(scores.view(np.int32), escores.view(np.int32)), "score bits differ"


@pytest.fixture
def chunk_rows(monkeypatch):
    def set_(v):
        if v is None:
            monkeypatch.delenv("SR_RANGE_CHUNK_ROWS", raising=False)
        else:
            monkeypatch.setenv("SR_RANGE_CHUNK_ROWS", str(v))
    return set_


@pytest.mark.parametrize("chunk", [None, 256, 512])
@pytest.mark.parametrize("nq", [1, 33, 130, 300])
@pytest.mark.parametrize("H", [48, 320])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_range_search_equals_oracle(layout, H, nq, chunk, chunk_rows):
    chunk_rows(chunk)
    rows, q, S = _data(LAYOUTS[layout][0], H)
    idx, ids_of_row = _index(layout, H, rows)
    thr = _thresholds(S, nq)
    want = _expected(S, thr, ids_of_row)
    if nq >= 8:
        counts = np.diff(want[0])
        assert counts.max() == S.shape[1] and counts.min() == 0 and (counts == 1).any()
    got = idx.range_search(q[:nq], thr)
    _assert_equal(got, want, f"{layout} H={H} nq={nq} chunk={chunk}")
    # every returned score is the pair scorer's, bit for bit
    pairs = idx.score_pairs(q[:nq], got[0], got[2])
    assert torch.equal(pairs.view(torch.int32), got[1].view(torch.int32))
    # two identical calls give identical bytes
    again = idx.range_search(q[:nq], torch.from_numpy(thr))
    assert all(torch.equal(a, b) for a, b in zip(got[:1] + got[2:], again[:1] + again[2:]))
    assert torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))
    idx.close()


@pytest.mark.parametrize("nq", [130, 300])
def test_sorted_lists_are_prefixes_of_the_full_ranking(nq):
    """sort=True: score descending, ties by ascending id = the first lims[q + 1] - lims[q] entries of search(q, k = N); at H = 320
    the search accumulates in the tiled order for every nq."""
    H, layout = 320, "strided"
    N = LAYOUTS[layout][0]
    rows, q, S = _data(N, H)
    idx, _ = _index(layout, H, rows)
    thr = _thresholds(S, nq)
    lims, scores, ids = idx.range_search(q[:nq], thr, sort=True)
    fs, fi = idx.search(q[:nq], N)
    lims = lims.cpu().numpy()
    assert lims[-1] > N
    fs, fi, scores, ids = fs.cpu().numpy(), fi.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()
    for i in range(nq):
        c = lims[i + 1] - lims[i]
        assert np.array_equal(ids[lims[i]:lims[i + 1]], fi[i, :c]), i
        assert np.array_equal(scores[lims[i]:lims[i + 1]].view(np.int32), fs[i, :c].view(np.int32)), i
    idx.close()


@pytest.mark.parametrize("nq", [33, 130])
def test_fp16_index_equals_its_fp32_twin(nq):
    H, layout = 320, "strided"
    rows, q, S = _data(LAYOUTS[layout][0], H)
    rows16 = rows.half()
    f16, _ = _index(layout, H, rows16, row_dtype="fp16")
    twin, _ = _index(layout, H, rows16.float())
    assert f16.stored_dtype() == "fp16" and twin.stored_dtype() == "fp32"
    thr = _thresholds(S, nq)          # from the fp32 rows' scores: any thresholds do, both sides see the same ones
    a, b = f16.range_search(q[:nq], thr), twin.range_search(q[:nq], thr)
    assert int(a[0][-1]) > 863
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    f16.close()
    twin.close()


def test_precision_mode_does_not_change_the_result():
    H, layout, nq = 320, "two", 130
    rows, q, S = _data(LAYOUTS[layout][0], H)
    idx, ids_of_row = _index(layout, H, rows)
    idx.set_precision("fp32_filtered")
    thr = _thresholds(S, nq)
    _assert_equal(idx.range_search(q[:nq], thr), _expected(S, thr, ids_of_row), "fp32_filtered")
    idx.close()


def test_workspace_limit_changes_the_chunking_not_the_result():
    """66 000 queries under the smallest limit (1 MiB = 3 chunks of 4 bytes per query) against the default chunking (4 chunks), whose
    lists the oracle pins above; one threshold for all.  Then a batch whose table cannot fit even one chunk: MemoryError."""
    H, layout, nq = 48, "one", 66000
    rows, q, _ = _data(LAYOUTS[layout][0], H)
    big = q.repeat(nq // NQ_MAX, 1).contiguous()
    idx, _ = _index(layout, H, rows)
    want = idx.range_search(big, 0.12)
    assert int(want[0][-1]) > nq                         # about 5 % of the pairs
    assert torch.equal(want[0][:NQ_MAX + 1], want[0][NQ_MAX:2 * NQ_MAX + 1] - want[0][NQ_MAX])
    idx.set_workspace_limit(1 << 20)
    got = idx.range_search(big, 0.12)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    with pytest.raises(MemoryError, match="bytes"):
        idx.range_search(torch.cat([big] * 5), 0.12)
    idx.close()


def _raw(idx, q, thr, capacity=None, pad=16, fill_thr=None, count=True):
    """count + fill through the C ABI with sentinel-filled outputs: (rc_count, rc_fill, total, lims, scores, ids)."""
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr
    nq = q.shape[0]
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(-1)
    rc_count = idx.lib.sr_dense_range_count(idx._h, _ptr(q), nq, _ptr(thr), _ptr(lims), ctypes.byref(total), _lib.stream_ptr()) if count else None
    n = max(total.value, 0)
    scores = torch.full((n + pad,), SENTINEL_S, dtype=torch.float32, device="cuda")
    ids = torch.full((n + pad,), SENTINEL_I, dtype=torch.int64, device="cuda")
    rc_fill = idx.lib.sr_dense_range_fill(idx._h, _ptr(q), nq, _ptr(thr if fill_thr is None else fill_thr), _ptr(lims), _ptr(scores), _ptr(ids),
                                          n if capacity is None else capacity(n), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc_count, rc_fill, total.value, lims, scores, ids


def test_errors_and_edges():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import DenseIndexHIP
    H, layout, nq = 48, "two", 33
    N = LAYOUTS[layout][0]
    rows, q, S = _data(N, H)
    q = q[:nq].contiguous()
    idx, ids_of_row = _index(layout, H, rows)
    thr_np = _thresholds(S, nq)
    thr = torch.from_numpy(thr_np).cuda()
    untouched = lambda s, i: bool((s == SENTINEL_S).all()) and bool((i == SENTINEL_I).all())

    # fill without a count
    rc_c, rc_f, _, _, s, i = _raw(idx, q, thr, count=False)
    assert rc_f == _lib.SR_ERR_INVALID and b"count" in idx.lib.sr_last_error() and untouched(s, i)
    # the padding behind the result is never written
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr)
    assert rc_c == 0 and rc_f == 0 and total == int(lims[-1]) > N and untouched(s[total:], i[total:])
    _assert_equal((lims, s[:total], i[:total]), _expected(S, thr_np, ids_of_row), "raw")
    # capacity = total - 1
    rc_c, rc_f, total, _, s, i = _raw(idx, q, thr, capacity=lambda n: n - 1)
    assert rc_c == 0 and rc_f == _lib.SR_ERR_INVALID and b"capacity" in idx.lib.sr_last_error() and untouched(s, i)
    # a fill with LOWER thresholds than the count's (every document a hit; the chunks of a query then overrun into each other's slots):
    # whatever lands in query q's segment is a score of query q and an id of the index, nothing lands outside the segments
    rc_c, rc_f, total, lims, s, i = _raw(idx, q, thr, fill_thr=torch.full((nq,), -np.inf, device="cuda"))
    assert rc_c == 0 and rc_f in (0, _lib.SR_ERR_INVALID) and untouched(s[total:], i[total:])
    lims_h, s_h, i_h = lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy()
    for qi in range(nq):
        seg_s, seg_i = s_h[lims_h[qi]:lims_h[qi + 1]], i_h[lims_h[qi]:lims_h[qi + 1]]
        assert np.isin(seg_s, np.append(S[qi], np.float32(SENTINEL_S))).all(), qi
        assert np.isin(seg_i, np.append(ids_of_row, SENTINEL_I)).all(), qi
    # the index changed between count and fill
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    total = ctypes.c_int64(0)
    from scaling_retriever_amd.scoring import _ptr
    assert idx.lib.sr_dense_range_count(idx._h, _ptr(q), nq, _ptr(thr), _ptr(lims), ctypes.byref(total), _lib.stream_ptr()) == 0
    idx.add_device_rows(rows[:16], id_base=5000)
    s = torch.full((total.value,), SENTINEL_S, dtype=torch.float32, device="cuda")
    i = torch.full((total.value,), SENTINEL_I, dtype=torch.int64, device="cuda")
    rc = idx.lib.sr_dense_range_fill(idx._h, _ptr(q), nq, _ptr(thr), _ptr(lims), _ptr(s), _ptr(i), total.value, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.SR_ERR_INVALID and b"changed" in idx.lib.sr_last_error() and untouched(s, i)
    # nq = 0
    lims, s, i = idx.range_search(q[:0], 0.0)
    assert lims.tolist() == [0] and s.numel() == 0 and i.numel() == 0
    idx.close()
    # empty index
    empty = DenseIndexHIP(H)
    lims, s, i = empty.range_search(q, -np.inf, sort=True)
    assert lims.tolist() == [0] * (nq + 1) and s.numel() == 0 and i.numel() == 0
    empty.close()


def test_indexer_range_search_returns_db_ids():
    from oracle import scoring as SC
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    H, N, nq = 64, 200, 5
    g = torch.Generator(device="cpu").manual_seed(5)
    rows = (torch.randn((N, H), generator=g) * (0.5 / math.sqrt(H))).numpy()
    q = (torch.randn((nq, H), generator=g) / math.sqrt(H)).numpy()
    S = SC.dense_scores_fma(q, rows, SC.mfma_korder(H))
    ix = DenseFlatIndexer()
    ix.init_index(H)
    ix.index_data(rows[:120], [f"doc-{j}" for j in range(120)])
    ix.index_data(rows[120:], [f"doc-{j}" for j in range(120, N)])
    thr = np.sort(S, axis=1)[:, -10].copy()          # the 10th best: 9 hits each
    for queries in (q, torch.from_numpy(q)):
        id_lists, score_lists = ix.range_search(queries, thr)
        for i in range(nq):
            hit = np.nonzero(S[i] > thr[i])[0]
            hit = hit[np.lexsort((hit, -S[i, hit]))]
            assert len(hit) == 9 and id_lists[i] == [f"doc-{j}" for j in hit]
            assert score_lists[i].dtype == np.float32 and np.array_equal(score_lists[i].view(np.int32), S[i, hit].view(np.int32))
    id_lists, _ = ix.range_search(q, float(thr.min()), sort=False)
    for i in range(nq):
        assert id_lists[i] == [f"doc-{j}" for j in np.nonzero(S[i] > thr.min())[0]]
