"""GPU: dense search under a document bitmap (sr_dense_search_masked, csrc/doc_mask.hip, dense_split_kernel<true, true>) and the two
routes of the subset searches.  Every comparison is for equal ids and equal score BITS: the mask route (the certified filter's pass with
the bitmap in its epilogue) against the gather route (csrc/subset_search.hip) against the oracle's fmaf chain over the allowed rows.
filter_stats() is what shows that the mask route ran: without it every comparison could pass on the gather route alone."""
import numpy as np
import pytest
import torch

from oracle import scoring as O

pytestmark = pytest.mark.gpu

FMIN = np.float32(-3.402823466e38)


def _route(monkeypatch, route):
    monkeypatch.setenv("SR_DEV_SWITCHES", "1")
    monkeypatch.setenv("SR_SUBSET_DENSE_ROUTE", route)


def _pack(flags):
    words = np.zeros((len(flags) + 31) // 32, np.uint32)
    for i in np.flatnonzero(flags):
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


def _same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


# ------------------------------------------------------------------------------------------------- conversions ---
@pytest.mark.parametrize("n_bits", [12000, 1001])
def test_list_mask_list_round_trip(n_bits):
    from scaling_retriever_amd.scoring import doc_list_from_mask, doc_mask_from_list
    sets = [np.zeros(0, np.int64), np.array([0]), np.array([31, 32]), np.array([63, 64, n_bits - 1]), np.arange(0, n_bits, 32),
            np.arange(n_bits)]
    for ids in sets:
        ids = ids.astype(np.int64)
        flags = np.zeros(n_bits, bool)
        flags[ids] = True
        words = doc_mask_from_list(ids[::-1].copy(), n_bits)                    # any order
        assert np.array_equal(words.cpu().numpy().view(np.uint32), _pack(flags))
        back, count = doc_list_from_mask(words, n_bits)
        assert count == len(ids) and np.array_equal(back.cpu().numpy(), ids)
        if len(ids) > 1:                                                        # a capacity below the count: the count is still reported
            short, count = doc_list_from_mask(words, n_bits, capacity=len(ids) - 1)
            assert count == len(ids) and np.array_equal(short.cpu().numpy(), ids[:-1])
    # bits of the last word at or beyond n_bits are ignored
    if n_bits % 32:
        words = torch.full(((n_bits + 31) // 32,), -1, dtype=torch.int32, device="cuda")
        back, count = doc_list_from_mask(words, n_bits)
        assert count == n_bits and np.array_equal(back.cpu().numpy(), np.arange(n_bits))
    with pytest.raises(ValueError, match="outside"):
        doc_mask_from_list(np.array([3, n_bits]), n_bits)


# ------------------------------------------------------------------------- masked = gather = oracle, every mask ---
J_OUT = (100, 6001, 11990)          # documents three queries are aimed at, masked out: first 256 rows, mid-corpus, the last partial tile
_CACHE = {}


def _corpus(H, N):
    key = ("D", H, N)
    if key not in _CACHE:
        rng = np.random.default_rng(H + N)
        D = (rng.standard_normal((N, H), dtype=np.float32) * (0.5 / np.sqrt(H))).astype(np.float32)
        D[7000 % N] = D[300]              # exact twins: 300 allowed, its twin not
        D[9002 % N] = D[301]              # both allowed; at N = 12 000 in different segments of either layout (at N = 9 000 it is row 2: same segment)
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


def _masks(N):
    rng = np.random.default_rng(N)
    j_out = [j for j in J_OUT if j < N] + [N - 10]
    t_out, t_in = 7000 % N, (300, 301, 9002 % N)

    def plant(flags, keep_twins=True):
        flags[j_out] = False
        flags[t_out] = False
        if keep_twins:
            flags[list(t_in)] = True
        return flags
    masks = {"empty": np.zeros(N, bool), "all": np.ones(N, bool)}
    single = np.zeros(N, bool)
    single[5000 % N] = True
    masks["single"] = single
    for name, p in (("1pct", 0.01), ("50pct", 0.5), ("99pct", 0.99)):
        masks[name] = plant(rng.random(N) < p)
    rng_ = np.zeros(N, bool)
    rng_[1003:N - 2445] = True            # one range that starts and ends mid-word and mid-tile
    masks["range"] = plant(rng_, keep_twins=False)
    every = np.zeros(N, bool)
    every[5::32] = True
    masks["every32"] = plant(every, keep_twins=False)
    for name, m in (("m40", 40), ("m1500", 1500)):
        f = np.zeros(N, bool)
        f[rng.choice(N, m, replace=False)] = True
        f = plant(f)
        masks[name] = f
    return masks, j_out


def _queries(H, N, nq, Ds, j_out):
    rng = np.random.default_rng(nq + H)
    Q = (rng.standard_normal((nq, H), dtype=np.float32) * (0.5 / np.sqrt(H))).astype(np.float32)
    for q, j in enumerate(j_out[:3]):
        Q[q] = Ds[j] * np.float32(3.0)    # aimed at a masked-out document
    Q[3] = Ds[301] * np.float32(2.0)      # twins, both allowed: tie order
    Q[4] = Ds[300] * np.float32(2.0)      # twins, one allowed
    return Q


def _check_all_masks(monkeypatch, H, N, layout, storage, nq, k):
    idx, Ds = _index(H, N, layout, storage)
    masks, j_out = _masks(N)
    Q = _queries(H, N, nq, Ds, j_out)
    q = torch.from_numpy(Q).cuda()
    key = ("oracle", H, N, storage, nq)
    if key not in _CACHE:                                   # the reference, once: scores of the first 8 queries against every row
        _CACHE[key] = O.dense_scores_fma(Q[:8], Ds, O.mfma_korder(H))
    full = _CACHE[key]
    for name, flags in masks.items():
        allowed = np.flatnonzero(flags).astype(np.int64)
        sub = torch.from_numpy(allowed).cuda()
        words = torch.from_numpy(_pack(flags).view(np.int32)).cuda()
        res = {}
        for route in ("mask", "gather"):
            _route(monkeypatch, route)
            before = idx.filter_stats()
            res[route, "mask"] = idx.search(q, k, mask=torch.from_numpy(flags).cuda())
            res[route, "words"] = idx.search(q, k, mask=words)
            res[route, "subset"] = idx.search(q, k, subset=sub)
            after = idx.filter_stats()
            delta = (after[0] - before[0], after[1] - before[1])
            print(f"{layout} {storage} H {H} nq {nq} k {k} mask {name} (m = {len(allowed)}) route {route}: filter_stats advanced by {delta}")
            assert delta == ((3, 0) if route == "mask" else (0, 0)), (name, route, delta)      # (1, 0) per search on the mask route
        ref = res["gather", "subset"]
        for key_, got in res.items():
            assert _same(got, ref), (name, key_)
        ids = ref[1].cpu().numpy()
        assert flags[ids[ids >= 0]].all(), name             # no returned id is masked out
        assert ((ids >= 0).sum(axis=1) == min(k, len(allowed))).all(), name
        os_, oi = O.topk_rows(full[:, allowed], k)
        want_i = np.where(oi >= 0, allowed[np.maximum(oi, 0)] if len(allowed) else -1, -1)
        assert np.array_equal(ids[:8], want_i) and np.array_equal(ref[0].cpu().numpy()[:8].view(np.uint32), os_.view(np.uint32)), name


@pytest.mark.parametrize("storage", ["fp32", "fp16"])
@pytest.mark.parametrize("k", [1, 100, 1000])
@pytest.mark.parametrize("nq", [70, 300])
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_masked_equals_gather_equals_oracle(monkeypatch, layout, nq, k, storage):
    _check_all_masks(monkeypatch, 256, 12000, layout, storage, nq, k)


def test_masked_equals_gather_equals_oracle_wide_rows(monkeypatch):
    _check_all_masks(monkeypatch, 2048, 9000, "contiguous", "fp32", 130, 100)


# ------------------------------------------------------------------------------------------- redo under a mask ---
def test_redo_under_a_mask(monkeypatch):
    """Three blocks of 3 000 exact twins, one query aimed at each; the mask allows all of blocks 1 and 2 but only 50 twins of block 3.  The
    first two queries cannot be certified (more than kp - k allowed ties at the cut) and are re-done by the gather route, those alone; the
    third has 50 allowed twins, which fit the candidates, and is certified."""
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
    idx = DenseIndexHIP(H)
    idx.set_precision("fp32_filtered")
    idx.add_host_rows(D[:20000])
    idx.add_host_rows(D[20000:])
    flags = np.ones(N, bool)
    flags[11050:14000] = False
    q = torch.from_numpy(Q).cuda()
    _route(monkeypatch, "gather")
    ref = idx.search(q, k, mask=flags)
    assert idx.filter_stats() == (0, 0)
    _route(monkeypatch, "mask")
    got = idx.search(q, k, mask=flags)
    cert, redone = idx.filter_query_stats()
    print(f"redo under a mask: certified {cert}, redone {redone}")
    assert idx.filter_stats() == (0, 1) and cert + redone == nq and 2 <= redone <= 15, (cert, redone)
    assert _same(got, ref)
    ids = got[1].cpu().numpy()
    assert flags[ids].all()
    assert set(ids[299, :50].tolist()) == set(range(11000, 11050))      # the 50 allowed twins lead query 299
    os_, oi = O.topk_rows(O.dense_scores_fma(Q[[4, 150, 299]], D[flags], O.mfma_korder(H)), k)
    allowed = np.flatnonzero(flags)
    assert np.array_equal(ids[[4, 150, 299]], allowed[oi]) and np.array_equal(got[0].cpu().numpy()[[4, 150, 299]].view(np.uint32), os_.view(np.uint32))
    # a zero query under a mask without the twin blocks: every score is 0, nothing can be separated - it is re-done alone
    flags2 = np.ones(N, bool)
    flags2[5000:14000] = False
    Q2 = rng.standard_normal((nq, H), dtype=np.float32)
    Q2[5] = 0
    q2 = torch.from_numpy(Q2).cuda()
    before = idx.filter_query_stats()
    got = idx.search(q2, k, mask=flags2)
    after = idx.filter_query_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (nq - 1, 1)
    _route(monkeypatch, "gather")
    assert _same(got, idx.search(q2, k, mask=flags2))
    assert np.array_equal(got[1][5].cpu().numpy(), np.flatnonzero(flags2)[:k])      # all ties: ascending doc index


# ----------------------------------------------------------------------------------------- inapplicable filter ---
def test_inapplicable_filter_is_served_by_gather(monkeypatch):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    rng = np.random.default_rng(23)
    H, N = 256, 12000
    D = rng.standard_normal((N, H), dtype=np.float32)
    flags = rng.random(N) < 0.5
    sub = torch.from_numpy(np.flatnonzero(flags)).cuda()
    Dn = D.copy()
    Dn[17, 3] = np.inf
    flags_n = flags.copy()
    flags_n[17] = False                                      # (an infinite score would order differently in no kernel, but keep it out)
    cases = [("nq 17", D, "fp32_filtered", 17, 100, flags), ("fp32 precision", D, "fp32", 100, 100, flags),
             ("k 3000", D, "fp32_filtered", 100, 3000, flags), ("non-finite index", Dn, "fp32_filtered", 100, 100, flags_n)]
    for name, rows, precision, nq, k, fl in cases:
        idx = DenseIndexHIP(H)
        idx.set_precision(precision)
        idx.add_host_rows(rows[:7000])
        idx.add_host_rows(rows[7000:])
        q = torch.from_numpy(rng.standard_normal((nq, H), dtype=np.float32)).cuda()
        _route(monkeypatch, "gather")
        ref = idx.search(q, k, subset=torch.from_numpy(np.flatnonzero(fl)).cuda())
        _route(monkeypatch, "mask")
        got = idx.search(q, k, mask=fl)
        got2 = idx.search(q, k, subset=torch.from_numpy(np.flatnonzero(fl)).cuda())
        assert _same(got, ref) and _same(got2, ref), name
        assert idx.filter_stats() == (0, 0) and idx.filter_query_stats() == (0, 0), (name, idx.filter_stats())
        idx.close()


# ------------------------------------------------------------------------------------------------------ errors ---
def test_mask_errors_leave_the_index_usable(monkeypatch):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    rng = np.random.default_rng(29)
    H = 256
    D = rng.standard_normal((5000, H), dtype=np.float32)
    idx = DenseIndexHIP(H)
    idx.set_precision("fp32_filtered")
    idx.add_host_rows(D[:3000], id_base=0, id_stride=2)      # ids 0, 2, .., 5998
    idx.add_host_rows(D[3000:], id_base=1, id_stride=2)      # ids 1, 3, .., 3999: the odd ids from 4001 on name no document
    assert idx.ntotal == 5000 and idx.id_end == 5999
    q = torch.from_numpy(rng.standard_normal((100, H), dtype=np.float32)).cuda()
    valid = np.zeros(5999, bool)
    valid[0::2] = True
    valid[1:4000:2] = True
    flags = valid & (rng.random(5999) < 0.5)
    for route in ("mask", "gather"):
        _route(monkeypatch, route)
        with pytest.raises(ValueError, match="n_bits=5998"):
            idx.search(q, 10, mask=flags[:5998])
        with pytest.raises(ValueError, match="n_bits=6000"):
            idx.search(q, 10, mask=np.zeros(6000, bool))
        with pytest.raises(ValueError, match="words"):
            idx.search(q, 10, mask=np.zeros(190, np.uint32))
        bad = flags.copy()
        bad[4001] = True
        bad[4411] = True
        with pytest.raises(ValueError, match="4001"):
            idx.search(q, 10, mask=bad)
        got = idx.search(q, 10, mask=flags)                  # a following valid search returns the right answer
        sub = torch.from_numpy(np.flatnonzero(flags)).cuda()
        _route(monkeypatch, "gather")
        assert _same(got, idx.search(q, 10, subset=sub))
    assert idx.filter_stats() == (1, 0)                      # the valid search on the mask route; an invalid mask never reaches the pass
    # an invalid mask leaves every output row as padding - also with a k beyond what its count of bits allows, where nothing is searched
    import ctypes
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import pack_doc_mask
    few = np.zeros(5999, bool)
    few[[0, 2, 4001]] = True
    words = pack_doc_mask(torch.from_numpy(few).cuda())
    for k in (10, 4200):                                     # 4200 - 4096 > 3 set bits
        out_s = torch.full((100, k), 7.0, device="cuda")
        out_i = torch.full((100, k), 7, dtype=torch.int64, device="cuda")
        rc = idx.lib.sr_dense_search_masked(idx._h, ctypes.c_void_p(q.data_ptr()), 100, k, ctypes.c_void_p(words.data_ptr()), 5999,
                                            ctypes.c_void_p(out_s.data_ptr()), ctypes.c_void_p(out_i.data_ptr()), _lib.stream_ptr())
        assert rc == _lib.SR_ERR_INVALID and b"4001" in idx.lib.sr_last_error()
        assert bool((out_i == -1).all()) and bool((out_s == float(FMIN)).all()), k
    gid = np.concatenate([np.arange(0, 6000, 2), np.arange(1, 4000, 2)])
    rows = np.concatenate([D[:3000], D[3000:]])
    order = np.argsort(gid)
    allowed = np.flatnonzero(flags[gid[order]])
    os_, oi = O.topk_rows(O.dense_scores_fma(q[:8].cpu().numpy(), rows[order][allowed], O.mfma_korder(H)), 10)
    assert np.array_equal(got[1][:8].cpu().numpy(), gid[order][allowed][oi]) and np.array_equal(got[0][:8].cpu().numpy().view(np.uint32), os_.view(np.uint32))


# ------------------------------------------------------------------------------------------------ upper layers ---
def test_search_knn_routes_and_allowed_mask(monkeypatch):
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    rng = np.random.default_rng(31)
    H, N, nq, k = 256, 6000, 80, 20
    D = rng.standard_normal((N, H), dtype=np.float32)
    ix = DenseFlatIndexer()
    ix.init_index(H)
    ix.index_data(D[:2500], [f"p{i}" for i in range(2500)])
    ix.index_data(D[2500:], [f"p{i}" for i in range(2500, N)])
    Q = rng.standard_normal((nq, H), dtype=np.float32)
    flags = rng.random(N) < 0.3
    ids = [f"p{i}" for i in np.flatnonzero(flags)][::-1]      # any order
    out = {}
    for route in ("gather", "mask"):
        _route(monkeypatch, route)
        before = ix.index.filter_stats()
        out[route, "ids"] = ix.search_knn(Q, k, allowed_ids=ids)
        out[route, "mask"] = ix.search_knn(Q, k, allowed_mask=flags)
        after = ix.index.filter_stats()
        assert (after[0] - before[0], after[1] - before[1]) == ((2, 0) if route == "mask" else (0, 0))
    ref_lists, ref_scores = out["gather", "ids"]
    assert all(flags[int(d[1:])] for row in ref_lists for d in row)
    for key_, (lists, scores) in out.items():
        assert lists == ref_lists and np.array_equal(np.asarray(scores).view(np.uint32), np.asarray(ref_scores).view(np.uint32)), key_
    with pytest.raises(ValueError, match="not both"):
        ix.search_knn(Q, k, allowed_ids=ids, allowed_mask=flags)
    with pytest.raises(ValueError, match="one flag per index position"):
        ix.search_knn(Q, k, allowed_mask=flags[:-1])
