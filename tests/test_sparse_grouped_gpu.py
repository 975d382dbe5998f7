"""GPU: sparse search under per-query document filters (sr_sparse_search_grouped; the grouped pass of csrc/sparse_cert.hip,
cert_score_kernel<KS, true, true>: the bit test reads the lane's own query's bitmap, the block skip the union of all groups').  Every
comparison is for equal counts, equal ids and equal score BITS: against the oracle's full ranking filtered to the query's own group,
against one masked search per group, and between the routes (pass, loop, the default rule).  The cert_stats() deltas keep a comparison
from passing on the hand-back route alone.

Inputs are those of tests/test_sparse_mask_gpu.py and the cases of tests/sparse_cert_cases.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import sparse_cert_cases as C
from test_sparse_cert_kernels_gpu import _env, _mask_of, _run
from test_sparse_mask_gpu import SHAPES, _expected, _masks, _np, _same, _shape

pytestmark = pytest.mark.gpu

ROUTE = "SR_GROUPED_SPARSE_ROUTE"
LARGE = ("all", "half", "anti_diag", "all_but_few", "odd_blocks")


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("SR_SPARSE_CERT", "1")        # build + use the certified scorer below its size threshold as well
    monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE", raising=False)
    monkeypatch.delenv(ROUTE, raising=False)


def _route(monkeypatch, route):
    if route is None:
        monkeypatch.delenv(ROUTE, raising=False)
    else:
        monkeypatch.setenv(ROUTE, route)


@functools.lru_cache(maxsize=None)
def _groups(n):
    """The ten groups of shape n (the eight masks of _masks, `empty`, `single`) plus one that no query uses, the group of every query and
    the expected rows: each query's own group's rows of _expected.  Computed once and never changed."""
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[n]
    full_i, full_s, full_c = _shape(n)[6:]
    masks = dict(_masks(N))
    masks["empty"] = np.zeros(N, bool)
    masks["single"] = np.arange(N) == 17
    names = list(masks)
    assert len(names) == 10
    flags = np.stack([masks[m] for m in names] + [np.arange(N) % 3 == 0])       # group 10: unused
    grp = np.arange(nq) % 10
    es, ei, ec = np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
    for g in range(10):
        qs = np.flatnonzero(grp == g)
        gs, gi, gc = _expected(full_i[qs], full_s[qs], full_c[qs], flags[g], k)
        es[qs], ei[qs], ec[qs] = gs, gi, gc
    return names, flags, grp, (es, ei, ec)


def _sub_csr(qi, qc, qv, qs):
    """The CSR of the queries qs alone, in that order."""
    lens = (qi[1:] - qi[:-1])[qs]
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    take = np.concatenate([np.arange(qi[q], qi[q + 1]) for q in qs]) if len(qs) else np.zeros(0, np.int64)
    return ip, qc[take], qv[take]


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_grouped_equals_per_group_masked_equals_oracle(forced, monkeypatch, n):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[n]
    indptr, ids, vals, qi, qc, qv = _shape(n)[:6]
    names, flags, grp, want = _groups(n)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    assert idx.cert_stats()["present"] == 1
    got = {}
    for route in ("pass", "loop", None):
        _route(monkeypatch, route)
        before = idx.cert_stats()
        got[route] = _np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr))
        after = idx.cert_stats()
        print(f"shape {n} route {route}: scorer searches {after['searches'] - before['searches']}, queries {after['queries'] - before['queries']}, "
              f"handed back {after['redone_exact'] - before['redone_exact']}")
        _same(got[route], want, f"shape {n} route {route} against the oracle")
        if route == "pass":
            assert after["searches"] - before["searches"] == 1 and after["queries"] - before["queries"] == nq
    _same(got["loop"], got["pass"], f"shape {n}: loop against pass")
    _same(got[None], got["pass"], f"shape {n}: default rule against pass")
    _route(monkeypatch, None)
    for g in range(10):                                  # one masked search per group: the baseline a caller had before
        qs = np.flatnonzero(grp == g)
        one = _np(idx.search(*_sub_csr(qi, qc, qv, qs), k, threshold=thr, mask=flags[g]))
        _same(tuple(x[qs] for x in got["pass"]), one, f"shape {n} group {names[g]} against search(mask=)")
    # ids with a base and a stride, on both routes
    shifted = (want[0], np.where(want[1] >= 0, 7 + 3 * want[1], -1), want[2])
    for route in ("pass", "loop"):
        _route(monkeypatch, route)
        _same(_np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr, id_base=7, id_stride=3)), shifted, f"ids 7 + 3 d, route {route}")


def test_the_mask_is_the_querys_own(forced, monkeypatch):
    """One query repeated 32 times = one full block of the score kernel, every lane a different group; group g allows the documents
    = g mod 32.  A wave-uniform word used in place of the lane's own would give every row the same documents."""
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[1]
    indptr, ids, vals, qi, qc, qv, full_i, full_s, full_c = _shape(1)
    q = 3
    cols, v = qc[qi[q]:qi[q + 1]], qv[qi[q]:qi[q + 1]]
    ip = (np.arange(33) * len(cols)).astype(np.int64)
    rc, rv = np.tile(cols, 32), np.tile(v, 32)
    flags = np.stack([np.arange(N) % 32 == g for g in range(32)])
    grp = np.arange(32)
    rep = lambda a: np.repeat(a[q:q + 1], 32, axis=0)          # noqa: E731
    es, ei, ec = np.zeros((32, k), np.float32), np.full((32, k), -1, np.int64), np.zeros(32, np.int32)
    for g in range(32):
        s1, i1, c1 = _expected(full_i[q:q + 1], full_s[q:q + 1], full_c[q:q + 1], flags[g], k)
        es[g], ei[g], ec[g] = s1[0], i1[0], c1[0]
    assert ec.min() > 0 and rep(full_i).shape[0] == 32
    idx = SparseIndexHIP(indptr, ids, vals, N)
    for route in ("pass", "loop"):
        _route(monkeypatch, route)
        before = idx.cert_stats()
        s, i, c = got = _np(idx.search_grouped(ip, rc, rv, k, flags, grp, threshold=thr))
        after = idx.cert_stats()
        for g in range(32):
            assert (i[g, :c[g]] % 32 == g).all(), (route, g)
        _same(got, (es, ei, ec), f"route {route}")
        if route == "pass":
            assert after["searches"] - before["searches"] == 1 and after["queries"] - before["queries"] == 32
            print(f"own-mask case: handed back {after['redone_exact'] - before['redone_exact']} of 32")


def test_the_pass_carries_the_call(forced, monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[0]
    indptr, ids, vals, qi, qc, qv, full_i, full_s, full_c = _shape(0)
    masks = _masks(N)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    _route(monkeypatch, "pass")
    # G = 1: the same batch under the same mask as search(mask=) on its mask route, so the same hand-backs
    for name in ("half", "sixteenth"):
        b0 = idx.cert_stats()
        got = _np(idx.search_grouped(qi, qc, qv, k, masks[name][None, :], np.zeros(nq, np.int64), threshold=thr))
        b1 = idx.cert_stats()
        monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", "mask")
        one = _np(idx.search(qi, qc, qv, k, threshold=thr, mask=masks[name]))
        monkeypatch.delenv("SR_SUBSET_SPARSE_ROUTE")
        b2 = idx.cert_stats()
        _same(got, one, f"G = 1 ({name})")
        assert b1["searches"] - b0["searches"] == 1 and b1["queries"] - b0["queries"] == nq
        assert b1["redone_exact"] - b0["redone_exact"] == b2["redone_exact"] - b1["redone_exact"], (name, b0, b1, b2)
    # the five large masks as groups: the cap test_sparse_mask_gpu holds for each of them over all queries
    flags = np.stack([masks[m] for m in LARGE])
    grp = np.arange(nq) % 5
    b0 = idx.cert_stats()
    got = _np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr))
    b1 = idx.cert_stats()
    redone = b1["redone_exact"] - b0["redone_exact"]
    assert b1["searches"] - b0["searches"] == 1 and b1["queries"] - b0["queries"] == nq
    per_group = 0
    monkeypatch.setenv("SR_SUBSET_SPARSE_ROUTE", "mask")
    for g in range(5):
        qs = np.flatnonzero(grp == g)
        c0 = idx.cert_stats()["redone_exact"]
        one = _np(idx.search(*_sub_csr(qi, qc, qv, qs), k, threshold=thr, mask=flags[g]))
        per_group += idx.cert_stats()["redone_exact"] - c0
        _same(tuple(x[qs] for x in got), one, f"group {LARGE[g]}")
    print(f"five large masks as groups: the grouped pass handed back {redone} of {nq}, the five masked searches {per_group} in sum")
    assert redone <= nq // 8, (redone, nq)


def test_grouped_search_in_several_query_batches(forced, monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[0]
    indptr, ids, vals, qi, qc, qv = _shape(0)[:6]
    names, flags, grp, want = _groups(0)                  # q % 10: every group straddles the batches of 32
    idx = SparseIndexHIP(indptr, ids, vals, N)
    _route(monkeypatch, "pass")
    monkeypatch.setenv("SR_SPARSE_CERT_BATCH", "32")
    several = _np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr))
    assert idx.cert_stats()["searches"] == (nq + 31) // 32 and idx.cert_stats()["queries"] == nq
    _same(several, want, "batches of 32 queries")


@pytest.mark.parametrize("cap", C.KS_CAPS)
def test_every_instantiation_of_the_grouped_twin(cap):
    case = C.ks_case(cap)
    run = _run(case)
    N, nq, k = case["N"], case["nq"], case["k"]
    assert run.present and run.idx.cert_stats()["dense_terms"] == C.EXPECTED_T[cap]
    flags = np.stack([_mask_of(N), ~_mask_of(N), np.ones(N, bool)])
    grp = np.arange(nq) % 3
    with _env(SR_GROUPED_SPARSE_ROUTE="pass", **{k_: v for k_, v in run.env.items() if k_ != "SR_SUBSET_SPARSE_ROUTE"}):
        before = run.idx.cert_stats()
        got = _np(run.idx.search_grouped(case["qi"], case["qc"], case["qv"], k, flags, grp))
        after = run.idx.cert_stats()
    assert after["searches"] - before["searches"] == 1 and after["queries"] - before["queries"] == nq
    print(f"{case['name']}: the grouped pass handed back {after['redone_exact'] - before['redone_exact']} of {nq}")
    es, ei, ec = np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
    for g in range(3):
        gs, gi, gc = run.oracle(flags[g])
        es[grp == g], ei[grp == g], ec[grp == g] = gs[grp == g], gi[grp == g], gc[grp == g]
    _same(got, (es, ei, ec), case["name"])
    assert run.idx.cert_readout("info")["KS"] == C.EXPECTED_T[cap] // 16


def test_hand_back_under_groups():
    case = C.uncertifiable_case()
    run = _run(case)
    N, nq, k = case["N"], case["nq"], case["k"]
    flags = np.stack([_mask_of(N) | (np.arange(N) == 7), np.ones(N, bool)])
    grp = np.array([0, 1, 0])
    env = {k_: v for k_, v in run.env.items() if k_ != "SR_SUBSET_SPARSE_ROUTE"}
    with _env(SR_GROUPED_SPARSE_ROUTE="pass", **env):
        before = run.idx.cert_stats()
        got = _np(run.idx.search_grouped(case["qi"], case["qc"], case["qv"], k, flags, grp))
        after = run.idx.cert_stats()
    assert after["searches"] - before["searches"] == 1 and after["redone_exact"] - before["redone_exact"] >= 2      # queries 0 and 1 cannot be certified
    with _env(SR_SUBSET_SPARSE_ROUTE="mask", **env):
        for g in range(2):
            qs = np.flatnonzero(grp == g)
            one = _np(run.idx.search(*_sub_csr(case["qi"], case["qc"], case["qv"], qs), k, mask=flags[g]))
            _same(tuple(x[qs] for x in got), one, f"group {g}")
    es, ei, ec = run.oracle(flags[0])
    es1, ei1, ec1 = run.oracle(flags[1])
    es[1], ei[1], ec[1] = es1[1], ei1[1], ec1[1]
    _same(got, (es, ei, ec), "uncertifiable queries under groups")


def test_bitmaps_that_do_not_fit_and_the_scorer_switched_off(forced, monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[1]
    indptr, ids, vals, qi, qc, qv = _shape(1)[:6]
    names, flags, grp, want = _groups(1)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    flags, grp = np.tile(flags, (20, 1)), grp + flags.shape[0] * (np.arange(nq) % 20)     # 220 groups: the same masks, twenty times
    G, n_tiles = flags.shape[0], (N + 1023) // 1024
    _route(monkeypatch, "pass")
    # the padded bitmaps need (G + 1) * n_tiles * 128 bytes; the list routes 8 bytes per (query, slab entry), the array route's smallest slab
    # being one tile of 8 192 documents
    limit = (G + 1) * n_tiles * 128 - 1
    assert limit >= 1 << 20                               # the smallest limit the handle takes; 16 queries of the array route per batch
    idx.set_workspace_limit(limit)
    before = idx.cert_stats()
    _same(_np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr)), want, "bitmaps do not fit: the loop")
    assert idx.cert_stats()["queries"] == before["queries"]          # every group's masked body found its own copy too large as well
    idx.set_workspace_limit(4 << 30)
    _same(_np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr)), want, "limit restored: the pass")
    assert idx.cert_stats()["searches"] - before["searches"] == 1 and idx.cert_stats()["queries"] - before["queries"] == nq
    monkeypatch.setenv("SR_SPARSE_CERT_SEARCH", "0")
    before = idx.cert_stats()
    _same(_np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr)), want, "SR_SPARSE_CERT_SEARCH=0: the loop")
    assert idx.cert_stats()["searches"] == before["searches"]


def test_errors_leave_padding_and_a_usable_index(forced, monkeypatch):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import SparseIndexHIP, pack_doc_masks
    V, N, L0_d, nq, L0_q, k, thr = SHAPES[1]
    indptr, ids, vals, qi, qc, qv = _shape(1)[:6]
    names, flags, grp, want = _groups(1)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    G = flags.shape[0]
    for route in ("pass", "loop"):
        _route(monkeypatch, route)
        for bad in (G, -1, 2 ** 31):
            g2 = grp.astype(np.int64).copy()
            g2[[5, 9]] = bad
            before = idx.cert_stats()
            with pytest.raises(ValueError, match=r"query 5 is in group"):
                idx.search_grouped(qi, qc, qv, k, flags, g2, threshold=thr)
            assert idx.cert_stats() == before
        _same(_np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr)), want, f"after a refused call, route {route}")
        words = pack_doc_masks(flags)
        _same(_np(idx.search_grouped(qi, qc, qv, k, words, grp, threshold=thr)), want, f"packed host words, route {route}")
        _same(_np(idx.search_grouped(qi, qc, qv, k, words.numpy().view(np.uint32), torch.from_numpy(grp).cuda(), threshold=thr)), want,
              f"uint32 words, cuda groups, route {route}")
    # the rows a refused call leaves behind, through the C ABI with outputs of our own
    dev = idx.device
    q = idx._query_csr(qi, qc, qv)[0]
    words = pack_doc_masks(flags, dev)
    g2 = torch.from_numpy(grp.astype(np.int32)).to(dev)
    g2[7] = G
    s = torch.full((nq, k), 5.0, device=dev)
    i = torch.full((nq, k), 5, dtype=torch.int64, device=dev)
    c = torch.full((nq,), 5, dtype=torch.int32, device=dev)
    P = lambda t: _lib.c_void_p(t.data_ptr())                     # noqa: E731
    args = lambda **kw: (idx._h, P(q[0]), P(q[1]), P(q[2]), kw.get("nq", nq), kw.get("k", k), float(thr), P(words), kw.get("G", G),      # noqa: E731
                         kw.get("n_bits", N), kw.get("groups", P(g2)), 0, 1, P(s), P(i), P(c), None)
    lib = idx.lib
    assert lib.sr_sparse_search_grouped(*args()) == _lib.SR_ERR_INVALID and b"query 7 is in group" in lib.sr_last_error()
    torch.cuda.synchronize()
    assert (s == 0).all() and (i == -1).all() and (c == 0).all()
    # refused before any device work
    for kw, needle in ((dict(n_bits=N + 1), b"n_bits="), (dict(G=0), b"n_groups=0"), (dict(k=0), b"outside [1"), (dict(groups=None), b"null pointer"),
                       (dict(G=(1 << 32) // (32 * ((N + 1023) // 1024))), b"exceed 2^32 words")):
        assert lib.sr_sparse_search_grouped(*args(**kw)) == _lib.SR_ERR_INVALID and needle in lib.sr_last_error(), (kw, lib.sr_last_error())
    assert lib.sr_sparse_search_grouped(*args(nq=0)) == _lib.SR_OK
    _route(monkeypatch, "pass")
    _same(_np(idx.search_grouped(qi, qc, qv, k, flags, grp, threshold=thr)), want, "after the refused C calls")


# ------------------------------------------------------------------------------------------------------ retrieval classes ---
@pytest.fixture(scope="module")
def tiny(golden_dir):
    from golden_weights import make_weights
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    return cfg, make_weights(cfg, int(z["weight_seed"]))


def test_sparse_retrieval_under_filter_groups(tiny, tmp_path, monkeypatch):
    """retrieve(allowed_masks=, query_group=) with the query set going through in several pieces equals one retrieve(allowed_mask=) per
    group, run entry by run entry."""
    from test_indexer_gpu import FakeLoader, _corpus
    from scaling_retriever_amd.indexer import SparseIndexer, SparseRetrieval
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    cfg, w = tiny
    V = cfg["vocab_size"]
    rng = np.random.default_rng(1)
    docs, queries = _corpus(rng, 50, V, 1, 6), _corpus(rng, 11, V, 1, 3)
    pids, qids = [f"p{i}" for i in range(len(docs))], [f"q{i}" for i in range(len(queries))]
    model = LlamaBiSparse.from_weights(cfg, w, precision="bf16").to("cuda").eval()
    index_dir = str(tmp_path / "index")
    SparseIndexer(model, index_dir=index_dir, compute_stats=True, dim_voc=model.vocab_size, device="cuda").index(
        FakeLoader(docs, pids, batch_size=8, pad_id=V - 1))
    monkeypatch.setattr(SparseRetrieval, "QUERY_GROUP_ROWS", 4)       # 11 queries in batches of 4: three pieces

    def retriever(name):
        return SparseRetrieval(config={"index_dir": index_dir, "out_dir": str(tmp_path / name)}, model=model, compute_stats=True,
                               dim_voc=model.vocab_size, device="cuda")
    loader = lambda: FakeLoader(queries, qids, batch_size=4, pad_id=V - 1)      # noqa: E731
    ret = retriever("groups")
    n = ret.hip_index.n_docs
    flags = np.stack([np.arange(n) % 2 == 0, np.arange(n) % 3 != 0, np.arange(n) < 5, np.zeros(n, bool)])
    grp = np.array([0, 1, 2, 3, 2, 1, 0, 0, 1, 1, 2])
    res = ret.retrieve(loader(), topk=5, threshold=0.0, allowed_masks=flags, query_group=grp)
    run = json.loads((tmp_path / "groups" / "run.json").read_bytes())
    assert res.to_dict() == run and len(run) >= 5
    assert "L0_q" in json.load(open(tmp_path / "groups" / "q_stats.json"))
    one = retriever("one")
    for g in range(4):
        want = one.retrieve(loader(), topk=5, threshold=0.0, allowed_mask=flags[g]).to_dict()
        for q in np.flatnonzero(grp == g):
            assert run.get(qids[q]) == want.get(qids[q]), (g, qids[q])
    # one piece (the whole set in one search) writes the same file
    monkeypatch.setattr(SparseRetrieval, "QUERY_GROUP_ROWS", 2048)
    assert ret.retrieve(loader(), topk=5, threshold=0.0, allowed_masks=torch.from_numpy(flags), query_group=torch.from_numpy(grp)).to_dict() == run
    with pytest.raises(ValueError, match="one group id per query"):
        ret.retrieve(loader(), topk=5, allowed_masks=flags, query_group=grp[:-1])
    with pytest.raises(ValueError, match="not both"):
        ret.retrieve(loader(), topk=5, allowed_mask=flags[0], allowed_masks=flags, query_group=grp)


def test_hybrid_retriever_under_filter_groups(golden_dir, tmp_path):
    """HybridRetriever.retrieve / retrieve_fused under groups equal the same call per group under allowed_ids = that group's ids, for the
    sparse/, dense/ and fused/ run.json entries of the group's queries."""
    from fake_tokenizer import FakeTokenizer
    from torch.utils.data import DataLoader
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    from scaling_retriever_amd.indexer import HybridIndexer, HybridRetriever
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiHybrid
    from test_hybrid_gpu import _case
    from test_pipeline import ListDataset, _corpus
    z, cfg, w = _case(golden_dir, "enc_tiny_a")
    tok = FakeTokenizer(vocab_size=cfg["vocab_size"], padding_side="left")
    corpus = _corpus(90, seed=1, max_words=20)
    docs, queries = ListDataset(corpus), ListDataset([(f"q{i}", t) for i, (_, t) in enumerate(_corpus(8, seed=2, max_words=6))])
    collate_d, collate_q = LlamaSparseCollectionCollator(tok, 24), LlamaSparseCollectionCollator(tok, 8)
    loader = lambda: DataLoader(docs, batch_size=16, shuffle=False, collate_fn=collate_d)      # noqa: E731
    q_loader = lambda: DataLoader(queries, batch_size=4, shuffle=False, collate_fn=collate_q)  # noqa: E731
    hyb = LlamaBiHybrid.from_weights(cfg, w).to("cuda").eval()
    sp_dir, de_dir, out = str(tmp_path / "sp"), str(tmp_path / "de"), str(tmp_path / "out")
    HybridIndexer(hyb, sp_dir, de_dir, device="cuda", chunk_size=40, compute_stats=True, dim_voc=hyb.vocab_size).index(loader())
    ret = HybridRetriever(hyb, sp_dir, de_dir, out, dim_voc=hyb.vocab_size, device="cuda")
    db_ids = list(ret.dense_index.index_id_to_db_id)
    group_ids = [db_ids[0::2], db_ids[5:40], db_ids[80:]]
    flags = np.stack([ret.allowed_mask(ids) for ids in group_ids])
    grp = np.array([0, 1, 2, 1, 0, 2, 1, 0])
    runs = lambda: {h: json.load(open(os.path.join(out, h, "run.json"))) for h in ("sparse", "dense", "fused")}      # noqa: E731
    s_res, d_res, f_res = ret.retrieve_fused(q_loader(), topk=10, allowed_masks=flags, query_group=grp)
    got = runs()
    assert got["fused"] == {q: dict(r) for q, r in f_res.items()} and len(got["fused"]) >= 5
    s2, d2 = ret.retrieve(q_loader(), topk=10, allowed_masks=flags, query_group=grp)
    assert {q: dict(r) for q, r in s2.items()} == got["sparse"] and {q: dict(r) for q, r in d2.items()} == got["dense"]
    for g, ids in enumerate(group_ids):
        ret.retrieve_fused(q_loader(), topk=10, allowed_ids=ids)
        want = runs()
        for q in np.flatnonzero(grp == g):
            for head in ("sparse", "dense", "fused"):
                assert got[head].get(f"q{q}") == want[head].get(f"q{q}"), (g, q, head)
                assert set(got[head].get(f"q{q}", {})) <= {str(d) for d in ids}
    with pytest.raises(ValueError, match="not both"):
        ret.retrieve(q_loader(), topk=10, allowed_ids=group_ids[0], allowed_masks=flags, query_group=grp)
