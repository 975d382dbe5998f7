"""GPU: the collapsed search - sr_topk_collapse against the plain model of tests/collapse_cases.py (torch.equal on all five outputs),
and the drivers of both heads against the definition applied to the numpy full ranking: ids, keys, counts and score BITS, the route
every query took, every filter.  All inputs are small integers, so the CPU's full ranking is the GPU's bit for bit."""
import numpy as np
import pytest
import torch

import collapse_cases as C

pytestmark = pytest.mark.gpu

CHUNK = 1024                                   # TC_CHUNK of csrc/topk_collapse.hip
ROW_LENS = [1, 63, 64, 65, 4095, 4096, 4097, 3 * CHUNK + 5]


def _max_topk():
    from scaling_retriever_amd import _lib
    return int(_lib.load().sr_max_topk())


def _collapse(scores, ids, keys, k, counts=None, exhaustive=False):
    from scaling_retriever_amd.scoring import topk_collapse
    out = topk_collapse(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(keys).cuda(), k,
                        counts=None if counts is None else torch.from_numpy(counts).cuda(), exhaustive=exhaustive)
    torch.cuda.synchronize()
    return out


def _same(got, want, what):
    names = ("scores", "ids", "keys", "counts", "complete")
    for name, g, w in zip(names, got, want):
        assert torch.equal(g.cpu(), torch.from_numpy(w)), (what, name)


def _pattern_rows(row_len):
    """One row per key pattern (keys are a function of the POSITION in the row; every row has ids of its own, shuffled): all one key,
    all distinct, clustered (p // 7), random with repeats, a key of the first chunk recurring at the row's end and in between, rows
    ending in padding - also with ids behind the first negative one.  Scores descend in runs of equal values across keys."""
    rng = np.random.default_rng(row_len)
    M = row_len + 8
    pos = np.arange(row_len)
    by_pos = [np.full(row_len, 3), pos.copy(), pos // 7, rng.integers(0, max(2, row_len // 4), row_len), pos.copy(), pos // 3, pos % 11]
    by_pos[4][-1] = by_pos[4][0]
    by_pos[4][row_len // 2] = by_pos[4][0]
    nq = len(by_pos)
    ids = np.empty((nq, row_len), np.int64)
    keys = np.full(nq * M + 1, 1 << 20, np.int32)
    for r in range(nq):
        ids[r] = r * M + rng.permutation(M)[:row_len]
        keys[ids[r]] = by_pos[r] + (r * M if r in (1, 4) else 0)
    scores = np.repeat(((row_len - pos) // 3).astype(np.float32)[None], nq, 0) - np.float32(0.5)
    cut = row_len // 2
    ids[5, cut:] = -1                              # a dense search's padding
    ids[6, cut] = -1                               # the row ends at the FIRST negative id, whatever follows
    return scores, ids, keys


@pytest.mark.parametrize("row_len", ROW_LENS)
def test_kernel_equals_the_model(row_len):
    scores, ids, keys = _pattern_rows(row_len)
    rng = np.random.default_rng(row_len + 1)
    counts = rng.integers(0, row_len + 1, size=ids.shape[0]).astype(np.int32)
    counts[:2] = (row_len, max(0, row_len - 1))
    ids_c = np.where(ids < 0, 0, ids)                # with counts every entry of the prefix is an id
    for k in (1, 7, 1000, _max_topk()):
        for exhaustive in (False, True):
            _same(_collapse(scores, ids, keys, k, exhaustive=exhaustive), C.collapse_model(scores, ids, keys, k, exhaustive=exhaustive),
                  (row_len, k, exhaustive, "padding ends the row"))
            _same(_collapse(scores, ids_c, keys, k, counts=counts, exhaustive=exhaustive),
                  C.collapse_model(scores, ids_c, keys, k, counts=counts, exhaustive=exhaustive), (row_len, k, exhaustive, "counts"))


@pytest.mark.parametrize("k", [7, 1000])
def test_kth_group_on_a_chunk_boundary(k):
    """The k-th distinct key sits on a chunk's last entry (row 0), on the next chunk's first (row 1), one entry before the last (row 2);
    a row of exactly k - 1 keys (row 3) is not complete."""
    row_len = 3 * CHUNK + 5
    at = [2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK - 2, row_len]
    ids = np.stack([np.random.default_rng(r).permutation(row_len) + r * row_len for r in range(4)]).astype(np.int64)
    keys = np.zeros(4 * row_len, np.int32)
    for r in range(4):
        by_pos = np.zeros(row_len, np.int32)
        by_pos[:k - 1] = np.arange(k - 1)            # k - 1 keys at once, then repeats of key 0 up to `at`, new keys from there on
        by_pos[at[r]:] = k + np.arange(row_len - at[r])
        keys[ids[r]] = by_pos
    scores = np.repeat(-np.arange(row_len, dtype=np.float32)[None], 4, 0)
    want = C.collapse_model(scores, ids, keys, k)
    assert want[3].tolist() == [k, k, k, k - 1] and want[4].tolist() == [1, 1, 1, 0]
    assert [int(want[1][r, k - 1]) for r in range(3)] == [int(ids[r, at[r]]) for r in range(3)]
    _same(_collapse(scores, ids, keys, k), want, k)


def test_empty_shapes():
    keys = np.zeros(4, np.int32)
    for exhaustive in (False, True):
        got = _collapse(np.zeros((3, 0), np.float32), np.zeros((3, 0), np.int64), keys, 5, exhaustive=exhaustive)
        _same(got, C.collapse_model(np.zeros((3, 0), np.float32), np.zeros((3, 0), np.int64), keys, 5, exhaustive=exhaustive), exhaustive)
        assert got[4].tolist() == [int(exhaustive)] * 3 and got[3].tolist() == [0, 0, 0]
    got = _collapse(np.zeros((0, 9), np.float32), np.zeros((0, 9), np.int64), keys, 5)
    assert got[0].shape == (0, 5) and got[4].shape == (0,)


def test_invalid_ids_and_keys_are_named_and_the_library_stays_usable():
    row_len, k = 2 * CHUNK + 100, 50
    rng = np.random.default_rng(3)
    ids = np.stack([rng.permutation(row_len) for _ in range(4)]).astype(np.int64)
    keys = (np.arange(row_len) // 2).astype(np.int32)
    scores = np.repeat(-np.arange(row_len, dtype=np.float32)[None], 4, 0)
    good = C.collapse_model(scores, ids, keys, k)
    bad = ids.copy()
    bad[2, 5] = row_len                               # one past the key table
    bad[3, 1] = row_len + 7
    with pytest.raises(ValueError, match=r"query 2, position 5: id %d is outside the key table \[0, %d\)" % (row_len, row_len)):
        _collapse(scores, bad, keys, k)
    _same(_collapse(scores, ids, keys, k), good, "after a bad id")
    bad_keys = keys.copy()
    bad_keys[ids[1, 17]] = -4                         # every row holds that id: the first (query, position) is in row 0, behind its
    at = int(np.flatnonzero(ids[0] == ids[1, 17])[0])  # k-th group but inside the chunk that was read
    with pytest.raises(ValueError, match=r"query 0, position %d: id %d has the negative group key -4" % (at, ids[1, 17])):
        _collapse(scores, ids, bad_keys, k)
    only = ids[1:2].copy()
    with pytest.raises(ValueError, match=r"query 0, position 17: id %d has the negative group key -4" % ids[1, 17]):
        _collapse(scores[1:2], only, bad_keys, k)
    counts = np.full(4, row_len, np.int32)
    neg = ids.copy()
    neg[0, 3] = -1                                    # inside a prefix given by counts a negative id is no padding
    with pytest.raises(ValueError, match="query 0, position 3"):
        _collapse(scores, neg, keys, k, counts=counts)
    # a workgroup stops reading behind the chunk in which it found its k-th group: what lies in later chunks is not checked
    late = ids.copy()
    late[:, CHUNK + 1:] = row_len + 1
    _same(_collapse(scores, late, keys, k), good, "entries behind the k-th group's chunk")


def test_two_runs_give_the_same_bytes():
    scores, ids, keys = _pattern_rows(4097)
    scores, ids = np.tile(scores, (40, 1)), np.tile(ids, (40, 1))
    a = _collapse(scores, ids, keys, 1000)
    b = _collapse(scores, ids, keys, 1000)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ the drivers
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(got, want, what):
    s, i, g, c = [x.cpu().numpy() for x in got[:4]]
    assert np.array_equal(c, want[3]), (what, "counts")
    assert np.array_equal(i, want[1]), (what, "ids")
    assert np.array_equal(g, want[2]), (what, "keys")
    assert np.array_equal(_bits(s), _bits(want[0])), (what, "score bits")


def _dense_index(rows, row_dtype, precision):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    idx = DenseIndexHIP(rows.shape[1], row_dtype=row_dtype)
    idx.add_host_rows(rows)
    idx.set_precision(precision)
    return idx


def _filters():
    rng = np.random.default_rng(11)
    flags = rng.random(C.N_DOCS) < 0.5
    group_flags = np.stack([rng.random(C.N_DOCS) < 0.6, rng.random(C.N_DOCS) < 0.1, np.zeros(C.N_DOCS, bool)])
    group_flags[2, :30] = True                     # a group of 30 documents: fewer groups than k may remain
    return flags, group_flags


@pytest.mark.parametrize("row_dtype,precision", [("fp32", "fp32"), ("fp32", "fp32_filtered"), ("fp16", "fp32"), ("fp16", "fp32_filtered")])
def test_dense_search_collapsed(row_dtype, precision):
    D, Q, keys, S = C.dense_case()
    idx = _dense_index(D, row_dtype, precision)
    flags, group_flags = _filters()
    k = 10
    for nq in (1, 8, 200):
        q = torch.from_numpy(Q[:nq]).cuda()
        query_group = (np.arange(nq) % 3).astype(np.int64)
        cases = {"all": ({}, None), "subset": (dict(subset=np.flatnonzero(flags)), flags), "mask": (dict(mask=flags), flags),
                 "groups": (dict(masks=group_flags, query_group=query_group), group_flags[query_group])}
        for name, (kw, keep) in cases.items():
            ranking = C.full_ranking(S[:nq], keep=keep)
            got = idx.search_collapsed(q, k, keys, **kw)
            _check(got, C.collapsed_ranking(ranking, keys, k), (nq, name))
            assert idx.batch_invariant is False                                        # the caller's setting is put back
            # every returned score is the pair scorer's
            s, i, _, c, _ = got
            valid = i >= 0
            indptr = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
            indptr[1:] = torch.cumsum(valid.sum(1), 0)
            pair = idx.score_pairs(q, indptr, i[valid])
            assert torch.equal(pair.view(torch.int32), s[valid].view(torch.int32)), (nq, name)
            assert torch.equal(valid.sum(1).to(torch.int32), c)
    idx.close()


def test_dense_routes():
    """depths = (16, 64): by the CPU's full ranking some queries complete at depth 0, some at depth 1, and those that point at the
    planted group of 500 passages only through the full-ranking route."""
    D, Q, keys, S = C.dense_case()
    idx = _dense_index(D, "fp32", "fp32")
    k, depths = 10, (16, 64)
    ranking = C.full_ranking(S)
    route = C.first_complete_depth(ranking, keys, k, depths, C.N_DOCS)
    for r in (-1, 0, 1):
        assert (route == r).sum() >= 8, r                                              # no route goes untested
    want = C.collapsed_ranking(ranking, keys, k)
    q = torch.from_numpy(Q).cuda()
    got = idx.search_collapsed(q, k, keys, depths=depths)
    _check(got, want, "routes")
    assert np.array_equal(got[4]["depth"], route) and got[4]["depths"] == depths
    assert np.array_equal(got[4]["groups_seen"], want[3])
    # the full-ranking route in several sub-batches: 3000 documents * 40 bytes per query, two queries at a time
    small = idx.search_collapsed(q, k, keys, depths=depths, fallback_bytes=250_000)
    _check(small, want, "sub-batches")
    assert np.array_equal(small[4]["depth"], route)
    with pytest.raises(MemoryError, match=r"query %d alone needs 120000 bytes" % int(np.flatnonzero(route == -1)[0])):
        idx.search_collapsed(q, k, keys, depths=depths, fallback_bytes=100_000)
    # depths beyond sr_max_topk() and beyond the index are legal: clipped to the document count, where a row is the whole ranking
    deep = idx.search_collapsed(q, k, keys, depths=(5000,))
    _check(deep, want, "one deep round")
    assert (deep[4]["depth"] == 0).all()
    # fewer groups than k: padding and counts, only the whole ranking proves it
    few = (np.arange(C.N_DOCS) % 4).astype(np.int32)
    got = idx.search_collapsed(q[:5], k, few, depths=depths)
    _check(got, C.collapsed_ranking(ranking[:5], few, k), "four groups")
    assert got[3].tolist() == [4] * 5 and (got[1][:, 4:] == -1).all() and (got[4]["depth"] == -1).all()
    with pytest.raises(ValueError, match="query 0, position"):                         # a negative key surfaces from the driver too
        idx.search_collapsed(q[:5], k, np.full(C.N_DOCS, -1, np.int32))
    idx.close()


@pytest.mark.parametrize("threshold", [0.0, -1.0])
def test_sparse_search_collapsed(threshold):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    indptr, doc_ids, vals, qi, qc, qv, keys, S = C.sparse_case()
    idx = SparseIndexHIP(indptr, doc_ids, vals, C.S_DOCS)
    k, depths = 10, (16, 64)
    above = S > threshold
    ranking = C.full_ranking(S, keep=above)
    route = C.first_complete_depth(ranking, keys, k, depths, C.S_DOCS)
    for r in (-1, 0, 1):
        assert (route == r).sum() >= 4, r
    want = C.collapsed_ranking(ranking, keys, k)
    got = idx.search_collapsed(qi, qc, qv, k, keys, threshold=threshold, depths=depths)
    _check(got, want, "routes")
    assert np.array_equal(got[4]["depth"], route)
    _check(idx.search_collapsed(qi, qc, qv, k, keys, threshold=threshold), want, "default depths")
    _check(idx.search_collapsed(qi, qc, qv, k, keys, threshold=threshold, depths=depths, fallback_bytes=250_000), want, "sub-batches")
    # ids = 5 + 3 * position: the key table is indexed by those; every other entry is a key the kernel must never read
    base, stride = 5, 3
    ext = np.full(base + (C.S_DOCS - 1) * stride + 1, -1, np.int32)
    ext[base + stride * np.arange(C.S_DOCS)] = keys
    got = idx.search_collapsed(qi, qc, qv, k, ext, threshold=threshold, id_base=base, id_stride=stride, depths=depths)
    moved = (want[0], np.where(want[1] >= 0, base + stride * want[1], -1), want[2], want[3])
    _check(got, moved, "id_base / id_stride")
    assert np.array_equal(got[4]["depth"], route)
    # filters
    flags, group_flags = _filters()
    nq = len(qi) - 1
    query_group = (np.arange(nq) % 3).astype(np.int64)
    for name, kw, keep in (("subset", dict(subset=np.flatnonzero(flags)), flags[None] & above), ("mask", dict(mask=flags), flags[None] & above),
                           ("groups", dict(masks=group_flags, query_group=query_group), group_flags[query_group] & above)):
        r = C.full_ranking(S, keep=keep)
        got = idx.search_collapsed(qi, qc, qv, k, keys, threshold=threshold, depths=depths, **kw)
        _check(got, C.collapsed_ranking(r, keys, k), name)
        assert np.array_equal(got[4]["depth"], C.first_complete_depth(r, keys, k, depths, C.S_DOCS)), name
    idx.close()


# ---------------------------------------------------------------------------------------------------------------- indexer level
def test_dense_flat_indexer_search_collapsed():
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    D, Q, keys, S = C.dense_case()
    db_ids = [f"p{i}" for i in range(C.N_DOCS)]
    labels = [f"g{g}" for g in keys.tolist()]
    ix = DenseFlatIndexer()
    ix.init_index(C.DIM)
    ix.index_data(D, db_ids)
    nq, k = 30, 10
    ranking = C.full_ranking(S[:nq])
    want = C.collapsed_ranking(ranking, keys, k)
    for group_of in (dict(zip(db_ids, labels)), lambda d: labels[int(d[1:])], labels):
        got = ix.search_collapsed(Q[:nq], k, group_of)
        assert len(got) == nq
        for q, (groups, scores, passages) in enumerate(got):
            c = int(want[3][q])
            assert groups == [f"g{g}" for g in want[2][q, :c]] and passages == [f"p{i}" for i in want[1][q, :c]], q
            assert np.array_equal(_bits(scores), _bits(want[0][q, :c])), q
    flags, _ = _filters()
    got, stats = ix.search_collapsed(Q[:nq], k, labels, allowed_mask=flags, depths=(16, 64), return_stats=True)
    r = C.full_ranking(S[:nq], keep=flags)
    want = C.collapsed_ranking(r, keys, k)
    assert [g[2] for g in got] == [[f"p{i}" for i in want[1][q, :int(want[3][q])]] for q in range(nq)]
    assert np.array_equal(stats["depth"], C.first_complete_depth(r, keys, k, (16, 64), int(flags.sum())))
    with pytest.raises(ValueError, match="aligned with the index"):
        ix.search_collapsed(Q[:nq], k, labels[:-1])
    with pytest.raises(ValueError, match="not both"):
        ix.search_collapsed(Q[:nq], k, labels, allowed_ids=["p1"], allowed_mask=flags)


def test_sparse_retrieval_writes_a_run_keyed_by_group(golden_dir, tmp_path):
    """SparseRetrieval.retrieve(collapse=): run.json equals the definition applied to the full ranking the plain retrieve writes (every
    document, topk = the collection), key order included; q_stats.json gains the route statistics."""
    import json
    import os
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
    want = {}
    for qid, row in full.items():
        out = {}
        for pid, score in row.items():                   # json keeps the file's order: best first
            if group_of[pid] not in out and len(out) < 5:
                out[group_of[pid]] = score
        want[qid] = out
    assert any(len(set(group_of[p] for p in row)) < len(row) for row in full.values())      # something is collapsed
    for name, how in (("dict", group_of), ("callable", lambda p: group_of[p])):
        res = retriever(name).retrieve(loader(), topk=5, threshold=0.0, collapse=how)
        got = json.loads((tmp_path / name / "run.json").read_text())
        assert got == want and [list(r) for r in got.values()] == [list(r) for r in want.values()] and list(got) == list(want)
        assert res.to_dict() == want
        stats = json.loads((tmp_path / name / "q_stats.json").read_text())
        assert sum(stats["collapse"]["queries_per_depth"]) + stats["collapse"]["full_ranking_queries"] == len(full) and "L0_q" in stats


from test_hybrid_search_gpu import toy  # noqa: E402,F401  (the module-scoped fixture: a tiny LlamaBiHybrid, 90 documents, 8 queries)


def test_hybrid_retriever_writes_both_runs_keyed_by_group(toy):  # noqa: F811
    """HybridRetriever.retrieve(collapse=): sparse/run.json and dense/run.json equal the definition applied to the full rankings the plain
    retrieve writes (topk = the collection), key order included; q_stats.json carries both heads' route statistics."""
    import json
    import os
    from test_hybrid_search_gpu import _retriever
    full_ret, full_dir = _retriever(toy, "collapse_full")
    n_docs = len(full_ret.dense_index.index_id_to_db_id)
    full_ret.retrieve(toy[3](), topk=n_docs)
    db_ids = list(full_ret.dense_index.index_id_to_db_id)
    group_of = {d: f"doc{i // 3}" for i, d in enumerate(db_ids)}
    ret, out_dir = _retriever(toy, "collapse_run")
    by_label = [group_of[d] for d in db_ids]                       # a sequence: aligned with the dense index's order
    for how in (group_of, by_label):
        sparse_res, dense_res = ret.retrieve(toy[3](), topk=5, collapse=how)
        for head, res in (("sparse", sparse_res), ("dense", dense_res)):
            full = json.load(open(os.path.join(full_dir, head, "run.json")))
            want = {}
            for qid, row in full.items():
                out = {}
                for pid, score in row.items():
                    if group_of[pid] not in out and len(out) < 5:
                        out[group_of[pid]] = score
                want[qid] = out
            got = json.load(open(os.path.join(out_dir, head, "run.json")))
            assert got == want and [list(r) for r in got.values()] == [list(r) for r in want.values()], head
            assert res.to_dict() == want
        stats = json.load(open(os.path.join(out_dir, "sparse", "q_stats.json")))
        assert "collapse" in stats and "collapse_dense" in stats and "L0_q" in stats
    with pytest.raises(NotImplementedError, match="not offered under collapse"):
        ret.retrieve_fused(toy[3](), topk=5, collapse=group_of)
