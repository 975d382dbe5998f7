"""GPU: sr_sparse_mmr (csrc/sparse_mmr.hip) against the numpy model of tests/mmr_sparse_cases.py - equal bits (uint32)
of the relevance and the marginal values, equal ids / positions / counts - and the Python layers over it.  One collection of 600
documents over 512 terms serves every test; its two similarity matrices are computed once."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import mmr_sparse_cases as M

pytestmark = pytest.mark.gpu
F32 = np.float32
SPECIAL = [3, 4, 17, 18] + list(range(20, 29)) + [30, 50, 31, 51, 60, 63, 599]          # empty, one-term, long, twin and disjoint rows

_built = {}


def _index():
    """(SparseIndexHIP, the documents' rows, {"ip": matrix, "cosine": matrix}), built once."""
    if not _built:
        from scaling_retriever_amd.scoring import SparseIndexHIP
        rows = M.collection()
        ip = M.ip_matrix(rows)
        _built["x"] = (SparseIndexHIP(*M.term_major_csr(rows), M.N_DOCS), rows, {"ip": ip, "cosine": M.cosine_matrix(ip)})
    return _built["x"]


def _candidates(nq, n, seed, special=True):
    """Relevance in steps of 1/8 inside [0, 4): many candidates share one f32(lambda * rel), the similarities decide between them."""
    ids, rel = M.candidates(M.N_DOCS, nq, n, seed)
    rel = (np.round(rel / 30 * 32) / 8).astype(F32)
    if special and n >= 63:
        ids[:, 5:5 + len(SPECIAL)] = SPECIAL
    return ids, rel


def _host(got):
    return [t.cpu().numpy() for t in got]


def _same(got, want, what=""):
    got = _host(got) if torch.is_tensor(got[0]) else got
    for name, g, w in zip(("ids", "rel", "mmr", "pos", "counts"), got, want):
        if name in ("rel", "mmr"):
            g, w = M.bits(g), M.bits(w)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


def _row_of(d):
    return d if 0 <= d < M.N_DOCS else None


@pytest.mark.parametrize("sim", ["ip", "cosine"])
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n,k,nq", [(1, 1, 1), (63, 10, 3), (64, 64, 2), (65, 20, 5), (130, 40, 4), (1024, 30, 2)])
def test_kernel_equals_the_model(n, k, nq, lam, sim):
    idx, rows, sims = _index()
    ids, rel = _candidates(nq, n, seed=n * 7 + nq)
    want = M.mmr(sims[sim], _row_of, ids, rel, k, lam)
    got = _host(idx.mmr(ids, rel, k, lam, sim=sim))
    _same(got, want, (n, k, nq, lam, sim))
    _same(idx.mmr(ids, rel, k, lam, sim=sim), got, "a second call returns the same bytes")
    assert want[4].tolist() == [min(k, n)] * nq
    if lam == 1.0:                                  # the first k candidates by (rel, id, position)
        for q in range(nq):
            order = np.lexsort((np.arange(n), ids[q], -rel[q].astype(np.float64)))[:k]
            assert np.array_equal(want[3][q], order)
    elif k > 2:
        assert (np.diff(want[2][:, 1:], axis=1) <= 0).all()


@pytest.mark.parametrize("sim", ["ip", "cosine"])
@pytest.mark.parametrize("chunk", [7, 48, 64])
def test_long_rows_cross_chunk_boundaries(monkeypatch, chunk, sim):
    """SR_MMR_SPARSE_CHUNK (read per call) stages the picked row 7 / 48 / 64 entries at a time.  k = n: every candidate is picked, so
    every row but the last pick's is staged - the rows of 63 .. 300 terms cross several chunks, and every chain against them continues
    from its saved sum."""
    idx, rows, sims = _index()
    ids, rel = _candidates(3, 65, seed=5)
    want = M.mmr(sims[sim], _row_of, ids, rel, 65, 0.5)
    assert all(len({23, 24, 25, 26, 27, 28} & {int(d) for d in want[0][q, :-1]}) >= 5 for q in range(3))      # the long rows are staged
    free = _host(idx.mmr(ids, rel, 65, 0.5, sim=sim))
    monkeypatch.setenv("SR_DEV_SWITCHES", "1")
    monkeypatch.setenv("SR_MMR_SPARSE_CHUNK", str(chunk))
    _same(idx.mmr(ids, rel, 65, 0.5, sim=sim), want, chunk)
    _same(free, want, "unchunked")


@pytest.mark.parametrize("sim", ["ip", "cosine"])
def test_counts_padding_and_k_beyond_the_valid_count(sim):
    """A prefix of 0, padding ids in the middle of a row, a repeated id, and k greater than what is valid: shorter rows, padded."""
    idx, rows, sims = _index()
    nq, n = 5, 130
    ids, rel = _candidates(nq, n, seed=11)
    counts = np.array([n, 0, n // 2, 3, n + 5], np.int32)          # beyond n: clipped
    ids[0, [1, 40, 63, 64]] = -1
    ids[2, :n // 2:3] = -7
    ids[3, :3] = -1                                                # a prefix that holds padding only
    ids[4, 5] = ids[4, 70] = ids[4, 0]                             # one document three times
    rel[4, 5] = rel[4, 0]
    for k in (n, 7):
        want = M.mmr(sims[sim], _row_of, ids, rel, k, 0.3, counts)
        _same(idx.mmr(ids, rel, k, 0.3, counts=counts, sim=sim), want, k)
    assert want[4].tolist() == [7, 0, 7, 0, 7]
    want = M.mmr(sims[sim], _row_of, ids, rel, n, 0.3, counts)
    assert want[4].tolist() == [n - 4, 0, n // 2 - len(range(0, n // 2, 3)), 0, n]
    assert (want[0][1] == -1).all() and (M.bits(want[2][1]) == M.bits(F32(-M.FLT_MAX))).all()
    twin = [int(p) for p in want[3][4] if ids[4, p] == ids[4, 0]]
    assert sorted(twin) == sorted({0, 5, 70})                      # each entry its own candidate


@pytest.mark.parametrize("sim", ["ip", "cosine"])
def test_repeated_ids_and_identical_rows_fall_by_id_then_position(sim):
    """Documents 50..59 repeat 30..39 (and 27, 28 the long rows 24, 23): twins with one relevance have one marginal value at every
    pick, the smaller id goes first; the same id twice with one relevance: the smaller position."""
    idx, rows, sims = _index()
    rng = np.random.default_rng(5)
    nq, n = 4, 64
    twins = list(range(30, 40)) + list(range(50, 60)) + [23, 24, 27, 28]
    ids = np.stack([rng.permutation(np.concatenate([twins, rng.choice(np.arange(100, 590), n - len(twins) - 2, replace=False), [33, 55]]))
                    for _ in range(nq)]).astype(np.int64)
    rel = (np.round(rng.uniform(0, 4, (nq, n)) * 2) / 2).astype(F32)
    for q in range(nq):
        where = {int(d): i for i, d in enumerate(ids[q])}
        for a, b in [(30 + t, 50 + t) for t in range(M.TWINS)] + [(24, 27), (23, 28)]:
            rel[q, ids[q] == b] = rel[q, where[a]]
            rel[q, ids[q] == a] = rel[q, where[a]]
    info = {}
    want = M.mmr(sims[sim], _row_of, ids, rel, n, 0.3, info=info)
    assert info["ties"] >= nq * M.TWINS // 2, info
    _same(idx.mmr(ids, rel, n, 0.3, sim=sim), want)
    _same(idx.mmr(ids, rel, n, 0.0, sim=sim), M.mmr(sims[sim], _row_of, ids, rel, n, 0.0))     # lambda = 0: relevance only picks the first


@pytest.mark.parametrize("sim", ["ip", "cosine"])
def test_empty_rows(sim):
    """An empty row is a candidate like any other: similarity +0.0f to everything (cosine: its norm is zero, never a NaN), picked and
    staged as a row of no entries.  Query 1 holds empty rows only."""
    idx, rows, sims = _index()
    ids, rel = _candidates(3, 20, seed=3, special=False)
    ids[0, :4] = M.EMPTY_ROWS
    rel[0, 0] = F32(9.0)                                           # an empty row is pick 0: every similarity of pick 1 is +0.0f
    ids[1] = np.resize(np.array(M.EMPTY_ROWS), 20)
    ids[2, 3:6] = (3, 4, 599)
    for lam in (0.0, 0.5):
        want = M.mmr(sims[sim], _row_of, ids, rel, 20, lam)
        _same(idx.mmr(ids, rel, 20, lam, sim=sim), want, lam)
    assert want[4].tolist() == [20, 20, 20] and np.isfinite(want[2]).all()
    assert want[0][0, 0] == M.EMPTY_ROWS[0] and M.bits(want[2][0, 1]) == M.bits(F32(F32(0.5) * want[1][0, 1]))


def test_every_inner_product_is_the_pair_scorers():
    """Two candidates (i, j) with rel = 0 under lambda = 0: pick 0 is the smaller id, pick 1 the other, and its marginal value is
    f32(0 - f32(1 * ip(i, j))): -ip(i, j) exactly (+0.0f where ip is +0.0f).  For random pairs, every pair of the special rows and every document with itself:
    the kernel's ip, the model's, and score_pairs of (row i as the query, document j) are the same bits."""
    from scaling_retriever_amd.mmr import forward_rows_of
    idx, rows, sims = _index()
    rng = np.random.default_rng(8)
    pairs = np.concatenate([rng.integers(0, M.N_DOCS, (3000, 2)), np.array([(a, b) for a in SPECIAL for b in SPECIAL]),
                            np.repeat(np.arange(M.N_DOCS), 2).reshape(-1, 2)]).astype(np.int64)
    got = _host(idx.mmr(pairs, np.zeros(pairs.shape, F32), 2, 0.0, sim="ip"))
    assert got[4].tolist() == [2] * len(pairs)
    want = sims["ip"][pairs[:, 0], pairs[:, 1]]
    want_v = (F32(0.0) - (F32(1.0) * want).astype(F32)).astype(F32)
    assert np.array_equal(M.bits(got[2][:, 1]), M.bits(want_v)), np.argwhere(M.bits(got[2][:, 1]) != M.bits(want_v))[:5].tolist()
    assert (want != 0).sum() > 1000 and (want == 0).sum() > 100
    dev = idx.device
    left = torch.from_numpy(pairs[:, 0]).to(dev)
    scored = idx.score_pairs(*forward_rows_of(idx, left), torch.arange(len(pairs) + 1, device=dev), torch.from_numpy(pairs[:, 1]).to(dev))
    assert np.array_equal(M.bits(scored.cpu().numpy()), M.bits(want))
    fwd = [t.cpu().numpy() for t in idx.forward_rows()]
    for a, b in zip(fwd, M.doc_major_csr(rows)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("sim", ["ip", "cosine"])
def test_kernel_equals_the_per_step_composition(sim):
    """scaling_retriever_amd.mmr.sparse_mmr_by_steps - per pick the picked rows gathered into a query CSR, one score_pairs call, torch
    operations - is what a caller had before the kernel and what tools/bench_mmr_sparse.py measures against: the same bits."""
    from scaling_retriever_amd.mmr import sparse_mmr_by_steps
    idx, rows, sims = _index()
    ids, rel = _candidates(5, 70, seed=9)
    ids[1, 3:9] = -1
    counts = np.array([70, 70, 33, 0, 70], np.int32)
    for lam in (0.3, 1.0):
        got = idx.mmr(ids, rel, 12, lam, counts=counts, sim=sim)
        _same(got, M.mmr(sims[sim], _row_of, ids, rel, 12, lam, counts), lam)
        _same(sparse_mmr_by_steps(idx, ids, rel, 12, lam, counts=counts, sim=sim), _host(got), lam)


def test_a_position_outside_the_index_is_named_and_nothing_is_selected():
    from scaling_retriever_amd import _lib
    idx, rows, sims = _index()
    ids, rel = _candidates(3, 20, seed=2, special=False)
    bad = ids.copy()
    bad[1, 2] = M.N_DOCS
    bad[2, 4] = 1 << 40
    with pytest.raises(ValueError, match=rf"candidate id {M.N_DOCS} \(query 1, entry 2\)"):
        idx.mmr(bad, rel, 5, 0.5)
    bad[1, 2] = -1                                                  # padding is skipped, a prefix hides the other offender
    cnt = np.array([20, 20, 4], np.int32)
    _same(idx.mmr(bad, rel, 5, 0.5, counts=cnt), M.mmr(sims["cosine"], _row_of, bad, rel, 5, 0.5, cnt))
    with pytest.raises(ValueError, match=rf"candidate id {1 << 40} \(query 2, entry 4\)"):
        idx.mmr(bad, rel, 5, 0.5, sim="ip")
    # the error return of the entry point itself: every output row is padding, for the queries without an offender too
    dev = idx.device
    fwd = idx.forward_rows()
    t_ids, t_rel = torch.from_numpy(bad).to(dev), torch.from_numpy(rel).to(dev)
    out = [torch.full((3, 5), 7, dtype=dt, device=dev) for dt in (torch.int64, torch.float32, torch.float32, torch.int32)]
    out_counts = torch.full((3,), 7, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = idx.lib.sr_sparse_mmr(p(fwd[0]), p(fwd[1]), p(fwd[2]), M.N_DOCS, p(t_ids), p(t_rel), None, 3, 20, 5, 0.5, _lib.SR_MMR_SIM_COSINE,
                               *map(p, out), p(out_counts), _lib.stream_ptr())
    assert rc == _lib.SR_ERR_INVALID and b"query 2, entry 4" in idx.lib.sr_last_error()
    o_ids, o_rel, o_mmr, o_pos = _host(out)
    assert (o_ids == -1).all() and (o_pos == -1).all() and (out_counts.cpu().numpy() == 0).all()
    assert (M.bits(o_rel) == M.bits(F32(-M.FLT_MAX))).all() and (M.bits(o_mmr) == M.bits(F32(-M.FLT_MAX))).all()
    with pytest.raises(ValueError, match="must lie in"):
        idx.mmr(ids, rel, 21, 0.5)
    with pytest.raises(ValueError, match="must be one of"):
        idx.mmr(ids, rel, 5, 0.5, sim="dot")
    with pytest.raises(ValueError, match="same shape"):
        idx.mmr(ids, rel[:, :5], 5, 0.5)
    _same(idx.mmr(ids, rel, 5, 0.5), M.mmr(sims["cosine"], _row_of, ids, rel, 5, 0.5))          # the library stays usable


def _queries(nq, seed, terms=10):
    rng = np.random.default_rng(seed)
    cols = np.concatenate([np.sort(rng.choice(M.V, terms, replace=False)) for _ in range(nq)]).astype(np.int32)
    return np.arange(nq + 1, dtype=np.int64) * terms, cols, rng.uniform(0.1, 2.0, nq * terms).astype(F32)


@pytest.mark.parametrize("nq", [1, 5])
def test_search_mmr_with_lambda_one_is_the_plain_search(nq):
    idx, rows, sims = _index()
    q = _queries(nq, 21)
    allowed = np.zeros(M.N_DOCS, bool)
    allowed[::3] = True
    for how in ({}, {"mask": allowed}, {"subset": np.nonzero(allowed)[0]}):
        scores, ids, counts = _host(idx.search(*q, 10, **how))
        assert counts.tolist() == [10] * nq
        for sim in ("ip", "cosine"):
            got = _host(idx.search_mmr(*q, 10, 40, lam=1.0, sim=sim, **how))
            assert np.array_equal(got[0], ids) and np.array_equal(M.bits(got[1]), M.bits(scores))
            assert np.array_equal(M.bits(got[2]), M.bits(got[1])) and np.array_equal(got[3], np.tile(np.arange(10, dtype=np.int32), (nq, 1)))
            assert got[4].tolist() == [10] * nq
            # and a real lambda: the model over the search's own rows and counts
            s40, i40, c40 = _host(idx.search(*q, 40, **how))
            _same(idx.search_mmr(*q, 10, 40, lam=0.3, sim=sim, **how), M.mmr(sims[sim], _row_of, i40, s40, 10, 0.3, c40), (how.keys(), sim))
    with pytest.raises(ValueError, match="not both"):
        idx.search_mmr(*q, 10, 40, subset=[1, 2], mask=allowed)
    with pytest.raises(ValueError, match="fetch_k = 5"):
        idx.search_mmr(*q, 10, 5)
    with pytest.raises(ValueError, match="must be one of"):
        idx.search_mmr(*q, 10, 40, sim="l2")


def test_search_mmr_under_filter_groups_equals_the_per_group_calls():
    idx, rows, sims = _index()
    nq = 6
    q = _queries(nq, 22)
    masks = np.zeros((3, M.N_DOCS), bool)
    masks[0, ::2] = True
    masks[1, 100:130] = True                                      # 30 documents: fewer hits than fetch_k, the rows end in padding
    masks[2, :] = True
    group = np.array([0, 1, 2, 1, 0, 2])
    got = _host(idx.search_mmr(*q, 25, 40, lam=0.3, masks=masks, query_group=group))
    s, i, c = _host(idx.search_grouped(*q, 40, masks, group))
    _same(got, M.mmr(sims["cosine"], _row_of, i, s, 25, 0.3, c))
    assert (got[4][group == 1] < 25).all() and got[4][group != 1].tolist() == [25] * 4
    for g in range(3):
        at = np.nonzero(group == g)[0]
        sub = (np.arange(len(at) + 1, dtype=np.int64) * 10, q[1].reshape(nq, 10)[at].ravel(), q[2].reshape(nq, 10)[at].ravel())
        _same(idx.search_mmr(*sub, 25, 40, lam=0.3, mask=masks[g]), [x[at] for x in got], g)


def test_search_mmr_maps_the_picks_to_id_base_and_stride():
    idx, rows, sims = _index()
    q = _queries(4, 23)
    plain = _host(idx.search_mmr(*q, 12, 40, lam=0.4, sim="ip", threshold=0.5))
    moved = _host(idx.search_mmr(*q, 12, 40, lam=0.4, sim="ip", threshold=0.5, id_base=1000, id_stride=3))
    assert np.array_equal(moved[0], np.where(plain[0] >= 0, 1000 + 3 * plain[0], -1))
    _same([plain[0]] + moved[1:], plain)
    s, i, c = _host(idx.search(*q, 40, threshold=0.5))
    _same(plain, M.mmr(sims["ip"], _row_of, i, s, 12, 0.4, c))
    # a mask that leaves fewer than k documents: the padding stays -1 under the mapping
    few = np.zeros(M.N_DOCS, bool)
    few[200:205] = True
    short = _host(idx.search_mmr(*q, 12, 40, lam=0.4, id_base=1000, id_stride=3, mask=few))
    assert (short[4] <= 5).all() and all((short[0][r, short[4][r]:] == -1).all() and (short[0][r, :short[4][r]] >= 1600).all() for r in range(4))


def test_eval_sparse_writes_the_diversified_run_beside_the_plain_one(golden_dir, tmp_path):
    from golden_weights import make_weights
    from test_eval_drivers import ROOT, _texts, _write_model
    sys.path.insert(0, ROOT)
    import eval_sparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    rng = np.random.default_rng(3)
    lora = _write_model(str(tmp_path), cfg, w, rng)["sparse"][0]
    docs, queries = _texts(rng, 60, 3, 20), _texts(rng, 6, 2, 6)
    docs[30:36] = docs[:6]                                          # near-duplicates under other ids: exact ones
    (tmp_path / "corpus.tsv").write_text("".join(f"d{i}\t{t}\n" for i, t in enumerate(docs)))
    (tmp_path / "queries.tsv").write_text("".join(f"q{i}\t{t}\n" for i, t in enumerate(queries)))
    index_dir, plain, div = (str(tmp_path / n) for n in ("sp_index", "out_plain", "out_mmr"))
    eval_sparse.main(["--task_name", "indexing", "--model_name_or_path", lora, "--corpus_path", str(tmp_path / "corpus.tsv"),
                      "--index_dir", index_dir, "--eval_batch_size", "8", "--doc_max_length", "16", "--token_budget", "0"])
    common = ["--task_name", "retrieval", "--model_name_or_path", lora, "--query_path", str(tmp_path / "queries.tsv"), "--index_dir", index_dir,
              "--top_k", "10", "--query_max_length", "8"]
    eval_sparse.main(common + ["--out_dir", plain])
    # lambda = 0: after pick 0 the similarity alone decides.  The toy model's rows are dense in its 512 terms and all alike (cosines near
    # one another), so a lambda that keeps the relevance would leave the top 10 of 60 documents as they are
    eval_sparse.main(common + ["--out_dir", div, "--mmr_lambda", "0", "--mmr_fetch_k", "40"])
    for name in ("run.json", "q_stats.json"):
        assert open(os.path.join(div, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    assert not os.path.exists(os.path.join(plain, "mmr"))
    run = json.load(open(os.path.join(div, "mmr", "run.json")))
    stats = json.load(open(os.path.join(div, "mmr", "q_stats.json")))
    plain_run = json.load(open(os.path.join(plain, "run.json")))
    assert list(run) == list(plain_run) == list(stats)
    moved = 0
    for qid, hits in run.items():
        n = len(hits)
        assert 0 < n <= 10 and list(hits.values()) == [float(n - t) for t in range(n)]      # the selection order, as a score every metric sorts by
        assert next(iter(hits)) == next(iter(plain_run[qid]))                               # pick 0 is the most relevant document
        assert stats[qid]["picks"] == n and set(stats[qid]) == {"picks", "mean_mmr", "picks_outside_top_k"}
        assert stats[qid]["picks_outside_top_k"] == len(set(hits) - set(plain_run[qid]))
        moved += stats[qid]["picks_outside_top_k"]
    assert moved > 0
