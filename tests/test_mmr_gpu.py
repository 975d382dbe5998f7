"""GPU: sr_dense_mmr (csrc/dense_mmr.hip) against the numpy model of tests/mmr_cases.py - equal bits (uint32) of the
relevance and the marginal values, equal ids / positions / counts - and the Python layers over it.  Indexes hold at most 400 rows."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import mmr_cases as M

pytestmark = pytest.mark.gpu
F32 = np.float32
N1, N2, BASE2, STRIDE2 = 150, 150, 1000, 2
TWINS = 10                                      # rows TWINS .. 2 TWINS - 1 repeat rows 0 .. TWINS - 1: equal similarities to everything

_built = {}


def _index(H, row_dtype="fp32", layout="two"):
    """(DenseIndexHIP, global ids of its rows, {global id: row}, the model's similarity matrix), built once per kind."""
    key = (H, row_dtype, layout)
    if key not in _built:
        from scaling_retriever_amd.scoring import DenseIndexHIP
        rng = np.random.default_rng(H + (7 if row_dtype == "fp16" else 0))
        D = rng.standard_normal((N1 + N2, H)).astype(F32)
        D[TWINS:2 * TWINS] = D[:TWINS]
        idx = DenseIndexHIP(H, row_dtype=row_dtype)
        if layout == "two":
            idx.add_host_rows(D[:N1])
            idx.add_host_rows(D[N1:], id_base=BASE2, id_stride=STRIDE2)
            gid = np.concatenate([np.arange(N1, dtype=np.int64), BASE2 + STRIDE2 * np.arange(N2, dtype=np.int64)])
        else:
            idx.add_host_rows(D)
            gid = np.arange(N1 + N2, dtype=np.int64)
        _built[key] = (idx, gid, {int(g): r for r, g in enumerate(gid)}, M.similarities(M.stored(D, row_dtype)), D)
    return _built[key][:4]


def _candidates(gid, nq, n, seed, quantum=None):
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.choice(gid, size=n, replace=n > gid.size) for _ in range(nq)]).astype(np.int64)
    rel = rng.standard_normal((nq, n)).astype(F32)
    if quantum:
        rel = (np.round(rel / quantum) * quantum).astype(F32)
    return ids, rel


def _host(got):
    return [t.cpu().numpy() for t in got]


def _same(got, want, what=""):
    got = _host(got) if torch.is_tensor(got[0]) else got
    for name, g, w in zip(("ids", "rel", "mmr", "pos", "counts"), got, want):
        if name in ("rel", "mmr"):
            g, w = M.bits(g), M.bits(w)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


def _cap():
    from scaling_retriever_amd import _lib
    return int(_lib.load().sr_mmr_max_candidates())


@pytest.mark.parametrize("H,n,k,nq,lam,row_dtype,layout", [
    (64, 1, 1, 1, 0.3, "fp32", "one"),
    (64, 63, 63, 1, 0.3, "fp32", "one"),
    (64, 64, 1, 1, 0.3, "fp32", "one"),
    (64, 64, 64, 5, 0.0, "fp32", "two"),
    (64, 65, 65, 1, 0.3, "fp16", "one"),
    (80, 130, 130, 5, 0.3, "fp32", "two"),          # a ragged last chunk, three tiles on three waves
    (80, 130, 1, 5, 1.0, "fp16", "two"),
    (80, 257, 257, 1, 0.0, "fp16", "two"),
    (192, 257, 257, 5, 0.3, "fp32", "two"),         # several chunks, five tiles
    (192, 130, 130, 1, 1.0, "fp32", "one"),
    (192, 65, 65, 5, 0.3, "fp16", "two"),
    (64, "cap", "cap", 1, 0.3, "fp32", "two"),      # more tiles than waves; ids repeat (the index holds 300 rows)
    (80, "cap", 1, 5, 0.3, "fp16", "one"),
])
def test_kernel_equals_the_model(H, n, k, nq, lam, row_dtype, layout):
    n = _cap() if n == "cap" else n
    k = _cap() if k == "cap" else k
    idx, gid, row_of, sim = _index(H, row_dtype, layout)
    ids, rel = _candidates(gid, nq, n, seed=n * 7 + nq)
    want = M.mmr(sim, row_of.get, ids, rel, k, lam)
    got = idx.mmr(torch.from_numpy(ids).cuda(), torch.from_numpy(rel).cuda(), k, lam)
    _same(got, want, (H, n, k, nq, lam))
    assert want[4].tolist() == [min(k, n)] * nq
    if lam == 1.0:                                  # the first k candidates by (rel, id, position)
        for q in range(nq):
            order = np.lexsort((np.arange(n), ids[q], -rel[q].astype(np.float64)))[:k]
            assert np.array_equal(want[3][q], order)
    elif k > 2:
        assert (np.diff(want[2][:, 1:], axis=1) <= 0).all()


@pytest.mark.parametrize("H,n,row_dtype", [(80, 130, "fp32"), (192, 65, "fp16")])
def test_counts_padding_and_k_beyond_the_valid_count(H, n, row_dtype):
    """A prefix of 0, padding ids in the middle of a row, a repeated id, and k greater than what is valid: shorter rows, padded."""
    idx, gid, row_of, sim = _index(H, row_dtype, "two")
    nq = 5
    ids, rel = _candidates(gid, nq, n, seed=11)
    counts = np.array([n, 0, n // 2, 3, n + 5], np.int32)          # beyond n: clipped
    ids[0, [1, 40, 63, 64]] = -1
    ids[2, :n // 2:3] = -7
    ids[3, :3] = -1                                                # a prefix that holds padding only
    ids[4, 5] = ids[4, 70 % n] = ids[4, 0]                         # one document three times
    rel[4, 5] = rel[4, 0]
    for k in (n, 7):
        want = M.mmr(sim, row_of.get, ids, rel, k, 0.3, counts)
        got = idx.mmr(ids, rel, k, 0.3, counts=counts)
        _same(got, want, k)
    assert want[4].tolist() == [7, 0, 7, 0, 7]
    want = M.mmr(sim, row_of.get, ids, rel, n, 0.3, counts)
    assert want[4].tolist() == [n - 4, 0, n // 2 - len(range(0, n // 2, 3)), 0, n]
    assert (want[0][1] == -1).all() and (M.bits(want[2][1]) == M.bits(F32(-M.FLT_MAX))).all()
    twin = [int(p) for p in want[3][4] if ids[4, p] == ids[4, 0]]
    assert sorted(twin) == sorted({0, 5, 70 % n})                  # each entry its own candidate


def test_ties_between_identical_rows_fall_by_id_then_position():
    """Rows 10..19 repeat rows 0..9, and relevance comes in steps of 0.5: twins with one relevance have one marginal value at every
    pick, the smaller id goes first; the same id twice with one relevance: the smaller position."""
    idx, gid, row_of, sim = _index(64, "fp32", "one")
    rng = np.random.default_rng(5)
    nq, n = 5, 64
    ids = np.stack([rng.permutation(np.concatenate([np.arange(2 * TWINS), rng.choice(np.arange(2 * TWINS, 300), n - 2 * TWINS - 2, replace=False),
                                                    [3, 25]])) for _ in range(nq)]).astype(np.int64)
    rel = (np.round(rng.standard_normal((nq, n)) * 2) / 2).astype(F32)
    for q in range(nq):
        where = {int(d): i for i, d in enumerate(ids[q])}
        for t in range(TWINS):
            rel[q, where[TWINS + t]] = rel[q, where[t]]
        rel[q, ids[q] == 3] = rel[q, where[3]]
        rel[q, ids[q] == 13] = rel[q, where[3]]
    info = {}
    want = M.mmr(sim, row_of.get, ids, rel, n, 0.3, info=info)
    assert info["ties"] >= nq * TWINS // 2, info
    _same(idx.mmr(ids, rel, n, 0.3), want)
    _same(idx.mmr(ids, rel, n, 0.0), M.mmr(sim, row_of.get, ids, rel, n, 0.0))     # lambda = 0: relevance only picks the first


def test_unknown_id_is_named_and_nothing_is_selected():
    idx, gid, row_of, sim = _index(80, "fp32", "two")
    ids, rel = _candidates(gid, 3, 20, seed=2)
    bad = ids.copy()
    bad[1, 2] = BASE2 + 1                                           # between two rows of the strided segment
    bad[2, 4] = 5000
    with pytest.raises(ValueError, match=rf"candidate id {BASE2 + 1} \(query 1, entry 2\)"):
        idx.mmr(bad, rel, 5, 0.5)
    bad[1, 2] = -1                                                  # padding is skipped, a prefix hides the other offender
    _same(idx.mmr(bad, rel, 5, 0.5, counts=np.array([20, 20, 4], np.int32)), M.mmr(sim, row_of.get, bad, rel, 5, 0.5, np.array([20, 20, 4])))
    with pytest.raises(ValueError, match=r"candidate id 5000 \(query 2, entry 4\)"):
        idx.mmr(bad, rel, 5, 0.5)
    with pytest.raises(ValueError, match="must lie in"):
        idx.mmr(ids, rel, 21, 0.5)
    with pytest.raises(ValueError, match="same shape"):
        idx.mmr(ids, rel[:, :5], 5, 0.5)
    _same(idx.mmr(ids, rel, 5, 0.5), M.mmr(sim, row_of.get, ids, rel, 5, 0.5))      # the library stays usable


@pytest.mark.parametrize("row_dtype", ["fp32", "fp16"])
def test_kernel_equals_the_per_step_composition(row_dtype):
    """scaling_retriever_amd.mmr.mmr_by_steps - per pick one score_pairs call with the picked rows as queries, plus torch operations -
    is what a caller had before the kernel and what tools/bench_mmr.py measures against: the same bits."""
    from scaling_retriever_amd.mmr import mmr_by_steps, stored_rows
    idx, gid, row_of, sim = _index(80, row_dtype, "two")
    ids, rel = _candidates(gid, 5, 70, seed=9, quantum=0.25)
    ids[1, 3:9] = -1
    counts = np.array([70, 70, 33, 0, 70], np.int32)
    for lam in (0.3, 1.0):
        got = idx.mmr(ids, rel, 12, lam, counts=counts)
        _same(got, M.mmr(sim, row_of.get, ids, rel, 12, lam, counts), lam)
        _same(mmr_by_steps(idx, ids, rel, 12, lam, counts=counts), _host(got), lam)
    rows = stored_rows(idx, torch.from_numpy(ids[0, :4]).cuda()).cpu().numpy()
    assert np.array_equal(M.bits(rows), M.bits(M.stored(_built[(80, row_dtype, "two")][4], row_dtype)[[row_of[int(d)] for d in ids[0, :4]]]))


def _queries(H, nq, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((nq, H)).astype(F32)).cuda()


@pytest.mark.parametrize("nq", [1, 5])
def test_search_mmr_with_lambda_one_is_the_plain_search(nq):
    idx, gid, row_of, sim = _index(80, "fp32", "two")
    q = _queries(80, nq, 21)
    allowed = np.zeros(idx.id_end, bool)
    allowed[gid[::3]] = True
    for how in ({}, {"mask": allowed}):
        scores, ids = idx.search(q, 10, **how)
        got = _host(idx.search_mmr(q, 10, 40, lam=1.0, **how))
        assert np.array_equal(got[0], ids.cpu().numpy()) and np.array_equal(M.bits(got[1]), M.bits(scores.cpu().numpy()))
        assert np.array_equal(M.bits(got[2]), M.bits(got[1])) and np.array_equal(got[3], np.tile(np.arange(10, dtype=np.int32), (nq, 1)))
        assert got[4].tolist() == [10] * nq
        # and a real lambda: the model over the search's own rows
        s40, i40 = idx.search(q, 40, **how)
        _same(idx.search_mmr(q, 10, 40, lam=0.3, **how), M.mmr(sim, row_of.get, i40.cpu().numpy(), s40.cpu().numpy(), 10, 0.3))
    with pytest.raises(ValueError, match="not both"):
        idx.search_mmr(q, 10, 40, subset=[1, 2], mask=allowed)
    with pytest.raises(ValueError, match="fetch_k = 5"):
        idx.search_mmr(q, 10, 5)


def test_search_mmr_under_filter_groups():
    idx, gid, row_of, sim = _index(192, "fp16", "two")
    nq = 5
    q = _queries(192, nq, 22)
    masks = np.zeros((3, idx.id_end), bool)
    masks[0, gid[::2]] = True
    masks[1, gid[5:25]] = True                                    # 20 documents: fewer than fetch_k, the rows end in padding
    masks[2, gid] = True
    group = np.array([0, 1, 2, 1, 0])
    s, i = idx.search_grouped(q, 30, masks, group)
    want = M.mmr(sim, row_of.get, i.cpu().numpy(), s.cpu().numpy(), 25, 0.3)
    _same(idx.search_mmr(q, 25, 30, lam=0.3, masks=masks, query_group=group), want)
    assert want[4].tolist() == [25, 20, 25, 20, 25]


def test_dense_flat_indexer_search_mmr_maps_the_ids_back():
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    rng = np.random.default_rng(4)
    D = rng.standard_normal((90, 64)).astype(F32)
    D[40:50] = D[:10]
    ix = DenseFlatIndexer()
    ix.init_index(64)
    db_ids = [f"doc-{i}" for i in range(90)]
    ix.index_data(D[:50], db_ids[:50])
    ix.index_data(D[50:], db_ids[50:])
    q = rng.standard_normal((5, 64)).astype(F32)
    sim = M.similarities(D)
    scores, pos = ix.search_arrays(q, 30)
    want = M.mmr(sim, lambda d: d, pos, scores, 8, 0.4)
    lists, rel, mmr = ix.search_mmr(q, 8, 30, lam=0.4)
    assert lists == [[db_ids[p] for p in row] for row in want[0]]
    assert np.array_equal(M.bits(rel), M.bits(want[1])) and np.array_equal(M.bits(mmr), M.bits(want[2]))
    allowed = [f"doc-{i}" for i in range(0, 90, 2)]
    scores, pos = ix.search_arrays(q, 30, allowed_ids=allowed)
    want = M.mmr(sim, lambda d: d, pos, scores, 8, 0.4)
    lists, rel, mmr = ix.search_mmr(q, 8, 30, lam=0.4, allowed_ids=allowed)
    assert lists == [[db_ids[p] for p in row] for row in want[0]] and np.array_equal(M.bits(mmr), M.bits(want[2]))
    with pytest.raises(ValueError, match="not both"):
        ix.search_mmr(q, 8, 30, allowed_ids=allowed, allowed_mask=np.ones(90, bool))


def test_eval_dense_writes_the_diversified_run_beside_the_plain_one(golden_dir, tmp_path):
    from golden_weights import make_weights
    from test_eval_drivers import ROOT, _texts, _write_model
    sys.path.insert(0, ROOT)
    import eval_dense
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    rng = np.random.default_rng(3)
    lora = _write_model(str(tmp_path), cfg, w, rng)["dense"][0]
    docs, queries = _texts(rng, 60, 3, 20), _texts(rng, 6, 2, 6)
    docs[30:36] = docs[:6]                                          # near-duplicates in embedding space: exact ones
    (tmp_path / "corpus.tsv").write_text("".join(f"d{i}\t{t}\n" for i, t in enumerate(docs)))
    (tmp_path / "queries.tsv").write_text("".join(f"q{i}\t{t}\n" for i, t in enumerate(queries)))
    emb_dir, plain, div = (str(tmp_path / n) for n in ("embs", "out_plain", "out_mmr"))
    eval_dense.main(["--task_name", "write_doc_embeds", "--model_name_or_path", lora, "--corpus_path", str(tmp_path / "corpus.tsv"),
                     "--doc_embed_dir", emb_dir, "--eval_batch_size", "16", "--doc_max_length", "16", "--chunk_size", "32", "--token_budget", "0"])
    common = ["--task_name", "retrieval", "--model_name_or_path", lora, "--query_path", str(tmp_path / "queries.tsv"),
              "--doc_embed_dir", emb_dir, "--top_k", "10", "--query_max_length", "8"]
    eval_dense.main(common + ["--out_dir", plain])
    eval_dense.main(common + ["--out_dir", div, "--mmr_lambda", "0.3", "--mmr_fetch_k", "40"])
    assert open(os.path.join(div, "run.json"), "rb").read() == open(os.path.join(plain, "run.json"), "rb").read()
    assert not os.path.exists(os.path.join(plain, "mmr"))
    run = json.load(open(os.path.join(div, "mmr", "run.json")))
    stats = json.load(open(os.path.join(div, "mmr", "q_stats.json")))
    plain_run = json.load(open(os.path.join(plain, "run.json")))
    assert list(run) == list(plain_run) == list(stats)
    moved = 0
    for qid, hits in run.items():
        assert list(hits.values()) == [float(10 - t) for t in range(10)]          # the selection order, as a score every metric can sort by
        assert next(iter(hits)) == next(iter(plain_run[qid]))                       # pick 0 is the most relevant document
        outside = len(set(hits) - set(plain_run[qid]))
        assert stats[qid] == {"picks": 10, "mean_mmr": stats[qid]["mean_mmr"], "picks_outside_top_k": outside}
        moved += outside
    assert moved > 0
