"""GPU parity of pair scoring (csrc/pair_score.hip: sr_dense_score_pairs / sr_sparse_score_pairs) - the scores of GIVEN (query,
document) pairs read from the resident indexes, in place of the reference's re-encoding rerank_forward
(scaling_retriever/modeling/llm_encoder.py:593-615 behind eval_reranker.py).  Every comparison is for equal bits: dense against the
oracle's fmaf chain in the exact kernel's k order, sparse against the oracle's term-serial numba_score_float
(scaling_retriever/indexer.py:324-340), and both against the scores the searches return for the same pairs."""
import numpy as np
import pytest
import torch

from oracle import scoring as O

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- dense ---
N1, N2, BASE2, STRIDE2 = 12000, 8000, 20000, 3          # N = 20 000 in two segments, the second numbered 20000, 20003, ...


def _dense_index(rng, H):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    D = rng.standard_normal((N1 + N2, H), dtype=np.float32)
    idx = DenseIndexHIP(H)
    idx.add_host_rows(D[:N1])
    idx.add_host_rows(D[N1:], id_base=BASE2, id_stride=STRIDE2)
    gid = np.concatenate([np.arange(N1, dtype=np.int64), BASE2 + STRIDE2 * np.arange(N2, dtype=np.int64)])
    return idx, D, gid


def _row_of(gid):
    return np.where(gid < N1, gid, N1 + (gid - BASE2) // STRIDE2)


def _ragged_lists(rng, nq, gid):
    edge = np.array([gid[0], gid[N1 - 1], gid[N1], gid[-1]], np.int64)      # first and last row of each segment
    lists = []
    for q in range(nq):
        if q == 0:                       # beyond sr_max_topk, with the edges and repeats
            l = np.concatenate([edge, rng.choice(gid, 5000 - 8), edge])
        elif q == 1:
            l = np.zeros(0, np.int64)
        elif q == 2:
            l = gid[-1:].copy()
        else:
            n = int(rng.integers(0, 41))
            l = rng.choice(gid, n)
            if n >= 4:
                l[1] = l[0]              # a repeated document
                l[-1] = edge[q % 4]
        lists.append(l.astype(np.int64))
    indptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return lists, indptr, np.concatenate(lists)


@pytest.mark.parametrize("nq", [1, 64, 65, 300])
@pytest.mark.parametrize("H", [64, 256, 2048])
def test_dense_pairs_equal_the_exact_kernels_chain(H, nq):
    rng = np.random.default_rng(100 * H + nq)
    idx, D, gid = _dense_index(rng, H)
    Q = rng.standard_normal((nq, H), dtype=np.float32)
    lists, indptr, ids = _ragged_lists(rng, nq, gid)
    got = idx.score_pairs(torch.from_numpy(Q).cuda(), indptr, ids).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (len(ids),)
    ko = O.mfma_korder(H)
    for q, l in enumerate(lists):
        want = O.dense_scores_fma(Q[q:q + 1], D[_row_of(l)], ko)[0] if len(l) else np.zeros(0, np.float32)
        assert np.array_equal(_bits(got[indptr[q]:indptr[q + 1]]), _bits(want)), (H, nq, q)
    # an empty call and a call whose lists are all empty
    assert idx.score_pairs(torch.from_numpy(Q).cuda(), np.zeros(nq + 1, np.int64), np.zeros(0, np.int64)).numel() == 0


@pytest.mark.parametrize("mode", ["fp32", "fp32_filtered"])
def test_dense_pairs_give_back_the_searchs_scores(mode):
    rng = np.random.default_rng(7)
    H, nq, k = 256, 300, 100
    idx, D, gid = _dense_index(rng, H)
    idx.set_precision(mode)
    Q = torch.from_numpy(rng.standard_normal((nq, H), dtype=np.float32)).cuda()
    s, i = idx.search(Q, k)
    indptr = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * k
    got = idx.score_pairs(Q, indptr, i.reshape(-1))
    assert torch.equal(got.view(torch.int32), s.reshape(-1).view(torch.int32))


def test_dense_pairs_give_back_a_small_batch_invariant_searchs_scores():
    rng = np.random.default_rng(8)
    H, nq, k = 256, 8, 100
    idx, D, gid = _dense_index(rng, H)
    idx.set_batch_invariant(True)
    Q = torch.from_numpy(rng.standard_normal((nq, H), dtype=np.float32)).cuda()
    s, i = idx.search(Q, k)
    got = idx.score_pairs(Q, np.arange(nq + 1, dtype=np.int64) * k, i.reshape(-1))
    assert torch.equal(got.view(torch.int32), s.reshape(-1).view(torch.int32))


def test_dense_pairs_reject_an_id_outside_the_index():
    rng = np.random.default_rng(9)
    idx, D, gid = _dense_index(rng, 64)
    Q = torch.from_numpy(rng.standard_normal((3, 64), dtype=np.float32)).cuda()
    for bad in (BASE2 + 1, N1, -1, BASE2 + STRIDE2 * N2):         # between two strided ids, in the gap, negative, past the end
        ids = np.array([0, 5, bad, 7, gid[-1]], np.int64)
        with pytest.raises(ValueError, match=str(bad)):
            idx.score_pairs(Q, np.array([0, 2, 2, 5], np.int64), ids)
    with pytest.raises(ValueError):                                # offsets that do not cover the ids
        idx.score_pairs(Q, np.array([0, 2, 2, 4], np.int64), np.arange(5, dtype=np.int64))
    # the handle still works
    got = idx.score_pairs(Q, np.array([0, 1, 1, 2], np.int64), np.array([3, gid[-1]], np.int64)).cpu().numpy()
    want = [O.dense_scores_fma(Q[:1].cpu().numpy(), D[3:4], O.mfma_korder(64))[0, 0],
            O.dense_scores_fma(Q[2:3].cpu().numpy(), D[-1:], O.mfma_korder(64))[0, 0]]
    assert np.array_equal(_bits(got), _bits(np.array(want, np.float32)))


# ------------------------------------------------------------------------------------------------------ sparse ---
def _sparse_case(seed=11, V=4096, N=20000, long_doc=False):
    """Zipf index in the style of tests/test_sparse_cert_gpu.py; long_doc: document 17 gets a posting in 1 500 terms."""
    from test_sparse_cert_gpu import _zipf_index
    rng = np.random.default_rng(seed)
    indptr, ids, vals = _zipf_index(rng, V, N, 40)
    if long_doc:
        lists_i, lists_v = [], []
        add = set(rng.choice(V, 1500, replace=False).tolist())
        for t in range(V):
            di, dv = ids[indptr[t]:indptr[t + 1]], vals[indptr[t]:indptr[t + 1]]
            if t in add and 17 not in di:
                p = int(np.searchsorted(di, 17))
                di, dv = np.insert(di, p, 17), np.insert(dv, p, np.float32(0.5 + (t % 7)))
            lists_i.append(di)
            lists_v.append(dv)
        indptr = np.concatenate([[0], np.cumsum([len(x) for x in lists_i])]).astype(np.int64)
        ids, vals = np.concatenate(lists_i).astype(np.int32), np.concatenate(lists_v).astype(np.float32)
        assert int((ids == 17).sum()) > 1024
    w = 1.0 / np.arange(1, V + 1)
    w /= w.sum()
    queries = []
    for n in (1, 32, 200, 400):                                   # sorted, distinct terms
        c = np.sort(rng.choice(V, n, replace=False, p=w)).astype(np.int32)
        queries.append((c, np.log1p(rng.uniform(0, 20, n)).astype(np.float32)))
    c = rng.choice(V, 40, replace=False, p=w).astype(np.int32)     # unsorted, with repeated terms
    c = np.concatenate([c, c[:7], c[3:5]])
    queries.append((c, np.log1p(rng.uniform(0, 20, len(c))).astype(np.float32)))
    c = np.sort(rng.choice(V, 20, replace=False, p=w)).astype(np.int32)
    c[5] = -1                                                     # an unknown term: the library skips it
    queries.append((c, np.log1p(rng.uniform(0, 20, 20)).astype(np.float32)))
    return indptr, ids, vals, N, V, queries


def _sparse_check(idx, indptr, ids, vals, N, queries, rng):
    qi = np.concatenate([[0], np.cumsum([len(c) for c, _ in queries])]).astype(np.int64)
    qc, qv = np.concatenate([c for c, _ in queries]), np.concatenate([v for _, v in queries])
    k = 200
    s, i, cnt = idx.search(qi, qc, qv, k)
    i, cnt = i.cpu().numpy(), cnt.cpu().numpy()
    lists, full = [], []
    for q, (c, v) in enumerate(queries):
        keep = c >= 0                                             # dropped before the oracle, which would index with it
        scores = np.zeros(N, np.float32)
        hit, neg = O.numba_score_float(indptr, ids, vals, c[keep], v[keep], -1.0, N)
        scores[hit] = -neg
        full.append(scores)
        none = np.flatnonzero(scores == 0)[:25]                   # documents that share no term with the query
        hits = i[q, :cnt[q]]
        l = np.concatenate([hits, none, hits[:9], [17, 0, N - 1]]).astype(np.int64)
        lists.append(l if q != 1 else np.concatenate([l, rng.integers(0, N, 3000)]))
    ci = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    got = idx.score_pairs(qi, qc, qv, ci, np.concatenate(lists)).cpu().numpy()
    for q, l in enumerate(lists):
        assert np.array_equal(_bits(got[ci[q]:ci[q + 1]]), _bits(full[q][l])), q
        assert len(none) == 0 or (got[ci[q]:ci[q + 1]][cnt[q]:cnt[q] + len(none)] == 0).all()
    return got


@pytest.mark.parametrize("long_doc", [False, True])
def test_sparse_pairs_equal_the_term_serial_chain_on_both_routes(monkeypatch, long_doc):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    monkeypatch.setenv("SR_SPARSE_CERT", "1")        # build the certified scorer (and its forward index) at this size as well
    indptr, ids, vals, N, V, queries = _sparse_case(long_doc=long_doc)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    # a document of more than 1 024 postings keeps the index from having a forward index: the posting lists serve it
    assert idx.cert_stats()["present"] == (0 if long_doc else 1)
    a = _sparse_check(idx, indptr, ids, vals, N, queries, np.random.default_rng(1))
    # long_doc = False: the first run took the forward route for the queries with ascending valid terms, this one the posting lists
    # for all of them - the two-route comparison.  long_doc = True: both runs are the posting-list route (there is no other).
    monkeypatch.setenv("SR_PAIR_SPARSE_ROUTE", "postings")
    b = _sparse_check(idx, indptr, ids, vals, N, queries, np.random.default_rng(1))
    assert np.array_equal(_bits(a), _bits(b))


def test_sparse_pairs_on_an_index_without_the_certified_scorer(monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    # Whether an index has the certified scorer (and with it the forward index) is decided inside sr_sparse_index_create from the
    # index's content and the free device memory; the workspace limit plays no part in it.  The public switch builds an index
    # without it; the 1 MiB limit below only makes the search that supplies the candidates run in its smallest doc tiles.
    monkeypatch.setenv("SR_SPARSE_SCORER", "exact")
    indptr, ids, vals, N, V, queries = _sparse_case()
    idx = SparseIndexHIP(indptr, ids, vals, N)
    idx.set_workspace_limit(1 << 20)
    assert idx.cert_stats()["present"] == 0
    _sparse_check(idx, indptr, ids, vals, N, queries, np.random.default_rng(1))


def test_sparse_pairs_give_back_the_searchs_scores_and_reject_unknown_documents():
    from scaling_retriever_amd.scoring import SparseIndexHIP
    from test_sparse_cert_gpu import _zipf_queries
    indptr, ids, vals, N, V, _ = _sparse_case(seed=12)
    idx = SparseIndexHIP(indptr, ids, vals, N)
    qi, qc, qv = _zipf_queries(np.random.default_rng(13), V, 70, 32)
    s, i, cnt = idx.search(qi, qc, qv, 1000)
    valid = torch.arange(1000, device="cuda")[None, :] < cnt[:, None]          # rows end in padding where fewer than k docs score > 0
    assert int(cnt.max()) == 1000
    ci = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(cnt.to(torch.int64), 0)])
    got = idx.score_pairs(qi, qc, qv, ci, i[valid])
    assert torch.equal(got.view(torch.int32), s[valid].view(torch.int32))
    for bad in (N, -1):
        with pytest.raises(ValueError, match=str(bad)):
            idx.score_pairs(qi[:2], qc, qv, np.array([0, 3], np.int64), np.array([1, bad, 2], np.int64))


# -------------------------------------------------------------------------------------------------- end to end ---
def test_retrieve_fused_writes_the_union_ranked_by_both_heads(golden_dir, tmp_path):
    import json
    import os
    from fake_tokenizer import FakeTokenizer
    from golden_weights import make_weights
    from torch.utils.data import DataLoader
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    from scaling_retriever_amd.indexer import HybridIndexer, HybridRetriever
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiHybrid
    from test_pipeline import ListDataset, _corpus
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    tok = FakeTokenizer(vocab_size=cfg["vocab_size"], padding_side="left")
    docs, queries = ListDataset(_corpus(90, seed=1, max_words=20)), ListDataset([(f"q{i}", t) for i, (_, t) in enumerate(_corpus(8, seed=2, max_words=6))])
    collate_d, collate_q = LlamaSparseCollectionCollator(tok, 24), LlamaSparseCollectionCollator(tok, 8)
    loader = lambda: DataLoader(docs, batch_size=16, shuffle=False, collate_fn=collate_d)      # noqa: E731
    q_loader = lambda: DataLoader(queries, batch_size=4, shuffle=False, collate_fn=collate_q)  # noqa: E731
    hyb = LlamaBiHybrid.from_weights(cfg, w).to("cuda").eval()
    sp_dir, de_dir = str(tmp_path / "sp"), str(tmp_path / "de")
    HybridIndexer(hyb, sp_dir, de_dir, device="cuda", chunk_size=40, compute_stats=True, dim_voc=hyb.vocab_size).index(loader())
    out_a, out_b = str(tmp_path / "a"), str(tmp_path / "b")
    HybridRetriever(hyb, sp_dir, de_dir, out_a, dim_voc=hyb.vocab_size, device="cuda").retrieve(q_loader(), topk=10)
    ret = HybridRetriever(hyb, sp_dir, de_dir, out_b, dim_voc=hyb.vocab_size, device="cuda")
    weights = (0.7, 1.3)
    sparse_res, dense_res, fused_res = ret.retrieve_fused(q_loader(), topk=10, weights=weights)
    for head in ("sparse", "dense"):                                  # the two existing runs: the same bytes
        assert open(os.path.join(out_a, head, "run.json"), "rb").read() == open(os.path.join(out_b, head, "run.json"), "rb").read()
    fused = json.load(open(os.path.join(out_b, "fused", "run.json")))
    assert fused == {q: dict(r) for q, r in fused_res.items()}
    # the same in numpy from the two heads' score_candidates over the union of the two runs
    sparse_q, dense_q, qids = ret._generate_query_vecs(q_loader())
    union = [sorted(set(sparse_res[q]) | set(dense_res[q])) if q in sparse_res else sorted(dense_res[q]) for q in qids]
    by_sparse = ret.score_candidates(sparse_q, qids, union)
    by_dense = ret.dense_index.score_candidates(dense_q, union, qids)
    spos = ret.inverse_id_map()
    for q, ids_ in zip(qids, union):
        d = np.array([by_dense[q][i] for i in ids_], np.float32)
        s = np.array([by_sparse[q][i] for i in ids_], np.float32)
        f = (np.float32(weights[0]) * d).astype(np.float32) + (np.float32(weights[1]) * s).astype(np.float32)
        order = np.lexsort((np.array([spos.get(i) for i in ids_]), -f.astype(np.float64)))[:10]
        assert list(fused[q].keys()) == [ids_[o] for o in order], q
        assert np.array_equal(np.array(list(fused[q].values()), np.float32), f[order]), q
        assert len(ids_) > 10                                          # the union is wider than either list
    with pytest.raises(KeyError, match="no-such-doc"):
        ret.dense_index.score_candidates(dense_q, [["no-such-doc"]] + [[]] * 7, qids)


def test_eval_rerank_driver_end_to_end(golden_dir, tmp_path):
    import json
    import os
    import sys
    from golden_weights import make_weights
    from test_eval_drivers import ROOT, _texts, _write_model
    sys.path.insert(0, ROOT)
    import eval_dense
    import eval_rerank
    import eval_sparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    rng = np.random.default_rng(3)
    models = _write_model(str(tmp_path), cfg, w, rng)
    docs, queries = _texts(rng, 60, 3, 20), _texts(rng, 70, 2, 6)         # 70 queries: the dense search runs the tiled kernels' k order
    (tmp_path / "corpus.tsv").write_text("".join(f"d{i}\t{t}\n" for i, t in enumerate(docs)))
    (tmp_path / "queries.tsv").write_text("".join(f"q{i}\t{t}\n" for i, t in enumerate(queries)))
    lora_d, lora_s = models["dense"][0], models["sparse"][0]
    emb_dir, out_d, idx_dir, out_s = (str(tmp_path / n) for n in ("embs", "out_dense", "sp_index", "out_sparse"))
    eval_dense.main(["--task_name", "write_doc_embeds", "--model_name_or_path", lora_d, "--corpus_path", str(tmp_path / "corpus.tsv"),
                     "--doc_embed_dir", emb_dir, "--eval_batch_size", "16", "--doc_max_length", "16", "--chunk_size", "32", "--token_budget", "0"])
    eval_dense.main(["--task_name", "retrieval", "--model_name_or_path", lora_d, "--query_path", str(tmp_path / "queries.tsv"),
                     "--doc_embed_dir", emb_dir, "--out_dir", out_d, "--top_k", "10", "--query_max_length", "8"])
    eval_sparse.main(["--task_name", "indexing", "--model_name_or_path", lora_s, "--corpus_path", str(tmp_path / "corpus.tsv"),
                      "--index_dir", idx_dir, "--eval_batch_size", "8", "--doc_max_length", "16", "--token_budget", "0"])
    eval_sparse.main(["--task_name", "retrieval", "--model_name_or_path", lora_s, "--query_path", str(tmp_path / "queries.tsv"),
                      "--index_dir", idx_dir, "--out_dir", out_s, "--top_k", "10", "--query_max_length", "8", "--eval_batch_size", "128"])
    run_d = json.load(open(os.path.join(out_d, "run.json")))
    run_s = json.load(open(os.path.join(out_s, "run.json")))
    # the sparse run re-scored by the dense model: for documents that are also in the dense run, exactly the dense run's scores
    rr = str(tmp_path / "rr_dense")
    eval_rerank.main(["--rerank_type", "dense_encoder", "--model_name_or_path", lora_d, "--query_path", str(tmp_path / "queries.tsv"),
                      "--run_path", os.path.join(out_s, "run.json"), "--index_dir", emb_dir, "--output_dir", rr, "--query_max_length", "8"])
    got = json.load(open(os.path.join(rr, "run.json")))
    assert list(got) == list(run_s)
    common = 0
    for q in run_s:
        assert set(got[q]) == set(run_s[q])
        vals = list(got[q].values())
        assert vals == sorted(vals, reverse=True)
        for d in set(got[q]) & set(run_d[q]):
            assert got[q][d] == run_d[q][d], (q, d)
            common += 1
    assert common > 50
    # the dense run re-scored by the sparse model, candidates given as jsonl: the sparse run's scores where the two overlap
    with open(tmp_path / "c.jsonl", "w") as f:
        for q in run_d:
            f.write(json.dumps({"qid": q, "docids": list(run_d[q])}) + "\n")
    rs = str(tmp_path / "rr_sparse")
    eval_rerank.main(["--rerank_type", "splade", "--model_name_or_path", lora_s, "--query_path", str(tmp_path / "queries.tsv"),
                      "--jsonl_path", str(tmp_path / "c.jsonl"), "--index_dir", idx_dir, "--output_dir", rs, "--query_max_length", "8",
                      "--eval_batch_size", "128"])       # the retrieval's batches: a bf16-regime query vector depends on its batch's padding
    got_s = json.load(open(os.path.join(rs, "run.json")))
    common = 0
    for q in run_d:
        assert set(got_s[q]) == set(run_d[q])
        for d in set(got_s[q]) & set(run_s.get(q, {})):
            assert got_s[q][d] == run_s[q][d], (q, d)
            common += 1
    assert common > 50
    # hybrid mode: the fused run of retrieve_fused, given back as candidates, is re-scored to the same fused scores in the same order
    from torch.utils.data import DataLoader
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    from scaling_retriever_amd.dataset.dataset import CollectionDataset, MSMARCOQueryDataset
    from scaling_retriever_amd.indexer import HybridIndexer, HybridRetriever
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiHybrid
    tok = eval_sparse._tokenizer(lora_s)
    tok.padding_side = "left"
    hyb = LlamaBiHybrid.load_from_lora(lora_s).to("cuda").eval()
    h_sp, h_de, h_out = (str(tmp_path / n) for n in ("h_sp", "h_de", "h_out"))
    d_loader = DataLoader(CollectionDataset(str(tmp_path / "corpus.tsv"), data_source="msmarco"), batch_size=16, shuffle=False,
                          collate_fn=LlamaSparseCollectionCollator(tok, 16))
    HybridIndexer(hyb, h_sp, h_de, device="cuda", chunk_size=32, compute_stats=True, dim_voc=hyb.vocab_size).index(d_loader)
    q_loader = DataLoader(MSMARCOQueryDataset(str(tmp_path / "queries.tsv")), batch_size=128, shuffle=False,
                          collate_fn=LlamaSparseCollectionCollator(tok, 8))
    HybridRetriever(hyb, h_sp, h_de, h_out, dim_voc=hyb.vocab_size, device="cuda").retrieve_fused(q_loader, topk=10, weights=(0.5, 2.0))
    fused_path = os.path.join(h_out, "fused", "run.json")
    rh = str(tmp_path / "rr_hybrid")
    eval_rerank.main(["--rerank_type", "hybrid", "--model_name_or_path", lora_s, "--query_path", str(tmp_path / "queries.tsv"),
                      "--run_path", fused_path, "--sparse_index_dir", h_sp, "--dense_index_dir", h_de, "--output_dir", rh,
                      "--query_max_length", "8", "--eval_batch_size", "128", "--weights", "0.5,2.0"])
    fused, got_h = json.load(open(fused_path)), json.load(open(os.path.join(rh, "run.json")))
    assert len(fused) == 70 and got_h == fused
    assert all(list(got_h[q]) == list(fused[q]) for q in fused)
