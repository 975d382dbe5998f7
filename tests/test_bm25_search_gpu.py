"""GPU: Bm25Indexer / Bm25Retrieval / eval_bm25.py end to end on synthetic word lists through tests/fake_tokenizer.py.  The expected
results are the oracle's term-serial fp32 scorer (oracle/scoring.py) over the numpy model's weights (tests/bm25_cases.py) - ids and score
bits - and the float64 textbook BM25 within the derived bound."""
import json
import os

import numpy as np
import pytest
import torch

import bm25_cases as bc

pytestmark = pytest.mark.gpu

V = 512
K1, B_ = 0.9, 0.4


def _tok():
    from fake_tokenizer import FakeTokenizer
    return FakeTokenizer(vocab_size=V, padding_side="left")


def _loader(pairs, max_length, batch_size):
    from test_pipeline import ListDataset
    from torch.utils.data import DataLoader
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    return DataLoader(ListDataset(pairs), batch_size=batch_size, shuffle=False, collate_fn=LlamaSparseCollectionCollator(_tok(), max_length))


def model_index(doc_tokens, k1=K1, b=B_, lucene=False):
    """(indptr, doc_ids, weights, n_docs) of the numpy model over token lists: term-major, documents ascending inside a term."""
    n = len(doc_tokens)
    triples = sorted((t, d, c) for d, toks in enumerate(doc_tokens) for t, c in zip(*np.unique(toks, return_counts=True)))
    term = np.array([x[0] for x in triples], np.int64)
    doc_ids = np.array([x[1] for x in triples], np.int32)
    tf = np.array([x[2] for x in triples], np.float32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(term, minlength=V))]).astype(np.int64)
    doc_len = np.array([len(t) for t in doc_tokens], np.int32)
    avgdl = float(doc_len.astype(np.int64).sum()) / n
    w = bc.model_bm25_weights(indptr, doc_ids, tf, doc_len, bc.model_idf(np.diff(indptr), n), *bc.model_scalars(k1, b, avgdl, lucene))
    return indptr, doc_ids, w, n


def oracle_topk(index, query_tokens, k, query_tf=True, allowed=None):
    from oracle import scoring as oracle
    indptr, doc_ids, w, n = index
    cols, cnt = np.unique(np.asarray(query_tokens, np.int64), return_counts=True) if len(query_tokens) else (np.zeros(0, np.int64), np.zeros(0))
    qv = cnt.astype(np.float32) if query_tf else np.ones(len(cols), np.float32)
    pos, neg = oracle.numba_score_float(indptr, doc_ids, w, cols, qv, 0.0, n)
    if allowed is not None:
        keep = np.isin(pos, allowed)
        pos, neg = pos[keep], neg[keep]
    return oracle.select_topk(pos, neg, k)


def assert_run_equals_oracle(res, index, query_tokens, k, **kw):
    assert len(res.scores) == len(query_tokens)
    for r, q in enumerate(query_tokens):
        ids, scores = oracle_topk(index, q, k, **kw)
        n = int(res.counts[r])
        assert n == len(ids) and np.array_equal(res.positions[r][:n], ids), r
        assert np.array_equal(res.scores[r][:n].view(np.uint32), scores.astype(np.float32).view(np.uint32)), r


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """300 documents (one of them empty) indexed in memory and searched: the shared state of most tests."""
    from scaling_retriever_amd.bm25 import Bm25Indexer, Bm25Retrieval
    doc_pairs, query_pairs = bc.search_case()
    tok = _tok()
    skip = [tok.bos_token_id, tok.eos_token_id]
    index_d = Bm25Indexer(None, "cuda", dim_voc=V, skip_ids=skip, k1=K1, b=B_).index(_loader(doc_pairs, bc.DOC_MAX_LENGTH, 64))
    out = str(tmp_path_factory.mktemp("bm25_out"))
    ret = Bm25Retrieval({"out_dir": out}, dim_voc=V, device="cuda", index_d=index_d, compute_stats=True)
    docs = bc.token_lists(doc_pairs, tok, bc.DOC_MAX_LENGTH, set(skip))
    queries = bc.token_lists(query_pairs, tok, bc.QUERY_MAX_LENGTH, set(skip))
    return dict(doc_pairs=doc_pairs, query_pairs=query_pairs, docs=docs, queries=queries, ret=ret, out=out, index_d=index_d, skip=skip,
                model=model_index(docs), q_loader=lambda: _loader(query_pairs, bc.QUERY_MAX_LENGTH, 10))


def test_index_holds_the_term_frequencies(small):
    d = small["index_d"]
    stats = d["bm25_stats"]
    lens = [len(t) for t in small["docs"]]
    assert stats["n_docs"] == 300 and stats["total_len"] == sum(lens) and stats["avgdl"] == sum(lens) / 300 and stats["skip_ids"] == [1, 2]
    assert d["doc_len"].cpu().tolist() == lens and lens[bc.EMPTY_DOC] == 0
    assert len(d["ids_mapping"]) == 299 and bc.EMPTY_DOC not in d["ids_mapping"] and d["ids_mapping"][0] == "d0"
    ret = small["ret"]
    indptr, doc_ids, w, _ = small["model"]
    assert torch.equal(ret.hip_index.indptr.cpu(), torch.from_numpy(indptr)) and torch.equal(ret.hip_index.doc_ids.cpu(), torch.from_numpy(doc_ids))
    assert np.array_equal(ret.hip_index.vals.cpu().numpy().view(np.uint32), w.view(np.uint32))


def test_retrieve_equals_the_oracle_over_the_model_weights(small):
    """(a) 300 documents, top 10: ids and score bits; run.json holds what the result holds."""
    res = small["ret"].retrieve(small["q_loader"](), topk=10)
    assert_run_equals_oracle(res, small["model"], small["queries"], 10)
    run = json.load(open(os.path.join(small["out"], "run.json")))
    assert run == res.to_dict() and len(run) == len(small["queries"]) and all(len(v) == 10 for v in run.values())
    assert json.load(open(os.path.join(small["out"], "q_stats.json")))["L0_q"] == np.mean([len(set(q)) for q in small["queries"]])


def test_scores_and_ranking_against_float64(small):
    """(c) every returned score within bound x query terms of the textbook score; the ranking agrees wherever adjacent float64 scores differ
    by more than that, and at most 2 % of the adjacent pairs are excused (tests/test_bm25_host.py counts them on the reference alone)."""
    k = 10
    res = small["ret"].retrieve(small["q_loader"](), topk=k)
    pairs = excused = 0
    worst = 0.0
    for r, q in enumerate(small["queries"]):
        book = bc.textbook_scores(small["docs"], q, K1, B_)
        bound = bc.rel_bound(K1) * len(set(q))
        got_ids, got_sc = res.positions[r][:res.counts[r]], res.scores[r][:res.counts[r]].astype(np.float64)
        for d, s in zip(got_ids.tolist(), got_sc.tolist()):
            worst = max(worst, abs(s - book[d]) / book[d] / bound)
            assert abs(s - book[d]) <= bound * book[d], (r, d, s, book[d])
        want = sorted(book.items(), key=lambda x: (-x[1], x[0]))[:k + 1]
        for i in range(len(want) - 1):                                  # the pair (i, i + 1): a clear gap is a cut both rankings share
            pairs += 1
            if want[i][1] - want[i + 1][1] > bound * want[i][1]:
                assert set(got_ids[:i + 1].tolist()) == {d for d, _ in want[:i + 1]}, (r, i)
            else:
                excused += 1
    print(f"largest error {worst:.3f} of the bound; {excused} of {pairs} adjacent pairs excused")
    assert pairs >= 200 and excused <= 0.02 * pairs


def test_8300_documents_on_the_certified_scorer(monkeypatch):
    """(b) k = 8: 8 (k + 1 024) = 8 256 <= 8 300 documents, so the search hands the call to the certified scorer without a switch; its
    statistics say so.  The same bit equality.  The scorer's side structures are built by default only for collections of at least
    65 536 documents (csrc/sparse_cert_build.hip); the dev switch SR_SPARSE_CERT=1 builds them for this one, as the certified scorer's
    own tests do.  Under the same switch the search also skips its own n_docs >= 8 (k + 1 024) check (csrc/sparse_search.hip); at 8 300
    documents and k = 8 that check holds anyway, so here the switch decides what is built and nothing else.  The statistics must show
    that the scorer was given every query and certified more than half of them itself."""
    monkeypatch.setenv("SR_SPARSE_CERT", "1")
    from scaling_retriever_amd.bm25 import Bm25Indexer, Bm25Retrieval
    doc_pairs, query_pairs = bc.search_case(n_docs=8300, n_queries=16, seed=21)
    tok = _tok()
    skip = [tok.bos_token_id, tok.eos_token_id]
    index_d = Bm25Indexer(None, "cuda", dim_voc=V, skip_ids=skip).index(_loader(doc_pairs, bc.DOC_MAX_LENGTH, 1024))
    ret = Bm25Retrieval({"out_dir": "unused"}, dim_voc=V, device="cuda", index_d=index_d)
    q, qids = ret._generate_query_vecs(_loader(query_pairs, bc.QUERY_MAX_LENGTH, 16))
    before = ret.hip_index.cert_stats()
    res, _ = ret._sparse_retrieve_multithreaded(q, qids, topk=8)
    after = ret.hip_index.cert_stats()
    print("cert stats", before, after)
    assert after["present"] == 1 and after["queries"] - before["queries"] == len(qids) and after["searches"] - before["searches"] == 1
    assert 2 * (after["redone_exact"] - before["redone_exact"]) < len(qids)    # fewer than half handed back to the exact kernels
    assert after["batches_without_memory"] == before["batches_without_memory"]
    docs = bc.token_lists(doc_pairs, tok, bc.DOC_MAX_LENGTH, set(skip))
    assert_run_equals_oracle(res, model_index(docs), bc.token_lists(query_pairs, tok, bc.QUERY_MAX_LENGTH, set(skip)), 8)


def test_reweighting_a_stored_index(small, tmp_path):
    """(d) an index written to a directory and reopened with other (k1, b) equals a fresh build with those values; set_params too."""
    from scaling_retriever_amd.bm25 import Bm25Indexer, Bm25Retrieval
    index_dir, out = str(tmp_path / "index"), str(tmp_path / "out")
    Bm25Indexer(index_dir, "cuda", dim_voc=V, skip_ids=small["skip"], k1=K1, b=B_).index(_loader(small["doc_pairs"], bc.DOC_MAX_LENGTH, 64))
    stats = json.load(open(os.path.join(index_dir, "bm25_stats.json")))
    assert stats == small["index_d"]["bm25_stats"] and set(stats) == {"n_docs", "total_len", "avgdl", "k1", "b", "lucene", "skip_ids", "dim_voc"}
    assert np.load(os.path.join(index_dir, "doc_len.npy")).tolist() == [len(t) for t in small["docs"]]
    assert os.path.exists(os.path.join(index_dir, "doc_ids.pkl"))
    same = Bm25Retrieval({"index_dir": index_dir, "out_dir": out}, dim_voc=V, device="cuda")
    assert (same.k1, same.b, same.lucene, same.skip_ids) == (K1, B_, False, [1, 2])
    assert torch.equal(same.hip_index.vals, small["ret"].hip_index.vals) and torch.equal(same.hip_index.doc_ids, small["ret"].hip_index.doc_ids)
    k1, b = 1.6, 0.75
    fresh = model_index(small["docs"], k1, b)
    other = Bm25Retrieval({"index_dir": index_dir, "out_dir": out}, dim_voc=V, device="cuda", k1=k1, b=b)
    assert np.array_equal(other.hip_index.vals.cpu().numpy().view(np.uint32), fresh[2].view(np.uint32))
    assert_run_equals_oracle(other.retrieve(small["q_loader"](), topk=10), fresh, small["queries"], 10)
    same.set_params(k1, b)
    assert torch.equal(same.hip_index.vals, other.hip_index.vals)
    assert same.retrieve(small["q_loader"](), topk=10).to_dict() == other.retrieve(small["q_loader"](), topk=10).to_dict()
    same.set_params(K1, B_, lucene=True)
    assert np.array_equal(same.hip_index.vals.cpu().numpy().view(np.uint32), model_index(small["docs"], lucene=True)[2].view(np.uint32))


def test_query_weights(small):
    """(e) a repeated token weighs its count, query_tf=False weighs 1, a query of special tokens only has no entry, an unseen term adds
    nothing."""
    from scaling_retriever_amd.bm25 import Bm25Retrieval
    tok, ret = _tok(), small["ret"]
    seen = {t for d in small["docs"] for t in d}
    absent = next(w for w in (f"zz{i}" for i in range(1000)) if tok._encode(w, 8, True)[1] not in seen)
    pairs = [("rep", "w3 w3 w3 w11"), ("empty", ""), ("unseen", f"w3 w11 {absent}"), ("plain", "w3 w11")]
    toks = bc.token_lists(pairs, tok, bc.QUERY_MAX_LENGTH, set(small["skip"]))
    q, qids = ret._generate_query_vecs(_loader(pairs, bc.QUERY_MAX_LENGTH, 4))
    ptr, vals = q.row_ptr.cpu().tolist(), q.vals.cpu().tolist()
    assert qids == ["rep", "empty", "unseen", "plain"] and ptr == [0, 2, 2, 5, 7]
    assert sorted(vals[0:2]) == [1.0, 3.0] and vals[2:] == [1.0] * 5
    res = ret.retrieve(_loader(pairs, bc.QUERY_MAX_LENGTH, 4), topk=10)
    assert_run_equals_oracle(res, small["model"], toks, 10)
    run = json.load(open(os.path.join(small["out"], "run.json")))
    assert set(run) == {"rep", "unseen", "plain"} and run["unseen"] == run["plain"] and run["rep"] != run["plain"]
    binary = Bm25Retrieval({"out_dir": small["out"]}, dim_voc=V, device="cuda", index_d=small["index_d"], query_tf=False)
    qb, _ = binary._generate_query_vecs(_loader(pairs, bc.QUERY_MAX_LENGTH, 4))
    assert torch.equal(qb.cols, q.cols) and qb.vals.cpu().tolist() == [1.0] * 7
    res_b = binary.retrieve(_loader(pairs, bc.QUERY_MAX_LENGTH, 4), topk=10)
    assert_run_equals_oracle(res_b, small["model"], toks, 10, query_tf=False)
    assert res_b["rep"] == res_b["plain"]


def test_inherited_methods_work_on_a_bm25_index(small):
    """(f) retrieve_prf without feedback weight equals retrieve; allowed_ids and collapse agree with the filtered / collapsed full ranking."""
    ret, n = small["ret"], 300
    plain = ret.retrieve(small["q_loader"](), topk=10).to_dict()
    assert ret.retrieve_prf(small["q_loader"](), topk=10, alpha=1.0, beta=0.0, gamma=0.0, max_terms=0).to_dict() == plain
    allowed = [f"d{i}" for i in range(0, n, 3) if i != bc.EMPTY_DOC]
    res = ret.retrieve(small["q_loader"](), topk=10, allowed_ids=allowed)
    assert_run_equals_oracle(res, small["model"], small["queries"], 10, allowed=np.array([int(x[1:]) for x in allowed]))
    group_of = {f"d{i}": f"g{i // 5}" for i in range(n)}
    res = ret.retrieve(small["q_loader"](), topk=10, collapse=group_of).to_dict()
    for r, (qid, _) in enumerate(small["query_pairs"]):
        ids, scores = oracle_topk(small["model"], small["queries"][r], n)
        best = {}
        for d, s in zip(ids.tolist(), scores.tolist()):
            best.setdefault(f"g{d // 5}", float(s))                     # ranked best first: the first passage of a group is its best
        want = dict(sorted(best.items(), key=lambda x: -x[1])[:10])
        assert res[qid] == want, qid
    scored = ret.score_candidates(*ret._generate_query_vecs(small["q_loader"]()), [["d0", "d5", "d7"]] * len(small["queries"]))
    assert len(scored) == len(small["queries"])


def test_driver_writes_the_run_retrieve_produces(small, tmp_path, monkeypatch):
    """(g) eval_bm25.py indexing then retrieval on a TSV pair: run.json has the bytes of Bm25Retrieval.retrieve on the same index."""
    import eval_bm25
    import eval_sparse
    from scaling_retriever_amd.bm25 import Bm25Retrieval
    monkeypatch.setattr(eval_sparse, "_tokenizer", lambda path: _tok())
    corpus, queries = str(tmp_path / "corpus.tsv"), str(tmp_path / "queries.tsv")
    docs = [p for p in small["doc_pairs"] if p[1]]
    with open(corpus, "w") as f:
        f.writelines(f"{i}\t{t}\n" for i, t in docs)
    with open(queries, "w") as f:
        f.writelines(f"{i}\t{t}\n" for i, t in small["query_pairs"])
    index_dir, out = str(tmp_path / "index"), str(tmp_path / "out")
    eval_bm25.main(["--task_name", "indexing", "--tokenizer_path", "fake", "--corpus_path", corpus, "--index_dir", index_dir, "--tokenize_workers", "0",
                    "--doc_max_length", str(bc.DOC_MAX_LENGTH)])
    eval_bm25.main(["--task_name", "retrieval", "--tokenizer_path", "fake", "--query_path", queries, "--index_dir", index_dir, "--out_dir", out,
                    "--top_k", "10", "--query_max_length", str(bc.QUERY_MAX_LENGTH), "--bm25_k1", "1.2", "--prf_depth", "3"])
    ret = Bm25Retrieval({"index_dir": index_dir, "out_dir": str(tmp_path / "direct")}, dim_voc=V, device="cuda", k1=1.2)
    assert ret.bm25_stats["n_docs"] == 299 and ret.bm25_stats["dim_voc"] == V
    ret.retrieve(small["q_loader"](), topk=10)
    got = open(os.path.join(out, "run.json"), "rb").read()
    assert got == open(os.path.join(str(tmp_path / "direct"), "run.json"), "rb").read() and len(json.loads(got)) == len(small["query_pairs"])
    assert len(json.load(open(os.path.join(out, "prf", "run.json")))) == len(small["query_pairs"])
