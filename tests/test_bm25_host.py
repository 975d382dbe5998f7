"""CPU: the BM25 models against a hand-computed example and against float64 within the derived bound (tests/bm25_cases.py), the host
formulas' edge values, the argument checks sr_token_counts / sr_bm25_weights make before any device call, the world-size guard, the
driver's argument parsing, and the near-tie census the GPU ranking test relies on."""
import ctypes
import math

import numpy as np
import pytest

import bm25_cases as bc


def test_models_on_a_hand_computed_example():
    """Three documents over the terms 5, 7, 9 (id 1 = BOS is skipped, the last slot of row 1 is padding):
         d0 = 5 5 7      d1 = 7 9      d2 = 5
       N = 3, lengths 3, 2, 1, avgdl = 2; df(5) = 2, df(7) = 2, df(9) = 1; k1 = 1, b = 0.5:
         idf(5) = idf(7) = log1p(1.5 / 2.5) = log(1.6),   idf(9) = log1p(2.5 / 1.5) = log(8 / 3)
         K(d) = 1 (0.5 + 0.5 |d| / 2):  K(d0) = 1.25, K(d1) = 1, K(d2) = 0.75
         w(5, d0) = log(1.6) . 2 . 2 / (2 + 1.25),  w(7, d0) = log(1.6) . 2 / 2.25,  w(7, d1) = log(1.6) . 2 / 2,  w(9, d1) = log(8/3) . 2 / 2,
         w(5, d2) = log(1.6) . 2 / 1.75."""
    ids = np.array([[1, 5, 5, 7], [1, 7, 9, 2], [2, 2, 1, 5]])
    mask = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [0, 0, 1, 1]])
    row_ptr, cols, vals, lens = bc.model_token_counts(ids, mask, skip_ids=(1, 2), n_terms=10)
    assert row_ptr.tolist() == [0, 2, 4, 5] and cols.tolist() == [5, 7, 7, 9, 5] and vals.tolist() == [2, 1, 1, 1, 1] and lens.tolist() == [3, 2, 1]
    # term-major: 5 -> (d0, 2), (d2, 1); 7 -> (d0, 1), (d1, 1); 9 -> (d1, 1)
    indptr = np.array([0, 0, 0, 0, 0, 0, 2, 2, 4, 4, 5])
    doc_ids, tf = np.array([0, 2, 0, 1, 1], np.int32), np.array([2, 1, 1, 1, 1], np.float32)
    numer, a, s = bc.model_scalars(1.0, 0.5, 2.0)
    assert (float(numer), float(a), float(s)) == (2.0, 0.5, 0.25)
    idf = bc.model_idf(np.diff(indptr), 3)
    w = bc.model_bm25_weights(indptr, doc_ids, tf, lens, idf, numer, a, s)
    l16, l83 = math.log(1.6), math.log(8.0 / 3.0)
    want = [l16 * 4 / 3.25, l16 * 2 / 1.75, l16 * 2 / 2.25, l16 * 2 / 2, l83 * 2 / 2]
    assert np.allclose(w, want, rtol=bc.rel_bound(1.0), atol=0)
    real = bc.real_weights(indptr, doc_ids, tf, lens, 3, 1.0, 0.5, 2.0)
    assert np.allclose(real, want, rtol=1e-15, atol=0)
    docs = [[5, 5, 7], [7, 9], [5]]
    book = bc.textbook_scores(docs, [5, 9, 9], 1.0, 0.5)
    assert book.keys() == {0, 1, 2}
    assert math.isclose(book[0], want[0], rel_tol=1e-15) and math.isclose(book[1], 2 * want[4], rel_tol=1e-15)
    assert math.isclose(book[2], want[1], rel_tol=1e-15)
    with pytest.raises(ValueError, match="row 1, position 2, id 10"):
        bc.model_token_counts(np.array([[1, 3, 4], [1, 4, 10]]), None, (1,), 10)


@pytest.mark.parametrize("k1,b,lucene", [(0.9, 0.4, False), (1.2, 0.75, False), (0.9, 0.4, True), (2.0, 1.0, False), (0.9, 0.0, False), (0.0, 0.5, False)])
def test_fp32_model_is_within_the_derived_bound_of_float64(k1, b, lucene):
    rng = np.random.default_rng(11)
    n_docs, n_terms, nnz = 20000, 3000, 200000
    indptr, doc_ids, tf, doc_len = bc.random_postings(rng, n_terms, n_docs, nnz)
    avgdl = float(doc_len.astype(np.int64).sum()) / n_docs
    numer, a, s = bc.model_scalars(k1, b, avgdl, lucene)
    w = bc.model_bm25_weights(indptr, doc_ids, tf, doc_len, bc.model_idf(np.diff(indptr), n_docs), numer, a, s)
    real = bc.real_weights(indptr, doc_ids, tf, doc_len, n_docs, k1, b, avgdl, lucene)
    rel = np.abs(w.astype(np.float64) - real) / real
    print(f"k1 {k1} b {b} lucene {lucene}: largest relative error {rel.max() / bc.U:.2f} u, bound {bc.rel_bound(k1) / bc.U:.2f} u")
    assert rel.max() <= bc.rel_bound(k1)
    assert rel.max() > 0.5 * bc.U or k1 == 0.0            # the comparison is not vacuous: roundings do show


def test_host_formulas_match_the_models_and_their_edge_values():
    from scaling_retriever_amd import bm25
    for k1, b, avgdl, lucene in [(0.9, 0.4, 56.3, False), (1.2, 0.75, 1.0, True), (0.9, 0.0, 7.5, False), (0.9, 1.0, 7.5, False), (0.9, 0.4, 0.0, False),
                                 (0.0, 0.4, 3.0, False)]:
        got = bm25.bm25_scalars(k1, b, avgdl, lucene)
        want = bc.model_scalars(k1, b, avgdl, lucene)
        assert got == tuple(float(x) for x in want), (k1, b, avgdl, lucene)
        assert all(np.float32(x) == x for x in got)                 # fp32 values
    assert bm25.bm25_scalars(0.9, 0.0, 7.5)[2] == 0.0                # b = 0: no length term, a = k1
    assert bm25.bm25_scalars(0.9, 0.0, 7.5)[1] == float(np.float32(0.9))
    assert bm25.bm25_scalars(0.9, 1.0, 7.5)[1] == 0.0                # b = 1: a = 0
    assert bm25.bm25_scalars(0.9, 0.4, 0.0)[2] == 0.0                # avgdl = 0: s = 0, no division
    assert bm25.bm25_scalars(0.9, 0.4, 5.0, lucene=True)[0] == 1.0
    for bad in [(-1.0, 0.4), (0.9, 1.5), (0.9, -0.1), (float("nan"), 0.4)]:
        with pytest.raises(ValueError):
            bm25.bm25_scalars(*bad, 1.0)
    N = 1000
    df = np.array([0, 1, 2, N // 2, N - 1, N])
    idf = bm25.idf_table(df, N)
    assert idf.dtype == np.float32 and np.array_equal(idf, bc.model_idf(df, N))
    assert np.all(idf > 0) and np.all(np.diff(idf) < 0)              # positive at df = N, decreasing in df
    assert idf[-1] == np.float32(math.log1p(0.5 / (N + 0.5))) and idf[1] == np.float32(math.log1p((N - 0.5) / 1.5))
    assert bm25.average_length(7, 2) == 3.5 and bm25.average_length(0, 0) == 0.0


def test_argument_errors_before_any_device_call():
    """Every SR_ERR_INVALID sr_token_counts / sr_bm25_weights promise before a device call; the device pointers are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    skip = (ctypes.c_int32 * 16)(*range(16))
    n = ctypes.c_int64(-7)
    max_len = lib.sr_token_counts_max_len()
    assert max_len == 8192

    def tc(**kw):
        a = dict(dict(ids=p, mask=p, B=4, L=16, skip=skip, n_skip=2, n_terms=100, row_ptr=p, cols=p, vals=p, len=p, cap=64, n=ctypes.byref(n)), **kw)
        return lib.sr_token_counts(a["ids"], a["mask"], a["B"], a["L"], a["skip"], a["n_skip"], a["n_terms"], a["row_ptr"], a["cols"], a["vals"],
                                   a["len"], a["cap"], a["n"], None)
    for change, text in [(dict(L=max_len + 1), b"at most 8192"), (dict(n_skip=17), b"n_skip = 17"), (dict(n_skip=-1), b"n_skip = -1"),
                         (dict(n_skip=1, skip=None), b"n_skip = 1"), (dict(n_terms=0), b"outside [1, 2^31)"), (dict(n_terms=1 << 31), b"outside [1, 2^31)"),
                         (dict(n_terms=-5), b"outside [1, 2^31)"), (dict(B=-1), b"bad sizes"), (dict(B=1 << 24), b"at most 2^24 - 1"), (dict(L=-1), b"bad sizes"), (dict(cap=-1), b"bad sizes"),
                         (dict(ids=None), b"null pointer"), (dict(row_ptr=None), b"null pointer"), (dict(len=None), b"null pointer"),
                         (dict(n=None), b"null pointer")]:
        rc = tc(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert n.value == -7
    with pytest.raises(ValueError):
        _lib.check(tc(L=max_len + 1), "sr_token_counts")

    def bw(**kw):
        a = dict(dict(indptr=p, ids=p, tf=p, n_terms=10, nnz=5, dl=p, n_docs=3, idf=p, out=p), **kw)
        return lib.sr_bm25_weights(a["indptr"], a["ids"], a["tf"], a["n_terms"], a["nnz"], a["dl"], a["n_docs"], a["idf"], 1.9, 0.5, 0.01, a["out"], None)
    for change, text in [(dict(nnz=-1), b"bad sizes"), (dict(n_terms=-1), b"bad sizes"), (dict(n_docs=-1), b"bad sizes"), (dict(n_docs=1 << 31), b"bad sizes"),
                         (dict(n_terms=1 << 31), b"bad sizes"), (dict(indptr=None), b"null pointer"), (dict(ids=None), b"null pointer"),
                         (dict(tf=None), b"null pointer"), (dict(dl=None), b"null pointer"), (dict(idf=None), b"null pointer"),
                         (dict(out=None), b"null pointer"), (dict(n_terms=0), b"null pointer")]:
        rc = bw(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert bw(nnz=0) == _lib.SR_OK and bw(nnz=0, indptr=None, ids=None, tf=None, out=None) == _lib.SR_OK


def test_world_size_two_is_not_implemented(monkeypatch, tmp_path):
    from scaling_retriever_amd import bm25
    monkeypatch.setattr(bm25, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="collection"):
        bm25.Bm25Indexer(str(tmp_path / "i"), "cuda", dim_voc=64, skip_ids=(1, 2))
    with pytest.raises(NotImplementedError, match="collection"):
        bm25.Bm25Retrieval({"index_dir": str(tmp_path / "i"), "out_dir": str(tmp_path / "o")}, dim_voc=64, device="cuda")


def test_driver_argument_parsing():
    import eval_bm25
    a = eval_bm25.parse_args(["--task_name", "retrieval", "--tokenizer_path", "t", "--index_dir", "i", "--out_dir", "o", "--query_path", "q",
                              "--bm25_k1", "1.2", "--bm25_b", "0.75", "--top_k", "1000", "--prf_depth", "10", "--device_eval",
                              "--eval_qrel_path", "qrels.json", "--eval_metric", "['mrr_10']", "--allowed_ids_file", "ids.txt"])
    assert (a.bm25_k1, a.bm25_b, a.bm25_lucene, a.top_k, a.prf_depth, a.device_eval, a.eval_metric) == (1.2, 0.75, False, 1000, 10, True, ["mrr_10"])
    assert a.allowed_ids_file == "ids.txt" and a.collapse_file is None and a.token_budget == 16384
    a = eval_bm25.parse_args(["--task_name", "indexing", "--tokenizer_path", "t", "--corpus_path", "c", "--index_dir", "i", "--bm25_lucene",
                              "--token_budget", "0"])
    assert a.bm25_k1 is None and a.bm25_b is None and a.bm25_lucene and a.token_budget == 0
    for bad in [["--task_name", "indexing"], ["--task_name", "train", "--tokenizer_path", "t"],
                ["--task_name", "retrieval", "--tokenizer_path", "t", "--bm25_b", "1.5"],
                ["--task_name", "retrieval", "--tokenizer_path", "t", "--bm25_k1", "-1"],
                ["--task_name", "retrieval", "--tokenizer_path", "t", "--prf_gamma", "0.5"],
                ["--task_name", "retrieval", "--tokenizer_path", "t", "--prf_depth", "65"],
                ["--task_name", "retrieval", "--tokenizer_path", "t", "--prf_depth", "5", "--collapse_file", "c.tsv"],
                ["--task_name", "retrieval", "--tokenizer_path", "t", "--collapse_hits", "3"]]:
        with pytest.raises(SystemExit):
            eval_bm25.parse_args(bad)

    class Tok:
        vocab_size, bos_token_id, eos_token_id, pad_token_id = 500, 1, 2, 2

        def __len__(self):
            return 512
    assert eval_bm25.term_space(Tok(), a) == (512, [1, 2])


def search_corpus():
    """The corpus, queries and parameters of tests/test_bm25_search_gpu.py's ranking test, with their float64 scores."""
    from fake_tokenizer import FakeTokenizer
    tok = FakeTokenizer(vocab_size=512)
    skip = {tok.bos_token_id, tok.eos_token_id}
    doc_pairs, query_pairs = bc.search_case()
    docs = bc.token_lists(doc_pairs, tok, bc.DOC_MAX_LENGTH, skip)
    queries = bc.token_lists(query_pairs, tok, bc.QUERY_MAX_LENGTH, skip)
    return docs, queries, [bc.textbook_scores(docs, q, 0.9, 0.4) for q in queries]


def test_near_ties_are_rare_on_the_search_test_corpus():
    """The GPU ranking test excuses adjacent pairs of the float64 ranking closer than bound x query terms; on its corpus fewer than 2 % of
    the adjacent pairs of the top 11 are that close, so the excuse cannot hide a wrong ranking."""
    docs, queries, scores = search_corpus()
    pairs, close = bc.near_tie_census(scores, 10, lambda q: bc.rel_bound(0.9) * len(set(queries[q])))
    print(f"{pairs} adjacent pairs, {close} closer than the bound")
    assert pairs >= 200 and close < 0.02 * pairs
