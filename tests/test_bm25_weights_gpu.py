"""GPU: sr_bm25_weights (csrc/bm25_weights.hip) against the numpy model of tests/bm25_cases.py, bit for bit, and against the float64
formula within the derived bound.  nnz 0, 1, 255, 256, 257, 5 000 and one above a single grid pass (the grid is capped at 8 workgroups
of 256 postings per compute unit, 256 CUs x 8 x 256 = 524 288 postings: the case uses 700 000); empty posting lists at the front, in the
middle and at the end of indptr; a term with df = N; tf and doc_len from 1 to 8 192; in place and out of place; lucene on and off; b in
0, 0.4, 1."""
import numpy as np
import pytest
import torch

import bm25_cases as bc

pytestmark = pytest.mark.gpu


def make_case(nnz, n_docs, n_terms, seed, full_term=False):
    """Term-major CSR with empty lists at the front (terms 0, 1), in the middle and at the end (the last 3 terms); full_term: term 2 holds
    every document once."""
    rng = np.random.default_rng(seed)
    doc_len = rng.integers(1, 8193, n_docs).astype(np.int32)
    doc_len[:2] = (1, 8192)
    n_full = n_docs if full_term and nnz >= n_docs else 0
    live = np.setdiff1d(np.arange(3, n_terms - 3), [n_terms // 2, n_terms // 2 + 1])
    term = np.sort(rng.choice(live, nnz - n_full)) if nnz - n_full else np.zeros(0, np.int64)
    counts = np.bincount(term, minlength=n_terms)
    counts[2] = n_full
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    doc_ids = np.concatenate([np.arange(n_full), rng.integers(0, n_docs, nnz - n_full)]).astype(np.int32)
    tf = rng.integers(1, 8193, nnz).astype(np.float32)
    if nnz >= 2:
        tf[:2] = (1, 8192)
        doc_ids[-2:] = (0, 1)
    return indptr, doc_ids, tf, doc_len


def run_case(case, n_docs, k1, b, lucene, in_place):
    from scaling_retriever_amd import bm25
    from scaling_retriever_amd.scoring import bm25_weights
    indptr, doc_ids, tf, doc_len = case
    avgdl = bm25.average_length(doc_len.astype(np.int64).sum(), n_docs)
    numer, a, s = bm25.bm25_scalars(k1, b, avgdl, lucene)
    idf = bm25.idf_table(np.diff(indptr), n_docs)
    want = bc.model_bm25_weights(indptr, doc_ids, tf, doc_len, idf, *bc.model_scalars(k1, b, avgdl, lucene))
    dev = [torch.from_numpy(x).cuda() for x in (indptr, doc_ids, tf, doc_len, idf)]
    steps = bm25.bm25_weights_by_steps(*dev, numer, a, s)
    got = bm25_weights(*dev, numer, a, s, out=dev[2] if in_place else None)
    assert got is dev[2] if in_place else got is not dev[2]
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (len(tf), k1, b, lucene)
    assert torch.equal(steps, got)
    if len(tf):
        real = bc.real_weights(indptr, doc_ids, tf, doc_len, n_docs, k1, b, avgdl, lucene)
        rel = np.abs(got.cpu().numpy().astype(np.float64) - real) / real
        assert rel.max() <= bc.rel_bound(k1), (rel.max() / bc.U, bc.rel_bound(k1) / bc.U)
        return rel.max()
    return 0.0


@pytest.mark.parametrize("nnz", [0, 1, 255, 256, 257, 5000])
def test_weights_equal_the_model_bit_for_bit(nnz):
    n_docs = 900
    case = make_case(nnz, n_docs, 64, seed=nnz + 1, full_term=True)
    for i, (k1, b, lucene) in enumerate([(0.9, 0.4, False), (0.9, 0.4, True), (1.2, 0.0, False), (2.0, 1.0, False), (0.9, 1.0, True)]):
        run_case(case, n_docs, k1, b, lucene, in_place=bool(i % 2))
    if nnz == 5000:
        df = np.diff(case[0])
        assert df[2] == n_docs and df[0] == df[1] == 0 and df[32] == 0 and not df[-3:].any()       # df = N, and the empty lists


def test_more_postings_than_one_grid_pass():
    """700 000 postings: a wave's run of postings is longer than one piece, the carried term crosses many list boundaries (3 000 terms)."""
    n_docs = 50000
    case = make_case(700000, n_docs, 3000, seed=9)
    worst = run_case(case, n_docs, 0.9, 0.4, False, in_place=False)
    print(f"largest relative error {worst / bc.U:.2f} u, bound {bc.rel_bound(0.9) / bc.U:.2f} u")
    run_case(case, n_docs, 0.9, 0.4, True, in_place=True)


def test_document_id_outside_the_collection_is_reported():
    from scaling_retriever_amd import bm25
    from scaling_retriever_amd.scoring import bm25_weights
    n_docs = 100
    indptr, doc_ids, tf, doc_len = make_case(1000, n_docs, 32, seed=2)
    doc_ids[700] = n_docs
    doc_ids[900] = -1
    dev = [torch.from_numpy(x).cuda() for x in (indptr, doc_ids, tf, doc_len, bm25.idf_table(np.diff(indptr), n_docs))]
    with pytest.raises(ValueError, match=rf"document id {n_docs} \(posting 700\)"):
        bm25_weights(*dev, *bm25.bm25_scalars(0.9, 0.4, 50.0))
    with pytest.raises(ValueError, match="indptr runs from 0 to 1000"):
        bm25_weights(dev[0], dev[1][:-1], dev[2][:-1], dev[3], dev[4], 1.9, 0.5, 0.01)
