"""Sparse range search under a document bitmap (sr_sparse_range_count_masked / _fill_masked, SparseIndexHIP.range_search(mask=)).

Collections, queries, thresholds and the cached oracle lists are those of tests/test_sparse_range_gpu.py (numba_score_float per query
and threshold); the expected list is the oracle's with the documents whose bit is clear removed.  Lims, ids and score bits are compared
for EQUALITY.

Masks over [0, n_docs): every bit (must equal the unmasked result byte for byte, the zero-score documents under threshold -1.0
included), no bit, random 50 % and 3 %, the last document alone, for 32 805 documents (five 8 192-document tiles) tiles 1 and 3
entirely clear, and packed words whose last word carries set bits at or beyond n_docs."""
import numpy as np
import pytest
import torch

import test_sparse_range_gpu as B

pytestmark = pytest.mark.gpu


def _masks(n_docs):
    rng = np.random.default_rng(500 + n_docs)
    last = np.zeros(n_docs, bool)
    last[-1] = True
    out = {"all": np.ones(n_docs, bool), "none": np.zeros(n_docs, bool), "r50": rng.random(n_docs) < 0.5, "r03": rng.random(n_docs) < 0.03,
           "last": last}
    if n_docs > 4 * 8192:
        tiles = rng.random(n_docs) < 0.5
        tiles[8192:2 * 8192] = False
        tiles[3 * 8192:4 * 8192] = False
        out["tiles"] = tiles
    return out


def _expected(n_docs, thr, allowed, id_base=0, id_stride=1):
    lims = np.zeros(len(thr) + 1, np.int64)
    scores, ids = [], []
    for q, t in enumerate(thr):
        pos, s = B._oracle(n_docs, q, t)
        keep = allowed[pos]
        lims[q + 1] = lims[q] + int(keep.sum())
        scores.append(s[keep])
        ids.append(id_base + pos[keep] * id_stride)
    return lims, np.concatenate(scores).astype(np.float32), np.concatenate(ids).astype(np.int64)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("nq", [1, 5, B.NQ_ALL])
@pytest.mark.parametrize("n_docs", B.SHAPES)
def test_masked_range_equals_filtered_oracle(n_docs, nq):
    from scaling_retriever_amd.scoring import pack_doc_mask
    idx = B._index(n_docs)
    for rot in ((0, 1, 3, 6) if nq < B.KINDS else (0,)):          # nq = 1: the thresholds 0.0, -1.0, the 3 000th best and -inf in turn
        thr = B._thresholds(n_docs, nq, rot)
        unmasked = idx.range_search(*B._csr(nq), thr)
        for name, allowed in _masks(n_docs).items():
            got = idx.range_search(*B._csr(nq), thr, mask=allowed)
            B._assert_equal(got, _expected(n_docs, thr, allowed), f"n_docs={n_docs} nq={nq} rot={rot} mask={name}")
            if name == "all":
                assert _same(got, unmasked)
            if name == "none":
                assert not bool(got[0].any())
            if name == "r50":
                # packed words whose last word has every bit at or beyond n_docs set: those bits are ignored
                words = pack_doc_mask(allowed).copy()
                if n_docs % 32:
                    words[-1] |= np.uint32((0xFFFFFFFF << (n_docs % 32)) & 0xFFFFFFFF)
                assert _same(idx.range_search(*B._csr(nq), thr, mask=words), got)
                assert _same(idx.range_search(*B._csr(nq), thr, mask=torch.from_numpy(allowed).cuda()), got)


def test_zero_score_documents_follow_their_bit():
    """Queries without any term: every score is +0.0, so under a negative threshold the hits are exactly the set bits."""
    n_docs = 32805
    idx = B._index(n_docs)
    allowed = _masks(n_docs)["tiles"]
    lims, s, i = idx.range_search(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.array([0.0, -0.5, np.nan], np.float32),
                                  mask=allowed)
    m = int(allowed.sum())
    assert lims.tolist() == [0, 0, m, m] and np.array_equal(i.cpu().numpy(), np.nonzero(allowed)[0]) and bool((s == 0).all())


def test_chunks_of_two_tiles_scores_ids_and_repeatability(monkeypatch):
    n_docs, nq = 32805, B.NQ_ALL
    idx = B._index(n_docs)
    thr = B._thresholds(n_docs, nq)
    allowed = _masks(n_docs)["tiles"]
    want = _expected(n_docs, thr, allowed, 7, 3)
    got = idx.range_search(*B._csr(nq), thr, id_base=7, id_stride=3, mask=allowed)
    B._assert_equal(got, want, "default chunking")
    monkeypatch.setenv("SR_SPARSE_RANGE_CHUNK_TILES", "2")
    again = idx.range_search(*B._csr(nq), thr, id_base=7, id_stride=3, mask=allowed)
    B._assert_equal(again, want, "two tiles per chunk")
    monkeypatch.delenv("SR_SPARSE_RANGE_CHUNK_TILES")
    plain = idx.range_search(*B._csr(nq), thr, mask=allowed)
    assert int(plain[0][-1]) > 1000
    pairs = idx.score_pairs(*B._csr(nq), plain[0], plain[2])
    assert torch.equal(pairs.view(torch.int32), plain[1].view(torch.int32))
    # sort=True under a mask
    ls, ss, si = (t.cpu().numpy() for t in idx.range_search(*B._csr(5), thr[:5], sort=True, mask=allowed))
    lu, su, iu = (t.cpu().numpy() for t in idx.range_search(*B._csr(5), thr[:5], mask=allowed))
    assert np.array_equal(ls, lu)
    for q in range(5):
        o = np.lexsort((iu[lu[q]:lu[q + 1]], -su[lu[q]:lu[q + 1]]))
        assert np.array_equal(si[ls[q]:ls[q + 1]], iu[lu[q]:lu[q + 1]][o])


def test_errors():
    import ctypes

    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import _ptr
    n_docs, nq = 8192, 5
    idx = B._index(n_docs)
    thr = B._thresholds(n_docs, nq)
    with pytest.raises(ValueError, match="words"):
        idx.range_search(*B._csr(nq), thr, mask=np.zeros(n_docs // 32 + 1, np.uint32))
    with pytest.raises(ValueError):
        idx.range_search(*B._csr(nq), thr, mask=np.ones(n_docs - 1, bool))
    with pytest.raises(ValueError):
        idx.range_search(*B._csr(nq), thr, mask=np.ones(n_docs, np.float32))
    # the raw ABI: wrong n_bits is refused by both halves; a masked fill after an unmasked count too
    qp, qc, qv = (torch.from_numpy(a).cuda() for a in B._csr(nq))
    t = torch.from_numpy(thr).cuda()
    lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    words = torch.full((n_docs // 32,), -1, dtype=torch.int32, device="cuda")
    total = ctypes.c_int64(-1)
    s = torch.full((64,), B.SENTINEL_S, dtype=torch.float32, device="cuda")
    i = torch.full((64,), B.SENTINEL_I, dtype=torch.int64, device="cuda")
    rc = idx.lib.sr_sparse_range_count_masked(idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(t), _ptr(words), n_docs - 1, _ptr(lims),
                                              ctypes.byref(total), _lib.stream_ptr())
    assert rc == _lib.SR_ERR_INVALID and b"n_bits" in idx.lib.sr_last_error()
    rc = idx.lib.sr_sparse_range_fill_masked(idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(t), _ptr(words), n_docs + 1, _ptr(lims), 0, 1,
                                             _ptr(s), _ptr(i), 64, _lib.stream_ptr())
    assert rc == _lib.SR_ERR_INVALID and b"n_bits" in idx.lib.sr_last_error()
    inf = torch.full((nq,), float("inf"), device="cuda")
    assert idx.lib.sr_sparse_range_count(idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(inf), _ptr(lims), ctypes.byref(total),
                                         _lib.stream_ptr()) == 0 and total.value == 0
    rc = idx.lib.sr_sparse_range_fill_masked(idx._h, _ptr(qp), _ptr(qc), _ptr(qv), nq, _ptr(inf), _ptr(words), n_docs, _ptr(lims), 0, 1,
                                             _ptr(s), _ptr(i), 64, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.SR_ERR_INVALID and b"without a mask" in idx.lib.sr_last_error()
    assert bool((s == B.SENTINEL_S).all()) and bool((i == B.SENTINEL_I).all())


def test_retrieval_allowed_ids_equal_allowed_mask(golden_dir, tmp_path):
    """SparseRetrieval.range_search on the tiny model: allowed_ids, allowed_mask and the filtered unrestricted lists agree."""
    import json
    import os

    from golden_weights import make_weights
    from test_indexer_gpu import FakeLoader, _corpus
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval, SparseIndexer, SparseRetrieval
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    Vm = cfg["vocab_size"]
    rng = np.random.default_rng(1)
    docs, queries = _corpus(rng, 50, Vm, 1, 6), _corpus(rng, 7, Vm, 1, 3)
    pids, qids = [f"p{i}" for i in range(len(docs))], [f"q{i}" for i in range(len(queries))]
    model = LlamaBiSparse.from_weights(cfg, w, precision="bf16").to("cuda").eval()
    index_dir = str(tmp_path / "index")
    SparseIndexer(model, index_dir=index_dir, compute_stats=False, dim_voc=model.vocab_size, device="cuda").index(
        FakeLoader(docs, pids, batch_size=8, pad_id=Vm - 1))
    retr = SparseRetrieval(config={"index_dir": index_dir, "out_dir": str(tmp_path / "out")}, model=model, dim_voc=model.vocab_size, device="cuda")
    qvecs, _ = retr._generate_query_vecs(FakeLoader(queries, qids, batch_size=4, pad_id=Vm - 1))
    inv = retr.inverse_id_map()
    allowed_ids = [p for p in pids if inv.pos.get(p) is not None][::3]
    flags = np.zeros(retr.hip_index.n_docs, bool)
    flags[[inv.pos.get(p) for p in allowed_ids]] = True
    keep = set(allowed_ids)
    for thr in (0.0, -1.0):
        full_ids, full_scores = retr.range_search(qvecs, thr)
        by_ids = retr.range_search(qvecs, thr, allowed_ids=allowed_ids[::-1])
        by_mask = retr.range_search(qvecs, thr, allowed_mask=flags)
        for qi in range(len(queries)):
            sel = np.array([d in keep for d in full_ids[qi]], bool)
            want = [d for d in full_ids[qi] if d in keep]
            for got in (by_ids, by_mask):
                assert got[0][qi] == want, (thr, qi)
                assert np.array_equal(got[1][qi].view(np.int32), full_scores[qi][sel].view(np.int32)), (thr, qi)
        assert thr == 0.0 or all(len(x) == len(allowed_ids) for x in by_mask[0])
    with pytest.raises(ValueError, match="not both"):
        retr.range_search(qvecs, 0.0, allowed_ids=allowed_ids, allowed_mask=flags)
    with pytest.raises(NotImplementedError):
        ShardedSparseRetrieval.range_search(retr, qvecs, allowed_mask=flags)
