"""CPU: sparse search under a document bitmap (sr_sparse_search_masked, csrc/subset_search.hip, cert_score_kernel<KS, true>) - the parts
that need no GPU.  The numpy specification of a masked result is defined HERE (masked_topk_spec) and checked against the subset
specification of tests/test_subset_host.py; tests/test_sparse_mask_gpu.py may import it.  Then the C ABI's declaration and binding and the
argument checks of the Python layer, which run before anything touches the device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ specification ---
def masked_topk_spec(scores, flags, k, thr):
    """scores fp32 [nq, N] of every document position, flags bool [N].  Per query: the allowed documents with score > thr ranked by
    (score descending, position ascending) - the order of sr_sparse_search -, cut to k, padded with (0, -1).  Returns (scores [nq, k],
    ids [nq, k], counts [nq])."""
    scores = np.asarray(scores, np.float32)
    flags = np.asarray(flags, bool)
    nq, N = scores.shape
    assert flags.shape == (N,)
    out_s = np.zeros((nq, k), np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    counts = np.zeros(nq, np.int32)
    pos = np.flatnonzero(flags)
    for q in range(nq):
        cand = pos[scores[q, pos] > np.float32(thr)]
        order = cand[np.lexsort((cand, -scores[q, cand].astype(np.float64)))][:k]
        counts[q] = len(order)
        out_s[q, :len(order)] = scores[q, order]
        out_i[q, :len(order)] = order
    return out_s, out_i, counts


def test_masked_spec_is_the_subset_spec_of_the_set_bits():
    from test_subset_host import subset_topk_spec
    rng = np.random.default_rng(17)
    for N, nq, k, thr, p in [(50, 4, 7, 0.0, 0.5), (97, 3, 200, 1.0, 0.3), (33, 5, 3, -1.0, 0.9), (64, 2, 5, 0.0, 0.0), (40, 2, 5, 2.0, 1.0)]:
        scores = rng.integers(0, 5, size=(nq, N)).astype(np.float32)          # five distinct values: ties everywhere, also at the cut
        flags = rng.random(N) < p if 0.0 < p < 1.0 else np.full(N, p == 1.0)
        s, i, c = masked_topk_spec(scores, flags, k, thr)
        es, ei, ec = subset_topk_spec(scores, np.arange(N), np.flatnonzero(flags), k, np.float32(0), threshold=thr)
        assert np.array_equal(i, ei) and np.array_equal(s.view(np.uint32), es.view(np.uint32)) and np.array_equal(c, ec)
        assert (c <= min(k, int(flags.sum()))).all()
    # hand-worked: positions 1 and 3 tie, 3 is masked out; the threshold is strict
    s, i, c = masked_topk_spec(np.array([[1.0, 2.0, 0.0, 2.0, 1.0]], np.float32), np.array([1, 1, 1, 0, 1], bool), 3, 0.0)
    assert i.tolist() == [[1, 0, 4]] and s.tolist() == [[2.0, 1.0, 1.0]] and c.tolist() == [3]
    s, i, c = masked_topk_spec(np.array([[1.0, 2.0, 0.0, 2.0, 1.0]], np.float32), np.array([1, 0, 1, 0, 1], bool), 3, 1.0)
    assert i.tolist() == [[-1, -1, -1]] and c.tolist() == [0]


# ------------------------------------------------------------------------------------------------------ C ABI ---
def test_masked_entry_point_is_declared_exported_and_bound():
    import ctypes
    from scaling_retriever_amd import _lib
    header = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    m = re.search(r"\bint sr_sparse_search_masked\(([^;]*)\);", header)
    assert m, "sr_sparse_search_masked is not declared in include/sr_hip.h"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 15
    assert "const uint32_t* d_mask_words" in m.group(1) and "int64_t n_bits" in m.group(1)
    sig = _lib.SIGNATURES["sr_sparse_search_masked"]
    assert sig[0] is ctypes.c_int and len(sig[1]) == 15
    # the subset entry's layout with (words, n_bits) where (list, m) stand
    assert sig[1] == _lib.SIGNATURES["sr_sparse_search_subset"][1]
    lib = _lib.load()
    assert hasattr(lib, "sr_sparse_search_masked") and lib.sr_sparse_search_masked.argtypes == sig[1]
    p = ctypes.c_void_p(4096)                             # never dereferenced: the null index is refused first
    assert lib.sr_sparse_search_masked(None, p, p, p, 1, 10, 0.0, p, 32, 0, 1, p, p, p, None) == _lib.SR_ERR_INVALID
    assert b"null index" in lib.sr_last_error()


# ------------------------------------------------------------------------------------------------ Python layer ---
def _handleless(n_docs):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    idx = object.__new__(SparseIndexHIP)                  # no handle, no device: the checks below must not need either
    idx.n_docs = n_docs
    return idx


def test_mask_argument_checks_run_before_the_device_is_touched():
    import torch
    idx = _handleless(100)
    qi, qc, qv = np.array([0, 1], np.int64), np.array([3], np.int32), np.array([1.0], np.float32)
    with pytest.raises(ValueError, match="not both"):
        idx.search(qi, qc, qv, 5, subset=np.array([1, 2], np.int64), mask=np.ones(100, bool))
    for bad in (np.ones(100, np.float32), np.ones(100, np.int64), torch.ones(100, dtype=torch.float16), [0.5] * 100):
        with pytest.raises(ValueError, match="bool"):
            idx.search(qi, qc, qv, 5, mask=bad)
    for bad in (np.ones((4, 25), bool), torch.ones((2, 50), dtype=torch.bool), np.ones((2, 2), np.uint32)):
        with pytest.raises(ValueError, match="1-D"):
            idx.search(qi, qc, qv, 5, mask=bad)
    # a packed mask of 100 documents holds 4 words: one too few and one too many are both refused, naming the count
    for n in (3, 5):
        with pytest.raises(ValueError, match=r"holds 4 words"):
            idx.search(qi, qc, qv, 5, mask=np.zeros(n, np.uint32))
        with pytest.raises(ValueError, match=r"holds 4 words"):
            idx.search(qi, qc, qv, 5, mask=torch.zeros(n, dtype=torch.int32))


def test_allowed_mask_of_the_retrieval_drivers():
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval, SparseRetrieval
    r = object.__new__(SparseRetrieval)
    r.hip_index = _handleless(12)
    r._dev = "cpu"
    for bad in (np.ones(11, bool), np.ones(13, bool), np.ones((3, 4), bool)):
        with pytest.raises(ValueError, match=r"one flag per document position \(12\)"):
            r.allowed_mask_words(bad)
    flags = np.zeros(12, bool)
    flags[[0, 5, 11]] = True
    words = r.allowed_mask_words(flags)                   # packed where the flags live: here the host
    assert words.numel() == 1 and int(words[0]) == (1 << 0) | (1 << 5) | (1 << 11)
    with pytest.raises(ValueError, match="not both"):
        r._sparse_retrieve_multithreaded(None, [], allowed_ids=["a"], allowed_mask=flags)
    with pytest.raises(ValueError, match="not both"):
        SparseRetrieval.retrieve(r, [], 5, allowed_ids=["a"], allowed_mask=flags)
    with pytest.raises(NotImplementedError, match="allowed_mask"):
        ShardedSparseRetrieval.retrieve(object.__new__(ShardedSparseRetrieval), None, 5, allowed_mask=flags)
