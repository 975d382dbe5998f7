"""Top-k beyond sr_max_topk() = 4096 (csrc/topk_large.hip): dense, sparse, merge and the retrieval drivers against the CPU oracle,
bit for bit.  The reference takes any k: faiss IndexFlatIP.search (indexer.py:210-211), numba_score_float returns every
document above the threshold and select_topk / retrieve take any k (indexer.py:315-344, 530-540)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import scoring as O

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MIN = np.float32(-3.402823466e38)


def _dense_index(D, segments=1, precision=None):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    idx = DenseIndexHIP(D.shape[1])
    bounds = np.linspace(0, len(D), segments + 1).astype(int)
    for a, b in zip(bounds[:-1], bounds[1:]):
        idx.add_host_rows(D[a:b])
    if precision:
        idx.set_precision(precision)
    return idx


def _search(idx, Q, k):
    s, i = idx.search(torch.from_numpy(Q).cuda(), k)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy()


def _oracle_dense(Q, D, k):
    return O.topk_rows(O.dense_scores_fma(Q, D, O.dense_korder(Q.shape[0], Q.shape[1])), k)


def _assert_rows(s, i, es, ei):
    bad = np.nonzero(~(np.all(s == es, axis=1) & np.all(i == ei, axis=1)))[0]
    assert len(bad) == 0, f"rows differ: {bad[:10]} ({len(bad)} of {len(s)})"


# ----------------------------------------------------------------------------------------------------------------- dense ---
@gpu
@pytest.mark.parametrize("nq,h,k,n,segments", [
    (1, 256, 20000, 50000, 1),      # streaming kernel, one query
    (1, 64, 4097, 10000, 1),        # tiled TN 32, one query
    (40, 256, 4097, 9000, 2),       # streaming, two segments
    (40, 128, 6000, 12000, 1),      # TN 64
    (100, 64, 6000, 8000, 1),       # TN 128
    (100, 128, 20000, 25000, 2),    # TN 128, two segments
    (300, 256, 6000, 10000, 1),     # TN 256
    (300, 64, 20000, 24000, 1),     # TN 256
    (40, 64, 6000, 5000, 1),        # k > N: padding (-FLT_MAX, -1)
    (300, 128, 4097, 3000, 2),      # k > N, two segments
])
def test_dense_large_k_bit_exact(nq, h, k, n, segments):
    rng = np.random.default_rng(nq * 7 + h + k)
    Q = rng.standard_normal((nq, h), dtype=np.float32)
    D = rng.standard_normal((n, h), dtype=np.float32)
    s, i = _search(_dense_index(D, segments), Q, k)
    es, ei = _oracle_dense(Q, D, k)
    _assert_rows(s, i, es, ei)
    if k > n:
        assert np.all(i[:, n:] == -1) and np.all(s[:, n:] == FLT_MIN)


@gpu
@pytest.mark.parametrize("precision", ["fp32", "fp32_filtered", "bf16x3", "bf16x6"])
def test_prefix_of_a_large_k_search_is_the_small_k_search(precision):
    rng = np.random.default_rng(11)
    Q = rng.standard_normal((100, 128), dtype=np.float32)
    D = rng.standard_normal((20000, 128), dtype=np.float32)
    idx = _dense_index(D, precision=precision)
    s8, i8 = _search(idx, Q, 8192)
    s1, i1 = _search(idx, Q, 1000)
    assert np.array_equal(i8[:, :1000], i1) and np.array_equal(s8[:, :1000], s1)
    if precision in ("fp32", "fp32_filtered"):
        es, ei = _oracle_dense(Q, D, 8192)
        _assert_rows(s8, i8, es, ei)


@gpu
@pytest.mark.parametrize("nq", [1, 100])
def test_ties_at_the_cut_keep_the_lowest_indices(nq):
    """A block of 3 000 identical rows straddles the k-th position: the select has to go down to the index bits."""
    rng = np.random.default_rng(5 + nq)
    n, h = 30000, 64
    Q = rng.standard_normal((nq, h), dtype=np.float32)
    D = rng.standard_normal((n, h), dtype=np.float32)
    F = O.dense_scores_fma(Q[:1], D, O.dense_korder(nq, h))[0]
    order = np.argsort(-F, kind="stable")
    src = order[5000]
    dup = rng.choice(np.setdiff1d(np.arange(n), [src]), 2999, replace=False)
    D[dup] = D[src]
    k = 6500
    s, i = _search(_dense_index(D), Q, k)
    es, ei = _oracle_dense(Q, D, k)
    _assert_rows(s, i, es, ei)
    tied = np.sort(np.concatenate([[src], dup]))
    kept = i[0][s[0] == s[0, k - 1]]
    assert 0 < len(kept) < len(tied) and np.array_equal(np.sort(kept), tied[:len(kept)])


@gpu
def test_one_query_with_k_close_to_n():
    rng = np.random.default_rng(3)
    n, h, k = 1_500_000, 64, 1_400_000
    Q = rng.standard_normal((1, h), dtype=np.float32)
    D = rng.standard_normal((n, h), dtype=np.float32)
    s, i = _search(_dense_index(D), Q, k)
    es, ei = _oracle_dense(Q, D, k)
    _assert_rows(s, i, es, ei)


@gpu
def test_workspace_limit_splits_the_batch_with_the_same_bits():
    rng = np.random.default_rng(4)
    Q = rng.standard_normal((300, 128), dtype=np.float32)
    D = rng.standard_normal((30000, 128), dtype=np.float32)
    idx = _dense_index(D)
    s0, i0 = _search(idx, Q, 20000)
    idx.set_workspace_limit(64 << 20)          # ~400 KB per query: two sub-batches of 150
    s1, i1 = _search(idx, Q, 20000)
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1)
    es, ei = _oracle_dense(Q, D, 20000)
    _assert_rows(s1, i1, es, ei)
    idx.set_workspace_limit(1 << 20)           # not even 65 queries fit: no partial result, an error with the byte count
    with pytest.raises(MemoryError, match="bytes"):
        _search(idx, Q, 20000)


@gpu
def test_dense_rejects_bad_arguments_large_k():
    """Up to 4096 rows of padding past the index's documents: k = 4106 over 10 rows is a valid large-k search, k = 5000 is still
    rejected there (tests/test_scoring_gpu.py), as are k outside [1, 2^30]."""
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import DenseIndexHIP
    with pytest.raises(ValueError):
        DenseIndexHIP(30)
    idx = DenseIndexHIP(64)
    idx.add_host_rows(np.zeros((10, 64), np.float32))
    s, i = idx.search(torch.zeros((2, 64), device="cuda"), 4106)
    assert torch.all(i[:, 10:] == -1) and torch.all(s[:, 10:] == float(FLT_MIN)) and torch.all(i[:, :10] >= 0)
    for k in (4107, 5000, 0):
        with pytest.raises(ValueError):
            idx.search(torch.zeros((2, 64), device="cuda"), k)
    assert idx.lib.sr_dense_search(idx._h, None, 0, (1 << 30) + 1, None, None, None) == _lib.SR_ERR_INVALID
    with pytest.raises(ValueError):
        idx.search(torch.zeros((2, 32), device="cuda"), 5)


# ---------------------------------------------------------------------------------------------------------------- sparse ---
def _sparse_collection(rng, V, N, per_term):
    indptr, ids, vals = [0], [], []
    for t in range(V):
        m = int(rng.integers(per_term // 4, per_term + 1))
        d = np.sort(rng.choice(N, m, replace=False)).astype(np.int32)
        ids.append(d)
        vals.append(rng.random(m, dtype=np.float32) * 2)
        indptr.append(indptr[-1] + m)
    return np.array(indptr, np.int64), np.concatenate(ids), np.concatenate(vals).astype(np.float32)


def _sparse_queries(rng, V, nq, lo, hi):
    qi, qc, qv = [0], [], []
    for _ in range(nq):
        m = int(rng.integers(lo, hi + 1))
        c = np.sort(rng.choice(V, m, replace=False)).astype(np.int32)
        qc.append(c)
        qv.append(rng.random(m, dtype=np.float32) + 0.1)
        qi.append(qi[-1] + m)
    return np.array(qi, np.int64), np.concatenate(qc), np.concatenate(qv).astype(np.float32)


def _sparse_check(idx, coll, N, q, k, thr, id_base=0, id_stride=1):
    indptr, ids, vals = coll
    qi, qc, qv = q
    s, i, c = idx.search(qi, qc, qv, k, threshold=thr, id_base=id_base, id_stride=id_stride)
    torch.cuda.synchronize()
    ei, es, ec = O.sparse_retrieve_c(indptr, ids, vals, qi, qc, qv, k, thr, N, q_threads=4)
    ei = np.where(ei >= 0, id_base + ei * id_stride, ei)
    s, i, c = s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(c, ec)
    _assert_rows(s, i, es, ei)
    return s, i, c


@gpu
@pytest.mark.parametrize("cert", [False, True])
def test_sparse_large_k_bit_exact(cert, monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    if cert:
        monkeypatch.setenv("SR_SPARSE_CERT", "1")      # the index carries the certified scorer: k > 3072 must route to the exact kernels
    rng = np.random.default_rng(21)
    V, N = 400, 40000
    coll = _sparse_collection(rng, V, N, 3000)
    q = _sparse_queries(rng, V, 24, 1, 12)             # short queries hit fewer than k documents: counts and (0, -1) padding
    idx = SparseIndexHIP(*coll, N)
    for k in (4097, 10000, N + 5):
        for thr in (0.0, 1.5):
            s, i, c = _sparse_check(idx, coll, N, q, k, thr)
            assert (c < k).any() and (thr > 0 or (c > 4096).any())
            for r in range(len(c)):
                assert np.all(i[r, c[r]:] == -1) and np.all(s[r, c[r]:] == 0)


@gpu
def test_sparse_workspace_limit_shrinks_the_batch():
    from scaling_retriever_amd.scoring import SparseIndexHIP
    rng = np.random.default_rng(22)
    V, N = 200, 30000
    coll = _sparse_collection(rng, V, N, 3000)
    q = _sparse_queries(rng, V, 40, 5, 15)
    idx = SparseIndexHIP(*coll, N)
    idx.set_workspace_limit(8 << 20)                   # ~200 KB + 64 KB per query at k = 10 000: batches of 31
    _sparse_check(idx, coll, N, q, 10000, 0.0)


@gpu
def test_numba_score_float_returns_every_hit():
    """The static helper asked for 4096 hits and cut longer lists short; it now returns every document above the threshold."""
    from scaling_retriever_amd.indexer import SparseRetrieval
    rng = np.random.default_rng(23)
    V, N = 60, 20000
    indptr, ids, vals = _sparse_collection(rng, V, N, 4000)
    d_ids = {t: ids[indptr[t]:indptr[t + 1]] for t in range(V)}
    d_vals = {t: vals[indptr[t]:indptr[t + 1]] for t in range(V)}
    cols = np.array([2, 5, 9, 17, 30, 41], np.int32)
    qv = np.array([0.5, 1.25, 0.75, 2.0, 0.3, 1.0], np.float32)
    for thr in (0.0, 1.0):
        fi, neg = SparseRetrieval.numba_score_float(d_ids, d_vals, cols, qv, threshold=thr, size_collection=N)
        ei, en = O.numba_score_float(indptr, ids, vals, cols, qv, thr, N)
        assert len(ei) > 4096
        assert fi.dtype == np.int64 and np.array_equal(fi, ei) and np.array_equal(neg, en)


# ----------------------------------------------------------------------------------------------------------------- merge ---
@gpu
def test_merge_of_two_dense_shards_equals_one_index():
    from scaling_retriever_amd.scoring import DenseIndexHIP, topk_merge
    g = torch.Generator(device="cuda").manual_seed(1)
    n, h, k = 15001, 64, 6000
    D = torch.randn((n, h), device="cuda", generator=g)
    Q = torch.randn((70, h), device="cuda", generator=g)
    full = DenseIndexHIP(h)
    full.add_device_rows(D)
    fs, fi = full.search(Q, k)
    ss, si = [], []
    for r in range(2):
        shard = DenseIndexHIP(h)
        shard.add_device_rows(D[r::2].contiguous(), id_base=r, id_stride=2)
        s, i = shard.search(Q, k)
        ss.append(s)
        si.append(i)
    ms, mi = topk_merge(torch.stack(ss), torch.stack(si))
    assert torch.equal(mi, fi) and torch.equal(ms, fs)


@gpu
def test_merge_of_two_sparse_shards_equals_one_index():
    from scaling_retriever_amd.scoring import SparseIndexHIP, topk_merge
    rng = np.random.default_rng(24)
    V, N, k = 300, 30000, 8000
    coll = _sparse_collection(rng, V, N, 2500)
    q = _sparse_queries(rng, V, 20, 1, 10)
    full_s, full_i, full_c = _sparse_check(SparseIndexHIP(*coll, N), coll, N, q, k, 0.0)
    indptr, ids, vals = coll
    ss, si = [], []
    for r in range(2):                                # doc d of shard r is global doc 2 d + r
        keep = ids % 2 == r
        counts = np.array([keep[indptr[t]:indptr[t + 1]].sum() for t in range(V)])
        sh = (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), (ids[keep] // 2).astype(np.int32), vals[keep])
        s, i, c = SparseIndexHIP(*sh, (N - r + 1) // 2).search(*q, k, threshold=0.0, id_base=r, id_stride=2)
        ss.append(s)
        si.append(i)
    ms, mi = topk_merge(torch.stack(ss), torch.stack(si), pad_score=0.0)
    assert np.array_equal(mi.cpu().numpy(), full_i) and np.array_equal(ms.cpu().numpy(), full_s)


# --------------------------------------------------------------------------------------------------------------- drivers ---
class FakeLoader:
    """DataLoader stand-in (as in tests/test_indexer_gpu.py): {"input_ids", "attention_mask", "ids"}, left padding."""

    def __init__(self, seqs, ids, batch_size, pad_id):
        self.seqs, self.ids, self.batch_size, self.pad_id = seqs, ids, batch_size, pad_id

    def __len__(self):
        return (len(self.seqs) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for b0 in range(0, len(self.seqs), self.batch_size):
            chunk = self.seqs[b0:b0 + self.batch_size]
            L = max(len(s) for s in chunk)
            ids = np.full((len(chunk), L), self.pad_id, np.int64)
            mask = np.zeros((len(chunk), L), np.int64)
            for r, s in enumerate(chunk):
                ids[r, L - len(s):] = s
                mask[r, L - len(s):] = 1
            yield {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask),
                   "ids": list(self.ids[b0:b0 + self.batch_size])}


@gpu
def test_dense_flat_indexer_search_knn_5000():
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    rng = np.random.default_rng(25)
    n, h = 12000, 128
    embs = rng.standard_normal((n, h), dtype=np.float32)
    pids = [f"p{j}" for j in range(n)]
    q = rng.standard_normal((9, h), dtype=np.float32)
    index = DenseFlatIndexer()
    index.init_index(h)
    index.index_data(embs, pids)
    top_ids, top_scores = index.search_knn(q, 5000)
    es, ei = _oracle_dense(q, embs, 5000)
    assert np.array_equal(top_scores, es)
    assert top_ids == [[pids[j] for j in row] for row in ei]


@gpu
def test_sparse_retrieval_retrieve_5000(golden_dir, tmp_path):
    from golden_weights import make_weights
    from oracle import scoring as SC
    from scaling_retriever_amd.indexer import SparseIndexer, SparseRetrieval
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    V = cfg["vocab_size"]
    rng = np.random.default_rng(26)
    docs = [rng.integers(0, V - 1, size=int(rng.integers(1, 7))) for _ in range(60)]
    queries = [rng.integers(0, V - 1, size=int(rng.integers(1, 4))) for _ in range(7)]
    pids, qids = [f"p{j}" for j in range(len(docs))], [f"q{j}" for j in range(len(queries))]
    model = LlamaBiSparse.from_weights(cfg, w, precision="bf16").to("cuda").eval()
    index_dir = str(tmp_path / "index")
    SparseIndexer(model, index_dir=index_dir, compute_stats=True, dim_voc=model.vocab_size, device="cuda").index(
        FakeLoader(docs, pids, batch_size=8, pad_id=V - 1))
    assert pickle.load(open(os.path.join(index_dir, "doc_ids.pkl"), "rb")) == {j: p for j, p in enumerate(pids)}
    retr = SparseRetrieval(config={"index_dir": index_dir, "out_dir": str(tmp_path / "out")}, model=model,
                           compute_stats=True, dim_voc=model.vocab_size, device="cuda")
    retr.retrieve(FakeLoader(queries, qids, batch_size=4, pad_id=V - 1), topk=5000, threshold=0.0)
    run_text = open(tmp_path / "out" / "run.json").read()
    indptr, ids, vals = retr.sparse_index.csr(V)
    qvecs, _ = retr._generate_query_vecs(FakeLoader(queries, qids, batch_size=4, pad_id=V - 1))
    expect = {}
    for qi, (cols, qv) in enumerate(qvecs):
        fi, neg = SC.numba_score_float(indptr, ids, vals, cols, qv, 0.0, len(docs))
        ei, es = SC.select_topk(fi, neg, 5000)
        if len(ei):
            expect[qids[qi]] = {pids[j]: float(s) for j, s in zip(ei, es)}
    assert run_text == json.dumps(expect)


# -------------------------------------------------------------------------------------------------------------- metadata ---
def _kernel_metadata(obj, tmp_path):
    """{mangled kernel name: {scratch bytes, spilled VGPRs / SGPRs, VGPRs}} of a built object (as in tests/test_abi.py)."""
    import re
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(obj) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("needs the built object and the ROCm LLVM tools")
    fat, dev = str(tmp_path / "k.fatbin"), str(tmp_path / "k_dev.o")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, str(tmp_path / "unused.o")])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={dev}", "--unbundle"])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", dev], capture_output=True, text=True).stdout
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", notes, flags=re.S):
        kernels[m.group(1)] = {key: int(v) for key, v in re.findall(r"(\.private_segment_fixed_size:|\.vgpr_spill_count:|\.sgpr_spill_count:|\.vgpr_count:)\s+(\d+)", m.group(2))}
    return kernels


def test_large_topk_kernels_use_no_scratch(tmp_path):
    meta = _kernel_metadata(os.path.join(ROOT, "scaling_retriever_amd", "csrc", "topk_large.o"), tmp_path)
    names = ("plan", "append", "hist", "pick", "holes", "fill", "finish", "sort_tile", "sort_step", "emit")
    for stem in names:
        found = [k for k in meta if f"topk_large_{stem}_kernel" in k]
        assert len(found) == 1, (stem, sorted(meta))
    for name, m in meta.items():
        assert m[".private_segment_fixed_size:"] == 0 and m[".vgpr_spill_count:"] == 0 and m[".sgpr_spill_count:"] == 0, (name, m)
