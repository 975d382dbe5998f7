"""GPU: the sparse head's per-row term budget - sr_sparse_compact_topm (csrc/sparse_prune.hip) against the numpy statement of its
contract, bit for bit, and the budget carried through SparseIndexer / SparseRetrieval on the tiny golden model.  The reference has
no such option (its SparseIndexer / SparseRetrieval keep every non-zero, scaling_retriever/indexer.py:259-260, :393-399); every
comparison here is exact."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from golden_weights import make_weights

pytestmark = pytest.mark.gpu

V_PROD = 128256


# ------------------------------------------------------------------ the contract, in numpy
def topm_row_reference(row, m):
    nz = np.flatnonzero(row != 0)
    order = np.lexsort((nz, -row[nz]))        # value descending, then column ascending
    return np.sort(nz[order[:m]]) if m else nz


def topm_reference(reps, m):
    keeps = [topm_row_reference(r, m) for r in reps]
    row_ptr = np.concatenate([[0], np.cumsum([len(k) for k in keeps])]).astype(np.int64)
    cols = np.concatenate(keeps).astype(np.int32)
    vals = np.concatenate([r[k] for r, k in zip(reps, keeps)]).astype(np.float32)
    return row_ptr, cols, vals


def prune_dense(reps, m):
    """reps with everything outside the budget set to zero."""
    out = np.zeros_like(reps)
    for r, row in enumerate(reps):
        k = topm_row_reference(row, m)
        out[r, k] = row[k]
    return out


# ------------------------------------------------------------------ the entry point
def compact_topm(reps_t, m, capacity=None):
    """(rc, needed, row_ptr, cols, vals) of one sr_sparse_compact_topm call on a cuda fp32 [B, V] tensor (any base alignment)."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    B, V = reps_t.shape
    cap = B * V if capacity is None else capacity
    row_ptr = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda")
    cols = torch.full((max(1, cap),), -1, dtype=torch.int32, device="cuda")
    vals = torch.full((max(1, cap),), -1.0, dtype=torch.float32, device="cuda")
    n = ctypes.c_int64(-1)
    rc = lib.sr_sparse_compact_topm(reps_t.data_ptr(), B, V, m, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), cap,
                                    ctypes.byref(n), _lib.stream_ptr())
    torch.cuda.synchronize()
    k = max(0, min(n.value, cap))
    return rc, n.value, row_ptr.cpu().numpy(), cols[:k].cpu().numpy(), vals[:k].cpu().numpy()


def compact_all(reps_t):
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    B, V = reps_t.shape
    row_ptr = torch.empty(B + 1, dtype=torch.int64, device="cuda")
    cols = torch.empty(B * V, dtype=torch.int32, device="cuda")
    vals = torch.empty(B * V, dtype=torch.float32, device="cuda")
    n = ctypes.c_int64(0)
    _lib.check(lib.sr_sparse_compact(reps_t.data_ptr(), B, V, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), B * V,
                                     ctypes.byref(n), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return row_ptr.cpu().numpy(), cols[:n.value].cpu().numpy(), vals[:n.value].cpu().numpy()


def assert_same_csr(got, want, what):
    for name, g, w in zip(("row_ptr", "cols", "vals"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)
    assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32)), (what, "value bits")


# ------------------------------------------------------------------ inputs (built once, never modified)
def _small_rows(V=1000, m=16):
    """The seven rows of the small case: values from four levels, so ties are everywhere."""
    rng = np.random.default_rng(11)
    levels = np.array([0.5, 1.0, 1.5, 2.0], np.float32)
    reps = np.zeros((7, V), np.float32)

    def put(r, nnz, vals=None):
        c = rng.choice(V, nnz, replace=False)
        reps[r, c] = levels[rng.integers(0, 4, nnz)] if vals is None else vals
    put(1, 5)                 # nnz < m
    put(2, m)                 # nnz == m
    put(3, m + 1)             # nnz == m + 1
    put(4, min(V, 400))       # nnz >> m
    put(5, 60, 1.0)           # every value equal: the cut is decided by the column alone
    c = rng.choice(V, 40, replace=False)          # row 6: 10 positives, 20 negatives (the cut falls among them), 10 times -0.0
    reps[6, c[:10]] = levels[rng.integers(0, 4, 10)]
    reps[6, c[10:30]] = -levels[rng.integers(0, 4, 20)]
    reps[6, c[30:]] = -0.0
    assert np.signbit(reps[6, c[30:]]).all()
    return reps


@pytest.fixture(scope="module")
def small():
    reps = _small_rows()
    reps_t = torch.from_numpy(reps).cuda()
    reps.setflags(write=False)
    return reps, reps_t


@pytest.fixture(scope="module")
def prod():
    """V = 128 256: 100 000 non-zeros (more than the kernel can stage in LDS: it reads the row again), 3 000 and 40."""
    rng = np.random.default_rng(12)
    reps = np.zeros((3, V_PROD), np.float32)
    for r, nnz in enumerate((100_000, 3_000, 40)):
        reps[r, rng.choice(V_PROD, nnz, replace=False)] = (rng.random(nnz) * 3.0 + 1e-3).astype(np.float32)
    assert ((reps != 0).sum(1) == (100_000, 3_000, 40)).all()
    reps_t = torch.from_numpy(reps).cuda()
    reps.setflags(write=False)
    return reps, reps_t


# ------------------------------------------------------------------ 1. small, ties everywhere
def test_small_rows_with_ties(small):
    reps, reps_t = small
    m = 16
    want = topm_reference(reps, m)
    nnz = (reps != 0).sum(1)
    assert nnz[0] == 0 and nnz[1] < m and nnz[2] == m and nnz[3] == m + 1 and nnz[4] > 10 * m
    assert nnz[6] == 30 and (reps[6] < 0).sum() == 20                     # -0.0 is not a candidate
    cut_inside_tie = 0
    for r in range(7):
        kept = want[1][want[0][r]:want[0][r + 1]]
        dropped = np.setdiff1d(np.flatnonzero(reps[r] != 0), kept)
        if len(kept) and len(dropped) and reps[r, dropped].max() == reps[r, kept].min():
            cut_inside_tie += 1
    assert cut_inside_tie >= 2                                            # kept and dropped entries of one value: the tie rule matters
    rc, n, *got = compact_topm(reps_t, m)
    assert rc == 0 and n == want[0][-1]
    assert_same_csr(got, want, "small")


@pytest.mark.parametrize("V", [999, 1001, 1, 3])
def test_widths_that_are_no_multiple_of_four(V):
    """1 000 is a multiple of 4 and takes the 16-byte loads; these widths (and a base that is not 16-byte aligned, below) take the
    element-wise path."""
    if V > 16:
        reps, m = _small_rows(V=V), 16
    else:
        reps, m = np.array([[1.0, 1.0, 1.0], [0.0, 2.0, 1.0], [-0.0, -1.0, 0.5], [0.0, 0.0, 0.0]], np.float32)[:, :V].copy(), min(V, 2)
    rc, n, *got = compact_topm(torch.from_numpy(reps).cuda(), m)
    assert rc == 0
    assert_same_csr(got, topm_reference(reps, m), V)


def test_unaligned_base(small):
    reps, _ = small
    flat = torch.zeros(reps.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(reps.reshape(-1).copy()).cuda()
    view = flat[1:].view(reps.shape)
    assert view.data_ptr() % 16 == 4
    rc, n, *got = compact_topm(view, 16)
    assert rc == 0
    assert_same_csr(got, topm_reference(reps, 16), "unaligned")


# ------------------------------------------------------------------ 2. production width
@pytest.mark.parametrize("m", [1, 256, 4096, V_PROD, V_PROD + 5])
def test_production_width(prod, m):
    reps, reps_t = prod
    want = topm_reference(reps, m)
    assert np.array_equal(np.diff(want[0]), np.minimum(m, (100_000, 3_000, 40)))
    rc, n, *got = compact_topm(reps_t, m)
    assert rc == 0 and n == want[0][-1]
    assert_same_csr(got, want, m)


# ------------------------------------------------------------------ 3. no budget = sr_sparse_compact
@pytest.mark.parametrize("which", ["small", "prod"])
def test_budget_zero_is_sparse_compact(small, prod, which):
    reps, reps_t = small if which == "small" else prod
    rc, n, *got = compact_topm(reps_t, 0)
    assert rc == 0
    want = compact_all(reps_t)
    assert n == len(want[1])
    assert_same_csr(got, want, which)
    assert_same_csr(got, topm_reference(reps, 0), which)


# ------------------------------------------------------------------ 4. capacity
def test_capacity_and_empty_batch(small):
    from scaling_retriever_amd import _lib
    reps, reps_t = small
    want = topm_reference(reps, 16)
    need = int(want[0][-1])
    rc, n, *_ = compact_topm(reps_t, 16, capacity=need - 1)
    assert rc == _lib.SR_ERR_NOMEM and n == need
    rc, n, *got = compact_topm(reps_t, 16, capacity=n)
    assert rc == 0 and n == need
    assert_same_csr(got, want, "exact capacity")
    lib = _lib.load()
    n0 = ctypes.c_int64(-1)
    row_ptr = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert lib.sr_sparse_compact_topm(reps_t.data_ptr(), 0, 1000, 16, row_ptr.data_ptr(), None, None, 0, ctypes.byref(n0),
                                      _lib.stream_ptr()) == 0
    assert n0.value == 0


def test_sparse_reps_to_csr_budget(small):
    from scaling_retriever_amd.indexer import sparse_reps_to_csr
    reps, reps_t = small
    got = [x.cpu().numpy() for x in sparse_reps_to_csr(reps_t, max_terms=16)]
    assert_same_csr(got, topm_reference(reps, 16), "sparse_reps_to_csr")
    with pytest.raises(ValueError, match="max_terms"):
        sparse_reps_to_csr(reps_t, max_terms=-1)


# ------------------------------------------------------------------ 5. end to end on the tiny golden model
class FakeLoader:
    """Stands in for DataLoader(collate_fn=LlamaSparseCollectionCollator): yields {"input_ids", "attention_mask", "ids"} with
    left padding to the longest row (as tests/test_indexer_gpu.py's)."""

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


DOC_TERMS, QUERY_TERMS, TOPK = 8, 4, 10


@pytest.fixture(scope="module")
def e2e(golden_dir):
    """Model, loaders, the full representations from the model's own encode, and their numpy-pruned versions."""
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    V = cfg["vocab_size"]
    rng = np.random.default_rng(3)
    docs = [rng.integers(0, V - 1, size=int(rng.integers(1, 7))) for _ in range(70)]
    queries = [rng.integers(0, V - 1, size=int(rng.integers(1, 4))) for _ in range(9)]
    pids, qids = [f"p{i}" for i in range(70)], [f"q{i}" for i in range(9)]
    model = LlamaBiSparse.from_weights(cfg, w, precision="bf16").to("cuda").eval()
    d_loader = lambda: FakeLoader(docs, pids, batch_size=8, pad_id=V - 1)          # noqa: E731
    q_loader = lambda: FakeLoader(queries, qids, batch_size=4, pad_id=V - 1)       # noqa: E731

    def encode(loader):
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):
            return np.concatenate([model.encode(input_ids=b["input_ids"].cuda(), attention_mask=b["attention_mask"].cuda()).float().cpu().numpy()
                                   for b in loader])
    d_reps, q_reps = encode(d_loader()), encode(q_loader())
    assert ((d_reps != 0).sum(1) > DOC_TERMS).mean() >= 0.5 and ((q_reps != 0).sum(1) > QUERY_TERMS).mean() >= 0.5
    return dict(model=model, V=V, pids=pids, qids=qids, d_loader=d_loader, q_loader=q_loader,
                d_pruned=prune_dense(d_reps, DOC_TERMS), q_pruned=topm_reference(q_reps, QUERY_TERMS))


def _index(e2e, **kw):
    from scaling_retriever_amd.indexer import SparseIndexer
    indexer = SparseIndexer(e2e["model"], index_dir=None, compute_stats=True, dim_voc=e2e["V"], device="cuda", **kw)
    return indexer, indexer.index(e2e["d_loader"]())


def test_indexer_with_doc_budget(e2e):
    indexer, out = _index(e2e, doc_max_terms=DOC_TERMS)
    P, V = e2e["d_pruned"], e2e["V"]
    indptr, doc_ids, vals = out["index"].csr(V)
    want_docs = [np.flatnonzero(P[:, t]) for t in range(V)]
    assert np.array_equal(indptr, np.concatenate([[0], np.cumsum([len(d) for d in want_docs])]))
    assert np.array_equal(doc_ids, np.concatenate(want_docs).astype(np.int32))
    assert np.array_equal(vals.view(np.int32), np.concatenate([P[d, t] for t, d in enumerate(want_docs)]).view(np.int32))
    assert out["ids_mapping"] == {i: p for i, p in enumerate(e2e["pids"]) if P[i].any()}
    assert out["stats"]["L0_d_kept"] == pytest.approx(np.mean([(P[i:i + 8] != 0).sum(1).mean() for i in range(0, 70, 8)]), rel=1e-6)
    assert out["stats"]["L0_d"] > out["stats"]["L0_d_kept"]              # L0_d stays the full representation's


@pytest.mark.parametrize("piecewise", [False, True])
def test_retrieval_with_query_budget(e2e, tmp_path, piecewise):
    from scaling_retriever_amd.indexer import SparseRetrieval
    _, out = _index(e2e, doc_max_terms=DOC_TERMS)
    retr = SparseRetrieval(config={"out_dir": str(tmp_path)}, model=e2e["model"], dim_voc=e2e["V"], device="cuda", index_d=out,
                           compute_stats=True, query_max_terms=QUERY_TERMS)
    if piecewise:
        retr.QUERY_GROUP_ROWS = 4                  # 9 queries in loader batches of 4: three groups, the piecewise branch
    res = retr.retrieve(e2e["q_loader"](), topk=TOPK, threshold=0.0)
    row_ptr, cols, vals = e2e["q_pruned"]
    s, i, c = retr.hip_index.search(row_ptr, cols, vals, TOPK, threshold=0.0)
    s, i, c = s.cpu().numpy(), i.cpu().numpy(), c.cpu().numpy()
    want = {}
    for q, qid in enumerate(e2e["qids"]):
        if c[q]:
            want[qid] = {out["ids_mapping"][int(d)]: float(sc) for d, sc in zip(i[q, :c[q]], s[q, :c[q]])}
    assert len(want) == 9 and res.to_dict() == want
    assert json.load(open(tmp_path / "run.json")) == want
    assert json.load(open(tmp_path / "q_stats.json"))["L0_q"] == pytest.approx(len(cols) / 9)      # the kept terms


def test_zero_budgets_change_nothing(e2e, tmp_path):
    from scaling_retriever_amd.indexer import SparseRetrieval
    runs = []
    for name, ikw, rkw in (("plain", {}, {}), ("zero", {"doc_max_terms": 0}, {"query_max_terms": 0})):
        indexer, out = _index(e2e, **ikw)
        retr = SparseRetrieval(config={"out_dir": str(tmp_path / name)}, model=e2e["model"], dim_voc=e2e["V"], device="cuda",
                               index_d=out, compute_stats=True, **rkw)
        assert indexer.doc_max_terms == 0 and retr.query_max_terms == 0
        assert "L0_d_kept" not in out["stats"]
        retr.retrieve(e2e["q_loader"](), topk=TOPK, threshold=0.0)
        runs.append((open(tmp_path / name / "run.json", "rb").read(), open(tmp_path / name / "q_stats.json", "rb").read(),
                     [x.tobytes() for x in out["index"].csr(e2e["V"])]))
    assert runs[0] == runs[1] and len(runs[0][0]) > 100
