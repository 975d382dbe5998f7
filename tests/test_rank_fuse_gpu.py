"""GPU: rank fusion on the device (scoring.rank_fuse over csrc/rank_fuse.hip, fusion.py, HybridRetriever.retrieve_rank_fused,
eval_fuse.py).  Every comparison is for equal bits (uint32 / int64) against the numpy model of tests/rank_fuse_cases.py."""
import json
import os

import numpy as np
import pytest
import torch

import rank_fuse_cases as R
from test_hybrid_search_gpu import _retriever, toy  # noqa: F401  (toy: the module-scoped fixture of the toy hybrid retriever)
from test_rank_fuse_host import _eval_fuse, expected_run, three_runs

pytestmark = pytest.mark.gpu
F32 = np.float32


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fuse(ids, k, counts=None, scores=None, **kw):
    from scaling_retriever_amd import scoring
    out = scoring.rank_fuse(_cuda(ids), k, counts=_cuda(counts), scores=_cuda(scores), return_ranks=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check(ids, k, counts=None, scores=None, **kw):
    """The device result equals the model's: score bits, ids, counts, ranks.  Returns the model's result."""
    got = _fuse(ids, k, counts, scores, **kw)
    want = R.rank_fuse(ids, k, counts=counts, scores=scores, **kw)
    assert got[2].dtype == np.int32 and got[3].dtype == np.int32 and got[1].dtype == np.int64
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(R.bits(got[0]), R.bits(want[0]))
    assert np.array_equal(got[3], want[3])
    return want


def draw_lists(rng, L, nq, depth, n_docs):
    """ids int64 [L, nq, depth]: every row drawn without replacement from n_docs documents."""
    return np.stack([np.stack([rng.choice(n_docs, size=depth, replace=False) for _ in range(nq)]) for _ in range(L)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------- 1: small lists ---
def small_case():
    rng = np.random.default_rng(1)
    ids = draw_lists(rng, 2, 5, 8, 40)
    ids[1, 0] = ids[0, 0][::-1]                             # full overlap
    ids[0, 1], ids[1, 1] = np.arange(8), np.arange(20, 28)  # disjoint lists
    ids[0, 2, 3] = -1                                       # padding in the middle of list 0
    ids[0, 2, 5] = -1
    counts = np.full((2, 5), 8, np.int32)
    counts[0, 3], counts[1, 3] = 5, 2                       # counts shorter than depth
    counts[:, 4] = 0                                        # empty in both lists
    return ids, counts


@pytest.mark.parametrize("k", [8, 20])
def test_small_rectangular_lists(k):
    ids, counts = small_case()
    s, i, n, r = _check(ids, k, counts=counts)
    assert n.tolist()[0] == 8 and n[4] == 0 and (i[4] == -1).all() and (R.bits(s[4]) == R.bits(-R.FLT_MAX)).all() and (r[4] == 0).all()
    if k == 20:                                             # more than the distinct documents: padding and counts
        assert n[1] == 16 and (n < 20).all() and (i[1, 16:] == -1).all()
    # ids without counts: a row ends nowhere, every non-negative id counts
    _check(ids, k)


# ----------------------------------------------------------------------------------- 2: order of the sum, ties ---
def test_order_of_the_sum_and_the_id_tie_rule():
    ids = draw_lists(np.random.default_rng(0), 3, 4, 50, 120)
    s, i, n, _ = _check(ids, 40, weights=(1.0, 1.0, 1.0))
    ties = sum(int(s[q, j] == s[q, j + 1]) for q in range(4) for j in range(n[q] - 1))
    assert ties >= 1                                        # the inputs exercise the id tie rule
    w = (0.3, 1.7, 0.9)
    s, i, n, _ = _check(ids, 40, weights=w)
    full = R.rank_fuse(ids, 120, weights=w)
    rev = R.rank_fuse(ids, 120, weights=w, order=(2, 1, 0))
    by_id = lambda res: {(q, int(d)): x for q in range(4) for d, x in zip(res[1][q], R.bits(res[0][q])) if d >= 0}    # noqa: E731
    a, b = by_id(full), by_id(rev)
    assert a.keys() == b.keys() and any(a[key] != b[key] for key in a)     # a wrong add order cannot pass


# The slots of the two sorts are the next power of two >= L * depth, sorted by 256 threads: beside 64 and 128, a single pair (2), one pair
# per thread (512) and two (1024); test_order_of_the_sum has 256 (fewer pairs than threads), test_at_the_limit the 8192 of the cap.
@pytest.mark.parametrize("L,depth", [pytest.param(4, 16, id="4"), pytest.param(8, 16, id="8"), pytest.param(2, 1, id="slots2"),
                                     pytest.param(2, 256, id="slots512"), pytest.param(2, 512, id="slots1024")])
def test_more_lists(L, depth):
    ids = draw_lists(np.random.default_rng(L), L, 3, depth, depth * 5 // 2)
    w = tuple(0.25 + 0.35 * l for l in range(L))
    _check(ids, 30, weights=w, c=0.5)
    sc = -np.sort(-np.random.default_rng(L + 1).standard_normal(ids.shape).astype(F32), axis=2)
    _check(ids, 30, scores=sc, weights=w, method="minmax")


# ------------------------------------------------------------------------------------------------ 3: the limit ---
def test_at_the_limit():
    from scaling_retriever_amd import _lib
    rng = np.random.default_rng(3)
    ids = draw_lists(rng, 2, 3, 4096, 6000)
    ids[0, 1, rng.choice(4096, size=100, replace=False)] = -1
    counts = np.full((2, 3), 4096, np.int32)
    counts[1, 1] = 4095
    s, i, n, _ = _check(ids, 4096, counts=counts, weights=(0.3, 1.7))
    assert (n == 4096).all()
    ids8 = draw_lists(rng, 8, 2, 1024, 3000)
    _check(ids8, 1000, weights=tuple(1.0 + 0.125 * l for l in range(8)))
    for bad_ids, k in ((np.zeros((2, 1, 4097), np.int64), 10), (np.zeros((8, 1, 1025), np.int64), 10), (np.zeros((2, 1, 8), np.int64), 4097)):
        with pytest.raises(_lib.SrHipError, match="sr_rank_fuse"):
            _fuse(bad_ids, k)


# -------------------------------------------------------------------------------------------------- 4: min-max ---
def minmax_case():
    rng = np.random.default_rng(4)
    ids = draw_lists(rng, 3, 6, 32, 80)
    sc = -np.sort(-rng.standard_normal(ids.shape).astype(F32), axis=2)
    counts = np.full((3, 6), 32, np.int32)
    sc[1, 0] = F32(0.75)                                    # a list whose valid scores are all equal: norm = 1.0
    counts[2, 1] = 1                                        # a list with a single valid entry
    sc[:, 2] = -np.sort(np.abs(sc[:, 2]), axis=1) - F32(0.5)   # negative scores only (descending)
    sc[0, 3, int(np.argmax(sc[0, 3] < 0))] = F32(-0.0)      # a -0.0f at the sign change of a descending row
    ids[0, 4, 7] = -1                                       # a pad inside a row: not part of min / max
    sc[0, 4, 7] = F32(1e30)
    return ids, sc, counts


def test_minmax():
    ids, sc, counts = minmax_case()
    assert np.signbit(sc[0, 3]).any() and (sc[0, 3] == 0).any() and (sc[:, 2] < 0).all()
    w = (0.3, 1.7, 0.9)
    want = _check(ids, 60, counts=counts, scores=sc, method="minmax", weights=w)
    once = R.rank_fuse_f64(ids, 60, counts=counts, scores=sc, method="minmax", weights=w)
    full = R.rank_fuse(ids, 80, counts=counts, scores=sc, method="minmax", weights=w)
    differ = sum(int(R.bits(full[0][q, j]).item() != R.bits(once[(q, int(full[1][q, j]))]).item()) for q in range(6) for j in range(full[2][q]))
    assert differ >= 1                                      # a contracted prev + w * norm would show in these inputs
    assert want[2].max() > 32
    _check(ids, 10, counts=counts, scores=sc, method="minmax")


# ----------------------------------------------------------------------------------------- 5: a weight-0 list ---
def test_a_list_of_weight_zero_still_brings_its_documents():
    ids = draw_lists(np.random.default_rng(6), 2, 3, 12, 30)
    s, i, n, r = _check(ids, 24, weights=(1.0, 0.0))
    for q in range(3):
        only = sorted(set(ids[1, q].tolist()) - set(ids[0, q].tolist()))
        assert only and i[q, 12:n[q]].tolist() == only and (R.bits(s[q, 12:n[q]]) == 0).all() and (s[q, :12] > 0).all()


# ----------------------------------------------------------------------------- 6: errors found on the device ---
def test_errors_found_on_the_device_leave_the_library_usable():
    ids = draw_lists(np.random.default_rng(7), 2, 4, 10, 50)
    bad = ids.copy()
    bad[1, 2, 7] = bad[1, 2, 3]
    with pytest.raises(ValueError, match=rf"id {bad[1, 2, 3]} \(list 1, query 2, entry [37]\).*twice"):
        _fuse(bad, 5)
    counts = np.full((2, 4), 10, np.int32)
    counts[1, 2] = 7                                        # the repeat lies beyond the row's count: not an error
    _check(bad, 5, counts=counts)
    big = ids.copy()
    big[0, 3, 4] = 1 << 32
    with pytest.raises(ValueError, match=rf"id {1 << 32} \(list 0, query 3, entry 4\)"):
        _fuse(big, 5)
    big[0, 3, 4] = (1 << 32) - 1                            # the largest id a key holds
    _check(big, 20)
    _check(ids, 5)


# --------------------------------------------------------------------------------------------- 7: determinism ---
def test_two_calls_and_another_stream_return_the_same_bytes():
    from scaling_retriever_amd import scoring
    ids, sc, counts = minmax_case()
    args = (_cuda(ids), 40)
    kw = dict(counts=_cuda(counts), scores=_cuda(sc), method="minmax", weights=(0.3, 1.7, 0.9), return_ranks=True)
    first = scoring.rank_fuse(*args, **kw)
    second = scoring.rank_fuse(*args, **kw)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        third = scoring.rank_fuse(*args, **kw)
    stream.synchronize()
    for a, b, c in zip(first, second, third):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------- 8: retrieve_rank_fused ---
def _model_run(ret, sparse_res, dense_res, method, weights, k):
    """The model applied to the two returned runs in tie space -> {qid: ([db ids], fp32 scores)}."""
    d2s, s2d = (t.cpu().numpy() for t in ret._position_maps())
    n_s2d = len(s2d)
    dp, sp = dense_res.positions, sparse_res.positions
    tie_d = np.where(dp < 0, -1, np.where(d2s[np.maximum(dp, 0)] >= 0, d2s[np.maximum(dp, 0)], n_s2d + dp))
    cols = np.arange(sp.shape[1])[None, :] < sparse_res.counts[:, None]
    tie_s = np.where(cols & (sp >= 0), sp, -1)
    assert tie_d.shape == tie_s.shape
    s, i, n, _ = R.rank_fuse(np.stack([tie_d, tie_s]), k, scores=np.stack([dense_res.scores, sparse_res.scores]), method=method, weights=weights)
    db = ret.dense_index.index_id_to_db_id
    out = {}
    for q in range(len(n)):
        back = [int(s2d[t]) if t < n_s2d else int(t - n_s2d) for t in i[q, :n[q]]]
        out[dense_res.qids.key(q)] = ([str(db[p]) for p in back], s[q, :n[q]])
    return out


def _same_run(path, want):
    run = json.load(open(path))
    assert set(run) == {q for q, (docs, _) in want.items() if docs}
    for q, row in run.items():
        assert list(row) == want[q][0], q
        assert np.array_equal(R.bits(np.array(list(row.values()), F32)), R.bits(want[q][1])), q
    return run


@pytest.fixture(scope="module")
def partial(toy):    # noqa: F811
    """The toy hybrid retriever with an inverted index over three quarters of its corpus: every fourth document of the dense index
    has no posting, and the two indexes number the rest differently."""
    from fake_tokenizer import FakeTokenizer
    from torch.utils.data import DataLoader
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    from scaling_retriever_amd.indexer import HybridIndexer
    from test_pipeline import ListDataset, _corpus
    hyb, _, de_dir, q_loader, tmp = toy
    docs = ListDataset([d for n, d in enumerate(_corpus(90, seed=1, max_words=20)) if n % 4 != 1])
    collate = LlamaSparseCollectionCollator(FakeTokenizer(vocab_size=hyb.vocab_size, padding_side="left"), 24)
    sp_dir = str(tmp / "sp_partial")
    HybridIndexer(hyb, sp_dir, str(tmp / "de_partial"), device="cuda", chunk_size=40, compute_stats=True,
                  dim_voc=hyb.vocab_size).index(DataLoader(docs, batch_size=16, shuffle=False, collate_fn=collate))
    return hyb, sp_dir, de_dir, q_loader, tmp


def test_retrieve_rank_fused_through_the_toy_model(partial):
    toy = partial    # noqa: F811
    k = 10
    ret_a, out_a = _retriever(toy, "rf_a")
    _, dense_res = ret_a.retrieve(toy[3](), topk=k)
    ret, out = _retriever(toy, "rf_b")
    d2s = ret._position_maps()[0]
    assert int((d2s < 0).sum()) == 23 and int(d2s.numel()) == 90           # documents without a posting
    assert bool((d2s.cpu().numpy()[dense_res.positions[dense_res.positions >= 0]] < 0).any())      # and the dense lists hold some
    for method, w in (("rrf", (1.0, 1.0)), ("minmax", (0.7, 1.3))):
        sparse_res, dense_res, fused_res = ret.retrieve_rank_fused(toy[3](), k, method=method, weights=w)
        for head, name in (("sparse", "run.json"), ("sparse", "q_stats.json"), ("dense", "run.json")):
            assert open(os.path.join(out_a, head, name), "rb").read() == open(os.path.join(out, head, name), "rb").read(), (head, name)
        run = _same_run(os.path.join(out, "rank_fused", "run.json"), _model_run(ret, sparse_res, dense_res, method, w, k))
        assert run == {q: dict(r) for q, r in fused_res.items()} and len(run) == 8
    # fused_topk cuts the run
    sparse_res, dense_res, fused_res = ret.retrieve_rank_fused(toy[3](), k, fused_topk=3)
    run = _same_run(os.path.join(out, "rank_fused", "run.json"), _model_run(ret, sparse_res, dense_res, "rrf", (1.0, 1.0), 3))
    assert all(len(r) == 3 for r in run.values())
    # under allowed_ids, and under allowed_masks + query_group
    db_ids = list(ret.dense_index.index_id_to_db_id)
    allowed = db_ids[0::2]
    sparse_res, dense_res, _ = ret.retrieve_rank_fused(toy[3](), k, allowed_ids=allowed)
    run = _same_run(os.path.join(out, "rank_fused", "run.json"), _model_run(ret, sparse_res, dense_res, "rrf", (1.0, 1.0), k))
    assert all(set(r) <= {str(d) for d in allowed} for r in run.values())
    groups = [db_ids[0::2], db_ids[5:40], db_ids[80:]]
    flags, grp = np.stack([ret.allowed_mask(g) for g in groups]), np.array([0, 1, 2, 1, 0, 2, 1, 0])
    sparse_res, dense_res, _ = ret.retrieve_rank_fused(toy[3](), k, method="minmax", allowed_masks=flags, query_group=grp)
    run = _same_run(os.path.join(out, "rank_fused", "run.json"), _model_run(ret, sparse_res, dense_res, "minmax", (1.0, 1.0), k))
    for q, g in enumerate(grp):
        assert set(run.get(f"q{q}", {})) <= {str(d) for d in groups[g]}
    with pytest.raises(NotImplementedError, match="collapse"):
        ret.retrieve_rank_fused(toy[3](), k, collapse={d: "g" for d in db_ids})


# ------------------------------------------------------------------------------------------------ 9: eval_fuse ---
def test_eval_fuse_end_to_end(tmp_path):
    E = _eval_fuse()
    runs = three_runs()
    paths = []
    for l, run in enumerate(runs):
        os.makedirs(tmp_path / f"r{l}")
        paths.append(str(tmp_path / f"r{l}" / "run.json"))
        with open(paths[-1], "w") as f:
            json.dump(run, f)
    for method, weights in (("rrf", "1,1,1"), ("minmax", "0.3,1.7,0.9")):
        out = tmp_path / f"out_{method}"
        res = E.main(["--run_paths", ",".join(paths), "--output_dir", str(out), "--method", method, "--weights", weights, "--topk", "6"])
        got = json.load(open(out / "run.json"))
        want = expected_run(runs, method, tuple(float(x) for x in weights.split(",")), 60.0, 6)
        assert got == want and res == want and [list(got[q]) for q in got] == [list(want[q]) for q in want]
