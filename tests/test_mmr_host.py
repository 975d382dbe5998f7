"""CPU: the numpy model of sr_dense_mmr against its own invariants (tests/mmr_cases.py), the argument rules of the MMR
entry points, and the eval driver's flag conflicts.  The GPU side is tests/test_mmr_gpu.py."""
import os
import sys

import numpy as np
import pytest

import mmr_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _random_case(seed, N=120, H=80, nq=3, n=50):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((N, H)).astype(F32)
    ids = np.stack([rng.choice(N, size=n, replace=False) for _ in range(nq)]).astype(np.int64)
    rel = rng.standard_normal((nq, n)).astype(F32)
    return rows, ids, rel


def test_lambda_one_returns_the_sorted_prefix():
    rows, ids, rel = _random_case(1)
    rel[0, 7] = rel[0, 3]                                         # a tie in rel: the smaller id first
    rel[1, 5], rel[1, 9] = F32(0.0), F32(-0.0)                    # -0.0 == +0.0: the id decides, the bits stay
    sim = M.similarities(rows)
    k = 20
    got = M.mmr(sim, lambda d: d, ids, rel, k, 1.0)
    for q in range(ids.shape[0]):
        order = np.lexsort((np.arange(ids.shape[1]), ids[q], -rel[q].astype(np.float64)))[:k]
        assert np.array_equal(got[3][q], order) and np.array_equal(got[0][q], ids[q, order])
        assert np.array_equal(M.bits(got[1][q]), M.bits(rel[q, order]))
        assert np.array_equal(M.bits(got[2][q]), M.bits(rel[q, order]))           # mu = 0: v = f32(1 * rel) - 0
    assert got[4].tolist() == [k] * ids.shape[0]


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7])
def test_marginal_values_never_increase_from_pick_one(lam):
    rows, ids, rel = _random_case(2)
    info = {}
    got = M.mmr(M.similarities(rows), lambda d: d, ids, rel, ids.shape[1], lam, info=info)
    assert got[4].tolist() == [ids.shape[1]] * ids.shape[0]
    assert (np.diff(got[2][:, 1:], axis=1) <= 0).all()
    assert sorted(got[3][0].tolist()) == list(range(ids.shape[1]))               # every candidate exactly once
    assert info["below_first"] > 0                # random rows: some similarity to pick 0 is negative, pick 1 then lies above pick 0


def test_hand_worked_six_candidates():
    """Six rows of small integers (every product and sum exact), lambda = 0.5.  Row 1 = -row 0: its similarity to pick 0 is -4, so its
    marginal value 0.5 * 0.9 + 0.5 * 4 lies ABOVE pick 0's 0.5 * 1.0 - the one place the sequence may rise."""
    rows = np.zeros((6, 16), F32)
    rows[0, 0], rows[1, 0], rows[2, 0] = 2, -2, 2
    rows[3, 1] = 1
    rows[4, 0], rows[4, 1] = 1, 1
    rows[5, 2] = 3
    rel = np.array([[1.0, 0.9, 0.95, 0.5, 0.8, 0.1]], F32)
    ids = np.arange(6, dtype=np.int64)[None]
    sim = M.similarities(rows)
    assert sim[1, 0] == -4 and sim[2, 0] == 4 and sim[4, 0] == 2 and sim[4, 3] == 1 and sim[2, 4] == 2 and sim[5, 5] == 9
    got = M.mmr(sim, lambda d: d, ids, rel, 6, 0.5)
    half = F32(0.5)
    lr = [F32(half * r) for r in rel[0]]
    # pick 0 by rel: 0.  Then m = (.., -4, 4, 0, 2, 0): v = (2.45, -1.525, 0.25, -0.6, 0.05) -> 1; nothing changes the maxima of the rest
    # later (row 4 meets row 3 at 1 < 2, row 2 meets row 4 at 2 < 4): 3, 5, 4, 2 follow by their values
    want_v = [lr[0], F32(lr[1] - F32(half * F32(-4))), F32(lr[3] - F32(0)), F32(lr[5] - F32(0)), F32(lr[4] - F32(half * F32(2))),
              F32(lr[2] - F32(half * F32(4)))]
    assert got[0][0].tolist() == [0, 1, 3, 5, 4, 2] and got[3][0].tolist() == [0, 1, 3, 5, 4, 2]
    assert np.array_equal(M.bits(got[2][0]), M.bits(np.array(want_v, F32)))
    assert np.array_equal(M.bits(got[1][0]), M.bits(rel[0, [0, 1, 3, 5, 4, 2]]))
    assert got[2][0, 1] > got[2][0, 0] and (np.diff(got[2][0, 1:]) <= 0).all()
    # k beyond the valid count, padding ids and a prefix: three candidates (entries 0, 2, 4 of the first five), the rest is padding
    ids2 = ids.copy()
    ids2[0, 1] = ids2[0, 3] = -1
    got = M.mmr(sim, lambda d: d, ids2, rel, 6, 0.5, counts=np.array([5]))
    assert got[4].tolist() == [3] and got[0][0].tolist() == [0, 4, 2, -1, -1, -1] and got[3][0].tolist() == [0, 4, 2, -1, -1, -1]
    assert np.array_equal(M.bits(got[2][0, 3:]), M.bits(np.full(3, -M.FLT_MAX, F32))) and np.array_equal(M.bits(got[1][0, 3:]), M.bits(got[2][0, 3:]))
    with pytest.raises(ValueError, match=r"id 77 \(query 0, entry 1\)"):
        ids2[0, 1] = 77
        M.mmr(sim, lambda d: d if d < 6 else None, ids2, rel, 6, 0.5)


def test_the_chain_order_shows_in_the_result():
    """The natural k order gives other similarity bits than the exact kernel's order, and on these inputs other marginal values:
    a kernel that accumulated in the wrong order cannot pass the GPU tests."""
    rows, ids, rel = _random_case(3, H=192)
    a = M.mmr(M.similarities(rows), lambda d: d, ids, rel, 10, 0.3)
    b = M.mmr(M.similarities(rows, np.arange(192, dtype=np.int32)), lambda d: d, ids, rel, 10, 0.3)
    assert not np.array_equal(M.bits(a[2]), M.bits(b[2])) or not np.array_equal(a[0], b[0])
    # and the model's similarity is symmetric (the products commute), fp16 storage rounds the rows first
    s = M.similarities(M.stored(rows, "fp16"))
    assert np.array_equal(M.bits(s), M.bits(s.T)) and not np.array_equal(M.bits(s), M.bits(M.similarities(rows)))


def test_argument_rules():
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.mmr import mmr_arguments
    cap = _lib.load().sr_mmr_max_candidates()
    assert cap >= 1024
    mmr_arguments("search_mmr", 10, 128, 0.5)
    mmr_arguments("search_mmr", cap, cap, 1.0, subset=[1, 2])
    with pytest.raises(ValueError, match="k = 11 must lie in"):
        mmr_arguments("search_mmr", 11, 10, 0.5)
    with pytest.raises(ValueError, match="k = 0 must lie in"):
        mmr_arguments("search_mmr", 0, 10, 0.5)
    with pytest.raises(ValueError, match=f"sr_mmr_max_candidates\\(\\) = {cap}"):
        mmr_arguments("search_mmr", 10, cap + 1, 0.5)
    for lam in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="must lie in \\[0, 1\\]"):
            mmr_arguments("search_mmr", 10, 128, lam)
    with pytest.raises(ValueError, match="not both"):
        mmr_arguments("search_mmr", 10, 128, 0.5, subset=[1], mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="not both"):
        mmr_arguments("search_mmr", 10, 128, 0.5, np.ones((1, 4), bool), [0], mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="go together"):
        mmr_arguments("search_mmr", 10, 128, 0.5, np.ones((1, 4), bool), None)
    # the C entry checks the same before any device work: the pointers below are never dereferenced
    import ctypes
    lib, p = _lib.load(), ctypes.c_void_p(4096)
    for n, k, lam, text in [(cap + 1, 1, 0.5, b"sr_mmr_max_candidates"), (0, 1, 0.5, b"candidates per query"), (8, 0, 0.5, b"k = 0"),
                            (8, 4, 1.5, b"lambda"), (8, 4, -0.5, b"lambda")]:
        rc = lib.sr_dense_mmr(p, p, p, None, 1, n, k, lam, p, p, p, p, p, None)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (n, k, lam, lib.sr_last_error())
    assert lib.sr_dense_mmr(None, p, p, None, 1, 8, 4, 0.5, p, p, p, p, p, None) == _lib.SR_ERR_INVALID
    assert lib.sr_dense_mmr(p, p, p, None, 0, 8, 4, 0.5, p, p, p, p, p, None) == _lib.SR_OK


def test_sharded_retriever_refuses():
    from scaling_retriever_amd.distributed import ShardedDenseRetriever
    with pytest.raises(NotImplementedError, match="doc-sharded"):
        ShardedDenseRetriever.search_mmr(None)


def test_eval_dense_flag_conflicts(capsys):
    sys.path.insert(0, ROOT)
    import eval_dense
    base = ["--task_name", "retrieval", "--top_k", "10"]
    a = eval_dense.parse_args(base + ["--mmr_lambda", "0.5", "--mmr_fetch_k", "40"])
    assert a.mmr_lambda == 0.5 and a.mmr_fetch_k == 40
    assert eval_dense.parse_args(base).mmr_lambda is None
    for extra, text in [(["--mmr_lambda", "0.5", "--mmr_fetch_k", "40", "--collapse_file", "x.tsv"], "--collapse_file"),
                        (["--mmr_lambda", "1.5", "--mmr_fetch_k", "40"], "[0, 1]"),
                        (["--mmr_lambda", "0.5", "--mmr_fetch_k", "5"], "--mmr_fetch_k >= top_k"),
                        (["--mmr_lambda", "0.5"], "--mmr_fetch_k >= top_k"),
                        (["--mmr_fetch_k", "40"], "needs --mmr_lambda")]:
        with pytest.raises(SystemExit):
            eval_dense.parse_args(base + extra)
        assert text in capsys.readouterr().err, extra
    a.world_size = 2                                              # the doc-sharded retrieval: refused before anything is loaded
    with pytest.raises(NotImplementedError, match="--mmr_lambda"):
        eval_dense.retrieval(a)
