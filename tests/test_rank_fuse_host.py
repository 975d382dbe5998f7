"""CPU: sr_rank_fuse's symbol, the argument checks that must come before any device work, the numpy model (tests/rank_fuse_cases.py)
against a hand-computed case, eval_fuse.py without a GPU (the library call monkeypatched to the model), and fusion.py's tie maps."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import rank_fuse_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _eval_fuse():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval_fuse
    return eval_fuse


def test_new_symbol_is_declared_exported_and_bound():
    from scaling_retriever_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    name = "sr_rank_fuse"
    assert re.search(rf"\b{name}\s*\(", src), name
    assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r"#define\s+SR_FUSE_RRF\s+0\b", src) and re.search(r"#define\s+SR_FUSE_MINMAX\s+1\b", src)
    assert (_lib.SR_FUSE_RRF, _lib.SR_FUSE_MINMAX) == (0, 1)
    from scaling_retriever_amd import fusion, scoring
    from scaling_retriever_amd.indexer import HybridRetriever
    assert callable(scoring.rank_fuse) and callable(fusion.fuse_hybrid_lists) and callable(HybridRetriever.retrieve_rank_fused)


def test_entry_point_validates_before_it_touches_a_device():
    """The device pointers below are never dereferenced; the weights are a host array."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    K = lib.sr_max_topk()

    def fuse(**kw):
        a = dict(dict(ids=p, counts=None, scores=p, L=2, nq=1, depth=8, method=0, w=(1.0,) * 8, c=60.0, k=8, os=p, oi=p, oc=p, ranks=None), **kw)
        w = None if a["w"] is None else (ctypes.c_float * len(a["w"]))(*a["w"])
        return lib.sr_rank_fuse(a["ids"], a["counts"], a["scores"], a["L"], a["nq"], a["depth"], a["method"], w, a["c"], a["k"], a["os"], a["oi"],
                                a["oc"], a["ranks"], None)
    invalid = [dict(nq=-1), dict(nq=1 << 30), dict(ids=None), dict(os=None), dict(oi=None), dict(oc=None), dict(w=None), dict(w=(-1.0, 1.0)),
               dict(w=(1.0, float("nan"))), dict(w=(float("inf"), 1.0)), dict(c=-1.0), dict(c=-2.0), dict(c=float("nan")), dict(c=float("inf")),
               dict(method=1, scores=None), dict(method=2), dict(method=-1)]
    for change in invalid:
        rc = fuse(**change)
        assert rc == _lib.SR_ERR_INVALID and b"sr_rank_fuse" in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    unsupported = [dict(L=0), dict(L=9), dict(depth=0), dict(depth=K + 1), dict(L=8, depth=K // 4 + 1), dict(L=3, depth=K), dict(k=0),
                   dict(k=K + 1)]
    for change in unsupported:
        rc = fuse(**change)
        assert rc == _lib.SR_ERR_UNSUPPORTED and b"sr_rank_fuse" in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    # legal shapes at the limits, and nq = 0
    for change in [dict(nq=0), dict(nq=0, L=2, depth=K, k=K), dict(nq=0, L=8, depth=K // 4), dict(nq=0, method=1), dict(nq=0, c=-0.5),
                   dict(nq=0, scores=None), dict(nq=0, w=(0.0, 0.0))]:
        assert fuse(**change) == _lib.SR_OK, (change, lib.sr_last_error())


def test_rank_fuse_raises_value_errors_before_the_library_is_asked_for_a_device(monkeypatch):
    from scaling_retriever_amd import _lib, fusion, scoring
    from scaling_retriever_amd.indexer import HybridRetriever

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    ids = torch.zeros((2, 3, 4), dtype=torch.int64)
    sc = torch.zeros((2, 3, 4))
    bad = [dict(k=0), dict(k=-1), dict(k=2.5), dict(k="ten"), dict(method="sum"), dict(weights=(1.0,)), dict(weights=(1.0, -1.0)),
           dict(weights=(float("nan"), 1.0)), dict(weights=(float("inf"), 1.0)), dict(weights=("a", 1.0)), dict(c=-1.0), dict(c=float("nan")),
           dict(c=float("inf")), dict(method="minmax"), dict(method="minmax", scores=sc[:, :, :3]), dict(counts=torch.zeros((2, 4), dtype=torch.int32)),
           dict(ids=ids[0]), dict(ids=[ids[0], ids[1][:, :2]]), dict(ids=torch.zeros((9, 3, 4), dtype=torch.int64)), dict(ids=[]),
           dict(ids=torch.zeros((2, 3, 0), dtype=torch.int64))]
    for change in bad:
        a = dict(dict(ids=ids, k=3), **change)
        with pytest.raises(ValueError):
            scoring.rank_fuse(a.pop("ids"), a.pop("k"), **a)
    assert scoring.rank_fuse_arguments(3, np.int64(7), "rrf", None, 60) == (7, 0, [1.0, 1.0, 1.0], 60.0)
    assert scoring.rank_fuse_arguments(2, 5, "minmax", (0, 2), float("nan"))[:3] == (5, 1, [0.0, 2.0])     # c is RRF's alone
    with pytest.raises(ValueError):
        fusion.fuse_hybrid_lists(ids[0], ids[1], None, ids[0, 0], ids[0, 0], 3, method="minmax")
    ret = object.__new__(HybridRetriever)                   # no index behind it: the checks come first
    for change in [dict(topk=0), dict(method="sum"), dict(weights=(1.0, -2.0)), dict(c=-1.0), dict(fused_topk=0), dict(weights=(1.0,))]:
        a = dict(dict(topk=10), **change)
        with pytest.raises(ValueError):
            ret.retrieve_rank_fused(None, a.pop("topk"), **a)
    with pytest.raises(NotImplementedError):
        ret.retrieve_rank_fused(None, 10, collapse={"d": "g"})


def test_sharded_classes_refuse_rank_fusion():
    from scaling_retriever_amd.distributed import ShardedDenseRetriever, ShardedSparseRetriever
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval
    for cls in (ShardedDenseRetriever, ShardedSparseRetriever, ShardedSparseRetrieval):
        with pytest.raises(NotImplementedError):
            cls.retrieve_rank_fused(object.__new__(cls), None, 10)


def test_model_on_a_hand_computed_case():
    a, b, c = 3, 7, 5                                       # lists [a, b] and [b, c]
    ids = np.array([[[a, b]], [[b, c]]], np.int64)
    s, i, n, r = R.rank_fuse(ids, 4, c=60.0)
    fb = F32(F32(F32(1) / F32(62)) + F32(F32(1) / F32(61)))     # list 0 (rank 2) first, then list 1 (rank 1)
    fa, fc = F32(F32(1) / F32(61)), F32(F32(1) / F32(62))
    assert i.tolist() == [[b, a, c, -1]] and n.tolist() == [3]
    assert R.bits(s[0, :3]).tolist() == R.bits([fb, fa, fc]).tolist() and s[0, 3] == -R.FLT_MAX
    assert r[0].tolist() == [[2, 1], [1, 0], [0, 2], [0, 0]]
    # equal fused scores break by id; a weight-0 list still brings its documents, with 0.0
    s, i, n, _ = R.rank_fuse(np.array([[[9, 4]], [[4, 9]]], np.int64), 2)
    assert i.tolist() == [[4, 9]] and s[0, 0] == s[0, 1]
    s, i, n, _ = R.rank_fuse(ids, 3, weights=(1.0, 0.0))
    assert i.tolist() == [[a, b, c]] and s[0, 2] == 0.0 and R.bits(s[0, :2]).tolist() == R.bits([fa, fc]).tolist()
    # counts cut a row, a pad in the middle keeps the ranks of what follows
    s, i, n, r = R.rank_fuse(np.array([[[1, -1, 2, 8]], [[2, 6, 6, 6]]], np.int64), 4, counts=np.array([[3], [1]], np.int32))
    assert i.tolist() == [[2, 1, -1, -1]] and n.tolist() == [2] and r[0, 0].tolist() == [3, 1]
    # min-max: the best of a list gets 1, its worst 0, a constant list 1 everywhere
    sc = np.array([[[4.0, 2.0, 1.0]], [[5.0, 5.0, 5.0]]], F32)
    s, i, n, _ = R.rank_fuse(np.array([[[0, 1, 2]], [[2, 1, 3]]], np.int64), 4, scores=sc, method="minmax")
    third = F32(F32(1.0) / F32(3.0))
    assert i.tolist() == [[1, 0, 2, 3]] and R.bits(s[0]).tolist() == R.bits([F32(third + F32(1)), 1.0, 1.0, 1.0]).tolist()


def test_eval_fuse_argument_parsing():
    E = _eval_fuse()
    a = E.parse_args(["--run_paths", "a/run.json,b/run.json,c/run.json", "--output_dir", "out"])
    assert a.run_paths == ["a/run.json", "b/run.json", "c/run.json"] and a.weights == (1.0, 1.0, 1.0)
    assert (a.method, a.c, a.topk) == ("rrf", 60.0, 1000)
    a = E.parse_args(["--run_paths", "a,b", "--output_dir", "o", "--method", "minmax", "--c", "10", "--weights", "0.3,1.7", "--topk", "7"])
    assert (a.method, a.c, a.weights, a.topk) == ("minmax", 10.0, (0.3, 1.7), 7)
    for argv in (["--output_dir", "o"], ["--run_paths", "a,b"], ["--run_paths", "a,b", "--output_dir", "o", "--weights", "1"],
                 ["--run_paths", "a,b", "--output_dir", "o", "--weights", "x,y"], ["--run_paths", "a,b", "--output_dir", "o", "--method", "sum"],
                 ["--run_paths", "a,b", "--output_dir", "o", "--topk", "0"], ["--run_paths", ",", "--output_dir", "o"]):
        with pytest.raises(SystemExit):
            E.parse_args(argv)


def test_eval_fuse_document_numbering():
    E = _eval_fuse()
    table, number = E.number_documents([{"q": {"10": 1.0, "9": 2.0}}, {"q": {"100": 1.0}, "p": {"9": 0.5}}])
    assert table == ["9", "10", "100"] and number == {"9": 0, "10": 1, "100": 2}            # numerically
    table, _ = E.number_documents([{"q": {"10": 1.0, "9": 2.0, "d7": 0.0}}])
    assert table == ["10", "9", "d7"]                                                        # one id is no integer: by the string
    table, _ = E.number_documents([{"q": {"-3": 1.0, "2": 2.0}}])
    assert table == ["-3", "2"]
    qids, ids, scores, counts = E.build_lists([{"q1": {"9": 1.0, "10": 3.0, "100": 3.0}, "q2": {"10": 0.5}}, {"q2": {"100": 2.0}, "q3": {"9": 1.0}}],
                                              {"9": 0, "10": 1, "100": 2})
    assert qids == ["q1", "q2"]                                                              # the first run's queries, in its order
    assert ids.tolist() == [[[1, 2, 0], [1, -1, -1]], [[-1, -1, -1], [2, -1, -1]]]           # score descending, then document number
    assert counts.tolist() == [[3, 1], [0, 1]] and scores[0, 0].tolist() == [3.0, 3.0, 1.0]


def _model_fuse(ids, counts, scores, k, method, weights, c):
    return R.rank_fuse(ids, k, counts=counts, scores=scores, method=method, weights=weights, c=c)[:3]


def expected_run(runs, method, weights, c, topk):
    """The fused run of eval_fuse.py from the model alone, with a numbering of its own: documents by int(id)."""
    docs = sorted({d for run in runs for hits in run.values() for d in hits}, key=int)
    num = {d: i for i, d in enumerate(docs)}
    qids = list(runs[0])
    depth = max(len(h) for run in runs for h in run.values())
    ids = np.full((len(runs), len(qids), depth), -1, np.int64)
    sc = np.zeros(ids.shape, F32)
    for l, run in enumerate(runs):
        for q, qid in enumerate(qids):
            row = sorted(run.get(qid, {}).items(), key=lambda kv: (-F32(kv[1]), num[kv[0]]))
            for r, (d, s) in enumerate(row):
                ids[l, q, r], sc[l, q, r] = num[d], s
    s, i, n, _ = R.rank_fuse(ids, topk, scores=sc, method=method, weights=weights, c=c)
    return {qid: {docs[i[q, j]]: float(s[q, j]) for j in range(n[q])} for q, qid in enumerate(qids) if n[q]}


def three_runs():
    rng = np.random.default_rng(5)
    runs = []
    for l in range(3):
        run = {}
        for q in range(4):
            if l == 2 and q == 1:
                continue                                    # a query missing from a later run
            docs = rng.choice(30, size=int(rng.integers(3, 9)), replace=False)
            run[f"q{q}"] = {str(int(d) * 7): float(F32(rng.integers(0, 6) / 4)) for d in docs}      # few score values: ties inside a run
        runs.append(run)
    return runs


def test_eval_fuse_run_ordering_with_the_model_in_place_of_the_library(tmp_path, monkeypatch):
    E = _eval_fuse()
    runs = three_runs()
    paths = []
    for l, run in enumerate(runs):
        os.makedirs(tmp_path / f"r{l}")
        paths.append(str(tmp_path / f"r{l}" / "run.json"))
        with open(paths[-1], "w") as f:
            json.dump(run, f)
    monkeypatch.setattr(E, "fuse_on_device", _model_fuse)
    for method, weights in (("rrf", "1,1,1"), ("minmax", "0.3,1.7,0.9")):
        out = tmp_path / f"out_{method}"
        res = E.main(["--run_paths", ",".join(paths), "--output_dir", str(out), "--method", method, "--weights", weights, "--topk", "6"])
        got = json.load(open(out / "run.json"))
        want = expected_run(runs, method, tuple(float(x) for x in weights.split(",")), 60.0, 6)
        assert got == want and res == want
        assert [list(got[q]) for q in got] == [list(want[q]) for q in want]             # the order inside a query, too
        assert list(got) == list(runs[0])
    # the limits: a list longer than sr_max_topk(), lists that together exceed the kernel's limit, and a k beyond it
    limit = E.max_topk()
    ids = np.zeros((2, 1, limit + 1), np.int64)
    with pytest.raises(ValueError, match="sr_max_topk"):
        E.check_limits(ids, np.array([[limit + 1], [1]], np.int32), 10, limit)
    with pytest.raises(ValueError, match="entries"):
        E.check_limits(np.zeros((3, 1, limit), np.int64), np.array([[limit], [1], [1]], np.int32), 10, limit)
    with pytest.raises(ValueError, match="topk"):
        E.check_limits(np.zeros((2, 1, 8), np.int64), np.array([[8], [8]], np.int32), limit + 1, limit)
    E.check_limits(np.zeros((2, 1, limit), np.int64), np.array([[limit], [limit]], np.int32), limit, limit)


def test_tie_maps_round_trip_on_random_position_maps():
    from scaling_retriever_amd import fusion
    rng = np.random.default_rng(11)
    n_dense, n_sparse = 57, 40
    with_posting = np.sort(rng.choice(n_dense, size=n_sparse - 5, replace=False))          # 22 documents have no posting
    d2s = np.full(n_dense, -1, np.int64)
    d2s[with_posting] = rng.permutation(n_sparse)[:len(with_posting)]                       # 5 sparse positions map to no document
    s2d = np.full(n_sparse, -1, np.int64)
    s2d[d2s[d2s >= 0]] = np.nonzero(d2s >= 0)[0]
    d2s_t, s2d_t = torch.from_numpy(d2s), torch.from_numpy(s2d)
    dense_pos = torch.from_numpy(np.stack([rng.permutation(n_dense)[:12] for _ in range(6)]))
    dense_pos[2, 4] = -1
    dense_pos[5, 9:] = -1
    tie = fusion.dense_to_tie(dense_pos, d2s_t, n_sparse)
    want = np.where(dense_pos.numpy() < 0, -1, np.where(d2s[dense_pos.numpy()] >= 0, d2s[dense_pos.numpy()], n_sparse + dense_pos.numpy()))
    assert tie.numpy().tolist() == want.tolist() and (want >= n_sparse).any() and ((want >= 0) & (want < n_sparse)).any()
    assert fusion.tie_to_dense(tie, s2d_t).numpy().tolist() == dense_pos.numpy().tolist()
    mapped = np.nonzero(s2d >= 0)[0]
    sparse_pos = torch.from_numpy(np.stack([rng.permutation(mapped)[:10] for _ in range(6)]))
    counts = torch.tensor([10, 0, 3, 10, 7, 1], dtype=torch.int32)
    tie_s = fusion.sparse_to_tie(sparse_pos, counts, s2d_t)
    cols = np.arange(10)[None, :] < counts.numpy()[:, None]
    assert tie_s.numpy().tolist() == np.where(cols, sparse_pos.numpy(), -1).tolist()
    assert fusion.tie_to_dense(tie_s, s2d_t).numpy().tolist() == np.where(cols, s2d[sparse_pos.numpy()], -1).tolist()
    # one document, found by both heads, has one tie; a document without a posting sorts after every indexed one
    both = int(with_posting[0])
    assert int(fusion.dense_to_tie(torch.tensor([[both]]), d2s_t, n_sparse)) == int(d2s[both])
    # a sparse position without a dense document: retrieve_fused's KeyError - but not beyond the row's count
    orphan = int(np.nonzero(s2d < 0)[0][0])
    bad = sparse_pos.clone()
    bad[1, 0] = orphan
    assert fusion.sparse_to_tie(bad, counts, s2d_t).numpy().tolist() == tie_s.numpy().tolist()
    bad[0, 0] = orphan
    with pytest.raises(KeyError, match="the inverted index holds a document the dense index does not"):
        fusion.sparse_to_tie(bad, counts, s2d_t)
