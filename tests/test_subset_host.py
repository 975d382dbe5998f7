"""CPU: search within a document subset (sr_dense_search_subset / sr_sparse_search_subset, csrc/subset_search.hip) - the parts that
need no GPU.  The numpy specification of the result (the full ranking in the project's tie order, filtered by the subset, cut to k) is
defined HERE and checked against hand-worked cases; tests/test_subset_search_gpu.py holds the kernels to it.  Then the allow-list
mapping of the Python layer, the drivers' flag and file reader, the doc-sharded classes' refusal, and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ specification ---
def subset_topk_spec(scores, gids, subset, k, pad_score, threshold=None):
    """scores fp32 [nq, N] of every document, gids int64 [N] their global doc indices (distinct), subset = allowed global doc indices.
    Per query: all documents ranked by (score descending, doc index ascending) - the order of sr_dense_search / sr_sparse_search -, those
    outside the subset removed (sparse: also those with score <= threshold), the list cut to k and padded with (pad_score, -1).
    Returns (scores [nq, k], ids [nq, k], counts [nq])."""
    scores = np.asarray(scores, np.float32)
    gids = np.asarray(gids, np.int64)
    allowed = np.isin(gids, np.asarray(subset, np.int64))
    nq = scores.shape[0]
    out_s = np.full((nq, k), pad_score, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    counts = np.zeros(nq, np.int32)
    for q in range(nq):
        order = np.lexsort((gids, -scores[q].astype(np.float64)))          # last key first: score descending, then doc index ascending
        keep = allowed[order]
        if threshold is not None:
            keep &= scores[q][order] > np.float32(threshold)
        order = order[keep][:k]
        counts[q] = len(order)
        out_s[q, :len(order)] = scores[q][order]
        out_i[q, :len(order)] = gids[order]
    return out_s, out_i, counts


def test_spec_on_hand_worked_cases():
    #            doc index:   3    5    8    9   20
    scores = np.array([[1.0, 2.0, 2.0, 0.5, 2.0],
                       [0.0, -1.0, 3.0, 3.0, 0.0]], np.float32)
    gids = np.array([3, 5, 8, 9, 20])
    FMIN = np.float32(-3.402823466e38)
    # query 0 ranks 5, 8, 20 (ties by ascending doc index), 3, 9; the subset {3, 8, 20} leaves 8, 20, 3
    s, i, c = subset_topk_spec(scores, gids, [3, 8, 20], 2, FMIN)
    assert i.tolist() == [[8, 20], [8, 3]] and s.tolist() == [[2.0, 2.0], [3.0, 0.0]] and c.tolist() == [2, 2]
    # k beyond the subset: padding; a tie across the subset boundary (9 scores as 8 for query 1) does not move 8
    s, i, c = subset_topk_spec(scores, gids, [3, 8, 20], 5, FMIN)
    assert i.tolist() == [[8, 20, 3, -1, -1], [8, 3, 20, -1, -1]] and c.tolist() == [3, 3]
    assert s[0].tolist() == [2.0, 2.0, 1.0, float(FMIN), float(FMIN)]
    # the empty subset: every row is padding
    s, i, c = subset_topk_spec(scores, gids, [], 3, FMIN)
    assert (i == -1).all() and (s == FMIN).all() and c.tolist() == [0, 0]
    # the whole collection: the plain ranking
    s, i, c = subset_topk_spec(scores, gids, gids, 5, FMIN)
    assert i.tolist() == [[5, 8, 20, 3, 9], [8, 9, 3, 20, 5]]
    # sparse: score > threshold as well, padding (0, -1), counts
    s, i, c = subset_topk_spec(scores, gids, [3, 5, 9, 20], 3, 0.0, threshold=0.0)
    assert i.tolist() == [[5, 20, 3], [9, -1, -1]] and c.tolist() == [3, 1] and s[1].tolist() == [3.0, 0.0, 0.0]
    s, i, c = subset_topk_spec(scores, gids, [3, 5, 9, 20], 3, 0.0, threshold=1.0)
    assert i.tolist() == [[5, 20, -1], [9, -1, -1]] and c.tolist() == [2, 1]


# ------------------------------------------------------------------------------------------- allow-list mapping ---
def test_allowed_ids_map_to_sorted_unique_positions():
    from scaling_retriever_amd.rerank import InverseIdMap
    from scaling_retriever_amd.scoring import allowed_positions
    inv = InverseIdMap(["p7", "p3", 11, "p9", "p1"])               # position -> database id; ids are compared as strings
    get = lambda d: inv.pos.get(str(d))                             # noqa: E731
    got = allowed_positions(["p9", "p7", "p9", "11", 11, "p3"], get)
    assert got.dtype == np.int64 and got.tolist() == [0, 1, 2, 3]   # duplicates dropped, order of the list irrelevant
    assert allowed_positions([], get).tolist() == [] and allowed_positions([], get).dtype == np.int64
    assert allowed_positions(["p1"], get).tolist() == [4]
    with pytest.raises(ValueError, match="p404"):
        allowed_positions(["p1", "p404", "p3"], get)
    # a doc_ids.pkl style dict (position -> id) maps the same way
    inv2 = InverseIdMap({0: "a", 2: "b", 5: "c"})
    assert allowed_positions(["c", "a"], lambda d: inv2.pos.get(str(d))).tolist() == [0, 5]


def test_allowed_ids_file_reader_and_driver_flags(tmp_path):
    from scaling_retriever_amd.scoring import read_allowed_ids_file
    import eval_dense
    import eval_sparse
    f = tmp_path / "allowed.txt"
    f.write_text("p3\n  p1 \n\np3\n17\n")
    assert read_allowed_ids_file(str(f)) == ["p3", "p1", "p3", "17"]
    for mod in (eval_dense, eval_sparse):
        assert mod.parse_args(["--task_name", "retrieval"]).allowed_ids_file is None
        assert mod.parse_args(["--task_name", "retrieval", "--allowed_ids_file", str(f)]).allowed_ids_file == str(f)
    # the dense driver maps the file through the id files of the embedding directory (rows in plan order)
    np.save(tmp_path / "ids_0_0.npy", np.array(["p0", "p1", "p2"]))
    np.save(tmp_path / "ids_0_1.npy", np.array(["p3", "17"]))
    id_files = [str(tmp_path / "ids_0_0.npy"), str(tmp_path / "ids_0_1.npy")]
    assert eval_dense.allowed_subset_positions(str(f), id_files).tolist() == [1, 3, 4]
    f.write_text("p3\nnope\n")
    with pytest.raises(ValueError, match="nope"):
        eval_dense.allowed_subset_positions(str(f), id_files)


def test_doc_sharded_classes_refuse_an_allow_list(tmp_path):
    import eval_dense
    from scaling_retriever_amd.distributed import ShardedDenseRetriever, ShardedSparseRetriever
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval
    # the refusal comes before anything else is touched: the objects below are never initialised
    with pytest.raises(NotImplementedError, match="allow-list"):
        ShardedSparseRetrieval.retrieve(object.__new__(ShardedSparseRetrieval), None, topk=10, allowed_ids=["p1"])
    with pytest.raises(NotImplementedError, match="allow-list"):
        ShardedSparseRetriever.search(object.__new__(ShardedSparseRetriever), None, None, None, 10, subset=[1])
    with pytest.raises(NotImplementedError, match="allow-list"):
        ShardedDenseRetriever.search(object.__new__(ShardedDenseRetriever), None, 10, subset=[1])
    with pytest.raises(NotImplementedError, match="allowed_ids_file"):
        eval_dense.allowed_subset_positions(str(tmp_path / "x"), [], world=2)


# --------------------------------------------------------------------------------------------------------- ABI ---
def _prototype_arg_count(name):
    src = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/sr_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_subset_entry_points_are_declared_and_bound():
    from scaling_retriever_amd import _lib
    assert _prototype_arg_count("sr_dense_search_subset") == 9
    assert _prototype_arg_count("sr_sparse_search_subset") == 15
    for name in ("sr_dense_search_subset", "sr_sparse_search_subset"):
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(args) == _prototype_arg_count(name), name
    # d_subset / m sit where the header puts them: a pointer followed by an int64
    dense = _lib.SIGNATURES["sr_dense_search_subset"][1]
    assert dense[4] is _lib.c_void_p and dense[5] is _lib.c_int64
    sparse = _lib.SIGNATURES["sr_sparse_search_subset"][1]
    assert sparse[6] is _lib.c_float and sparse[7] is _lib.c_void_p and sparse[8:11] == [_lib.c_int64] * 3
    lib = _lib.load()
    assert hasattr(lib, "sr_dense_search_subset") and hasattr(lib, "sr_sparse_search_subset")


def test_subset_argument_checks_without_gpu():
    """Checks made before anything touches a device (the pointers are never dereferenced)."""
    import ctypes
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.sr_dense_search_subset(None, p, 1, 10, p, 1, p, p, None) == _lib.SR_ERR_INVALID and b"null index" in lib.sr_last_error()
    assert lib.sr_sparse_search_subset(None, p, p, p, 1, 10, 0.0, p, 1, 0, 1, p, p, p, None) == _lib.SR_ERR_INVALID
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    try:
        for nq, k, m, text in [(1, 0, 0, b"outside [1"), (1, 10, -1, b"m=-1"), (1, 10, 1, b"m=1"),       # an empty index holds no subset
                               (1, 5000, 0, b"more than the subset"), (-1, 10, 0, b"bad nq")]:
            rc = lib.sr_dense_search_subset(h, p, nq, k, p, m, p, p, None)
            assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (nq, k, m, lib.sr_last_error())
        assert lib.sr_dense_search_subset(h, p, 0, 10, p, 0, p, p, None) == _lib.SR_OK            # no queries: nothing to do
    finally:
        lib.sr_dense_index_destroy(h)
