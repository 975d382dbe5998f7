"""Host-side checks of the collapsed search (no GPU): the C entry point's argument validation with pointers that are never
dereferenced (the pattern of tests/test_abi.py), the Python drivers' argument checks, which raise before anything is uploaded, and the
label -> int32 key table."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from scaling_retriever_amd import _lib


def _collapse(lib, scores=1, ids=1, counts=None, nq=1, row_len=8, exhaustive=0, keys=1, n_keys=8, k=4, outs=(1, 1, 1, 1, 1)):
    p = lambda v: ctypes.c_void_p(0x1000) if v else None      # noqa: E731  (never dereferenced: every case fails, or has nq == 0)
    return lib.sr_topk_collapse(p(scores), p(ids), p(counts), nq, row_len, exhaustive, p(keys), n_keys, k, *[p(o) for o in outs], None)


def test_entry_point_rejects_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    max_k = lib.sr_max_topk()
    for kw in (dict(scores=0), dict(ids=0), dict(keys=0)) + tuple(dict(outs=tuple(int(j != i) for j in range(5))) for i in range(5)):
        assert _collapse(lib, **kw) == _lib.SR_ERR_INVALID, kw
        assert b"null pointer" in lib.sr_last_error()
    assert _collapse(lib, k=0) == _lib.SR_ERR_INVALID
    assert _collapse(lib, k=-3) == _lib.SR_ERR_INVALID
    assert _collapse(lib, k=max_k + 1) == _lib.SR_ERR_UNSUPPORTED
    assert str(max_k).encode() in lib.sr_last_error()
    assert _collapse(lib, row_len=-1) == _lib.SR_ERR_INVALID
    assert b"row_len" in lib.sr_last_error()
    assert _collapse(lib, row_len=1 << 31) == _lib.SR_ERR_INVALID
    assert _collapse(lib, n_keys=-1) == _lib.SR_ERR_INVALID
    assert _collapse(lib, nq=-1) == _lib.SR_ERR_INVALID
    assert _collapse(lib, nq=0) == _lib.SR_OK
    assert _collapse(lib, nq=0, row_len=0, k=max_k, exhaustive=1) == _lib.SR_OK


def _dense_stub(precision="fp32", id_end=12):
    """What dense_search_collapsed asks of an index before it uploads anything - no handle, no device."""
    from scaling_retriever_amd.scoring import DenseIndexHIP
    stub = SimpleNamespace(precision=precision, id_end=id_end, dim=4)
    stub._mask = lambda mask, ndim=1: DenseIndexHIP._mask(stub, mask, ndim)
    stub._check_queries = lambda q: DenseIndexHIP._check_queries(stub, q)
    return stub


def test_dense_driver_checks_its_arguments_before_any_upload():
    import torch
    from scaling_retriever_amd.collapse import dense_search_collapsed
    keys = np.zeros(12, np.int32)
    q = torch.zeros((3, 4))                                    # a CPU tensor: reaching the device check means every host check passed
    cases = [
        (dict(keys=np.zeros(12, np.int64)), "int32"),
        (dict(keys=[0] * 12), "int32"),
        (dict(keys=np.zeros((12, 1), np.int32)), "1-D"),
        (dict(keys=np.zeros(11, np.int32)), r"one group key per document index \(12\), got 11"),
        (dict(subset=[1], mask=np.ones(12, bool)), "not both"),
        (dict(mask=np.ones(12, bool), masks=np.ones((2, 12), bool), query_group=np.zeros(3, np.int64)), "not both"),
        (dict(masks=np.ones((2, 12), bool)), "go together"),
        (dict(depths=(9, 64)), "at least k = 10"),
        (dict(depths=()), "at least k"),
        (dict(k=0), "integer >= 1"),
        (dict(k=2.5), "integer >= 1"),
        (dict(k=_lib.load().sr_max_topk() + 1), "beyond sr_max_topk"),
    ]
    for kw, needle in cases:
        args = dict(k=10, keys=keys)
        args.update(kw)
        with pytest.raises(ValueError, match=needle):
            dense_search_collapsed(_dense_stub(), q, **args)
    for precision in ("bf16x3", "bf16x6"):
        with pytest.raises(ValueError, match="precision"):
            dense_search_collapsed(_dense_stub(precision), q, 10, keys)


def test_sparse_driver_checks_its_arguments_before_any_upload():
    from scaling_retriever_amd.scoring import SparseIndexHIP
    idx = object.__new__(SparseIndexHIP)                       # no handle, no device
    idx.n_docs = 12
    qi, qc, qv = np.array([0, 1], np.int64), np.array([0], np.int32), np.array([1.0], np.float32)
    with pytest.raises(ValueError, match="int32"):
        idx.search_collapsed(qi, qc, qv, 5, np.zeros(12, np.float32))
    with pytest.raises(ValueError, match=r"\(12\), got 13"):
        idx.search_collapsed(qi, qc, qv, 5, np.zeros(13, np.int32))
    with pytest.raises(ValueError, match=r"\(27\), got 12"):      # ids run to 4 + 11 * 2
        idx.search_collapsed(qi, qc, qv, 5, np.zeros(12, np.int32), id_base=4, id_stride=2)
    with pytest.raises(ValueError, match="not both"):
        idx.search_collapsed(qi, qc, qv, 5, np.zeros(12, np.int32), subset=[1], mask=np.ones(12, bool))
    with pytest.raises(ValueError, match="at least k = 5"):
        idx.search_collapsed(qi, qc, qv, 5, np.zeros(12, np.int32), depths=(4,))


def test_topk_collapse_front_end_checks_keys_and_shapes():
    import torch
    from scaling_retriever_amd.scoring import topk_collapse
    s, i = torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="int32"):
        topk_collapse(s, i, np.zeros(4, np.int64), 2)
    with pytest.raises(ValueError, match="one shape"):
        topk_collapse(s, i[:, :3], np.zeros(4, np.int32), 2)


def test_key_table_builder():
    from scaling_retriever_amd.collapse import group_keys, labels_of, read_collapse_file
    db_ids = ["p0", "p1", "p2", "p3", "p4"]
    by_dict = labels_of({"p0": "a", "p1": "b", "p2": "a", "p3": "c", "p4": "b", "unused": "z"}, db_ids)
    by_call = labels_of(lambda d: "abacb"[int(d[1:])], db_ids)
    by_seq = labels_of(["a", "b", "a", "c", "b"], db_ids)
    assert by_dict == by_call == by_seq == ["a", "b", "a", "c", "b"]
    keys, table = group_keys(by_dict)
    assert keys.dtype == np.int32 and keys.tolist() == [0, 1, 0, 2, 1] and table == ["a", "b", "c"]
    keys, table = group_keys([7, 7, (1, 2), 7])                # any hashable label
    assert keys.tolist() == [0, 0, 1, 0] and table == [7, (1, 2)]
    keys, table = group_keys([])
    assert keys.shape == (0,) and table == []
    with pytest.raises(ValueError, match="'p3' has no group"):
        labels_of({"p0": "a", "p1": "b", "p2": "a"}, db_ids)
    with pytest.raises(ValueError, match="aligned with the index"):
        labels_of(["a", "b"], db_ids)


def test_collapse_file_reader(tmp_path):
    from scaling_retriever_amd.collapse import read_collapse_file
    path = tmp_path / "groups.tsv"
    path.write_text("p0\tdocA\np1\tdocA\n\np2\tdocB\n")
    assert read_collapse_file(str(path)) == {"p0": "docA", "p1": "docA", "p2": "docB"}
    path.write_text("p0 docA\n")
    with pytest.raises(ValueError, match="passage_id<TAB>group_id"):
        read_collapse_file(str(path))


def test_model_matches_the_definition_on_a_hand_made_row():
    from collapse_cases import collapse_model
    keys = np.array([5, 5, 9, 5, 2, 9], np.int32)
    scores = np.array([[9, 8, 8, 7, 6, 5]], np.float32)
    ids = np.array([[1, 0, 2, 3, 4, 5]], np.int64)
    s, i, g, c, done = collapse_model(scores, ids, keys, 2)
    assert i.tolist() == [[1, 2]] and g.tolist() == [[5, 9]] and s.tolist() == [[9, 8]] and c.tolist() == [2] and done.tolist() == [1]
    s, i, g, c, done = collapse_model(scores, ids, keys, 4)
    assert i.tolist() == [[1, 2, 4, -1]] and c.tolist() == [3] and done.tolist() == [0]
    assert collapse_model(scores, ids, keys, 4, counts=[5])[4].tolist() == [1]
    assert collapse_model(scores, ids, keys, 4, exhaustive=True)[4].tolist() == [1]


def test_what_is_not_offered_says_so():
    from scaling_retriever_amd.distributed import ShardedDenseRetriever, ShardedSparseRetriever
    from scaling_retriever_amd.indexer import HybridRetriever, ShardedSparseRetrieval
    with pytest.raises(NotImplementedError, match="collapse"):
        ShardedSparseRetrieval.retrieve(object.__new__(ShardedSparseRetrieval), None, 5, collapse={"p0": "a"})
    for cls in (ShardedDenseRetriever, ShardedSparseRetriever):
        with pytest.raises(NotImplementedError, match="doc-sharded"):
            cls.search_collapsed(object.__new__(cls), None, 5, None)
    h = object.__new__(HybridRetriever)
    with pytest.raises(NotImplementedError, match="not offered under collapse"):
        h.retrieve_fused([], 5, collapse={"p0": "a"})
    with pytest.raises(NotImplementedError, match="not offered under collapse"):
        h.search_fused(None, None, 5, collapse={"p0": "a"})
    with pytest.raises(NotImplementedError, match="not offered under collapse"):
        h.retrieve_fused_exact([], 5, collapse={"p0": "a"})


def test_route_stats_are_plain_json():
    import json
    from scaling_retriever_amd.collapse import key_table, route_stats
    out = route_stats({"depth": np.array([0, 0, 1, -1]), "groups_seen": np.array([5, 5, 5, 3]), "depths": (16, 64)})
    assert json.loads(json.dumps(out)) == {"depths": [16, 64], "queries_per_depth": [2, 1], "full_ranking_queries": 1, "mean_groups": 4.5}
    keys, table = key_table({"a": "x", "b": "x"}, ["a", None, "b"])          # a position without an id: a group of its own
    assert keys.tolist() == [0, 1, 0] and table[0] == "x" and table[1] != "x"
