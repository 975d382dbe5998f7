"""CPU: the range searches and the exact hybrid search under filter groups (a document bitmap per query) - the new C-ABI symbols, the
argument checks that come before any device work or upload, what the doc-sharded classes still refuse, and the kernels' metadata."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_dense_range_count_grouped", "sr_dense_range_fill_grouped", "sr_sparse_range_count_grouped", "sr_sparse_range_fill_grouped")


def test_new_symbols_are_declared_exported_and_bound():
    from scaling_retriever_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the grouped pairs take the masked arguments with (d_group_words, n_groups, n_bits, d_query_group) for (d_mask_words, n_bits)
    for head in ("dense", "sparse"):
        for half in ("count", "fill"):
            assert len(_lib.SIGNATURES[f"sr_{head}_range_{half}_grouped"][1]) == len(_lib.SIGNATURES[f"sr_{head}_range_{half}_masked"][1]) + 2


def test_entry_points_validate_before_they_touch_a_device():
    """The pointers below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    total = ctypes.c_int64(-1)
    err = lib.sr_last_error
    assert lib.sr_dense_range_count_grouped(None, p, 4, p, p, 1, 0, p, p, ctypes.byref(total), None) == _lib.SR_ERR_INVALID and b"null index" in err()
    assert lib.sr_dense_range_fill_grouped(None, p, 4, p, p, 1, 0, p, p, p, p, 10, None) == _lib.SR_ERR_INVALID and b"null index" in err()
    assert lib.sr_sparse_range_count_grouped(None, p, p, p, 4, p, p, 1, 0, p, p, ctypes.byref(total), None) == _lib.SR_ERR_INVALID and b"null index" in err()
    assert lib.sr_sparse_range_fill_grouped(None, p, p, p, 4, p, p, 1, 0, p, p, 0, 1, p, p, 10, None) == _lib.SR_ERR_INVALID and b"null index" in err()
    # an empty dense index numbers its documents in [0, 0)
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    try:
        cases = [
            (dict(n_bits=32), b"n_bits=32"),
            (dict(n_groups=0), b"n_groups=0"),
            (dict(n_groups=-3), b"n_groups=-3"),
            (dict(n_groups=1 << 32), b"2^32"),
            (dict(groups=None), b"null masks or query groups"),
            (dict(queries=None), b"null queries or thresholds"),
            (dict(lims=None), b"null d_lims or total"),
            (dict(queries=ctypes.c_void_p(4100)), b"16-byte aligned"),
        ]
        for change, text in cases:
            a = dict(dict(queries=p, n_groups=1, n_bits=0, groups=p, lims=p), **change)
            rc = lib.sr_dense_range_count_grouped(h, a["queries"], 4, p, p, a["n_groups"], a["n_bits"], a["groups"], a["lims"], ctypes.byref(total), None)
            assert rc == _lib.SR_ERR_INVALID and text in err(), (change, rc, err())
            assert total.value == -1
        for change, text in cases[:5]:
            a = dict(dict(queries=p, n_groups=1, n_bits=0, groups=p, lims=p), **change)
            rc = lib.sr_dense_range_fill_grouped(h, a["queries"], 4, p, p, a["n_groups"], a["n_bits"], a["groups"], a["lims"], p, p, 10, None)
            assert rc == _lib.SR_ERR_INVALID and text in err(), (change, rc, err())
        rc = lib.sr_dense_range_fill_grouped(h, p, 4, p, p, 1, 0, p, p, p, p, 10, None)
        assert rc == _lib.SR_ERR_INVALID and b"no sr_dense_range_count precedes" in err()
    finally:
        lib.sr_dense_index_destroy(h)


def _no_device(monkeypatch):
    from scaling_retriever_amd import _lib

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)


def test_python_layer_rejects_bad_arguments_before_any_upload(monkeypatch):
    from scaling_retriever_amd import _lib, hybrid
    from scaling_retriever_amd.indexer import DenseFlatIndexer, HybridRetriever, SparseRetrieval
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    dense = object.__new__(DenseIndexHIP)
    dense.lib, dense._h, dense.dim = lib, h, 64                 # an empty index: id_end = 0, asked of the handle without a device
    sparse = object.__new__(SparseIndexHIP)
    sparse.n_docs = 100
    try:
        _no_device(monkeypatch)
        q = torch.zeros((5, 64))
        ok_masks, ok_groups = np.zeros((2, 0), bool), np.zeros(5, np.int64)
        bad = [("not both", dict(mask=np.zeros(0, bool), masks=ok_masks, query_group=ok_groups)),
               ("go together", dict(query_group=ok_groups)),
               ("go together", dict(masks=ok_masks)),
               ("2-D", dict(masks=np.zeros(4, bool), query_group=ok_groups)),
               ("bool", dict(masks=np.zeros((2, 4), np.float32), query_group=ok_groups)),
               ("at least one group", dict(masks=np.zeros((0, 4), bool), query_group=ok_groups)),
               ("words", dict(masks=np.zeros((2, 3), np.uint32), query_group=ok_groups)),
               ("float32", dict(queries=torch.zeros((5, 32)), masks=ok_masks, query_group=ok_groups)),
               ("one group id per query", dict(masks=ok_masks, query_group=np.zeros(4, np.int64))),
               ("one group id per query", dict(masks=ok_masks, query_group=np.zeros((5, 1), np.int64))),
               ("integer", dict(masks=ok_masks, query_group=np.zeros(5, np.float32))),
               ("integer", dict(masks=ok_masks, query_group=torch.zeros(5, dtype=torch.bool))),
               ("cuda", dict(masks=ok_masks, query_group=ok_groups))]
        for needle, kw in bad:
            kw = dict(kw)
            queries = kw.pop("queries", q)
            with pytest.raises(ValueError, match=needle):
                dense.range_search(queries, 0.0, **kw)
            with pytest.raises(ValueError, match=needle):
                dense.range_count(queries, 0.0, **kw)
            with pytest.raises(ValueError, match=needle):
                dense.range_fill(queries, None, None, 0, **kw)
        # the sparse index: 100 documents, 4 words; 5 queries
        indptr = np.zeros(6, np.int64)
        flags = np.ones((2, 100), bool)
        for needle, kw in [("not both", dict(mask=flags[0], masks=flags, query_group=ok_groups)),
                           ("go together", dict(masks=flags)),
                           ("go together", dict(query_group=ok_groups)),
                           ("2-D", dict(masks=flags[0], query_group=ok_groups)),
                           ("4 words", dict(masks=np.zeros((2, 5), np.uint32), query_group=ok_groups)),
                           ("one group id per query", dict(masks=flags, query_group=np.zeros(4, np.int64))),
                           ("integer", dict(masks=flags, query_group=np.zeros(5, np.float64)))]:
            with pytest.raises(ValueError, match=needle):
                sparse.range_search(indptr, None, None, 0.0, **kw)
        # hybrid.search_fused: the argument rules come before the indexes are touched
        fake = type("Fake", (), {"precision": "fp32", "id_end": 64, "device": "cpu"})()
        monkeypatch.setattr(_lib, "load", lambda: type("L", (), {"sr_max_topk": staticmethod(lambda: 4096)})())
        words = np.zeros((2, 2), np.uint32)
        for needle, kw in [("not both", dict(mask=words[0], masks=words, query_group=ok_groups)),
                           ("go together", dict(masks=words)),
                           ("packed", dict(masks=np.zeros((2, 64), bool), query_group=ok_groups)),
                           ("words", dict(masks=np.zeros((2, 3), np.uint32), query_group=ok_groups)),
                           ("one group id per query", dict(masks=words, query_group=np.zeros(4, np.int64))),
                           ("integer", dict(masks=words, query_group=np.zeros(5, np.float32)))]:
            with pytest.raises(ValueError, match=needle):
                hybrid.search_fused(fake, None, None, None, q, None, None, None, 10, **kw)
        _no_device(monkeypatch)
        # the indexer classes: the rules of the grouped searches, word for word
        groups, rows = np.zeros(3, np.int64), np.ones((2, 4), bool)
        calls = [lambda **kw: DenseFlatIndexer.range_search(object.__new__(DenseFlatIndexer), None, 0.0, **kw),
                 lambda **kw: SparseRetrieval.range_search(object.__new__(SparseRetrieval), None, **kw),
                 lambda **kw: HybridRetriever.range_search(object.__new__(HybridRetriever), None, **kw)]
        for fn in calls:
            with pytest.raises(ValueError, match="not both"):
                fn(allowed_mask=rows[0], allowed_masks=rows, query_group=groups)
            with pytest.raises(ValueError, match="not both"):
                fn(allowed_ids=["a"], allowed_masks=rows, query_group=groups)
            with pytest.raises(ValueError, match="go together"):
                fn(allowed_masks=rows)
            with pytest.raises(ValueError, match="go together"):
                fn(query_group=groups)
        ret = object.__new__(HybridRetriever)
        for fn in (lambda **kw: ret.search_fused(None, None, 10, **kw), lambda **kw: ret.retrieve_fused_exact(None, 10, **kw)):
            with pytest.raises(ValueError, match="not both"):
                fn(allowed_mask=rows[0], allowed_masks=rows, query_group=groups)
            with pytest.raises(ValueError, match="go together"):
                fn(allowed_masks=rows)
            with pytest.raises(ValueError, match="go together"):
                fn(query_group=groups)
            with pytest.raises(ValueError):                   # the weights come before the masks
                fn(weights=(-1.0, 1.0), allowed_masks=rows, query_group=groups)
            with pytest.raises(NotImplementedError, match=r"allowed_mask=ret\.allowed_mask\(ids\)"):
                fn(allowed_ids=["d1"], allowed_masks=rows, query_group=groups)
    finally:
        monkeypatch.undo()
        dense.close()


def test_what_the_sharded_classes_still_refuse(monkeypatch):
    from scaling_retriever_amd.indexer import ShardedSparseRetrieval
    _no_device(monkeypatch)
    sh = object.__new__(ShardedSparseRetrieval)
    rows, groups = np.ones((2, 3), bool), np.zeros(4, np.int64)
    with pytest.raises(NotImplementedError, match="filter groups"):
        sh.range_search(None, allowed_masks=rows, query_group=groups)
    with pytest.raises(NotImplementedError, match="filter groups"):
        sh.search_fused(None, None, 10, allowed_masks=rows, query_group=groups)
    with pytest.raises(NotImplementedError, match="doc-sharded"):
        sh.range_search(None)
    with pytest.raises(NotImplementedError, match="doc-sharded"):
        sh.search_fused(None, None, 10)


def test_documents_say_what_is_offered():
    header = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    assert "Not offered under groups: range searches" not in header
    assert "Not offered: per-query masks" not in header
    from scaling_retriever_amd import hybrid
    assert "query_group" in hybrid.__doc__ and "doc-sharded indexes, per-query masks" not in hybrid.__doc__
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sr_dense_range_count_grouped" in readme and "### 4.21" in design and "2m" in integration


def test_grouped_range_kernels_use_no_scratch_and_the_existing_ones_are_unchanged(tmp_path):
    """Every grouped instantiation: no scratch, no spilled register (DESIGN.md 4.21 holds the tables of every instantiation, before and
    after the third filter mode)."""
    from test_abi import _kernel_metadata
    csrc = os.path.join(ROOT, "scaling_retriever_amd", "csrc")
    grouped = _kernel_metadata(os.path.join(csrc, "dense_range_grouped.o"), tmp_path)
    tiles = {k: v for k, v in grouped.items() if "dense_range_count_kernel" in k or "dense_range_fill_kernel" in k}
    assert len(tiles) == 8, sorted(grouped)          # {count, fill} x {128, 256 queries} x {fp32, fp16 rows}
    for name, m in tiles.items():
        assert m[".private_segment_fixed_size:"] == 0 and m[".vgpr_spill_count:"] == 0 and m[".vgpr_count:"] <= 256, (name, m)
    for obj in ("dense_range.o", "dense_range_masked.o"):      # the existing instantiations: still eight each, still without scratch
        meta = _kernel_metadata(os.path.join(csrc, obj), tmp_path)
        tiles = {k: v for k, v in meta.items() if "dense_range_count_kernel" in k or "dense_range_fill_kernel" in k}
        assert len(tiles) == 8, (obj, sorted(meta))
        for name, m in tiles.items():
            assert m[".private_segment_fixed_size:"] == 0 and m[".vgpr_spill_count:"] == 0, (obj, name, m)
    sparse = _kernel_metadata(os.path.join(csrc, "sparse_range.o"), tmp_path)
    kernels = {k: v for k, v in sparse.items() if "sparse_range_count_kernel" in k or "sparse_range_fill_kernel" in k}
    assert len(kernels) == 6, sorted(sparse)          # {count, fill} x {unrestricted, masked, grouped}
    for name, m in kernels.items():
        assert m[".private_segment_fixed_size:"] == 0 and m[".vgpr_spill_count:"] == 0, (name, m)
    # the grouped sparse kernels differ from the masked ones by the base of the mask words only: the same vector registers
    for half in ("count", "fill"):
        regs = {("ILb1ELb1E" in k): v[".vgpr_count:"] for k, v in kernels.items() if f"sparse_range_{half}_kernel" in k and "ILb1E" in k}
        assert regs[True] == regs[False], (half, regs)
