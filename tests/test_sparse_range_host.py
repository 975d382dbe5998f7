"""CPU side of the sparse range search: the two entry points are declared, exported and bound, a null index is rejected before any
device work with `total` untouched, and the built kernels use no scratch."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_sparse_range_count", "sr_sparse_range_fill")


def test_sparse_range_symbols_declared_exported_and_bound():
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    for name in NAMES:
        assert f"int {name}(" in header
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["sr_sparse_range_count"][1]) == 9 and len(_lib.SIGNATURES["sr_sparse_range_fill"][1]) == 13
    # declared next to sr_sparse_search_subset, and the comment cites the reference's scorer
    at = header.index("int sr_sparse_range_count(")
    assert header.index("int sr_sparse_search_subset(") < at < header.index("int sr_sparse_index_destroy(")
    assert "scaling_retriever/indexer.py:324-344" in header[header.index("int sr_sparse_search_subset("):at]


def test_sparse_range_calls_reject_a_null_index():
    """SR_ERR_INVALID with a message; the pointers below are never dereferenced, no device exists, `total` keeps its value."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    total = ctypes.c_int64(-5)
    rc = lib.sr_sparse_range_count(None, p, p, p, 4, p, p, ctypes.byref(total), None)
    assert rc == _lib.SR_ERR_INVALID and b"sr_sparse_range_count: null index" in lib.sr_last_error(), (rc, lib.sr_last_error())
    assert total.value == -5
    rc = lib.sr_sparse_range_fill(None, p, p, p, 4, p, p, 0, 1, p, p, 10, None)
    assert rc == _lib.SR_ERR_INVALID and b"sr_sparse_range_fill: null index" in lib.sr_last_error(), (rc, lib.sr_last_error())


def test_sparse_range_kernels_use_no_scratch(tmp_path):
    """Count and fill keep two register sets of posting loads and the cursor of the group walk: every kernel of the object builds
    without scratch and without a spilled register."""
    from test_abi import _kernel_metadata
    meta = _kernel_metadata(os.path.join(ROOT, "scaling_retriever_amd", "csrc", "sparse_range.o"), tmp_path)
    assert any("sparse_range_count_kernel" in k for k in meta) and any("sparse_range_fill_kernel" in k for k in meta), sorted(meta)
    for name, m in meta.items():
        assert m[".private_segment_fixed_size:"] == 0 and m[".vgpr_spill_count:"] == 0, (name, m)


def test_the_gpu_cases_are_what_their_docstring_says():
    """The fixtures of tests/test_sparse_range_gpu.py against the oracle alone: ties at the 3 000th best score, strictness that matters,
    empty and full lists."""
    from test_sparse_range_gpu import KINDS, NQ_ALL, SHAPES, _all_scores, _expected, _thresholds
    for n_docs in SHAPES:
        thr = _thresholds(n_docs, NQ_ALL)
        counts = np.diff(_expected(n_docs, thr)[0])
        assert counts.max() == n_docs and counts.min() == 0
        tied = 0
        for q in range(NQ_ALL):
            if (q % KINDS) == 3:
                s = _all_scores(n_docs, q)
                tied += int((s == thr[q]).sum() >= 2)
                assert (s > thr[q]).sum() < (s >= thr[q]).sum()          # >= would return more
        assert tied >= 2, (n_docs, tied)
