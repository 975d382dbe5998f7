"""CPU side of the dense range search: the two entry points are exported and bound, reject bad arguments before any device work,
the Python sort helper orders as numpy's lexsort does, and the built kernels use no scratch."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_symbols_exported_and_bound():
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    for name in ("sr_dense_range_count", "sr_dense_range_fill"):
        assert f"int {name}(" in header
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_range_calls_validate_before_any_device_work():
    """Null and bad arguments: SR_ERR_INVALID with a message; the pointers below are never dereferenced and no device exists."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    total = ctypes.c_int64(-5)
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    count_cases = [
        ((None, p, 4, p, p, ctypes.byref(total), None), b"null index"),
        ((h, p, -1, p, p, ctypes.byref(total), None), b"bad nq"),
        ((h, p, 4, p, None, ctypes.byref(total), None), b"null d_lims or total"),
        ((h, p, 4, p, p, None, None), b"null d_lims or total"),
        ((h, None, 4, p, p, ctypes.byref(total), None), b"null queries or thresholds"),
        ((h, p, 4, None, p, ctypes.byref(total), None), b"null queries or thresholds"),
        ((h, ctypes.c_void_p(4100), 4, p, p, ctypes.byref(total), None), b"16-byte aligned"),
    ]
    for args, text in count_cases:
        rc = lib.sr_dense_range_count(*args)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (text, rc, lib.sr_last_error())
    assert total.value == -5
    with pytest.raises(ValueError):
        _lib.check(lib.sr_dense_range_count(h, p, -1, p, p, ctypes.byref(total), None), "sr_dense_range_count")
    fill_cases = [
        ((None, p, 4, p, p, p, p, 10, None), b"null index"),
        ((h, p, -1, p, p, p, p, 10, None), b"bad nq"),
        ((h, p, 4, p, p, p, p, -1, None), b"capacity"),
        ((h, p, 4, p, p, p, p, 10, None), b"no sr_dense_range_count precedes"),
    ]
    for args, text in fill_cases:
        rc = lib.sr_dense_range_fill(*args)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (text, rc, lib.sr_last_error())
    assert lib.sr_dense_index_destroy(h) == 0


def test_range_sort_orders_like_lexsort():
    """Per query: score descending, ties by ascending id; lims untouched.  Ties, negative scores, empty lists and a single entry."""
    from scaling_retriever_amd.scoring import range_sort
    rng = np.random.default_rng(3)
    counts = np.array([0, 7, 1, 0, 40, 13, 0], np.int64)
    lims = np.concatenate([[0], np.cumsum(counts)])
    total = int(lims[-1])
    scores = rng.choice(np.array([-1.5, -0.25, 0.125, 0.5, 2.0, 3.75], np.float32), size=total)      # many ties
    ids = rng.permutation(10 * total)[:total].astype(np.int64)
    s, i = range_sort(torch.from_numpy(lims), torch.from_numpy(scores), torch.from_numpy(ids))
    query = np.repeat(np.arange(len(counts)), counts)
    order = np.lexsort((ids, -scores, query))
    assert np.array_equal(i.numpy(), ids[order]) and np.array_equal(s.numpy(), scores[order])
    e = torch.zeros(0)
    s, i = range_sort(torch.zeros(3, dtype=torch.int64), e, e.long())
    assert s.numel() == 0 and i.numel() == 0


def test_range_kernels_use_no_scratch(tmp_path):
    """The count and fill kernels keep 128 accumulators through a tile loop; a lane-derived value hoisted out of that loop is spilled
    through the k-loop (it was, before the per-query state moved to LDS).  Every instantiation: no scratch, no spilled register."""
    from test_abi import _kernel_metadata
    meta = _kernel_metadata(os.path.join(ROOT, "scaling_retriever_amd", "csrc", "dense_range.o"), tmp_path)
    tiles = {k: v for k, v in meta.items() if "dense_range_count_kernel" in k or "dense_range_fill_kernel" in k}
    assert len(tiles) == 8, sorted(meta)          # {count, fill} x {128, 256 queries} x {fp32, fp16 rows}
    for name, m in meta.items():
        if "dense_range" in name:
            assert m[".private_segment_fixed_size:"] == 0 and m[".vgpr_spill_count:"] == 0 and m[".vgpr_count:"] <= 256, (name, m)
