"""CPU: document bitmaps for the masked dense search (sr_dense_search_masked, csrc/doc_mask.hip) - the parts that need no GPU: the host
side packing against its numpy definition, the C ABI's declarations and bindings, and the argument checks of the Python layer."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack_spec(flags):
    """bit (i & 31) of word i >> 5 is flags[i]"""
    words = np.zeros((len(flags) + 31) // 32, np.uint32)
    for i in np.flatnonzero(flags):
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 200, 1001])
def test_pack_doc_mask_against_numpy(n):
    import torch
    from scaling_retriever_amd.scoring import pack_doc_mask
    rng = np.random.default_rng(n)
    cases = [np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.5]
    edge = np.zeros(n, bool)                                   # bits at the word boundaries and at both ends
    edge[[i for i in (0, 30, 31, 32, 33, 63, 64, 95, 96, n - 2, n - 1) if 0 <= i < n]] = True
    cases.append(edge)
    for flags in cases:
        want = _pack_spec(flags)
        got = pack_doc_mask(flags)
        assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want)
        t = pack_doc_mask(torch.from_numpy(flags))             # the tensor path (the device's, here on the host): the same bits as int32
        assert t.dtype == torch.int32 and np.array_equal(t.numpy().view(np.uint32), want)
    assert np.array_equal(pack_doc_mask(list(cases[2])), _pack_spec(cases[2]))
    with pytest.raises(ValueError):
        pack_doc_mask(np.zeros((2, 3), bool))


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/sr_hip.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",") if a.strip()]


def test_mask_entry_points_are_declared_and_bound():
    from scaling_retriever_amd import _lib
    arity = {"sr_dense_index_id_end": 1, "sr_doc_mask_from_list": 5, "sr_doc_list_from_mask": 6, "sr_dense_search_masked": 9}
    lib = _lib.load()
    for name, n in arity.items():
        ret, args = _prototype(name)
        assert len(args) == n, (name, args)
        res, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == n, name
        assert res is (_lib.c_int64 if ret == "int64_t" else _lib.c_int), name
        for decl, ct in zip(args, argtypes):                   # pointers and streams are void*, sizes int64, k int
            want = _lib.c_void_p if ("*" in decl or decl.startswith("sr_stream")) else (_lib.c_int64 if decl.startswith("int64_t") else _lib.c_int)
            assert ct is want, (name, decl, ct)
        assert hasattr(lib, name)
    # d_mask_words / n_bits sit where the header puts them
    masked = _lib.SIGNATURES["sr_dense_search_masked"][1]
    assert masked[4] is _lib.c_void_p and masked[5] is _lib.c_int64


def test_mask_argument_checks_without_gpu():
    """Checks made before anything touches a device (the pointers are never dereferenced)."""
    import ctypes
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.sr_dense_index_id_end(None) == -1
    assert lib.sr_dense_search_masked(None, p, 1, 10, p, 0, p, p, None) == _lib.SR_ERR_INVALID and b"null index" in lib.sr_last_error()
    assert lib.sr_doc_mask_from_list(p, -1, p, 64, None) == _lib.SR_ERR_INVALID
    assert lib.sr_doc_list_from_mask(p, 64, p, 10, None, None) == _lib.SR_ERR_INVALID and b"null pointer" in lib.sr_last_error()
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    try:
        assert lib.sr_dense_index_id_end(h) == 0               # an empty index
        rc = lib.sr_dense_search_masked(h, p, 1, 10, p, 32, p, p, None)
        assert rc == _lib.SR_ERR_INVALID and b"n_bits=32" in lib.sr_last_error(), lib.sr_last_error()
        assert lib.sr_dense_search_masked(h, p, 1, 0, p, 0, p, p, None) == _lib.SR_ERR_INVALID and b"outside [1" in lib.sr_last_error()
        assert lib.sr_dense_search_masked(h, p, 0, 10, p, 0, p, p, None) == _lib.SR_OK          # no queries: nothing to do
    finally:
        lib.sr_dense_index_destroy(h)


def test_subset_and_mask_together_raise():
    """The check comes before anything else is touched: the objects below are never initialised."""
    from scaling_retriever_amd.distributed import ShardedDenseRetriever
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    from scaling_retriever_amd.scoring import DenseIndexHIP
    with pytest.raises(ValueError, match="not both"):
        DenseIndexHIP.search(object.__new__(DenseIndexHIP), None, 10, subset=[1], mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="not both"):
        DenseFlatIndexer.search_arrays(object.__new__(DenseFlatIndexer), None, 10, allowed_ids=["a"], allowed_mask=np.ones(4, bool))
    with pytest.raises(NotImplementedError, match="allow-list"):
        ShardedDenseRetriever.search(object.__new__(ShardedDenseRetriever), None, 10, mask=np.ones(4, bool))
