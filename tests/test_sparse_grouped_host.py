"""CPU: the grouped sparse search (sr_sparse_search_grouped: a document bitmap per query, csrc/subset_search.hip, cert_score_kernel<KS, true,
true>) - the parts that need no GPU: the C ABI's declaration and binding, the argument checks of the library and of the Python layer, and
the register budget of every instantiation of cert_score_kernel as the built object records it."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_grouped_mask_host import _kernel_metadata, _prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sr_sparse_search_grouped"


def test_grouped_entry_point_is_declared_and_bound():
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    ret, args = _prototype(NAME)
    assert ret == "int" and len(args) == 17, args
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is _lib.c_int and len(argtypes) == 17
    for decl, ct in zip(args, argtypes):                       # pointers and streams are void*, sizes int64, k int, the threshold float
        want = _lib.c_void_p if ("*" in decl or decl.startswith("sr_stream")) else (
            _lib.c_int64 if decl.startswith("int64_t") else (_lib.c_float if decl.startswith("float") else _lib.c_int))
        assert ct is want, (decl, ct)
    assert hasattr(lib, NAME) and getattr(lib, NAME).argtypes == argtypes
    # the masked entry's layout with (d_group_words, n_groups, n_bits, d_query_group) where (d_mask_words, n_bits) stand
    assert [a.split()[-1].lstrip("*") for a in args[7:11]] == ["d_group_words", "n_groups", "n_bits", "d_query_group"]
    masked = _lib.SIGNATURES["sr_sparse_search_masked"][1]
    assert argtypes[:7] == masked[:7] and argtypes[11:] == masked[9:]


def test_grouped_argument_checks_without_gpu():
    """The null index is refused before anything else (the pointers are never dereferenced).  A sparse handle cannot be made without a
    device, so the checks against the handle (n_bits, n_groups, the word count, k, null pointers) are in tests/test_sparse_grouped_gpu.py."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.sr_sparse_search_grouped(None, p, p, p, 1, 10, 0.0, p, 1, 32, p, 0, 1, p, p, p, None) == _lib.SR_ERR_INVALID
    assert b"null index" in lib.sr_last_error()


def _handleless(n_docs):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    idx = object.__new__(SparseIndexHIP)                       # no handle, no device: the checks below must not need either
    idx.n_docs = n_docs
    return idx


def test_python_layer_rejects_bad_arguments_before_any_upload():
    import torch
    idx = _handleless(100)
    qi, qc, qv = np.array([0, 1, 2, 2, 3, 3], np.int64), np.array([3, 4, 5], np.int32), np.ones(3, np.float32)      # five queries
    ok_masks, ok_groups = np.zeros((2, 100), bool), np.zeros(5, np.int64)
    bad = [("2-D", dict(masks=np.zeros(100, bool), query_group=ok_groups)),
           ("2-D", dict(masks=np.zeros((1, 2, 50), bool), query_group=ok_groups)),
           ("bool", dict(masks=np.zeros((2, 100), np.float32), query_group=ok_groups)),
           ("at least one group", dict(masks=np.zeros((0, 100), bool), query_group=ok_groups)),
           (r"holds 4 words", dict(masks=np.zeros((2, 3), np.uint32), query_group=ok_groups)),
           (r"holds 4 words", dict(masks=torch.zeros((2, 5), dtype=torch.int32), query_group=ok_groups)),
           ("one group id per query", dict(masks=ok_masks, query_group=np.zeros(4, np.int64))),
           ("one group id per query", dict(masks=ok_masks, query_group=np.zeros((5, 1), np.int64))),
           ("integer", dict(masks=ok_masks, query_group=np.zeros(5, np.float32))),
           ("integer", dict(masks=ok_masks, query_group=torch.zeros(5, dtype=torch.bool)))]
    for needle, kw in bad:
        with pytest.raises(ValueError, match=needle):
            idx.search_grouped(qi, qc, qv, 10, kw["masks"], kw["query_group"])


def test_filter_groups_of_the_retrieval_drivers():
    from scaling_retriever_amd.indexer import HybridRetriever, ShardedSparseRetrieval, SparseRetrieval
    r = object.__new__(SparseRetrieval)
    r.hip_index = _handleless(12)
    r._dev = "cpu"
    flags, groups = np.ones((2, 12), bool), np.zeros(3, np.int64)
    for call in (lambda **kw: r._sparse_retrieve_multithreaded(None, [], **kw), lambda **kw: SparseRetrieval.retrieve(r, [], 5, **kw),
                 lambda **kw: r._resolve("x", **kw)):
        with pytest.raises(ValueError, match="not both"):
            call(allowed_mask=flags[0], allowed_masks=flags, query_group=groups)
        with pytest.raises(ValueError, match="not both"):
            call(allowed_ids=["a"], allowed_masks=flags, query_group=groups)
        with pytest.raises(ValueError, match="go together"):
            call(allowed_masks=flags)
        with pytest.raises(ValueError, match="go together"):
            call(query_group=groups)
    for bad in (np.ones((2, 11), bool), np.ones(12, bool), np.ones((0, 12), bool)):
        with pytest.raises(ValueError, match=r"one flag per document position \(12\)"):
            r._resolve("x", allowed_masks=bad, query_group=groups)
    with pytest.raises(ValueError, match="integer"):
        r._resolve("x", allowed_masks=flags, query_group=np.zeros(3, np.float32))
    filt = r._resolve("x", allowed_masks=flags, query_group=groups)       # packed where the flags live: here the host
    assert filt.kind == "groups" and tuple(filt.data.shape) == (2, 1) and int(filt.data[0, 0]) == (1 << 12) - 1 and filt.groups.tolist() == [0, 0, 0]
    with pytest.raises(NotImplementedError, match="allowed_masks"):
        ShardedSparseRetrieval.retrieve(object.__new__(ShardedSparseRetrieval), None, 5, allowed_masks=flags, query_group=groups)
    h = object.__new__(HybridRetriever)
    for fn in (HybridRetriever.retrieve, HybridRetriever.retrieve_fused):
        with pytest.raises(ValueError, match="not both"):
            fn(h, [], 5, allowed_ids=["a"], allowed_masks=flags, query_group=groups)
        with pytest.raises(ValueError, match="go together"):
            fn(h, [], 5, allowed_masks=flags)
        with pytest.raises(ValueError, match="go together"):
            fn(h, [], 5, query_group=groups)


def _figures(path):
    """{kernel name: (scratch, vgpr, vspill)} of the `after` section of profiles/sparse_mask_kernel_meta.txt"""
    text = open(path).read().split("== after")[1]
    return {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4)))
            for m in re.finditer(r"^(\S+) scratch=(\d+) sgpr=\d+ vgpr=(\d+) vspill=(\d+)", text, flags=re.M)}


def test_score_kernel_twins_keep_their_register_budget(tmp_path):
    """cert_score_kernel sits exactly at 128 VGPRs (16 waves of one workgroup per CU).  Every grouped twin <KS, true, true> must stay inside
    that budget with no more scratch than its masked twin and no spilled vector register (scalar registers parked in lanes of a vector
    register are inside the 128 and are what every twin does: profiles/sparse_grouped_kernel_meta.txt); the masked and the plain twins keep the figures recorded for them
    before the grouped twin existed (profiles/sparse_mask_kernel_meta.txt).  Registers, scratch and spills only."""
    meta = _kernel_metadata(os.path.join(ROOT, "scaling_retriever_amd", "csrc", "sparse_cert.o"), tmp_path)
    twins = {}
    for name, v in meta.items():
        m = re.match(r"_Z17cert_score_kernelILi(\d+)ELb([01])ELb([01])EEv8CertArgs$", name)
        if m:
            twins[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = v
    ks_all = (1, 2, 4, 5, 6, 7, 8)
    assert sorted(twins) == sorted((ks, mk, gr) for ks in ks_all for mk, gr in ((0, 0), (1, 0), (1, 1))), sorted(twins)
    recorded = _figures(os.path.join(ROOT, "profiles", "sparse_mask_kernel_meta.txt"))
    assert len(recorded) == 14
    for ks in ks_all:
        plain, masked, grouped = twins[(ks, 0, 0)], twins[(ks, 1, 0)], twins[(ks, 1, 1)]
        for mk, v in ((0, plain), (1, masked)):
            want = recorded[f"_Z17cert_score_kernelILi{ks}ELb{mk}EEv8CertArgs"]
            got = (v[".private_segment_fixed_size:"], v[".vgpr_count:"], v[".vgpr_spill_count:"])
            assert got == want, (ks, mk, got, want)
        assert grouped[".vgpr_count:"] <= 128, (ks, grouped)
        assert grouped[".private_segment_fixed_size:"] <= masked[".private_segment_fixed_size:"] <= 68, (ks, grouped, masked)
        assert grouped[".vgpr_spill_count:"] == 0, (ks, grouped)
