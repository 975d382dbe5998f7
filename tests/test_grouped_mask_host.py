"""CPU: the grouped dense search (sr_dense_search_grouped: a document bitmap per query) - the parts that need no GPU: the packing of
stacked bitmaps against its numpy definition, the C ABI's declaration and binding, the argument checks of the library and of the
Python layer, and the register budget of the grouped instantiation of dense_split_kernel as the built object records it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack_spec(flags):
    """bit (i & 31) of word i >> 5 is flags[i]"""
    words = np.zeros((len(flags) + 31) // 32, np.uint32)
    for i in np.flatnonzero(flags):
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 1001])
def test_pack_doc_masks_against_numpy(n, n_groups):
    import torch
    from scaling_retriever_amd.scoring import pack_doc_mask, pack_doc_masks
    rng = np.random.default_rng(n + 7 * n_groups)
    edge = np.zeros((n_groups, n), bool)                       # bits at the word boundaries and at both ends, another set per group
    for g in range(n_groups):
        edge[g, [i for i in (0, 30 + g, 31, 32, 33 + g, 63, 64, 95, 96, n - 2, n - 1) if 0 <= i < n]] = True
    for flags in (np.zeros((n_groups, n), bool), np.ones((n_groups, n), bool), rng.random((n_groups, n)) < 0.5, edge):
        for given in (flags, torch.from_numpy(flags)):
            got = pack_doc_masks(given)
            assert torch.is_tensor(got) and got.dtype == torch.int32 and tuple(got.shape) == (n_groups, (n + 31) // 32)
            for g in range(n_groups):
                assert np.array_equal(got[g].numpy().view(np.uint32), _pack_spec(flags[g])), g
                assert np.array_equal(got[g].numpy().view(np.uint32), pack_doc_mask(flags[g])), g
    with pytest.raises(ValueError, match="2-D"):
        pack_doc_masks(np.zeros(5, bool))
    with pytest.raises(ValueError, match="boolean"):
        pack_doc_masks(torch.zeros((2, 5), dtype=torch.int32))


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/sr_hip.h"
    return m.group(1), [a.strip() for a in m.group(2).split(",") if a.strip()]


def test_grouped_entry_point_is_declared_and_bound():
    from scaling_retriever_amd import _lib
    name = "sr_dense_search_grouped"
    lib = _lib.load()
    ret, args = _prototype(name)
    assert ret == "int" and len(args) == 11, args
    res, argtypes = _lib.SIGNATURES[name]
    assert res is _lib.c_int and len(argtypes) == 11
    for decl, ct in zip(args, argtypes):                       # pointers and streams are void*, sizes int64, k int
        want = _lib.c_void_p if ("*" in decl or decl.startswith("sr_stream")) else (_lib.c_int64 if decl.startswith("int64_t") else _lib.c_int)
        assert ct is want, (decl, ct)
    assert hasattr(lib, name)
    # d_group_words, n_groups, n_bits, d_query_group sit where the header puts them
    assert [a.split()[-1].lstrip("*") for a in args[4:8]] == ["d_group_words", "n_groups", "n_bits", "d_query_group"]
    assert argtypes[4] is _lib.c_void_p and argtypes[5] is _lib.c_int64 and argtypes[6] is _lib.c_int64 and argtypes[7] is _lib.c_void_p


def test_grouped_argument_checks_without_gpu():
    """Checks made before anything touches a device (the pointers are never dereferenced)."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    assert lib.sr_dense_search_grouped(None, p, 1, 10, p, 1, 0, p, p, p, None) == _lib.SR_ERR_INVALID and b"null index" in lib.sr_last_error()
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    try:
        rc = lib.sr_dense_search_grouped(h, p, 1, 10, p, 2, 32, p, p, p, None)
        assert rc == _lib.SR_ERR_INVALID and b"n_bits=32" in lib.sr_last_error(), lib.sr_last_error()
        assert lib.sr_dense_search_grouped(h, p, 1, 0, p, 1, 0, p, p, p, None) == _lib.SR_ERR_INVALID and b"outside [1" in lib.sr_last_error()
        rc = lib.sr_dense_search_grouped(h, p, 1, lib.sr_max_topk() + 1, p, 1, 0, p, p, p, None)
        assert rc == _lib.SR_ERR_INVALID and b"outside [1" in lib.sr_last_error()
        assert lib.sr_dense_search_grouped(h, p, 1, 10, p, 0, 0, p, p, p, None) == _lib.SR_ERR_INVALID and b"n_groups=0" in lib.sr_last_error()
        rc = lib.sr_dense_search_grouped(h, p, 1, 10, p, 1, 0, None, p, p, None)         # no group ids
        assert rc == _lib.SR_ERR_INVALID and b"null pointer" in lib.sr_last_error()
        assert lib.sr_dense_search_grouped(h, None, 1, 10, p, 1, 0, p, p, p, None) == _lib.SR_ERR_INVALID and b"null pointer" in lib.sr_last_error()
        assert lib.sr_dense_search_grouped(h, p, 0, 10, p, 1, 0, p, p, p, None) == _lib.SR_OK    # no queries: nothing to do
    finally:
        lib.sr_dense_index_destroy(h)


def test_python_layer_rejects_bad_arguments_before_any_upload():
    """DenseIndexHIP.search_grouped on a handle of an empty index (no device needed: id_end = 0) and the indexer's argument rules on
    objects that were never initialised - every error below is raised before a tensor goes to a device."""
    import torch
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    from scaling_retriever_amd.scoring import DenseIndexHIP
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    idx = object.__new__(DenseIndexHIP)
    idx.lib, idx._h, idx.dim = lib, h, 64                      # close() below destroys the handle
    try:
        q = torch.zeros((5, 64))
        ok_masks, ok_groups = np.zeros((2, 0), bool), np.zeros(5, np.int64)
        bad = [("float32", dict(queries=torch.zeros((5, 64), dtype=torch.float64), masks=ok_masks, query_group=ok_groups)),
               ("float32", dict(queries=torch.zeros((5, 32)), masks=ok_masks, query_group=ok_groups)),
               ("2-D", dict(queries=q, masks=np.zeros(4, bool), query_group=ok_groups)),
               ("bool", dict(queries=q, masks=np.zeros((2, 4), np.float32), query_group=ok_groups)),
               ("at least one group", dict(queries=q, masks=np.zeros((0, 4), bool), query_group=ok_groups)),
               ("words", dict(queries=q, masks=np.zeros((2, 3), np.uint32), query_group=ok_groups)),
               ("words", dict(queries=q, masks=torch.zeros((2, 1), dtype=torch.int32), query_group=ok_groups)),
               ("one group id per query", dict(queries=q, masks=ok_masks, query_group=np.zeros(4, np.int64))),
               ("one group id per query", dict(queries=q, masks=ok_masks, query_group=np.zeros((5, 1), np.int64))),
               ("integer", dict(queries=q, masks=ok_masks, query_group=np.zeros(5, np.float32))),
               ("integer", dict(queries=q, masks=ok_masks, query_group=torch.zeros(5, dtype=torch.bool))),
               ("cuda", dict(queries=q, masks=ok_masks, query_group=ok_groups))]
        for needle, kw in bad:
            with pytest.raises(ValueError, match=needle):
                idx.search_grouped(kw["queries"], 10, kw["masks"], kw["query_group"])
    finally:
        idx.close()
    ix = object.__new__(DenseFlatIndexer)
    flags, groups = np.ones((2, 4), bool), np.zeros(3, np.int64)
    for fn in (DenseFlatIndexer.search_knn, DenseFlatIndexer.search_arrays):
        with pytest.raises(ValueError, match="not both"):
            fn(ix, None, 10, allowed_mask=flags[0], allowed_masks=flags, query_group=groups)
        with pytest.raises(ValueError, match="not both"):
            fn(ix, None, 10, allowed_ids=["a"], allowed_masks=flags, query_group=groups)
        with pytest.raises(ValueError, match="go together"):
            fn(ix, None, 10, allowed_masks=flags)
        with pytest.raises(ValueError, match="go together"):
            fn(ix, None, 10, query_group=groups)


def _kernel_metadata(obj, tmp_path):
    """{mangled kernel name: {scratch bytes, spilled VGPRs / SGPRs, VGPRs}} of a built object (llvm-objcopy + clang-offload-bundler +
    llvm-readelf --notes), as tests/test_abi.py reads it."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(obj) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("needs the built object and the ROCm LLVM tools")
    tag = os.path.basename(obj)
    fat, dev = str(tmp_path / f"{tag}.fatbin"), str(tmp_path / f"{tag}.dev.o")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, str(tmp_path / f"{tag}.unused.o")])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={dev}", "--unbundle"])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", dev], capture_output=True, text=True).stdout
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", notes, flags=re.S):
        kernels[m.group(1)] = {key: int(v) for key, v in re.findall(r"(\.private_segment_fixed_size:|\.vgpr_spill_count:|\.sgpr_spill_count:|\.vgpr_count:)\s+(\d+)", m.group(2))}
    return kernels


def test_grouped_split_kernel_uses_no_scratch_and_no_more_registers(tmp_path):
    """The grouped pass is a third instantiation of a kernel that sits at the register limit: the built object must hold exactly that one
    instantiation, with no scratch and no spilled vector register, in no more vector registers than the single-mask instantiation."""
    csrc = os.path.join(ROOT, "scaling_retriever_amd", "csrc")
    grouped = {k: v for k, v in _kernel_metadata(os.path.join(csrc, "dense_split_grouped.o"), tmp_path).items() if "dense_split_kernel" in k}
    masked = {k: v for k, v in _kernel_metadata(os.path.join(csrc, "dense_split_masked.o"), tmp_path).items() if "dense_split_kernel" in k}
    assert len(grouped) == 1 and len(masked) == 1, (sorted(grouped), sorted(masked))
    (g_name, g), (m_name, m) = next(iter(grouped.items())), next(iter(masked.items()))
    assert g_name != m_name
    assert g[".private_segment_fixed_size:"] == 0 and g[".vgpr_spill_count:"] == 0, g
    assert g[".vgpr_count:"] <= m[".vgpr_count:"], (g, m)
