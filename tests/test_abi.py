"""CPU: libsr_hip.so loads and exports every symbol include/sr_hip.h declares; argument
validation that needs no GPU behaves like the reference's asserts."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "sr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound():
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in sr_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert set(_lib.SIGNATURES) == set(names)


def test_status_codes_and_error_strings_without_gpu():
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    assert lib.sr_version() >= 1 and lib.sr_max_topk() >= 1000
    h = ctypes.c_void_p()
    rc = lib.sr_dense_index_create(ctypes.byref(h), 30)
    assert rc == _lib.SR_ERR_INVALID and b"multiple of 16" in lib.sr_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "sr_dense_index_create")
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0
    assert lib.sr_dense_index_ntotal(h) == 0
    assert lib.sr_dense_index_destroy(h) == 0


def test_attention_f32_hook_validates_before_it_launches():
    """sr_attention_varlen_f32 rejects what it cannot run with SR_ERR_INVALID before anything touches a device: the pointers
    below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    ok = dict(qkv=p, f32=p, planes=None, fp32_planes=0, cu=p, kv=p, B=1, nh=4, nkv=1, hd=64, max_seqlen=8)
    for change, text in [(dict(qkv=None), b"null pointer"), (dict(cu=None), b"null pointer"), (dict(kv=None), b"null pointer"),
                         (dict(planes=p, fp32_planes=3), b"exactly one"), (dict(f32=None), b"exactly one"),
                         (dict(f32=None, planes=p, fp32_planes=16), b"fp32_planes 16"), (dict(f32=None, planes=p, fp32_planes=0), b"fp32_planes 0"),
                         (dict(B=-1), b"bad sizes"), (dict(max_seqlen=-1), b"bad sizes"), (dict(nkv=0), b"bad sizes"),
                         (dict(nh=6, nkv=4), b"not a multiple")]:
        a = dict(ok, **change)
        rc = lib.sr_attention_varlen_f32(a["qkv"], a["f32"], a["planes"], a["fp32_planes"], a["cu"], a["kv"], a["B"], a["nh"], a["nkv"],
                                         a["hd"], a["max_seqlen"], None)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())


def test_fp16_plane_hooks_validate_before_they_launch():
    """sr_rows_split_f16, sr_gu_cmax_f16 and sr_gemm_f16_planes reject what they cannot run with SR_ERR_INVALID before anything
    touches a device: the pointers below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def split(**kw):
        a = dict(dict(src=p, embed=None, tok=None, w=p, eps=1e-5, T=4, K=64, nseg=3, planes=p, inv=p, cmax=None, sc=None, si=None), **kw)
        return lib.sr_rows_split_f16(a["src"], a["embed"], a["tok"], a["w"], a["eps"], a["T"], a["K"], a["nseg"], a["planes"], a["inv"],
                                     a["cmax"], a["sc"], a["si"], None)
    for change, text in [(dict(src=None), b"null pointer"), (dict(planes=None), b"null pointer"), (dict(inv=None), b"null pointer"),
                         (dict(embed=p), b"both d_embed and d_tok_id"), (dict(tok=p), b"both d_embed and d_tok_id"),
                         (dict(embed=p, tok=p, w=None), b"needs d_norm_w"), (dict(cmax=p), b"needs d_act_sc"),
                         (dict(cmax=p, sc=p), b"needs d_act_sc"), (dict(nseg=1), b"nseg 1"), (dict(nseg=4), b"nseg 4"),
                         (dict(K=66), b"multiple of 4"), (dict(K=0), b"bad sizes"), (dict(T=-1), b"bad sizes"),
                         (dict(src=ctypes.c_void_p(4100)), b"aligned"), (dict(planes=ctypes.c_void_p(4100)), b"aligned")]:
        rc = split(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert split(T=0) == _lib.SR_OK

    for args, text in [((None, p, 32, 64, 3, p), b"null pointer"), ((p, None, 32, 64, 3, p), b"null pointer"),
                       ((p, p, 32, 64, 3, None), b"null pointer"), ((p, p, 32, 64, 4, p), b"nseg 4"), ((p, p, 32, 64, 0, p), b"nseg 0"),
                       ((p, p, 24, 64, 3, p), b"bad sizes"), ((p, p, 32, 0, 3, p), b"bad sizes")]:
        rc = lib.sr_gu_cmax_f16(*args, None)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (args, rc, lib.sr_last_error())

    def gemm(**kw):
        a = dict(dict(A=p, W=p, M=8, N=128, K=192, epi=10, a_nseg=3, a_sc=p, w_sc=p, C=p, pos=None, cos=None, sin=None, n_rope=0, hd=64,
                      bias=None, seq=None, osc=None, out_nseg=0), **kw)
        return lib.sr_gemm_f16_planes(a["A"], a["W"], a["M"], a["N"], a["K"], a["epi"], a["a_nseg"], a["a_sc"], a["w_sc"], a["C"],
                                      a["pos"], a["cos"], a["sin"], a["n_rope"], a["hd"], a["bias"], a["seq"], a["osc"], a["out_nseg"], None)
    for change, text in [(dict(A=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(C=None), b"null pointer"),
                         (dict(a_sc=None), b"null pointer"), (dict(w_sc=None), b"null pointer"),
                         (dict(epi=8), b"unknown epilogue 8"), (dict(epi=14), b"unknown epilogue 14"), (dict(epi=1), b"unknown epilogue 1"),
                         (dict(a_nseg=0), b"a_nseg 0"), (dict(a_nseg=4), b"a_nseg 4"), (dict(K=200), b"bad shape"),
                         (dict(K=128), b"bad shape"), (dict(M=-1), b"bad shape"), (dict(N=0), b"bad shape"),
                         (dict(epi=9), b"needs d_pos"), (dict(epi=9, pos=p, cos=p), b"needs d_pos"), (dict(bias=p), b"takes a bias"),
                         (dict(epi=12), b"needs d_seq_of"), (dict(epi=13, out_nseg=3), b"needs d_out_scale"),
                         (dict(epi=13, osc=p, out_nseg=1), b"out_nseg 1"), (dict(epi=13, osc=p, out_nseg=4), b"out_nseg 4"),
                         (dict(epi=9, pos=p, cos=p, sin=p, hd=96, n_rope=96), b"head_dim 96"),
                         (dict(epi=9, pos=p, cos=p, sin=p, hd=64, n_rope=32), b"bad rope arguments"),
                         (dict(epi=11, N=144), b"multiple of 16 (32 for SwiGLU)")]:
        rc = gemm(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert gemm(M=0) == _lib.SR_OK
    n = ctypes.c_int64(0)
    rc = lib.sr_model_fused_act_layers(None, None, 0, ctypes.byref(n))
    assert rc == _lib.SR_ERR_INVALID and b"null argument" in lib.sr_last_error()


def test_bf16_regime_hooks_validate_before_they_launch():
    """sr_rmsnorm_bf16, sr_dense_head_pool, sr_sparse_finish and sr_encode_plan reject what they cannot run with SR_ERR_INVALID before
    anything touches a device: the pointers below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p, odd8, odd16 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)

    def norm(**kw):
        a = dict(dict(x=p, embed=None, tok=None, delta=None, w=p, xn=p, f32=None, eps=1e-5, T=4, H=64), **kw)
        return lib.sr_rmsnorm_bf16(a["x"], a["embed"], a["tok"], a["delta"], a["w"], a["xn"], a["f32"], a["eps"], a["T"], a["H"], None)
    for change, text in [(dict(x=None), b"null pointer"), (dict(embed=p), b"both d_embed and d_tok_id"), (dict(tok=p), b"both d_embed and d_tok_id"),
                         (dict(w=None), b"needs d_norm_w"), (dict(w=None, xn=None, f32=p), b"needs d_norm_w"),
                         (dict(H=66), b"multiple of 4"), (dict(H=0), b"bad sizes"), (dict(T=-1), b"bad sizes"),
                         (dict(x=odd16), b"aligned"), (dict(w=odd16), b"aligned"), (dict(f32=odd16), b"aligned"),
                         (dict(embed=odd16, tok=p), b"aligned"), (dict(delta=odd8), b"aligned"), (dict(xn=odd8), b"aligned")]:
        rc = norm(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert norm(T=0) == _lib.SR_OK and norm(T=0, w=None, xn=None, delta=p) == _lib.SR_OK

    def pool(**kw):
        a = dict(dict(x=p, w=p, cu=p, pos=p, ps=p, eps=1e-5, B=2, T=4, H=64, stats=p, out=p), **kw)
        return lib.sr_dense_head_pool(a["x"], a["w"], a["cu"], a["pos"], a["ps"], a["eps"], a["B"], a["T"], a["H"], a["stats"], a["out"], None)
    for change, text in [(dict(x=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(cu=None), b"null pointer"),
                         (dict(pos=None), b"null pointer"), (dict(ps=None), b"null pointer"), (dict(stats=None), b"null pointer"),
                         (dict(out=None), b"null pointer"), (dict(B=-1), b"bad sizes"), (dict(T=-1), b"bad sizes"), (dict(H=0), b"bad sizes"),
                         (dict(H=130), b"multiple of 4"), (dict(x=odd16), b"aligned"), (dict(w=odd16), b"aligned"), (dict(stats=odd8), b"aligned")]:
        rc = pool(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert pool(B=0) == _lib.SR_OK

    for args, text in [((None, 8, 1.0, 1), b"null pointer"), ((p, -1, 1.0, 1), b"bad size"), ((p, 1 << 39, 1.0, 0), b"bad size"),
                       ((p, 8, 1.0, 2), b"round_bf16"), ((p, 8, 1.0, -1), b"round_bf16")]:
        rc = lib.sr_sparse_finish(*args, None)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (args, rc, lib.sr_last_error())
    assert lib.sr_sparse_finish(p, 0, 1.0, 1, None) == _lib.SR_OK

    n = ctypes.c_int64(-1)

    def plan(**kw):
        a = dict(dict(ids=p, mask=p, B=2, L=8, mode=0, vocab=100, shift=None, st=p, ln=p, ps=p, rl=p, cu=p, tok=p, pos=p, kv=p, sq=p,
                      cap=16, n=ctypes.byref(n)), **kw)
        return lib.sr_encode_plan(a["ids"], a["mask"], a["B"], a["L"], a["mode"], a["vocab"], a["shift"], a["st"], a["ln"], a["ps"], a["rl"],
                                  a["cu"], a["tok"], a["pos"], a["kv"], a["sq"], a["cap"], a["n"], None)
    for change, text in [(dict(ids=None), b"null pointer"), (dict(mask=None), b"null pointer"), (dict(st=None), b"null pointer"),
                         (dict(ln=None), b"null pointer"), (dict(ps=None), b"null pointer"), (dict(rl=None), b"null pointer"),
                         (dict(cu=None), b"null pointer"), (dict(n=None), b"null pointer"),
                         (dict(tok=None), b"null token array"), (dict(pos=None), b"null token array"), (dict(kv=None), b"null token array"),
                         (dict(sq=None), b"null token array"), (dict(cap=-1), b"null token array"),
                         (dict(mode=3), b"mode 3"), (dict(mode=-1), b"mode -1"), (dict(B=0), b"bad sizes"), (dict(L=0), b"bad sizes"),
                         (dict(vocab=0), b"bad sizes"), (dict(B=65537), b"bad sizes"), (dict(B=65536, L=32768), b"bad sizes")]:
        rc = plan(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert n.value == -1


def test_split_bf16_hook_validates_before_it_launches():
    """sr_split_bf16 rejects what it cannot run with SR_ERR_INVALID before anything touches a device: the pointers below are never
    dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p, odd8, odd4 = ctypes.c_void_p(4096), ctypes.c_void_p(4104), ctypes.c_void_p(4100)
    for args, text in [((None, 8, p, p, p), b"null pointer"), ((p, 8, None, p, p), b"null pointer"), ((p, 8, None, None, None), b"null pointer"),
                       ((p, 6, p, p, p), b"multiple of 4"), ((p, 1, p, None, None), b"multiple of 4"), ((p, -4, p, p, p), b"bad size"),
                       ((odd8, 8, p, p, p), b"aligned"), ((p, 8, odd4, p, p), b"aligned"), ((p, 8, p, odd4, p), b"aligned"),
                       ((p, 8, p, p, odd4), b"aligned")]:
        rc = lib.sr_split_bf16(*args, None)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (args, rc, lib.sr_last_error())
    assert lib.sr_split_bf16(p, 0, p, None, None, None) == _lib.SR_OK and lib.sr_split_bf16(p, 0, p, p, p, None) == _lib.SR_OK


def test_topk_replay_hook_validates_before_it_launches():
    """sr_topk_replay rejects what it cannot run with SR_ERR_INVALID before anything touches a device: the device pointers below are
    never dereferenced (h_steps is host memory and is read)."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    max_k = lib.sr_max_topk()

    def replay(**kw):
        a = dict(dict(sc=p, ids=p, nq=3, n=100, steps=[0, 40, 40, 100], k=10, k2=0, over=20, filter=1, seg_n=0, seg_group=1, out_s=p,
                      out_i=p, out_c=p, t_tau=p, t_tau2=p, t_cand=p, t_run=p, t_keys=None), **kw)
        steps = a["steps"]
        h = None if steps is None else (ctypes.c_int64 * len(steps))(*steps)
        n_steps = a.get("n_steps", 0 if steps is None else len(steps) - 1)
        return lib.sr_topk_replay(a["sc"], a["ids"], a["nq"], a["n"], h, n_steps, a["k"], a["k2"], a["over"], a["filter"], a["seg_n"],
                                  a["seg_group"], float("-inf"), -1.0, a["out_s"], a["out_i"], a["out_c"], a["t_tau"], a["t_tau2"],
                                  a["t_cand"], a["t_run"], a["t_keys"], None)
    for change, text in [(dict(sc=None), b"null pointer"), (dict(ids=None), b"null pointer"), (dict(steps=None, n_steps=1), b"null pointer"),
                         (dict(out_s=None), b"null pointer"), (dict(out_i=None), b"null pointer"), (dict(out_c=None), b"null pointer"),
                         (dict(t_tau=None), b"null pointer"), (dict(t_tau2=None), b"null pointer"), (dict(t_cand=None), b"null pointer"),
                         (dict(t_run=None), b"null pointer"),
                         (dict(nq=-1), b"bad sizes"), (dict(n=-1), b"bad sizes"), (dict(n_steps=-1), b"bad sizes"),
                         (dict(k=0), b"k = 0"), (dict(k=(1 << 20) + 1), b"k = 1048577"),
                         (dict(k2=-1), b"k2 = -1"), (dict(k2=10), b"k2 = 10"), (dict(k=max_k + 1, k2=1), b"k2 = 1"),
                         (dict(filter=2), b"filter 2"),
                         (dict(seg_n=6), b"seg_n = 6"), (dict(seg_n=-4), b"seg_n = -4"), (dict(k=max_k + 1, seg_n=8), b"seg_n = 8"),
                         (dict(seg_n=8, seg_group=0), b"seg_group = 0"),
                         (dict(steps=[0, 50, 40, 100]), b"steps must ascend"), (dict(steps=[-1, 40]), b"steps must ascend"),
                         (dict(steps=[0, 40, 101]), b"steps must ascend"),
                         (dict(n=1 << 23, steps=[0, (1 << 22) + 1]), b"more than 2^22")]:
        rc = replay(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert replay(nq=0) == _lib.SR_OK and replay(nq=0, k=max_k + 1, over=0, t_keys=p) == _lib.SR_OK


def test_attention_bf16_hook_empty_batch_and_head_geometry():
    """sr_attention_varlen: B = 0 is SR_OK, and num_heads that is no multiple of num_kv_heads is SR_ERR_INVALID - both before
    anything touches a device: the pointers below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    for hd in (64, 128):
        assert lib.sr_attention_varlen(p, p, p, None, p, None, None, 0, 4, 1, hd, None) == _lib.SR_OK
        rc = lib.sr_attention_varlen(p, p, p, None, p, None, None, 0, 6, 4, hd, None)
        assert rc == _lib.SR_ERR_INVALID and b"not a multiple" in lib.sr_last_error(), (rc, lib.sr_last_error())


def test_missing_extension_fails_loudly(monkeypatch, tmp_path):
    from scaling_retriever_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.SrHipError):
        _lib.load()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "scaling_retriever_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "liboracle" not in txt, f


def test_four_wave_gemm_kernels_use_no_scratch(tmp_path):
    """The four-wave GEMM loop pins its 256 accumulators to registers with inline-asm constraints; an epilogue that raises the
    register pressure makes hipcc spill ACCUMULATORS inside the k-loop (the QKV + RoPE epilogues did: fp32-regime query encode
    300 -> 670 ms, every parity test still green).  The built object's kernel metadata must show no scratch and no spill for
    every instantiation of that loop (..., KL = 1)."""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(ROOT, "scaling_retriever_amd", "csrc", "gemm_bf16.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("needs the built object and the ROCm LLVM tools")
    fat, dev = str(tmp_path / "g.fatbin"), str(tmp_path / "g_dev.o")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, str(tmp_path / "unused.o")])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={dev}", "--unbundle"])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", dev], capture_output=True, text=True).stdout
    # one YAML map per kernel; its keys are sorted, so everything between two `.name:` lines past a kernel's own name up to
    # `.wavefront_size:` belongs to it (.private_segment_fixed_size, .sgpr_spill_count, .vgpr_spill_count all sort after .name)
    import re
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", notes, flags=re.S):
        body = m.group(2)
        kernels[m.group(1)] = {key: int(v) for key, v in re.findall(r"(\.private_segment_fixed_size:|\.vgpr_spill_count:|\.sgpr_spill_count:)\s+(\d+)", body)}
    four_wave = {k: v for k, v in kernels.items() if k.startswith("_Z16gemm_bf16_kernel") and k.endswith("ELi1EEv8GemmArgs")}
    assert len(four_wave) >= 4, sorted(kernels)[:5]
    for name, meta in four_wave.items():
        assert meta[".private_segment_fixed_size:"] == 0 and meta[".vgpr_spill_count:"] == 0, (name, meta)


def _kernel_metadata(obj, tmp_path):
    """{mangled kernel name: {scratch bytes, spilled VGPRs / SGPRs, VGPRs}} of a built object (llvm-objcopy + clang-offload-bundler + llvm-readelf --notes)."""
    import re
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(obj) and os.path.exists(os.path.join(llvm, "clang-offload-bundler"))):
        pytest.skip("needs the built object and the ROCm LLVM tools")
    fat, dev = str(tmp_path / "k.fatbin"), str(tmp_path / "k_dev.o")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj, str(tmp_path / "unused.o")])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={dev}", "--unbundle"])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", dev], capture_output=True, text=True).stdout
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size:", notes, flags=re.S):
        kernels[m.group(1)] = {key: int(v) for key, v in re.findall(r"(\.private_segment_fixed_size:|\.vgpr_spill_count:|\.sgpr_spill_count:|\.vgpr_count:)\s+(\d+)", m.group(2))}
    return kernels


def test_dense_split_and_head128_attention_kernels_use_no_scratch(tmp_path):
    """Round 6: the headline's dominant kernel had sat at 0.45 of peak for four rounds because hipcc hoisted lane-derived values out of the
    persistent tile loop and spilled 29 of them through the 256-register k-loop - a chain of scratch round trips in front of every tile
    that no parity test could see.  The built objects must show no scratch for both instantiations of dense_split_kernel, and for the
    head-128 attention kernels (1 300 spilled registers until their occupancy bound was lowered)."""
    csrc = os.path.join(ROOT, "scaling_retriever_amd", "csrc")
    split = {k: v for k, v in _kernel_metadata(os.path.join(csrc, "dense_split.o"), tmp_path).items() if "dense_split_kernel" in k}
    assert len(split) == 2, sorted(split)
    for name, meta in split.items():
        assert meta[".private_segment_fixed_size:"] == 0 and meta[".vgpr_spill_count:"] == 0, (name, meta)
    # + the head-128 long kernel's default plans (2 or 3 key blocks per chunk: what an 8B batch with a passage over 64 tokens runs; 9-25
    # spilled registers until its occupancy bound was lowered to two waves per SIMD as well)
    attn = {k: v for k, v in _kernel_metadata(os.path.join(csrc, "attention.o"), tmp_path).items()
            if "attention_small_kernelILi128" in k or "attention_long_kernelILi128ELi2" in k or "attention_long_kernelILi128ELi3" in k}
    assert len(attn) >= 6, sorted(attn)
    for name, meta in attn.items():
        assert meta[".private_segment_fixed_size:"] == 0 and meta[".vgpr_spill_count:"] == 0, (name, meta)


def test_index_build_kernels_fit_two_workgroups_per_cu(tmp_path):
    """radix_scatter_tile_kernel (round 6) is sized for TWO workgroups of 512 threads per CU - one's barriers overlap the other's
    stores: at most 128 registers per lane, no scratch, and its 56 KB of dynamic LDS twice in the CU's 160 KB (checked where the
    launch computes it: csrc/sparse_build.hip)."""
    meta = _kernel_metadata(os.path.join(ROOT, "scaling_retriever_amd", "csrc", "sparse_build.o"), tmp_path)
    tile = [v for k, v in meta.items() if "radix_scatter_tile_kernel" in k]
    assert len(tile) == 1, sorted(meta)
    assert tile[0][".private_segment_fixed_size:"] == 0 and tile[0][".vgpr_spill_count:"] == 0 and tile[0][".vgpr_count:"] <= 128, tile[0]
    for name, m in meta.items():
        if "radix_" in name:
            assert m[".private_segment_fixed_size:"] == 0, (name, m)


def test_sparse_cert_readout_hook_validates_before_it_touches_a_device():
    """sr_sparse_index_cert_readout without an index (or without a size pointer) is SR_ERR_INVALID; nothing is dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    for idx, np_ in [(None, ctypes.byref(n)), (ctypes.c_void_p(4096), None)]:
        rc = lib.sr_sparse_index_cert_readout(idx, 0, None, 0, np_)
        assert rc == _lib.SR_ERR_INVALID and b"null argument" in lib.sr_last_error()
    assert n.value == -1


def test_model_readout_and_lora_merge_validate_before_they_touch_a_device():
    """sr_model_readout without a model or without one of its size pointers, and sr_lora_merge with a null pointer or 2^21 rows, are
    SR_ERR_INVALID; nothing is dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    n, rows, elems = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    p = ctypes.c_void_p(4096)
    for m, a, b, c in [(None, ctypes.byref(n), ctypes.byref(rows), ctypes.byref(elems)), (p, None, ctypes.byref(rows), ctypes.byref(elems)),
                       (p, ctypes.byref(n), None, ctypes.byref(elems)), (p, ctypes.byref(n), ctypes.byref(rows), None)]:
        rc = lib.sr_model_readout(m, -1, 0, 0, None, 0, a, b, c)
        assert rc == _lib.SR_ERR_INVALID and b"null argument" in lib.sr_last_error()
    assert (n.value, rows.value, elems.value) == (-1, -1, -1)
    rc = lib.sr_lora_merge(None, p, p, 4, 4, 1, 1.0, None)
    assert rc == _lib.SR_ERR_INVALID and b"bad argument" in lib.sr_last_error()
    rc = lib.sr_lora_merge(p, p, p, 1 << 21, 4, 1, 1.0, None)
    assert rc == _lib.SR_ERR_INVALID and b"too large" in lib.sr_last_error()
