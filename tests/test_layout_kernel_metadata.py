"""CPU: code-object metadata of the kernels whose launch plan rests on registers - the classes of attention_f32_mfma_kernel and the
four-wave fp16-plane GEMMs the default dispatch reaches at 2 plane segments.  Read from the built objects the way tests/test_abi.py
does (llvm-objcopy + clang-offload-bundler + llvm-readelf --notes); no GPU."""
import os

from test_abi import ROOT, _kernel_metadata

CSRC = os.path.join(ROOT, "scaling_retriever_amd", "csrc")


def _clean(name, m):
    assert m[".private_segment_fixed_size:"] == 0 and m[".vgpr_spill_count:"] == 0 and m[".sgpr_spill_count:"] == 0, (name, m)


def test_every_attention_f32_mfma_instantiation_is_free_of_scratch(tmp_path):
    """2 head dims x (the form before the class plan + 4 classes): no scratch, no spilled register.  Registers bound the workgroups
    per CU (one wave per SIMD each, 512 registers per SIMD lane) and must not bind before the class's LDS does: class 1 at head
    dim 64 - 97 % of a query batch - fits 8 workgroups (64 registers); the other classes at 64 and classes 1 / 2 at 128 use no
    more than the form before the plan (80 / 96); classes 3 / 4 at 128 hold 50 / 66 KB of LDS, i.e. 3 / 2 workgroups per CU, and
    stay within the 128 registers that admit 4."""
    meta = {k: v for k, v in _kernel_metadata(os.path.join(CSRC, "attention_f32.o"), tmp_path).items() if "attention_f32_mfma_kernel" in k}
    assert len(meta) == 10, sorted(meta)
    limit = {(64, 0): 80, (64, 1): 64, (64, 2): 80, (64, 3): 80, (64, 4): 80, (128, 0): 96, (128, 1): 96, (128, 2): 96, (128, 3): 128, (128, 4): 128}
    for (hd, nkb), regs in limit.items():
        name = f"_Z25attention_f32_mfma_kernelILi{hd}ELi{nkb}EEv11AttnF32Args"
        _clean(name, meta[name])
        print(name, meta[name])
        assert meta[name][".vgpr_count:"] <= regs, (name, meta[name], regs)


def test_four_wave_f16_plane_gemms_of_the_default_dispatch_are_free_of_scratch(tmp_path):
    """launch_big sends the fp16-plane SwiGLU-split GEMM (gate-up) to the four-wave loop when its operands have 2 plane segments:
    <EPI_SWIGLU_SPLIT_H = 13, 2, 2, 8, 8, true, 2, 1>; SR_GEMM_BIG=4w adds the residual one (10).  Both: no scratch, no spilled
    vector register and no scalar register parked in the lanes of a vector register (instantiation 13 had 9 of those until its
    epilogue read its pointer arguments from the kernel-argument segment per tile instead of carrying them through the tile loop)."""
    meta = _kernel_metadata(os.path.join(CSRC, "gemm_bf16.o"), tmp_path)
    for epi in (10, 13):
        name = f"_Z16gemm_bf16_kernelILi{epi}ELi2ELi2ELi8ELi8ELb1ELi2ELi1EEv8GemmArgs"
        assert name in meta, [k for k in meta if k.endswith("ELi1EEv8GemmArgs")]
        print(name, meta[name])
        _clean(name, meta[name])


def test_attention_f32_hook_rejects_misaligned_buffers():
    """The short-sequence kernel moves 16 bytes per lane (q / k / v loads, fp32 stores) and 8 bytes per plane-segment store:
    sr_attention_varlen_f32 rejects a buffer that is not aligned for that before anything is launched (the pointers are never
    dereferenced)."""
    import ctypes

    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p, odd8, odd4 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 4)
    for qkv, f32, planes, fp32_planes in ((odd8, p, None, 0), (p, odd8, None, 0), (p, None, odd4, 3)):
        rc = lib.sr_attention_varlen_f32(qkv, f32, planes, fp32_planes, p, p, 1, 4, 1, 64, 8, None)
        assert rc == _lib.SR_ERR_INVALID and b"aligned" in lib.sr_last_error(), (rc, lib.sr_last_error())
    assert lib.sr_attention_varlen_f32(p, None, odd8, 3, p, p, 0, 4, 1, 64, 0, None) == _lib.SR_OK      # 8 bytes suffice for planes; B = 0
