"""GPU: what loading a checkpoint leaves on the device, buffer by buffer and bit for bit against the numpy model of
tests/model_load_cases.py (test_model_load_host.py shows on the CPU that the model holds its own properties and that the checker
sees a truncating conversion, swapped gate / up, rolled q / k / v bases, permuted plane segments, a w_inv off by 2, a dropped low
plane and an unrounded bias copy).  Test hook: sr_model_readout (include/sr_hip.h, "building blocks"): raw device bytes in the
internal row order.  Model shape: hidden 128, 2 heads over 1 kv head of 64 (n_qkv = 256), intermediate 192 (12 sixteen-row blocks),
vocabulary 320 (2.5 column tiles of 128), 2 layers; tied, untied and with attention_bias; fp32_planes 0, 2, 3 and 16.

  kernel of csrc/model_weights.hip   source dtype   reached by
  convert_rows_kernel                fp32           test_layouts_from_fp32_storage[*]: bf16 layout of every matrix, fp32 embedding and norms
                                     bf16           test_bf16_storage_equals_fp32_storage[*] (all bf16, and mixed tensor by tensor; the
                                                    one-column norm tensors included), test_encode_*, test_load_from_files
  convert_bias_kernel                fp32           test_layouts_from_fp32_storage[bias-*]: both copies
                                     bf16           test_bf16_storage_equals_fp32_storage[*], test_encode_bf16_tensors_equal_fp32_arrays[enc_qwen2_hd64-*]
  convert_rows_split_kernel          fp32           test_layouts_from_fp32_storage[*-2] [*-3]: segment order, saturated first plane
                                     bf16           test_bf16_storage_equals_fp32_storage[2] [3], test_encode_*[*-3]
  convert_rows_split_h_kernel        fp32           test_layouts_from_fp32_storage[*-16]: planes, w_inv (zero row, power-of-two maximum
                                                    and one ulp below, maximum beyond 3e38), lo_nz through the segment counts
                                     bf16           test_bf16_storage_equals_fp32_storage[16], test_segments_of_a_bf16_valued_model
  pack_rows_2seg_kernel              (planes)       test_segments_of_a_bf16_valued_model: [g0 | g0] bytes, per matrix;
                                                    test_layouts_from_fp32_storage[*-16] after finalize (nothing packed: 3 segments)
  lora_merge_kernel                  fp32           test_lora_merge[*]: r 1 8 64, in 1 255 256 257, out 1 3 300, both signs, guard rows;
                                                    test_load_from_lora_over_a_bf16_base (bf16 base widened by the loader)
  rope_tables (host)                 -              test_rope_tables_equal_the_restatement[*], test_rope_tables_against_transformers[*],
                                                    test_long_positions_against_the_reference[*]

RoPE against transformers (tests/golden/rope_hf.npz).  rope_tables forms inv_freq in double and rounds once, transformers in fp32:
measured 12 of 32 entries differ by up to 3 ulps (1B parameters), 21 of 64 up to 3 (8B), 24 of 64 up to 1 (Qwen2); asserted <= 4.
The tables then differ by up to 2.8e-4 (Llama) / 4.6e-4 (Qwen2) at position 8191, 0.6 of the derived p |delta inv| + 2^-23 p inv +
2^-23.  End to end it is harmless (only relative positions enter the scores): enc_rope_long.npz, L = 512, holds both regimes to
the project's bars.

Measured on MI355X (information, not asserted): every layout buffer equals the model bit for bit; the RoPE tables equal the float64
restatement word for word (0 of 3 x 2 x 8192 x hd/2 differ); sr_lora_merge's worst error / bound (L) 0.166 (r 1), 0.212 (r 8),
0.051 (r 64); maxGridSize[1] = 65 536; enc_rope_long relative L2 4.9e-7 / 8.5e-7 dense left / right and 1.7e-7 sparse with fp16
planes, 4.4e-7 / 8.9e-7 / 1.6e-7 with three bf16 planes (bar 2e-5), 4.7e-3 dense and 1.6e-3 sparse in the bf16 regime (bar 1.5e-2,
the reference's own autocast-to-fp32 distance r = 4.8e-3)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import bf16_regime_cases as G
import model_load_cases as M
from golden_weights import make_weights

pytestmark = pytest.mark.gpu

F32 = np.float32
FP32_TOL = 2e-5          # the project's fp32-regime bar


def _L():
    from scaling_retriever_amd import _lib
    return _lib, _lib.load()


def _c_config(cfg, planes, has_lm_head=True):
    from scaling_retriever_amd.modeling.llm_encoder import HipLlamaBackbone
    return HipLlamaBackbone(dict(cfg), {}, has_lm_head=has_lm_head, max_batch_tokens=128, max_batch_seqs=4, fp32_planes=planes)._c_config()


class DeviceModel:
    """sr_model_create / sr_model_set_weight / sr_model_finalize / sr_model_readout over ctypes."""

    def __init__(self, cfg, planes, has_lm_head=True):
        self.L, self.lib = _L()
        self.h = ctypes.c_void_p()
        c = _c_config(cfg, planes, has_lm_head)
        self.L.check(self.lib.sr_model_create(ctypes.byref(self.h), ctypes.byref(c)), "sr_model_create")

    def set(self, name, values, as_bf16):
        """values: fp32 array; as_bf16: stored as bf16 words (the values must be bf16 numbers) and handed as SR_DTYPE_BF16."""
        v = np.array(values, F32)                   # a writable copy: the shared value sets are read-only
        rows, cols = (v.shape[0], v.shape[1]) if v.ndim == 2 else (v.shape[0], 1)
        if as_bf16:
            t = torch.from_numpy(M.to_bf16_words(v).view(np.int16)).cuda()
            dt = self.L.SR_DTYPE_BF16
        else:
            t = torch.from_numpy(v).cuda()
            dt = self.L.SR_DTYPE_F32
        self.L.check(self.lib.sr_model_set_weight(self.h, name.encode(), t.data_ptr(), dt, rows, cols, self.L.stream_ptr()), name)
        torch.cuda.current_stream().synchronize()

    def load(self, tensors, as_bf16=lambda name: False):
        for name, v in tensors.items():
            self.set(name, v, as_bf16(name))
        return self

    def finalize(self):
        self.L.check(self.lib.sr_model_finalize(self.h), "sr_model_finalize")
        return self

    def readout(self, layer, buf, kind):
        n, rows, elems = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
        self.L.check(self.lib.sr_model_readout(self.h, layer, buf, kind, None, 0, ctypes.byref(n), ctypes.byref(rows), ctypes.byref(elems)),
                     "sr_model_readout (size)")
        dtype = np.uint16 if kind in (M.K_BF16, M.K_PLANES) else F32
        assert n.value == rows.value * elems.value * np.dtype(dtype).itemsize
        out = np.empty((rows.value, elems.value), dtype)
        out.view(np.uint8)[:] = 0xAB
        self.L.check(self.lib.sr_model_readout(self.h, layer, buf, kind, out.ctypes.data_as(ctypes.c_void_p), out.nbytes, ctypes.byref(n),
                                               ctypes.byref(rows), ctypes.byref(elems)), "sr_model_readout")
        return out

    def readout_all(self, keys):
        return {k: self.readout(*k) for k in keys}

    def segments(self):
        n = ctypes.c_int64(0)
        self.L.check(self.lib.sr_model_weight_segments(self.h, None, 0, ctypes.byref(n)), "sr_model_weight_segments")
        out = (ctypes.c_int32 * max(n.value, 1))()
        self.L.check(self.lib.sr_model_weight_segments(self.h, out, n.value, ctypes.byref(n)), "sr_model_weight_segments")
        return [int(v) for v in out[:n.value]]

    def close(self):
        if self.h:
            self.lib.sr_model_destroy(self.h)
            self.h = None


VARIANTS = {"untied": dict(tied=False, bias=False), "tied": dict(tied=True, bias=False), "bias": dict(tied=False, bias=True)}


# ---------------------------------------------------------------------------------------------- layouts, fp32 storage
@pytest.mark.parametrize("planes", M.PLANE_MODES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_layouts_from_fp32_storage(variant, planes):
    """Every buffer of the model equals the numpy model at the mapped rows, bit for bit, before and after sr_model_finalize."""
    cfg = M.config(**VARIANTS[variant])
    t = M.tensors(cfg)
    m = DeviceModel(cfg, planes)
    try:
        m.load(t)
        want = M.expected(cfg, t, planes, finalized=False)
        assert M.mismatches(planes, m.readout_all(want), want) == []
        m.finalize()
        want = M.expected(cfg, t, planes, finalized=True)
        assert M.mismatches(planes, m.readout_all(want), want) == []
        assert m.segments() == M.expected_segments(cfg, t, planes)
        # what this model does not hold is refused, not read
        n = ctypes.c_int64(0)
        absent = [(0, M.BIAS, M.K_F32)] if variant != "bias" else []
        absent += [(-1, M.LM_HEAD, M.K_PLANES)] if planes == 0 else []
        absent += [(-1, M.LM_HEAD, M.K_W_INV)] if planes != 16 else []
        absent += [(2, M.QKV, M.K_BF16), (-2, M.EMBED, M.K_F32), (-1, M.QKV, M.K_BF16), (0, M.EMBED, M.K_F32), (0, M.QKV, M.K_F32)]
        for key in absent:
            rc = m.lib.sr_model_readout(m.h, *key, None, 0, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n))
            assert rc == m.L.SR_ERR_INVALID, key
        small = np.zeros(4, np.uint8)
        rc = m.lib.sr_model_readout(m.h, -1, M.NORM, M.K_F32, small.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(n), ctypes.byref(n),
                                    ctypes.byref(n))
        assert rc == m.L.SR_ERR_INVALID and b"too small" in m.lib.sr_last_error() and not small.any()
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------- bf16 storage
@pytest.mark.parametrize("planes", M.PLANE_MODES)
def test_bf16_storage_equals_fp32_storage(planes):
    """The bf16-representable value set handed as SR_DTYPE_BF16, widened to fp32, and mixed tensor by tensor: every buffer is
    byte-identical between the three (and equals the model)."""
    cfg = M.config(tied=False, bias=True)
    t = M.tensors(cfg, bf16_only=True)
    want = M.expected(cfg, t, planes, finalized=True)
    names = list(t)
    routes = {"fp32": lambda name: False, "bf16": lambda name: True, "mixed": lambda name: names.index(name) % 2 == 0}
    got = {}
    for route, as_bf16 in routes.items():
        m = DeviceModel(cfg, planes)
        try:
            got[route] = m.load(t, as_bf16).finalize().readout_all(want)
            assert m.segments() == M.expected_segments(cfg, t, planes)
        finally:
            m.close()
    for route in ("bf16", "mixed"):
        for key in want:
            assert got[route][key].tobytes() == got["fp32"][key].tobytes(), (route, key)
    assert M.mismatches(planes, got["bf16"], want) == []


def test_segments_of_a_bf16_valued_model():
    """fp32_planes = 16.  A bf16-valued model reports 2 segments for every matrix and holds [g0 | g0] - the row with an element 2^-31
    below its maximum included: there g0 loses bits, but what it loses is at most half of fp16's smallest subnormal and rounds to a
    zero g1 (model_load_cases.py; test_model_load_host.py enumerates every bf16 number), so no bf16 value can keep a third segment.
    One entry with more significand bits than g0 holds keeps ITS matrix at 3 segments, and that matrix alone."""
    cfg = M.config(tied=False, bias=False)
    t = M.tensors(cfg, bf16_only=True)
    m = DeviceModel(cfg, 16)
    try:
        m.load(t, lambda name: True).finalize()
        assert m.segments() == [2] * 9 == M.expected_segments(cfg, t, 16)
        want = M.expected(cfg, t, 16, finalized=True)
        got = m.readout_all(want)
        assert M.mismatches(16, got, want) == []
        for (layer, buf, kind), a in got.items():
            if kind == M.K_PLANES:
                K = a.shape[1] // 2
                assert a.shape[1] == 2 * got[(layer, buf, M.K_BF16)].shape[1] and np.array_equal(a[:, :K], a[:, K:])
    finally:
        m.close()
    name = "model.layers.1.mlp.down_proj.weight"
    w = t[name].copy()
    w[7, 100] *= F32(1 + 2.0 ** -20)
    t3 = dict(t, **{name: w})
    expect = [2] * 9
    expect[4 * 1 + 3] = 3
    assert M.expected_segments(cfg, t3, 16) == expect
    m = DeviceModel(cfg, 16)
    try:
        m.load(t3, lambda n: n != name).finalize()
        assert m.segments() == expect
        want = M.expected(cfg, t3, 16, finalized=True)
        assert M.mismatches(16, m.readout_all(want), want) == []
    finally:
        m.close()


# ---------------------------------------------------------------------------------------------- encode level
def _golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    for k in z.files:
        if k.startswith("bias:"):
            w[k[5:]] = z[k]
    return z, cfg, w


def _classes(cfg):
    from scaling_retriever_amd.modeling import llm_encoder as E
    return (E.Qwen2BiDense, E.Qwen2BiSparse) if cfg.get("model_type") == "qwen2" else (E.LlamaBiDense, E.LlamaBiSparse)


def _enc(model, ids, mask, autocast=False):
    ids, mask = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(mask, np.int64)).cuda()
    with torch.no_grad():
        if autocast:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return model.encode(input_ids=ids, attention_mask=mask)
        return model.encode(input_ids=ids, attention_mask=mask)


PRECISIONS = {"bf16": dict(precision="bf16", fp32_planes=0), "3": dict(precision="fp32", fp32_planes=3),
              "16": dict(precision="fp32", fp32_planes=16)}


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("name", ["enc_tiny_a", "enc_hd64", "enc_qwen2_hd64"])
def test_encode_bf16_tensors_equal_fp32_arrays(golden_dir, name, prec):
    """tied / untied / with bias, rounded to bf16: from_weights over torch bf16 tensors (SR_DTYPE_BF16) and over the fp32 arrays of the
    same values give identical bits, both heads."""
    z, cfg, w = _golden(golden_dir, name)
    as_bf16 = {k: torch.from_numpy(v).bfloat16() for k, v in w.items()}
    as_f32 = {k: v.float().numpy() for k, v in as_bf16.items()}
    for cls in _classes(cfg):
        a = cls.from_weights(cfg, as_bf16, **PRECISIONS[prec]).to("cuda").eval()
        b = cls.from_weights(cfg, as_f32, **PRECISIONS[prec]).to("cuda").eval()
        for side in ("left", "right"):
            ids, mask = z[f"{side}:input_ids"], z[f"{side}:attention_mask"]
            out_a, out_b = _enc(a, ids, mask), _enc(b, ids, mask)
            assert torch.isfinite(out_a).all() and out_a.abs().max() > 0
            assert torch.equal(out_a, out_b), (name, prec, cls.__name__, side)


def _write_dir(path, cfg, sd, how):
    from safetensors.torch import save_file
    os.makedirs(path)
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    if how == "single":
        save_file(sd, os.path.join(path, "model.safetensors"))
    elif how == "sharded":
        second = {k: v for k, v in sd.items() if ".layers.1." in k or k.startswith("lm_head")}
        first = {k: v for k, v in sd.items() if k not in second}
        files = {"model-00001-of-00002.safetensors": first, "model-00002-of-00002.safetensors": second}
        for fn, part in files.items():
            save_file(part, os.path.join(path, fn))
        json.dump({"metadata": {}, "weight_map": {k: fn for fn, part in files.items() for k in part}},
                  open(os.path.join(path, "model.safetensors.index.json"), "w"))
    else:
        torch.save(sd, os.path.join(path, "pytorch_model.bin"))


def test_load_from_files(golden_dir, tmp_path):
    """load() from a bf16 single-file, sharded and .bin checkpoint: the bits of from_weights over the same values, both heads, fp32
    regime (fp16 planes, load()'s default) and under autocast."""
    z, cfg, w = _golden(golden_dir, "enc_hd64")
    sd = {k: torch.from_numpy(v).bfloat16() for k, v in w.items()}
    values = {k: v.float().numpy() for k, v in sd.items()}
    ids, mask = z["left:input_ids"], z["left:attention_mask"]
    ref = {}
    for cls in _classes(cfg):
        m = cls.from_weights(cfg, values).to("cuda").eval()
        ref[cls] = (_enc(m, ids, mask), _enc(m, ids, mask, autocast=True))
    for how in ("single", "sharded", "bin"):
        d = str(tmp_path / how)
        _write_dir(d, cfg, sd, how)
        for cls in _classes(cfg):
            m = cls.load(d).to("cuda").eval()
            assert torch.equal(_enc(m, ids, mask), ref[cls][0]), (how, cls.__name__, "fp32 regime")
            assert torch.equal(_enc(m, ids, mask, autocast=True), ref[cls][1]), (how, cls.__name__, "bf16 regime")


def test_load_from_lora_over_a_bf16_base(golden_dir, tmp_path):
    """load_from_lora over a bf16-stored base gives the bits of the same adapter over the fp32-stored base of the same values."""
    from safetensors.torch import save_file
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    z, cfg, w = _golden(golden_dir, "enc_hd64")
    sd16 = {k: torch.from_numpy(v).bfloat16() for k, v in w.items()}
    sd32 = {k: v.float() for k, v in sd16.items()}
    rng = np.random.default_rng(3)
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    nq = cfg["num_attention_heads"] * (H // cfg["num_attention_heads"])
    nkv = cfg["num_key_value_heads"] * (H // cfg["num_attention_heads"])
    shapes = {"self_attn.q_proj": (nq, H), "self_attn.k_proj": (nkv, H), "self_attn.v_proj": (nkv, H), "self_attn.o_proj": (H, nq),
              "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    ad = {}
    for i in range(cfg["num_hidden_layers"]):
        for mod, (o, inn) in shapes.items():
            ad[f"base_model.model.model.layers.{i}.{mod}.lora_A.weight"] = torch.from_numpy((rng.standard_normal((4, inn)) / inn ** 0.5).astype(F32))
            ad[f"base_model.model.model.layers.{i}.{mod}.lora_B.weight"] = torch.from_numpy((rng.standard_normal((o, 4)) * 0.3).astype(F32))
    outs = {}
    ids, mask = z["left:input_ids"], z["left:attention_mask"]
    for tag, sd in (("bf16", sd16), ("fp32", sd32)):
        base, lora = str(tmp_path / f"base_{tag}"), str(tmp_path / f"lora_{tag}")
        _write_dir(base, cfg, sd, "single")
        os.makedirs(lora)
        save_file(ad, os.path.join(lora, "adapter_model.safetensors"))
        json.dump({"base_model_name_or_path": base, "r": 4, "lora_alpha": 8, "peft_type": "LORA",
                   "target_modules": list(m.split(".")[1] for m in shapes)}, open(os.path.join(lora, "adapter_config.json"), "w"))
        m = LlamaBiSparse.load_from_lora(lora).to("cuda").eval()
        outs[tag] = (_enc(m, ids, mask), _enc(m, ids, mask, autocast=True))
    plain = LlamaBiSparse.from_weights(cfg, {k: v.numpy() for k, v in sd32.items()}).to("cuda").eval()
    assert not torch.equal(_enc(plain, ids, mask), outs["fp32"][0])               # the adapter really changed the model
    assert torch.equal(outs["bf16"][0], outs["fp32"][0]) and torch.equal(outs["bf16"][1], outs["fp32"][1])


# ---------------------------------------------------------------------------------------------- LoRA merge
@pytest.mark.parametrize("r", M.LORA_R)
def test_lora_merge(r):
    """sr_lora_merge against float64 under the derived bound (L) of model_load_cases.py, W nearly cancelled by the update, scales of
    both signs; guard rows around W come back untouched."""
    L, lib = _L()
    worst = 0.0
    for in_f in M.LORA_IN:
        for out_f in M.LORA_OUT:
            for scale in (2.0, -0.375):
                W, A, B = M.lora_case(r, in_f, out_f, scale)
                g = M.LORA_GUARD
                buf = np.full((out_f + 2 * g, in_f), np.nan, F32)
                buf.view(np.uint32)[:g] = 0x7FC0BEEF
                buf.view(np.uint32)[-g:] = 0x7FC0BEEF
                buf[g:g + out_f] = W
                dW, dA, dB = (torch.from_numpy(np.array(x)).cuda() for x in (buf, A, B))
                L.check(lib.sr_lora_merge(dW.data_ptr() + g * in_f * 4, dA.data_ptr(), dB.data_ptr(), out_f, in_f, r, scale, L.stream_ptr()),
                        "sr_lora_merge")
                torch.cuda.synchronize()
                out = dW.cpu().numpy()
                assert (out.view(np.uint32)[:g] == 0x7FC0BEEF).all() and (out.view(np.uint32)[-g:] == 0x7FC0BEEF).all(), (in_f, out_f)
                err = np.abs(out[g:g + out_f].astype(np.float64) - M.lora_truth(W, A, B, scale))
                bound = M.lora_bound(W, A, B, scale)
                ratio = float((err / bound).max())
                worst = max(worst, ratio)
                assert (err <= bound).all(), (r, in_f, out_f, scale, ratio)
    print(f"sr_lora_merge r = {r}: worst error / bound {worst:.3f}")


def _hip_runtime():
    """The HIP runtime this process already holds (torch's), by its mapped path."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime mapped")


def test_lora_merge_refuses_more_rows_than_the_grid_takes():
    """out_features is the grid's y dimension.  maxGridSize[1] comes from the device properties; nothing is launched near it: what
    exceeds it is refused by the argument check, by name, before a launch."""
    L, lib = _L()
    torch.cuda.init()
    hip = _hip_runtime()
    attr = {}
    for name, idx in (("block_x", 26), ("block_y", 27), ("block_z", 28), ("grid_x", 29), ("grid_y", 30), ("grid_z", 31)):
        v = ctypes.c_int(0)
        assert hip.hipDeviceGetAttribute(ctypes.byref(v), idx, torch.cuda.current_device()) == 0
        attr[name] = v.value
    # hipDeviceAttributeMaxBlockDimX .. MaxGridDimZ are consecutive; the block limits of every AMD device pin the numbering
    assert (attr["block_x"], attr["block_y"], attr["block_z"]) == (1024, 1024, 1024) and attr["grid_x"] >= attr["grid_y"] >= 65535, attr
    limit = attr["grid_y"]
    print("maxGridSize[1] =", limit)
    x = torch.zeros(64, device="cuda")
    p = x.data_ptr()
    if limit < (1 << 21) - 1:
        rc = lib.sr_lora_merge(p, p, p, limit + 1, 1, 1, 1.0, L.stream_ptr())
        assert rc == L.SR_ERR_INVALID and b"grid limit" in lib.sr_last_error() and str(limit).encode() in lib.sr_last_error()
    rc = lib.sr_lora_merge(p, p, p, 1 << 21, 1, 1, 1.0, L.stream_ptr())
    assert rc == L.SR_ERR_INVALID and b"too large" in lib.sr_last_error()
    torch.cuda.synchronize()
    assert not x.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------- RoPE tables
def _rope_readout(s):
    hd = s["head_dim"]
    cfg = dict(vocab_size=16, hidden_size=128, intermediate_size=64, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1,
               head_dim=hd, rms_norm_eps=1e-5, rope_theta=s["rope_theta"], tie_word_embeddings=False, rope_scaling=s["rope_scaling"])
    m = DeviceModel(cfg, 0, has_lm_head=False)
    try:
        cos, sin = m.readout(-1, M.ROPE_COS, M.K_F32), m.readout(-1, M.ROPE_SIN, M.K_F32)
    finally:
        m.close()
    assert cos.shape == sin.shape == (M.MAX_POS, hd // 2)
    return cos, sin


_TABLES = {}


def _tables(name):
    if name not in _TABLES:
        _TABLES[name] = _rope_readout(M.ROPE_SETS[name])
    return _TABLES[name]


@pytest.mark.parametrize("name", list(M.ROPE_SETS))
def test_rope_tables_equal_the_restatement(name):
    """The device tables equal the float64 restatement of rope_tables - inv_freq in double rounded once, angle = fp32(p) * inv in fp32,
    cos and sin in double rounded once - to one fp32 rounding, 2^-24 absolute; row 1 holds cos / sin of inv_freq itself."""
    s = M.ROPE_SETS[name]
    cos, sin = _tables(name)
    inv = M.rope_inv_freq(s["head_dim"], s["rope_theta"], s["rope_scaling"])
    rc, rs = M.rope_tables(inv)
    for what, got, ref in (("cos", cos, rc), ("sin", sin, rs)):
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        bad = np.argwhere(err > 2.0 ** -24)
        print(f"rope {name} {what}: max |device - restatement| {err.max():.3e}, {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} words differ")
        assert len(bad) == 0, (name, what, [(int(p), int(i), float(got[p, i]), float(ref[p, i])) for p, i in bad[:8]])
    assert (cos[0] == 1).all() and (sin[0] == 0).all()


@pytest.mark.parametrize("name", list(M.ROPE_SETS))
def test_rope_tables_against_transformers(golden_dir, name):
    """rope_hf.npz: inv_freq (as the previous test pins it on the device) within 4 ulps of transformers' - measured 3 (1B: 12 of 32
    entries differ), 3 (8B: 21 of 64), 1 (Qwen2: 24 of 64) - and the device tables within p |delta inv| + 2^-23 p inv + 2^-23 of its
    cos / sin at positions 0, 1, 63, 191, 511 and 8191."""
    z = np.load(os.path.join(golden_dir, "rope_hf.npz"))
    s = M.ROPE_SETS[name]
    assert tuple(z["positions"]) == M.ROPE_POSITIONS
    hf = z[f"{name}:inv_freq"]
    inv = M.rope_inv_freq(s["head_dim"], s["rope_theta"], s["rope_scaling"])
    ulps = M.ulps_apart(inv, hf)
    print(f"rope {name}: {int((ulps > 0).sum())} of {len(inv)} inv_freq entries differ from transformers', max {int(ulps.max())} ulps")
    assert ulps.max() <= 4
    cos, sin = _tables(name)
    p = np.array(M.ROPE_POSITIONS, np.float64)[:, None]
    hf64 = hf.astype(np.float64)[None, :]
    bound = p * np.abs(inv.astype(np.float64)[None, :] - hf64) + 2.0 ** -23 * p * hf64 + 2.0 ** -23
    for what, got, ref in (("cos", cos, z[f"{name}:cos"]), ("sin", sin, z[f"{name}:sin"])):
        err = np.abs(got[list(M.ROPE_POSITIONS)].astype(np.float64) - ref.astype(np.float64))
        print(f"rope {name} {what}: max |device - transformers| per position {err.max(axis=1)}, worst / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (name, what)


@pytest.mark.parametrize("regime", ["16", "3", "bf16"])
def test_long_positions_against_the_reference(golden_dir, regime):
    """enc_rope_long.npz: the reference's LlamaBiDense / LlamaBiSparse at L = 512 with the 1B RoPE parameters.  fp32 regime (fp16
    planes, three bf16 planes): the project's 2e-5; bf16 regime: max(1.5e-2, 2.5 r) with the fixture's own r_autocast."""
    z, cfg, w = _golden(golden_dir, "enc_rope_long")
    r = float(z["r_autocast"])
    bar = FP32_TOL if regime != "bf16" else max(1.5e-2, 2.5 * r)
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))
    for cls, key in zip(_classes(cfg), ("dense", "sparse")):
        model = cls.from_weights(cfg, w, **PRECISIONS[regime]).to("cuda").eval()
        for side in ("left", "right"):
            out = _enc(model, z[f"{side}:input_ids"], z[f"{side}:attention_mask"]).cpu().numpy()
            e = rel(out, z[f"{side}:{key}"])
            print(f"enc_rope_long regime {regime} {key} {side}: rel L2 {e:.3e} (bar {bar:.3e}, reference autocast r {r:.3e})")
            assert e <= bar, (regime, key, side, e, bar)
