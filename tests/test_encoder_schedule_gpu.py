"""GPU: the encoder IS the composition of its tested launches.

Every kernel the encoder launches has a per-kernel float64 parity test through a hook of csrc/api.hip (test_bf16_regime_gpu.py,
test_fp32_planes_gpu.py, test_attention_*_gpu.py), and the whole model is held to goldens within a tolerance.  This file closes the
gap between the two: it replays one encode call launch by launch through those hooks - same order, same arguments, with the
internal weight layouts restated on the host - and asserts that the dense output, the sparse output and sr_model_last_hidden are
torch.equal to the encoder's.  A wrong scale pointer, segment count, K or output buffer in the layer loop changes bits here.

Regimes: bf16 (fp32_planes = 0, the autocast regime) and fp16 planes (fp32_planes = 16, the no-autocast regime).  The bf16-plane
regimes (2 and 3 planes) have no hooks for their norm and SwiGLU-split kernels and are not replayed.

Shapes (every dimension that could be swapped differs):
  A  hidden 256, 2 heads, 1 kv head, head_dim 64 (nq = 128 != hidden), intermediate 384, vocab 320, 2 layers
  B  hidden 256, 2 heads, 2 kv heads, head_dim 128, intermediate 320, vocab 336, 2 layers, q / k / v bias
  batch: left-padded, L = 80, lengths 1 17 64 65 33 and one row whose mask is all zero: 180 packed tokens."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import fp32_plane_cases as C
from golden_weights import make_weights

pytestmark = pytest.mark.gpu

CFG_A = dict(vocab_size=320, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2,
             num_key_value_heads=1, head_dim=64, rms_norm_eps=1e-5, rope_theta=10000.0, tie_word_embeddings=False, attention_bias=0)
CFG_B = dict(vocab_size=336, hidden_size=256, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2,
             num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-6, rope_theta=500000.0, tie_word_embeddings=False, attention_bias=1)
CONFIGS = {"A": CFG_A, "B": CFG_B}
L, LENS = 80, [1, 17, 64, 65, 33, 0]
EPI_STORE_BF16, EPI_SWIGLU, EPI_SEGMAX = 0, 2, 3
PAD = 256                           # activation buffers are zero-filled up to a multiple of the largest GEMM tile, as the model's are


def _lib():
    from scaling_retriever_amd import _lib as LIB
    return LIB, LIB.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).bfloat16().cuda()


# ------------------------------------------------------------------------------------------ weights and inputs
@functools.lru_cache(maxsize=None)
def weights(name, kind):
    """kind: "fp32" as generated, "bf16" rounded to bf16 (every fp16-plane matrix drops to 2 segments), "loose" with the gate / up
    rows of pair 7 of layer 1 scaled as in fp32_plane_cases.loose_case (sr_model_finalize picks the unfused route there)."""
    cfg = CONFIGS[name]
    w = make_weights(cfg, 77 if name == "A" else 78)
    if cfg["attention_bias"]:
        rng = np.random.default_rng(500)
        nq, nkv = cfg["num_attention_heads"] * cfg["head_dim"], cfg["num_key_value_heads"] * cfg["head_dim"]
        for i in range(cfg["num_hidden_layers"]):
            for p, n in (("q", nq), ("k", nkv), ("v", nkv)):
                w[f"model.layers.{i}.self_attn.{p}_proj.bias"] = (rng.standard_normal(n) * 0.5).astype(np.float32)
    if kind == "bf16":
        w = {k: torch.from_numpy(v).bfloat16().float().numpy() for k, v in w.items()}
    if kind == "loose":
        for p in ("gate", "up"):
            m = w[f"model.layers.1.mlp.{p}_proj.weight"].copy()
            m[7] *= np.float32(1024.0)
            w[f"model.layers.1.mlp.{p}_proj.weight"] = m
    return w


def batch(cfg, side="left", holes=False, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, cfg["vocab_size"], size=(len(LENS), L)).astype(np.int64)
    mask = np.zeros((len(LENS), L), np.int64)
    for r, n in enumerate(LENS):
        if side == "left":
            mask[r, L - n:] = 1
        else:
            mask[r, :n] = 1
    if holes:
        mask[2, 5] = 0
        mask[2, 40:43] = 0
        mask[3, 0] = 0
        mask[4, 31] = 0
    return ids, mask


def rope_tables(cfg, n_pos):
    """rope_tables of csrc/model_weights.hip for rope_type "default": inv_freq rounded to fp32, angle = fp32(pos) * inv_freq in fp32,
    cos / sin in double (libm, as the C code) rounded to fp32."""
    hd = cfg["head_dim"]
    theta = float(np.float32(cfg["rope_theta"]))
    inv = np.array([1.0 / math.pow(theta, (2 * i) / hd) for i in range(hd // 2)], np.float64).astype(np.float32)
    cs, sn = np.empty((n_pos, hd // 2), np.float32), np.empty((n_pos, hd // 2), np.float32)
    for p in range(n_pos):
        for i in range(hd // 2):
            ang = float(np.float32(p) * inv[i])
            cs[p, i], sn[p, i] = math.cos(ang), math.sin(ang)
    return cs, sn


# ------------------------------------------------------------------------------------------ the encoder
class Model:
    """sr_model through the C ABI, with what the replay reads back from it."""

    def __init__(self, cfg, w, fp32_planes):
        LIB, lib = _lib()
        self.lib, self.LIB, self.cfg = lib, LIB, cfg
        c = LIB.SrModelConfig(
            vocab_size=cfg["vocab_size"], hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
            num_layers=cfg["num_hidden_layers"], num_heads=cfg["num_attention_heads"], num_kv_heads=cfg["num_key_value_heads"],
            head_dim=cfg["head_dim"], rms_norm_eps=cfg["rms_norm_eps"], rope_theta=cfg["rope_theta"], rope_llama3=0, rope_factor=1.0,
            rope_low_freq_factor=1.0, rope_high_freq_factor=1.0, rope_original_max_pos=0, tie_word_embeddings=0, has_lm_head=1,
            max_batch_tokens=256, max_batch_seqs=8, fp32_planes=fp32_planes, attention_bias=cfg["attention_bias"])
        self.h = ctypes.c_void_p()
        LIB.check(lib.sr_model_create(ctypes.byref(self.h), ctypes.byref(c)), "sr_model_create")
        for name, a in w.items():
            t = _dev(a)
            LIB.check(lib.sr_model_set_weight(self.h, name.encode(), t.data_ptr(), LIB.SR_DTYPE_F32, a.shape[0],
                                              a.shape[1] if a.ndim == 2 else 1, LIB.stream_ptr()), name)
            torch.cuda.synchronize()
        LIB.check(lib.sr_model_finalize(self.h), "sr_model_finalize")

    def _ints(self, fn, what):
        n = ctypes.c_int64(0)
        self.LIB.check(fn(self.h, None, 0, ctypes.byref(n)), what)
        out = (ctypes.c_int32 * max(n.value, 1))()
        self.LIB.check(fn(self.h, out, n.value, ctypes.byref(n)), what)
        return [int(v) for v in out[:n.value]]

    def weight_segments(self):
        return self._ints(self.lib.sr_model_weight_segments, "sr_model_weight_segments")

    def fused_act_layers(self):
        return [bool(v) for v in self._ints(self.lib.sr_model_fused_act_layers, "sr_model_fused_act_layers")]

    def encode(self, ids, mask, shift, mode, fp32):
        """sr_encode_rows + sr_model_last_hidden -> (dense or None, sparse or None, hidden)."""
        B = ids.shape[0]
        d_ids, d_mask = _dev(ids), _dev(mask)
        d_shift = None if shift is None else _dev(np.asarray(shift, np.int32))
        dense = torch.full((B, self.cfg["hidden_size"]), float("nan"), device="cuda") if mode != 1 else None
        sparse = torch.full((B, self.cfg["vocab_size"]), float("nan"), device="cuda") if mode != 0 else None
        self.LIB.check(self.lib.sr_encode_rows(self.h, d_ids.data_ptr(), d_mask.data_ptr(), B, ids.shape[1], _ptr(d_shift), mode, fp32,
                                               _ptr(sparse), _ptr(dense), self.LIB.stream_ptr()), "sr_encode_rows")
        hidden = torch.full((256 + 128, self.cfg["hidden_size"]), float("nan"), device="cuda")
        n = ctypes.c_int64(0)
        self.LIB.check(self.lib.sr_model_last_hidden(self.h, hidden.data_ptr(), hidden.shape[0], ctypes.byref(n), self.LIB.stream_ptr()),
                       "sr_model_last_hidden")
        torch.cuda.synchronize()
        return dense, sparse, hidden[:n.value].clone()

    def close(self):
        if self.h:
            self.lib.sr_model_destroy(self.h)
            self.h = None


# ------------------------------------------------------------------------------------------ the replay
class Replay:
    """One encode call as the launches of the hooks, on buffers of its own."""

    def __init__(self, cfg, w):
        self.LIB, self.lib = _lib()
        self.cfg, self.w = cfg, w
        self.H, self.I, self.V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
        self.nh, self.nkv_h, self.hd = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
        self.nq, self.nkv = self.nh * self.hd, self.nkv_h * self.hd
        self.n_qkv = self.nq + 2 * self.nkv
        self.eps = cfg["rms_norm_eps"]
        self.nl = cfg["num_hidden_layers"]
        self.s = self.LIB.stream_ptr()
        cs, sn = rope_tables(cfg, L)
        self.cos, self.sin = _dev(cs), _dev(sn)
        self.embed = _dev(w["model.embed_tokens.weight"])
        self.norm_w = _dev(w["model.norm.weight"])
        self.ln = [(_dev(self.lw(i, "input_layernorm.weight")), _dev(self.lw(i, "post_attention_layernorm.weight"))) for i in range(self.nl)]

    def lw(self, i, rest):
        return self.w[f"model.layers.{i}.{rest}"]

    def qkv_rows(self, i, what="weight"):
        return np.concatenate([self.lw(i, f"self_attn.{p}_proj.{what}") for p in "qkv"], axis=0)

    def gate_up(self, i):
        return C.interleave_gate_up(self.lw(i, "mlp.gate_proj.weight"), self.lw(i, "mlp.up_proj.weight"))

    def ok(self, rc, what):
        self.LIB.check(rc, what)

    # ---- plan
    def plan(self, ids, mask, shift, mode):
        B = ids.shape[0]
        self.B = B
        self.d_ids, self.d_mask = _dev(ids), _dev(mask)
        d_shift = None if shift is None else _dev(np.asarray(shift, np.int32))
        i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda")         # noqa: E731
        self.span_start, self.span_len, self.pool_start, self.row_len, self.cu = i32(B), i32(B), i32(B), i32(B), i32(B + 1)
        cap = B * L
        self.tok, self.pos, self.seq_of = i32(cap), i32(cap), i32(cap)
        self.key_valid = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
        n = ctypes.c_int64(0)
        self.ok(self.lib.sr_encode_plan(self.d_ids.data_ptr(), self.d_mask.data_ptr(), B, L, mode, self.V, _ptr(d_shift),
                                        self.span_start.data_ptr(), self.span_len.data_ptr(), self.pool_start.data_ptr(),
                                        self.row_len.data_ptr(), self.cu.data_ptr(), self.tok.data_ptr(), self.pos.data_ptr(),
                                        self.key_valid.data_ptr(), self.seq_of.data_ptr(), cap, ctypes.byref(n), self.s), "sr_encode_plan")
        self.T = int(n.value)
        cu = self.cu.cpu().numpy()
        self.max_len = int((cu[1:] - cu[:-1]).max())
        self.Tp = (self.T + PAD - 1) // PAD * PAD
        return self.T

    def buf(self, cols, dtype):
        return torch.zeros((self.Tp, cols), dtype=dtype, device="cuda")

    def rmsnorm(self, x, embed, tok, delta, w, xn, xn_f32):
        self.ok(self.lib.sr_rmsnorm_bf16(x.data_ptr(), _ptr(embed), _ptr(tok), _ptr(delta), _ptr(w), _ptr(xn), _ptr(xn_f32), self.eps,
                                         self.T, self.H, self.s), "sr_rmsnorm_bf16")

    def gemm(self, A, W, N, K, epi, out, seq_of=None):
        self.ok(self.lib.sr_gemm_bf16(A.data_ptr(), W.data_ptr(), self.T, N, K, epi, out.data_ptr(), _ptr(seq_of), self.s), "sr_gemm_bf16")

    # ---- heads (both regimes), given the final residual stream x
    def dense_head(self, x):
        stats = torch.zeros((self.Tp, 2), dtype=torch.float32, device="cuda")
        out = torch.full((self.B, self.H), float("nan"), device="cuda")
        self.ok(self.lib.sr_dense_head_pool(x.data_ptr(), self.norm_w.data_ptr(), self.cu.data_ptr(), self.pos.data_ptr(),
                                            self.pool_start.data_ptr(), self.eps, self.B, self.T, self.H, stats.data_ptr(), out.data_ptr(),
                                            self.s), "sr_dense_head_pool")
        return out

    def sparse_finish(self, out, round_bf16):
        scale = float(np.float32(self.H) ** np.float32(-0.25))
        self.ok(self.lib.sr_sparse_finish(out.data_ptr(), self.B * self.V, scale, round_bf16, self.s), "sr_sparse_finish")

    def last_hidden(self, x):
        out = torch.full((self.Tp, self.H), float("nan"), device="cuda")
        self.rmsnorm(x, None, None, None, self.norm_w, None, out)
        return out[:self.T]

    # ---- bf16 regime
    def run_bf16(self, mode):
        H, I, nq, T = self.H, self.I, self.nq, self.T
        bf = torch.bfloat16
        x, xn, qkv, attn, act, delta = (self.buf(H, torch.float32), self.buf(H, bf), self.buf(self.n_qkv, bf), self.buf(nq, bf),
                                        self.buf(I, bf), self.buf(H, bf))
        self.rmsnorm(x, self.embed, self.tok, None, self.ln[0][0], xn, None)
        for i in range(self.nl):
            if i > 0:
                self.rmsnorm(x, None, None, delta, self.ln[i][0], xn, None)
            wqkv, wo = _bf16(self.qkv_rows(i)), _bf16(self.lw(i, "self_attn.o_proj.weight"))
            wgu, wdown = _bf16(self.gate_up(i)), _bf16(self.lw(i, "mlp.down_proj.weight"))
            bias = None
            if self.cfg["attention_bias"]:
                bias = torch.from_numpy(self.qkv_rows(i, "bias")).bfloat16().float().cuda()
            self.ok(self.lib.sr_gemm_qkv_rope_bias(xn.data_ptr(), wqkv.data_ptr(), T, self.n_qkv, H, qkv.data_ptr(), self.pos.data_ptr(),
                                                   self.cos.data_ptr(), self.sin.data_ptr(), nq + self.nkv, self.hd, _ptr(bias), 0, self.s),
                    "sr_gemm_qkv_rope_bias")
            self.ok(self.lib.sr_attention_varlen(qkv.data_ptr(), attn.data_ptr(), self.cu.data_ptr(), self.pos.data_ptr(),
                                                 self.key_valid.data_ptr(), None, None, self.B, self.nh, self.nkv_h, self.hd, self.s),
                    "sr_attention_varlen")
            self.gemm(attn, wo, H, nq, EPI_STORE_BF16, delta)
            self.rmsnorm(x, None, None, delta, self.ln[i][1], xn, None)
            self.gemm(xn, wgu, 2 * I, H, EPI_SWIGLU, act)
            self.gemm(act, wdown, H, I, EPI_STORE_BF16, delta)
        self.rmsnorm(x, None, None, delta, None, None, None)
        dense = self.dense_head(x) if mode != 1 else None
        sparse = None
        if mode != 0:
            sparse = torch.zeros((self.B, self.V), dtype=torch.float32, device="cuda")
            self.rmsnorm(x, None, None, None, self.norm_w, xn, None)
            self.gemm(xn, _bf16(self.w["lm_head.weight"]), self.V, H, EPI_SEGMAX, sparse, self.seq_of)
            self.sparse_finish(sparse, 1)
        hidden = self.last_hidden(x)
        torch.cuda.synchronize()
        return dense, sparse, hidden

    # ---- fp16-plane regime
    def split(self, src, embed, tok, w, K, nseg, planes, inv, cmax=None, act_sc=None, act_inv=None):
        self.ok(self.lib.sr_rows_split_f16(src.data_ptr(), _ptr(embed), _ptr(tok), _ptr(w), self.eps, self.T, K, nseg, planes.data_ptr(),
                                           inv.data_ptr(), _ptr(cmax), _ptr(act_sc), _ptr(act_inv), self.s), "sr_rows_split_f16")

    def gemm_h(self, A, W, N, K0, nseg, epi, a_inv, w_inv, out, rope=False, bias=None, seq_of=None, out_scale=None, out_nseg=0):
        self.ok(self.lib.sr_gemm_f16_planes(A.data_ptr(), W.data_ptr(), self.T, N, nseg * K0, epi, nseg, a_inv.data_ptr(), w_inv.data_ptr(),
                                            out.data_ptr(), _ptr(self.pos) if rope else None, _ptr(self.cos) if rope else None,
                                            _ptr(self.sin) if rope else None, self.nq + self.nkv if rope else 0, self.hd if rope else 0,
                                            _ptr(bias), _ptr(seq_of), _ptr(out_scale), out_nseg, self.s), "sr_gemm_f16_planes")

    def planes(self, w, nseg):
        p, inv = C.weight_planes(w, nseg)
        return _dev(p.view(np.int16)), _dev(inv)

    def run_f16(self, mode, segs, fused):
        H, I, nq, T = self.H, self.I, self.nq, self.T
        f32, i16 = torch.float32, torch.int16
        x, qkv_f, attn_f, act_f = self.buf(H, f32), self.buf(self.n_qkv, f32), self.buf(nq, f32), self.buf(I, f32)
        xs, attn_s, act_s = self.buf(3 * H, i16), self.buf(3 * nq, i16), self.buf(3 * I, i16)
        vec = lambda: torch.zeros((self.Tp,), dtype=f32, device="cuda")            # noqa: E731
        xs_i, attn_i, act_i, act_sc = vec(), vec(), vec(), vec()
        for i in range(self.nl):
            qkv_seg, o_seg, gu_seg, down_seg = segs[4 * i:4 * i + 4]
            wqkv, wqkv_i = self.planes(self.qkv_rows(i), qkv_seg)
            wo, wo_i = self.planes(self.lw(i, "self_attn.o_proj.weight"), o_seg)
            wgu, wgu_i = self.planes(self.gate_up(i), gu_seg)
            wdown, wdown_i = self.planes(self.lw(i, "mlp.down_proj.weight"), down_seg)
            bias = _dev(self.qkv_rows(i, "bias")) if self.cfg["attention_bias"] else None
            ln1, ln2 = self.ln[i]
            self.split(x, self.embed if i == 0 else None, self.tok if i == 0 else None, ln1, H, qkv_seg, xs, xs_i)
            self.gemm_h(xs, wqkv, self.n_qkv, H, qkv_seg, C.EPI_QKV, xs_i, wqkv_i, qkv_f, rope=True, bias=bias)
            self.ok(self.lib.sr_attention_varlen_f32(qkv_f.data_ptr(), attn_f.data_ptr(), None, 16, self.cu.data_ptr(),
                                                     self.key_valid.data_ptr(), self.B, self.nh, self.nkv_h, self.hd, self.max_len, self.s),
                    "sr_attention_varlen_f32")
            self.split(attn_f, None, None, None, nq, o_seg, attn_s, attn_i)
            self.gemm_h(attn_s, wo, H, nq, o_seg, C.EPI_RESID, attn_i, wo_i, x)
            if fused[i]:
                cmax = torch.full((1,), 123.0, device="cuda")
                self.ok(self.lib.sr_gu_cmax_f16(wgu.data_ptr(), wgu_i.data_ptr(), I, H, gu_seg, cmax.data_ptr(), self.s), "sr_gu_cmax_f16")
                self.split(x, None, None, ln2, H, gu_seg, xs, xs_i, cmax, act_sc, act_i)
                self.gemm_h(xs, wgu, 2 * I, H, gu_seg, C.EPI_SPLIT, xs_i, wgu_i, act_s, out_scale=act_sc, out_nseg=down_seg)
            else:
                self.split(x, None, None, ln2, H, gu_seg, xs, xs_i)
                self.gemm_h(xs, wgu, 2 * I, H, gu_seg, C.EPI_SWIGLU, xs_i, wgu_i, act_f)
                self.split(act_f, None, None, None, I, down_seg, act_s, act_i)
            self.gemm_h(act_s, wdown, H, I, down_seg, C.EPI_RESID, act_i, wdown_i, x)
        dense = self.dense_head(x) if mode != 1 else None
        sparse = None
        if mode != 0:
            lm_seg = segs[4 * self.nl]
            lm, lm_i = self.planes(self.w["lm_head.weight"], lm_seg)
            sparse = torch.zeros((self.B, self.V), dtype=f32, device="cuda")
            self.split(x, None, None, self.norm_w, H, lm_seg, xs, xs_i)
            self.gemm_h(xs, lm, self.V, H, lm_seg, C.EPI_SEGMAX, xs_i, lm_i, sparse, seq_of=self.seq_of)
            self.sparse_finish(sparse, 0)
        hidden = self.last_hidden(x)
        torch.cuda.synchronize()
        return dense, sparse, hidden


# ------------------------------------------------------------------------------------------ the tests
def check(cfg_name, kind, regime, mode=2, shift=None, side="left", holes=False, expect_segs=None, expect_fused=None):
    cfg, w = CONFIGS[cfg_name], weights(cfg_name, kind)
    ids, mask = batch(cfg, side, holes)
    m = Model(cfg, w, 16 if regime == "f16" else 0)
    try:
        segs, fused = m.weight_segments(), m.fused_act_layers()
        if expect_segs is not None:
            assert segs == [expect_segs] * (4 * cfg["num_hidden_layers"] + 1), segs
        if expect_fused is not None:
            assert fused == expect_fused, fused
        dense, sparse, hidden = m.encode(ids, mask, shift, mode, int(regime == "f16"))
    finally:
        m.close()
    r = Replay(cfg, w)
    T = r.plan(ids, mask, shift, mode)
    assert hidden.shape[0] == T
    if side == "left" and not holes:
        assert T == sum(LENS) == 180
    r_dense, r_sparse, r_hidden = r.run_f16(mode, segs, fused) if regime == "f16" else r.run_bf16(mode)
    what = (cfg_name, kind, regime, mode)
    assert torch.isfinite(hidden).all(), what
    assert torch.equal(r_hidden, hidden), (what, "sr_model_last_hidden")
    if mode != 1:
        assert torch.equal(r_dense, dense), (what, "dense")
        assert not dense[LENS.index(0)].any() and dense[0].any(), what
    if mode != 0:
        assert torch.equal(r_sparse, sparse), (what, "sparse")
        assert not sparse[LENS.index(0)].any() and sparse[0].any(), what


@pytest.mark.parametrize("cfg_name", ["A", "B"])
def test_bf16_regime_is_its_launches(cfg_name):
    check(cfg_name, "fp32", "bf16")


@pytest.mark.parametrize("cfg_name", ["A", "B"])
def test_f16_planes_three_segments(cfg_name):
    check(cfg_name, "fp32", "f16", expect_segs=3, expect_fused=[True, True])


@pytest.mark.parametrize("cfg_name", ["A", "B"])
def test_f16_planes_two_segments(cfg_name):
    check(cfg_name, "bf16", "f16", expect_segs=2, expect_fused=[True, True])


@pytest.mark.parametrize("cfg_name", ["A", "B"])
def test_f16_planes_one_layer_unfused(cfg_name):
    check(cfg_name, "loose", "f16", expect_fused=[True, False])


@pytest.mark.parametrize("regime", ["bf16", "f16"])
def test_row_shift(regime):
    """Rows that moved right by d_row_shift keep the positions of their own batch: RoPE and the pooled span follow the shift."""
    check("A", "fp32", regime, shift=[3, 10, 16, 15, 7, 0])


@pytest.mark.parametrize("regime", ["bf16", "f16"])
def test_sparse_span_with_holes(regime):
    """Mode 1, right padding, zeros inside the rows: the span is [first 1, last 1], masked tokens inside it are computed, are no keys
    and take no part in the sparse head's maximum."""
    check("B", "fp32", regime, mode=1, side="right", holes=True)
