"""CPU-only pieces shared by test_model_load_host.py and test_model_load_gpu.py: what loading a checkpoint leaves on the device
(csrc/model_weights.hip: sr_model_set_weight, sr_model_finalize, sr_lora_merge, the RoPE tables of sr_model_create) as a numpy model
of the contract, written from the comments of csrc/common.h (f32_to_bf16_sat, split_bf16x3, split_f16x2, row_scale_pow2),
csrc/kernels.h (split_map_w) and csrc/model_weights.hip (WeightDst, the LayerTensor table, pack_f16_weights) - not from the kernels -
with seeded tensor values that sit on the edges of every conversion, and the checker the GPU test runs over sr_model_readout.

Row maps (the internal row order; sr_model_readout does no un-permuting):
  q, k, v rows sit at row bases 0, nq, nq + nkv of the fused QKV matrix [(nh + 2 nkv) hd, H]  (nq = nh hd, nkv = n_kv hd)
  gate row r -> row (r // 16) * 32 + r % 16, up row r -> row (r // 16) * 32 + 16 + r % 16 of the gate-up matrix [2 I, H]
  a tied embedding is written to the fp32 embedding table AND to every lm_head buffer
Conversions of a weight row w (fp32, finite):
  bf16 layout    bf16(w), round to nearest even (a value at or above 0x7F7F8000 rounds to infinity there)
  fp32_planes 3  p0 = bf16_sat(w), p1 = bf16(w - p0), p2 = bf16(w - p0 - p1); segments along K in the order of split_map_w(3):
                 planes 0, 2, 1, 0, 1, 0
  fp32_planes 2  planes 0, 1, 0
  fp32_planes 16 sc = row_scale_pow2(max |row|) (1 for an all-zero row and for a maximum at or beyond 3e38), g0 = fp16(w sc),
                 g1 = fp16(w sc - g0); [g0 | g1 | g0], w_inv = 1 / sc; sr_model_finalize re-packs a MATRIX whose g1 is all zero to [g0 | g0]
  embedding table, norm weights: the values as fp32.  q / k / v bias: the values as fp32 and their bf16 roundings held as fp32.
The sign of a zero fp16 plane element is not part of the contract (tests/fp32_plane_cases.py: the device fuses scale, conversion and
subtraction, which does not keep IEEE's +0 for (-0) - (-0)): zeros of fp16 planes are compared as values, everything else as bits.

bf16-valued weights never have a low fp16 plane.  g0 holds 11 significand bits, a bf16 number 8; where w sc falls below fp16's normal
range (under 2^-14, i.e. more than 2^-28 below the row maximum) g0 keeps multiples of 2^-24 and the remainder is at most 2^-25, half of
fp16's smallest subnormal, which rounds (ties to even) to zero: g1 = 0 for every bf16 number at every scale
(test_model_load_host.py enumerates them all).  So the row with an element 2^-31 below its maximum - where g0 LOSES bits - does not
keep a third segment either; only an element with more significand bits than g0 holds does.

LoRA merge.  Truth: W + s (B @ A) in float64.  The kernel forms acc = sum_k B[o, k] A[k, i] in an fp32 chain (r products and r
additions, the first onto +0; fewer roundings under FMA contraction), then W + s acc: with e = 2^-24

    |w~ - truth| <= d = (r + 2) e (1 + 2^-10) (|W| + |s| sum_k |B[o, k] A[k, i]|)                                      (L)

r roundings of the chain, one of the scale, one of the add; the factor 1 + 2^-10 covers second order for r <= 64.

RoPE.  rope_tables: inv_freq in double (the llama3 arithmetic included), rounded to fp32 once; angle = fp32(p) * inv_freq in fp32;
cos and sin of the angle in double, rounded to fp32 once."""
import functools
import math

import numpy as np

import bf16_regime_cases as G
import dense_split_cases as D
import fp32_plane_cases as P

F32 = np.float32
E = 2.0 ** -24
PLANE_MODES = (0, 2, 3, 16)
SPLIT_ORDER = {3: (0, 2, 1, 0, 1, 0), 2: (0, 1, 0)}          # split_map_w
MAX_POS = 8192

# include/sr_hip.h: sr_model_readout's buffers and kinds
EMBED, LM_HEAD, NORM, ROPE_COS, ROPE_SIN, QKV, O, GATE_UP, DOWN, LN1, LN2, BIAS = range(12)
K_F32, K_BF16, K_PLANES, K_W_INV, K_BF16_AS_F32 = range(5)
BUFFER_NAMES = ["embed", "lm_head", "norm", "rope_cos", "rope_sin", "qkv", "o", "gate_up", "down", "ln1", "ln2", "bias"]
KIND_NAMES = ["f32", "bf16", "planes", "w_inv", "bf16_as_f32"]
MATRICES = (QKV, O, GATE_UP, DOWN)

# the smallest shape sr_model_create accepts that still has odd edges: n_qkv = 256, intermediate = 12 sixteen-row blocks, vocabulary =
# 2.5 column tiles of 128, 2 layers
BASE_CFG = dict(vocab_size=320, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=1, head_dim=64, rms_norm_eps=1e-5, rope_theta=500000.0, max_position_embeddings=512)


def config(tied=False, bias=False):
    c = dict(BASE_CFG, tie_word_embeddings=bool(tied))
    if bias:
        c["model_type"] = "qwen2"
    return c


def dims(cfg):
    nh, nkv, hd = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    return dict(H=cfg["hidden_size"], I=cfg["intermediate_size"], V=cfg["vocab_size"], nq=nh * hd, nkv=nkv * hd, hd=hd,
                n_qkv=(nh + 2 * nkv) * hd, layers=cfg["num_hidden_layers"])


def has_bias(cfg):
    return cfg.get("model_type") == "qwen2"


# ------------------------------------------------------------------------------------------ tensor values
SPECIAL_ROWS = {"halfway": 1, "zeros_subnormals": 17, "saturating": 18, "all_zero": 33, "pow2_max": 40, "below_pow2_max": 47,
                "far_below_max": 63}          # every matrix has at least 64 rows; 17 / 18 / 33 / 40 / 47 / 63 are not in block 0 of gate / up


def _bits(words):
    return np.asarray(words, np.uint32).view(F32)


def halfway_values(n, rng):
    """n fp32 values on and next to bf16 rounding boundaries: element c has a bf16 word of parity c & 1 under it and sits exactly
    halfway to the next one ((c >> 1) % 3 == 0), one fp32 ulp below (1) or above (2) the halfway point; random signs."""
    h = rng.integers(0x3C00, 0x4000, n).astype(np.uint32)                   # magnitudes 2^-7 .. 2
    c = np.arange(n, dtype=np.uint32)
    h = (h & np.uint32(0xFFFE)) | (c & np.uint32(1))
    low = np.array([0x8000, 0x7FFF, 0x8001], np.uint32)[(c >> 1) % 3]
    sign = rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)
    return _bits(sign | (h << np.uint32(16)) | low)


ZERO_WORDS_F32 = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x80008001, 0x00010000, 0x807F0000,
                  0x00800000, 0x80800001]     # +0, -0, fp32 subnormals (ties between bf16 subnormals among them), the smallest normals
ZERO_WORDS_BF16 = [w for w in ZERO_WORDS_F32 if not w & 0xFFFF]


def special_matrix(rows, cols, rng, bf16_only):
    """[rows, cols] fp32: gaussian rows / sqrt(cols), with the rows of SPECIAL_ROWS overwritten.  bf16_only: every value is a bf16
    number (the halfway and saturating rows then hold plain bf16 numbers: their edges are not representable)."""
    assert rows >= 64 and cols >= 64
    w = (rng.standard_normal((rows, cols)) / np.sqrt(cols)).astype(F32)
    if bf16_only:
        w = G.bf16_round(w)
    r = SPECIAL_ROWS
    if not bf16_only:
        w[r["halfway"]] = halfway_values(cols, rng)
        w[r["saturating"], 3] = _bits([0x7F7F8000])[0]                       # the smallest value the split's first plane saturates
        w[r["saturating"], 5] = _bits([0xFF7FFFFF])[0]                       # -FLT_MAX
    zw = ZERO_WORDS_BF16 if bf16_only else ZERO_WORDS_F32
    w[r["zeros_subnormals"], 2:2 + len(zw)] = _bits(zw)
    w[r["all_zero"]] = 0
    for name, top in (("pow2_max", F32(0.5)), ("below_pow2_max", F32(0.5 - 2.0 ** -9) if bf16_only else np.nextafter(F32(0.5), F32(0)))):
        row = w[r[name]]
        row *= F32(0.25) / np.abs(row).max()                                 # an exact power-of-two factor is not needed: rounded below
        if bf16_only:
            row[:] = G.bf16_round(row)
        row[7] = top
    row = w[r["far_below_max"]]
    _, ex = np.frexp(np.abs(row).max())                                      # max = m 2^ex, m in [0.5, 1)
    tail = 1 + 2.0 ** -7 + (0 if bf16_only else 2.0 ** -20)
    row[9] = F32(tail * 2.0 ** (int(ex) - 1 - 31))                           # 2^-31 below the maximum's binade
    assert np.isfinite(w).all()
    return np.ascontiguousarray(w, F32)


def special_vector(n, rng, bf16_only, centre=1.0):
    """[n] fp32 for a norm weight (centre 1) or a bias (centre 0): U(centre - 0.5, centre + 0.5) with the same edges as elements."""
    v = (centre - 0.5 + rng.random(n)).astype(F32)
    if bf16_only:
        v = G.bf16_round(v)
    else:
        v[1:13] = halfway_values(12, rng)
    zw = ZERO_WORDS_BF16 if bf16_only else ZERO_WORDS_F32
    v[16:16 + len(zw)] = _bits(zw)
    return np.ascontiguousarray(v, F32)


def tensor_shapes(cfg):
    d = dims(cfg)
    out = [("model.embed_tokens.weight", (d["V"], d["H"]))]
    for i in range(d["layers"]):
        p = f"model.layers.{i}."
        out += [(p + "self_attn.q_proj.weight", (d["nq"], d["H"])), (p + "self_attn.k_proj.weight", (d["nkv"], d["H"])),
                (p + "self_attn.v_proj.weight", (d["nkv"], d["H"])), (p + "self_attn.o_proj.weight", (d["H"], d["nq"])),
                (p + "mlp.gate_proj.weight", (d["I"], d["H"])), (p + "mlp.up_proj.weight", (d["I"], d["H"])),
                (p + "mlp.down_proj.weight", (d["H"], d["I"])), (p + "input_layernorm.weight", (d["H"],)),
                (p + "post_attention_layernorm.weight", (d["H"],))]
        if has_bias(cfg):
            out += [(p + "self_attn.q_proj.bias", (d["nq"],)), (p + "self_attn.k_proj.bias", (d["nkv"],)),
                    (p + "self_attn.v_proj.bias", (d["nkv"],))]
    out.append(("model.norm.weight", (d["H"],)))
    if not cfg["tie_word_embeddings"]:
        out.append(("lm_head.weight", (d["V"], d["H"])))
    return out


@functools.lru_cache(maxsize=None)
def _tensors(tied, bias, bf16_only, seed):
    cfg = config(tied, bias)
    out = {}
    for t, (name, shape) in enumerate(tensor_shapes(cfg)):
        rng = np.random.default_rng([seed, t, int(bf16_only)])
        if len(shape) == 2:
            out[name] = special_matrix(shape[0], shape[1], rng, bf16_only)
        else:
            out[name] = special_vector(shape[0], rng, bf16_only, centre=0.0 if name.endswith(".bias") else 1.0)
        out[name].setflags(write=False)
    return out


def tensors(cfg, bf16_only=False, seed=0):
    """name -> fp32 array (read-only, shared between tests) of every checkpoint tensor of cfg."""
    return dict(_tensors(bool(cfg["tie_word_embeddings"]), has_bias(cfg), bool(bf16_only), seed))


def to_bf16_words(a):
    """bf16-valued fp32 array -> the uint16 words a bf16 checkpoint stores."""
    return G.bf16_bits(a)


# ------------------------------------------------------------------------------------------ the model of the device layouts
def gate_row(r):
    r = np.asarray(r)
    return (r // 16) * 32 + r % 16


def up_row(r):
    return gate_row(r) + 16


def _bf16_words(w, defect):
    if defect == "truncation":
        return G.bf16_bits(G.bf16_trunc(w))
    with np.errstate(over="ignore"):
        return G.bf16_bits(G.bf16_round(w))


def _bf16_planes(w, planes, defect):
    with np.errstate(over="ignore", invalid="ignore"):
        p = list(D.split_planes(w))
    if defect == "truncation":                     # every plane by dropping bits: the planes still add up, but to other words
        p[0] = G.bf16_trunc(w)
        r1 = (w - p[0]).astype(F32)
        p[1] = G.bf16_trunc(r1)
        p[2] = G.bf16_trunc((r1 - p[1]).astype(F32))
    order = list(SPLIT_ORDER[planes])
    if defect == "segments_permuted":
        order[0], order[1] = order[1], order[0]
    if defect == "low_plane_dropped":
        low = planes - 1
        p[low] = np.zeros_like(p[low])
    return np.ascontiguousarray(np.concatenate([D.plane_words(p[i]) for i in order], axis=1))


def _f16_planes(w, defect):
    """([rows, 3 K] uint16 fp16 words [g0 | g1 | g0], w_inv fp32 [rows, 1], any g1 nonzero)."""
    with np.errstate(over="ignore", invalid="ignore"):
        pl, inv = P.weight_planes(w, 3)
    K = w.shape[1]
    g0, g1 = pl[:, :K].copy(), pl[:, K:2 * K].copy()
    if defect == "low_plane_dropped":
        g1[:] = 0
    segs = [g1, g0, g0] if defect == "segments_permuted" else [g0, g1, g0]
    if defect == "w_inv_off_by_2":
        inv = inv * F32(2)
    lo_nz = bool((g1.view(np.uint16) & np.uint16(0x7FFF)).any())
    return np.ascontiguousarray(np.concatenate(segs, axis=1)).view(np.uint16), inv.astype(F32).reshape(-1, 1), lo_nz


def _matrix_buffers(out, layer, buf, w, planes, finalized, defect):
    """The forms of one internal weight matrix w (rows already mapped)."""
    out[(layer, buf, K_BF16)] = _bf16_words(w, defect)
    if planes in (2, 3):
        out[(layer, buf, K_PLANES)] = _bf16_planes(w, planes, defect)
    elif planes == 16:
        pl, inv, lo_nz = _f16_planes(w, defect)
        if finalized and not lo_nz:
            K = w.shape[1]
            pl = np.ascontiguousarray(pl[:, :2 * K])
            pl[:, K:] = pl[:, :K]                                            # [g0 | g0]
        out[(layer, buf, K_PLANES)] = pl
        out[(layer, buf, K_W_INV)] = inv


def expected(cfg, t, planes, finalized=True, defect=None):
    """{(layer, buffer, kind): array [rows, elements per row]} of every buffer sr_model_readout reaches but the RoPE tables, for the
    checkpoint tensors t (name -> fp32 values).  uint16 for the bf16 layout and the plane segments, fp32 otherwise.
    defect: one of DEFECTS - what a wrong loader would leave; the checker must see each."""
    assert planes in PLANE_MODES and (defect is None or defect in DEFECTS)
    d = dims(cfg)
    out = {}
    col = lambda v: np.ascontiguousarray(v, F32).reshape(-1, 1)
    out[(-1, EMBED, K_F32)] = np.ascontiguousarray(t["model.embed_tokens.weight"], F32)
    out[(-1, NORM, K_F32)] = col(t["model.norm.weight"])
    head = t["model.embed_tokens.weight"] if cfg["tie_word_embeddings"] else t["lm_head.weight"]
    _matrix_buffers(out, -1, LM_HEAD, np.ascontiguousarray(head, F32), planes, finalized, defect)
    for i in range(d["layers"]):
        p = f"model.layers.{i}."
        parts = [t[p + f"self_attn.{n}_proj.weight"] for n in "qkv"]
        if defect == "qkv_bases_rolled":
            parts = [parts[2], parts[0], parts[1]]                           # v at base 0, q behind it
        qkv = np.concatenate(parts, axis=0)
        gu = np.empty((2 * d["I"], d["H"]), F32)
        g, u = t[p + "mlp.gate_proj.weight"], t[p + "mlp.up_proj.weight"]
        if defect == "gate_up_swapped":
            g, u = u, g
        gu[gate_row(np.arange(d["I"]))] = g
        gu[up_row(np.arange(d["I"]))] = u
        for buf, w in ((QKV, qkv), (O, t[p + "self_attn.o_proj.weight"]), (GATE_UP, gu), (DOWN, t[p + "mlp.down_proj.weight"])):
            _matrix_buffers(out, i, buf, np.ascontiguousarray(w, F32), planes, finalized, defect)
        out[(i, LN1, K_F32)] = col(t[p + "input_layernorm.weight"])
        out[(i, LN2, K_F32)] = col(t[p + "post_attention_layernorm.weight"])
        if has_bias(cfg):
            b = np.concatenate([t[p + f"self_attn.{n}_proj.bias"] for n in "qkv"])
            out[(i, BIAS, K_F32)] = col(b)
            out[(i, BIAS, K_BF16_AS_F32)] = col(b if defect == "bias_rounding_missing" else G.bf16_round(b))
    return out


# defect -> the plane modes in which it changes a buffer
DEFECTS = {"truncation": PLANE_MODES, "gate_up_swapped": PLANE_MODES, "qkv_bases_rolled": PLANE_MODES,
           "segments_permuted": (2, 3, 16), "w_inv_off_by_2": (16,), "low_plane_dropped": (2, 3, 16),
           "bias_rounding_missing": PLANE_MODES}


def expected_segments(cfg, t, planes):
    """sr_model_weight_segments of the finalized model: 4 per layer (qkv, o, gate-up, down), then the lm_head."""
    ex = expected(cfg, t, planes, finalized=True)
    d = dims(cfg)
    keys = [(i, b) for i in range(d["layers"]) for b in MATRICES] + [(-1, LM_HEAD)]
    if not planes:
        return [0] * len(keys)
    return [ex[(i, b, K_PLANES)].shape[1] // ex[(i, b, K_BF16)].shape[1] for i, b in keys]


def _same(key, planes, got, want):
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if key[2] == K_PLANES and planes == 16:                                  # zeros of fp16 planes are compared as values
        zero = lambda a: np.where((a & np.uint16(0x7FFF)) == 0, np.uint16(0), a)
        return np.array_equal(zero(got), zero(want))
    return np.array_equal(got.view(np.uint32) if got.dtype == F32 else got, want.view(np.uint32) if want.dtype == F32 else want)


def mismatches(planes, got, want):
    """Names of the buffers of `want` that `got` lacks or holds with other bits, shape or type."""
    bad = []
    for key, w in want.items():
        if key not in got or not _same(key, planes, got[key], w):
            layer, buf, kind = key
            where = ""
            if key in got and got[key].shape == w.shape and got[key].dtype == w.dtype:
                a, b = (x.view(np.uint32) if x.dtype == F32 else x for x in (got[key], w))
                rr, cc = np.nonzero(a != b)
                where = f" first at row {rr[0]} element {cc[0]}: {a[rr[0], cc[0]]:#x} != {b[rr[0], cc[0]]:#x}, {len(rr)} differ" if len(rr) else ""
            bad.append(f"layer {layer} {BUFFER_NAMES[buf]} {KIND_NAMES[kind]}{where}")
    return bad


# ------------------------------------------------------------------------------------------ LoRA merge
LORA_R = (1, 8, 64)
LORA_IN = (1, 255, 256, 257)
LORA_OUT = (1, 3, 300)
LORA_GUARD = 2            # rows in front of and behind W that must come back untouched


@functools.lru_cache(maxsize=None)
def lora_case(r, in_f, out_f, scale, seed=0):
    """(W, A, B) fp32.  W nearly cancels the update: W = -s (B @ A) (1 + 2^-12 g) rounded to fp32, g gaussian - the sum's terms are
    2^12 times its value, the regime in which a wrong accumulation order or a dropped term shows."""
    rng = np.random.default_rng([r, in_f, out_f, int(scale * 64) & 0xFFFF, seed])
    A = (rng.standard_normal((r, in_f)) / np.sqrt(in_f)).astype(F32)
    B = (rng.standard_normal((out_f, r)) * 0.3).astype(F32)
    upd = scale * (B.astype(np.float64) @ A.astype(np.float64))
    W = (-upd * (1 + 2.0 ** -12 * rng.standard_normal((out_f, in_f)))).astype(F32)
    for x in (W, A, B):
        x.setflags(write=False)
    return W, A, B


def lora_truth(W, A, B, scale):
    return W.astype(np.float64) + float(scale) * (B.astype(np.float64) @ A.astype(np.float64))


def lora_bound(W, A, B, scale):
    """(L), float64 [out, in]."""
    r = A.shape[0]
    mag = np.abs(B.astype(np.float64)) @ np.abs(A.astype(np.float64))
    return (r + 2) * E * (1 + 2.0 ** -10) * (np.abs(W.astype(np.float64)) + abs(float(scale)) * mag)


# ------------------------------------------------------------------------------------------ RoPE tables
ROPE_SETS = {
    "llama_1b": dict(head_dim=64, rope_theta=500000.0, rope_scaling={"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0,
                                                                     "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}),
    "llama_8b": dict(head_dim=128, rope_theta=500000.0, rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                                                      "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}),
    "qwen2": dict(head_dim=128, rope_theta=1000000.0, rope_scaling=None),
}
ROPE_POSITIONS = (0, 1, 63, 191, 511, 8191)


def rope_inv_freq(head_dim, rope_theta, rope_scaling=None):
    """inv_freq fp32 [head_dim / 2] as rope_tables forms it: element by element in double, one rounding."""
    out = np.empty(head_dim // 2, F32)
    for i in range(head_dim // 2):
        f = 1.0 / math.pow(float(rope_theta), (2 * i) / float(head_dim))
        if rope_scaling:
            factor, lo, hi = (float(rope_scaling[k]) for k in ("factor", "low_freq_factor", "high_freq_factor"))
            old = float(rope_scaling["original_max_position_embeddings"])
            low_wl, high_wl = old / lo, old / hi
            wl = 2.0 * math.pi / f
            f_l = f / factor if wl > low_wl else f
            if not wl < high_wl and not wl > low_wl:
                smooth = (old / wl - lo) / (hi - lo)
                f = (1.0 - smooth) * f_l / factor + smooth * f_l
            else:
                f = f_l
        out[i] = F32(f)
    return out


def rope_tables(inv, positions=None):
    """(cos, sin) fp32 [positions, head_dim / 2]: angle = fp32(p) * inv in fp32, cos / sin in double, rounded once."""
    p = np.arange(MAX_POS) if positions is None else np.asarray(positions)
    ang = (p.astype(F32)[:, None] * np.asarray(inv, F32)[None, :]).astype(F32).astype(np.float64)
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def ulps_apart(a, b):
    """fp32 arrays of one sign -> how many representable numbers apart."""
    a, b = (np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)
