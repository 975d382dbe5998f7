"""CPU-only pieces shared by test_fp32_planes_host.py and test_fp32_planes_gpu.py: what the fp32 regime on fp16 planes
(fp32_planes = 16, layer_f16_planes in csrc/encoder.hip) launches around the attention - the row split with its norm, the gate/up
bound, and the fp16-plane GEMM with each of its epilogues - as seeded cases, numpy restatements of the format arithmetic
(row_scale_pow2, split_f16x2 of csrc/common.h), float64 references, and the element-wise error bound of every kernel.

Every bound is derived here, never fitted and never computed from what a kernel returns.  e = 2^-24 is the unit roundoff of fp32
(round to nearest even); hipcc's default keeps fp32 division and square root correctly rounded and fp32 / fp16 denormals alive.

Split.  vs = v sc is exact (sc a power of two).  h0 = fp16(vs) is within 2^-11 |vs| (or, below 2^-14, within half a subnormal step
= 2^-25) of vs; r = vs - h0 is exact in fp32; h1 = fp16(r) is within max(2^-11 |r|, 2^-25) <= max(2^-22 |vs|, 2^-25) of r:

    |(h0 + h1) / sc - v| <= max(2^-22 |v sc|, 2^-25) / sc                                                           (S)

Without a norm the kernel's planes and inverse scales are bit-exact against the restatement (except the sign of a zero plane
element: hipcc fuses scale, conversion and subtraction into v_fma_mix instructions, which do not keep IEEE's +0 for (-0) - (-0) -
on MI355X the low plane of a -0 input is -0 - and a zero of either sign adds exactly nothing to a product; zeros are compared as
values, everything else as bits): a_inv = 1 / sc with sc the power of two
that puts max|row| into [2^14, 2^15) (1 for an all-zero row; an exact power of two 2^k lands on 2^14), segment order
[low | high | high] (two segments: [low | high]), third segment = second bit for bit.

Split with norm.  y = (v rs) w with rs = 1 / sqrt(ss / K + eps), ss = sum v^2 in fp32 in an unspecified order.  ss carries one
rounding per square and at most K - 1 per-term additions of positive numbers: relative (K + 1) e at most (K e first order).  / K and
+ eps: 2 e.  The square root halves that and adds e, the division adds e, the two products 2 e:

    |y~ - y| <= RN |y|,  RN = ((K + 3) / 2 + 4) e = (K / 2 + 5.5) e                                                 (N)

The kernel takes its scale from ITS maximum, which can sit on the other side of a power of two than the reference's: a_inv is
checked on its own (a power of two with max|y| sc in [2^14 (1 - RN), 2^15 (1 + RN))), and the reconstruction against
RN |y| + max(2^-22 (1 + RN) |y| sc_ref, 2^-24) / sc_ref: (S) with the floor of a scale one step below the reference's.

gate/up bound.  cmax~ = max_j fl(sqrt(n_gate_j) sqrt(n_up_j) 1.001), n = fp32 sum of K squares of (w0 + w1) (exact sum of two
planes, exact power-of-two inverse scale): (K + 1) e on each n, halved by the root, e per root, e per product, e for the factor:
cmax (1.001)(1 - (K + 5) e) <= cmax~ <= cmax (1.001)(1 + (K + 5) e); the first is what makes it a BOUND (cmax~ >= cmax for K < 2^13).
Row scale of the SwiGLU output: B = s2 cmax~ 1.02 with s2 = fp32 sum of y~^2, act_sc the power of two with B act_sc in
[2^14, 2^15): against B from float64 y with tolerance (2 RN + (K + 3) e), and act_inv act_sc == 1 exactly.

GEMM on planes.  The operands are exact fp16 numbers and their products exact in fp32, so float64 of the segment sum is the truth:
T[m, n] = a_inv[m] w_inv[n] sum_k A'[m, k] W'[n, k].  The MFMA chain adds K' = nseg K0 terms in fp32:

    |t~ - T| <= d = K' e a_inv[m] w_inv[n] sum_k |A'[m, k] W'[n, k]|      (sum in float64; the scales are exact powers of two)   (G)

Epilogues on t~:
  residual (10)   c = fl(c0 + t~):  |c - (c0 + T)| <= d + e (|c0 + T| + d).
  QKV (9)         x = fl(t~ + bias): dx = d + e (|T + bias| + d)  (no bias: dx = d, nothing is added).  Rotation of the first half
                  x1 and second half x2 of a head, products and sum rounded separately (three roundings):
                  a = fl(x1 c), b = fl(x2 s), y = fl(a - b):  ea = |c| dx1 + e (|x1 c| + |c| dx1), eb likewise,
                  |y - Y| <= ea + eb + e (|Y| + ea + eb); the second half x2 c + x1 s likewise.  v features: dx.
  SwiGLU (11)     y = fl(fl(g / fl(1 + expf(-g))) u).  |silu'| <= 1.1 carries dg; expf is within one ulp (2 e relative, times
                  exp / (1 + exp) < 1), the sum and the division add e each: es = 1.1 dg + 4 e (|silu(G)| + 1.1 dg) + 2^-121.  The
                  last term: expf(-g) overflows fp32 for g < -88.72, the kernel then returns -0 where |silu| < 2^-121.
                  |y - Y| <= ep + e (|Y| + ep) + 2^-149,  ep = es (|U| + du) + |silu(G)| du.
  split (13)      y as above, y osc exact, then (S) with osc in place of sc:
                  |(f0 + f1) / osc - Y| <= ey + max(2^-22 (|Y| + ey) , 2^-25 / osc),  and with osc B in [2^14, 2^15) the floor is
                  2^-25 / osc <= 2^-39 B: relative to the row's largest element r it is 2^-39 B / r, which passes the 2^-22 of
                  the split once B / r > 2^17 (the loose-bound case of the GPU test).
  max (12)        out[q, n] = max(+0, max over the rows m of sequence q of t~[m, n]).  With w the true winner, a row can win in the
                  kernel only if T[m] + d[m] >= T[w] - d[w]; the bound is the largest d among those rows.  A column whose rows all
                  have T + d < 0 gives exactly +0.  Rows with seq_of = -2 take no part.

Case kinds are seeded and built on the CPU; see gemm_case() and split_case()."""
import functools

import numpy as np

E = 2.0 ** -24
EPI_QKV, EPI_RESID, EPI_SWIGLU, EPI_SEGMAX, EPI_SPLIT = 9, 10, 11, 12, 13
EPILOGUES = {"qkv": EPI_QKV, "resid": EPI_RESID, "swiglu": EPI_SWIGLU, "segmax": EPI_SEGMAX, "split": EPI_SPLIT}
STAGED_4W = {EPI_RESID, EPI_SPLIT}            # fp16-plane epilogues with a staged four-wave form (EpiTraits::STAGED_4W)
MAX_POS = 512

# (a_nseg, K0): K' = nseg K0 of 3, 4, 5, 12, 12 and 15 k-steps of 64 - below the pipelined loops, their minimum, odd, longer
K_CONFIGS = [(3, 64), (2, 128), (2, 160), (3, 256), (2, 384), (3, 320)]
GEMM_M = [1, 17, 33, 65, 200, 300]
GEMM_N = [128, 320]


# ------------------------------------------------------------------------------------------ format arithmetic
def row_scale_pow2(mx):
    """csrc/common.h: the power of two sc with mx sc in [2^14, 2^15); 1 for a maximum that is zero, NaN or beyond 3e38."""
    mx = np.asarray(mx, np.float32)
    ok = (mx > 0) & (mx < np.float32(3.0e38))
    _, e = np.frexp(np.where(ok, mx, np.float32(1)))
    return np.where(ok, np.ldexp(np.float32(1), np.clip(15 - e, -100, 100)), np.float32(1)).astype(np.float32)


def split_f16x2(vs):
    """csrc/common.h: fp32 -> (high, low) fp16 planes."""
    vs = np.asarray(vs, np.float32)
    h0 = vs.astype(np.float16)
    h1 = (vs - h0.astype(np.float32)).astype(np.float16)
    return h0, h1


def act_planes(x, nseg, defect=None):
    """Rows of fp32 x -> ([low | high | high] or [low | high] fp16, a_inv fp32): what rows_split_h_kernel writes without a norm."""
    x = np.asarray(x, np.float32)
    mx = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(len(x), np.float32)
    sc = row_scale_pow2(mx)
    if defect == "scale_off_at_pow2":            # frexp's exponent used as if the mantissa were in [1, 2)
        m, _ = np.frexp(mx)
        sc = np.where(m == 0.5, sc * np.float32(2), sc).astype(np.float32)
    h0, h1 = split_f16x2(x * sc[:, None])
    if defect == "low_dropped":
        h1 = np.zeros_like(h1)
    segs = [h1, h0, h1 if defect == "third_from_low" else h0][:nseg]
    return np.ascontiguousarray(np.concatenate(segs, axis=1)), (np.float32(1) / sc).astype(np.float32)


def weight_planes(w, nseg):
    """Rows of fp32 w -> ([high | low | high] or [high | high] fp16, w_inv fp32) as convert_rows_split_h_kernel / pack_f16_weights
    lay them out.  nseg = 2 needs an all-zero low plane (see fp16_valued)."""
    w = np.asarray(w, np.float32)
    sc = row_scale_pow2(np.abs(w).max(axis=1))
    g0, g1 = split_f16x2(w * sc[:, None])
    if nseg == 2:
        assert not g1.any(), "two segments need weights without a low plane"
        segs = [g0, g0]
    else:
        segs = [g0, g1, g0]
    return np.ascontiguousarray(np.concatenate(segs, axis=1)), (np.float32(1) / sc).astype(np.float32)


def fp16_valued(w):
    """w with every row rounded to what its high fp16 plane holds: the low plane is zero."""
    w = np.asarray(w, np.float32)
    sc = row_scale_pow2(np.abs(w).max(axis=1))[:, None]
    return ((w * sc).astype(np.float16).astype(np.float32) / sc).astype(np.float32)


def planes_value(planes, inv, nseg, activation=True):
    """float64 value the plane segments stand for: (low + high) inv."""
    K = planes.shape[1] // nseg
    p = planes.astype(np.float64)
    v = p[:, :K] + p[:, K:2 * K] if (activation or nseg == 3) else p[:, :K]
    return v * np.asarray(inv, np.float64)[:, None]


def is_pow2(x):
    m, _ = np.frexp(np.asarray(x, np.float32))
    return m == 0.5


# ------------------------------------------------------------------------------------------ row split
SPLIT_K = [64, 192, 320, 2048, 4096, 8192]        # generic kernel (K % 256 != 0) x 3, register kernels x 3
SPLIT_T = [1, 3, 4, 5, 9]                         # a block holds four rows
VOCAB = 23


@functools.lru_cache(maxsize=None)
def split_case(K, T, seed=0):
    """Rows [T, K] fp32 whose first rows are the edges (as many as T has room for, the rest random with a per-row magnitude),
    a norm weight, an embedding table with token ids out of order, eps."""
    rng = np.random.default_rng(1000 * K + 10 * T + seed)
    x = (rng.standard_normal((T, K)) * np.exp(rng.uniform(-4, 4, (T, 1)))).astype(np.float32)
    edges = []
    e0 = np.zeros(K, np.float32); e0[1::2] = -0.0; edges.append(("zero", e0))                                         # noqa: E702
    e1 = (rng.standard_normal(K) * 1e-3).astype(np.float32); e1[K // 3] = np.float32(2.0 ** 20 * 1e-3); edges.append(("outlier", e1))   # noqa: E702
    e2 = (rng.uniform(-1, 1, K) * 3.9).astype(np.float32); e2[K - 1] = np.float32(-4.0); edges.append(("pow2_in_tail", e2))             # noqa: E702
    e3 = e2.copy(); e3[K - 1] = np.nextafter(np.float32(4.0), np.float32(0)); edges.append(("below_pow2", e3))                          # noqa: E702
    e4 = (rng.integers(-900, 900, K).astype(np.float32) * np.float32(2.0 ** -149)); edges.append(("denormal", e4))                      # noqa: E702
    order = [2, 1, 0, 4, 3] if T >= 5 else [2, 0, 1, 3, 4]        # T = 1: the power-of-two maximum in the last K tail
    names = []
    for r, i in enumerate(order[:T]):
        x[r] = edges[i][1]
        names.append(edges[i][0])
    w = rng.uniform(0.5, 1.5, K).astype(np.float32)
    embed = (rng.standard_normal((VOCAB, K)) * np.exp(rng.uniform(-2, 2, (VOCAB, 1)))).astype(np.float32)
    embed[5] = e1
    tok = rng.permutation(VOCAB)[:T].astype(np.int32) if T <= VOCAB else rng.integers(0, VOCAB, T).astype(np.int32)
    if T >= 3:
        tok[1] = 5
    return dict(K=K, T=T, x=x, w=w, embed=embed, tok=tok, eps=1e-5, edge_names=names)


def norm_reference(x, w, eps):
    """float64 RMSNorm of fp32 rows + (N)."""
    x64 = np.asarray(x, np.float64)
    K = x64.shape[1]
    y = x64 / np.sqrt((x64 * x64).mean(axis=1, keepdims=True) + eps) * np.asarray(w, np.float64)
    return y, (K / 2 + 5.5) * E


def norm_ideal(x, w, eps):
    """The kernel's norm in numpy fp32, every operation rounded once (numpy's own summation order)."""
    x = np.asarray(x, np.float32)
    ss = (x * x).sum(axis=1, dtype=np.float32)
    rs = np.float32(1) / np.sqrt(ss / np.float32(x.shape[1]) + np.float32(eps), dtype=np.float32)
    return ((x * rs[:, None]) * np.asarray(w, np.float32)).astype(np.float32)


def _zero_signs_off(planes):
    """fp16 bits with -0 written as +0."""
    u = planes.view(np.uint16).copy()
    u[u == 0x8000] = 0
    return u


def check_split_exact(x, nseg, planes, a_inv):
    """Split without norm: bit-exact against the restatement, and the properties that make the restatement right.  Returns a
    list of failure strings (empty = pass)."""
    x = np.asarray(x, np.float32)
    K = x.shape[1]
    bad = []
    ref_p, ref_i = act_planes(x, nseg)
    if planes.shape != ref_p.shape:
        return [f"planes shape {planes.shape} != {ref_p.shape}"]
    if not np.array_equal(a_inv.view(np.uint32), ref_i.view(np.uint32)):
        bad.append(f"a_inv differs in rows {np.flatnonzero(a_inv != ref_i)[:8].tolist()}")
    if not np.array_equal(_zero_signs_off(planes), _zero_signs_off(ref_p)):
        r, c = np.nonzero(_zero_signs_off(planes) != _zero_signs_off(ref_p))
        bad.append(f"planes differ at {list(zip(r[:6].tolist(), c[:6].tolist()))} ({len(r)} elements)")
    if nseg == 3 and not np.array_equal(planes[:, K:2 * K].view(np.uint16), planes[:, 2 * K:].view(np.uint16)):
        bad.append("third segment != second segment")
    mx = np.abs(x.astype(np.float64)).max(axis=1)
    sc = 1.0 / a_inv.astype(np.float64)
    if not np.all(is_pow2(a_inv)):
        bad.append("a_inv is not a power of two")
    live = (mx > 0) & (mx * 2.0 ** 100 >= 2.0 ** 14)          # the scale is capped at 2^100 (denormal rows)
    if not np.all((mx[live] * sc[live] >= 2.0 ** 14) & (mx[live] * sc[live] < 2.0 ** 15)):
        bad.append("max|row| sc outside [2^14, 2^15)")
    if not np.all(a_inv[mx == 0] == 1):
        bad.append("a_inv of an all-zero row is not 1")
    rec = planes_value(planes, a_inv, nseg)
    bound = np.maximum(2.0 ** -22 * np.abs(x.astype(np.float64)) * sc[:, None], 2.0 ** -25) / sc[:, None]
    if not np.all(np.abs(rec - x.astype(np.float64)) <= bound):
        bad.append(f"reconstruction leaves (S): worst ratio {np.max(np.abs(rec - x) / bound):.3g}")
    return bad


def check_split_norm(x, w, eps, nseg, planes, a_inv):
    """Split with norm against float64 RMSNorm: a_inv on its own, the reconstruction within (N) + (S).  Failure strings."""
    y, rn = norm_reference(x, w, eps)
    K = y.shape[1]
    bad = []
    mx = np.abs(y).max(axis=1)
    sc = 1.0 / a_inv.astype(np.float64)
    if not np.all(is_pow2(a_inv)):
        bad.append("a_inv is not a power of two")
    live = mx * 2.0 ** 100 >= 2.0 ** 15           # the scale is capped at 2^100 (denormal rows)
    if not np.all((mx[live] * sc[live] >= 2.0 ** 14 * (1 - rn)) & (mx[live] * sc[live] < 2.0 ** 15 * (1 + rn))):
        bad.append("max|y| sc outside [2^14, 2^15)")
    if not np.all(a_inv[mx == 0] == 1):
        bad.append("a_inv of an all-zero row is not 1")
    if nseg == 3 and not np.array_equal(planes[:, K:2 * K].view(np.uint16), planes[:, 2 * K:].view(np.uint16)):
        bad.append("third segment != second segment")
    sc_ref = row_scale_pow2(mx.astype(np.float32)).astype(np.float64)[:, None]
    bound = rn * np.abs(y) + np.maximum(2.0 ** -22 * (1 + rn) * np.abs(y) * sc_ref, 2.0 ** -24) / sc_ref
    rec = planes_value(planes, a_inv, nseg)
    if not np.all(np.abs(rec - y) <= bound):
        bad.append(f"reconstruction leaves (N) + (S): worst ratio {np.max(np.abs(rec - y) / bound):.3g}")
    return bad


def cmax_reference(wgu_planes, wgu_inv, nseg):
    """float64 max_j |w_gate_j||w_up_j| of an interleaved gate/up matrix given as plane segments, and every p_j."""
    w = planes_value(wgu_planes, wgu_inv, nseg, activation=False)
    n = np.sqrt((w * w).sum(axis=1)).reshape(-1, 2, 16)
    p = (n[:, 0] * n[:, 1]).reshape(-1)
    return p.max(), p


def check_cmax(cmax, wgu_planes, wgu_inv, nseg):
    K = wgu_planes.shape[1] // nseg
    true, _ = cmax_reference(wgu_planes, wgu_inv, nseg)
    t = (K + 5) * E
    bad = []
    if not cmax >= true:
        bad.append(f"cmax {cmax} is below the true maximum {true}: not a bound")
    if not (true * 1.001 * (1 - t) <= cmax <= true * 1.001 * (1 + t)):
        bad.append(f"cmax {cmax} outside 1.001 x {true} (1 +- {t:.2g})")
    return bad


def check_act_scale(x, w, eps, cmax, act_sc, act_inv):
    """act_sc: the power of two with B act_sc in [2^14, 2^15), B = |y|^2 cmax 1.02; act_inv act_sc == 1."""
    y, rn = (norm_reference(x, w, eps) if w is not None else (np.asarray(x, np.float64), 0.0))
    K = y.shape[1]
    B = (y * y).sum(axis=1) * float(cmax) * 1.02
    t = 2 * rn + (K + 3) * E
    bad = []
    if not np.all(is_pow2(act_sc)):
        bad.append("act_sc is not a power of two")
    if not np.all(act_sc.astype(np.float64) * act_inv.astype(np.float64) == 1.0):
        bad.append("act_inv act_sc != 1")
    live = (y * y).sum(axis=1) > 2.0 ** -60          # below, the fp32 squares underflow (denormal rows): no claim on the scale
    bs = B[live] * act_sc.astype(np.float64)[live]
    if not np.all((bs >= 2.0 ** 14 * (1 - t)) & (bs < 2.0 ** 15 * (1 + t))):
        bad.append("B act_sc outside [2^14, 2^15)")
    if not np.all(act_sc[B == 0] == 1):
        bad.append("act_sc of a zero row is not 1")
    return bad


# ------------------------------------------------------------------------------------------ GEMM cases
def rope_tables(hd, theta=10000.0):
    inv = theta ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    ang = np.arange(MAX_POS, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def interleave_gate_up(wg, wu):
    """[I, K] gate and up rows -> [2 I, K], alternating in blocks of 16 (the layout the SwiGLU epilogues read)."""
    I, K = wg.shape
    return np.stack([wg.reshape(I // 16, 16, K), wu.reshape(I // 16, 16, K)], axis=1).reshape(2 * I, K)


def seq_ids(M):
    """Ascending sequence ids for M token rows with -2 (masked) rows inside: a sequence of 1 next to one of 200 when M has room,
    lengths that straddle the 16-row slabs of a wave and the tile borders; one trailing sequence without a row."""
    if M >= 250:
        lens = [1, 200, M - 201]
    elif M >= 8:
        a = M // 2 + 1
        lens = [1, a, M - 1 - a]
    else:
        lens = [M]
    ids = np.concatenate([np.full(n, q, np.int32) for q, n in enumerate(lens)])
    masked = np.arange(3, M, 7)
    ids[masked] = -2
    return ids, len(lens) + 1


@functools.lru_cache(maxsize=None)
def gemm_case(epi, M, N, nseg, K0, seed=0, hd=64, bias=True, n_rope=None, out_nseg=3, a_seg=None):
    """One fp16-plane GEMM problem as numpy arrays.  Activation and weight rows carry distinct power-of-two scales (magnitudes over
    e^+-3), positions are shuffled, so that a wrong row offset of a_scale / out_scale / pos / seq_of changes the result.
    a_seg: segment count of the ACTIVATION planes if it differs from the weights' (2 segments against [w0 | 0 | w0] never occurs in
    the encoder; used for the 2-equals-3 check through zero_low below)."""
    rng = np.random.default_rng([epi, M, N, nseg, K0, seed, hd])
    a = (rng.standard_normal((M, K0)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float32)
    w = (rng.standard_normal((N, K0)) / np.sqrt(K0) * np.exp(rng.uniform(-3, 3, (N, 1)))).astype(np.float32)
    c = dict(epi=epi, M=M, N=N, nseg=nseg, K0=K0, K=nseg * K0)
    if epi == EPI_SEGMAX:
        # column 0 of the activations is large and positive in every row, feature 5 of W points against it: an all-negative column
        a[:, 0] = np.abs(a).max(axis=1) * 2
        w[5] = 0
        w[5, 0] = -1.0
        c["seq_of"], c["n_seq"] = seq_ids(M)
        a[c["seq_of"] == -2] *= 64.0              # masked rows carry the largest values
    if epi in (EPI_SWIGLU, EPI_SPLIT):
        # large |g| of both signs: output features 1 and 2 get gate rows along / against activation row 0 (and whatever the other
        # rows make of them), scaled so that |g| reaches ~100 (expf(-g) overflows below -88.7) and ~30
        I = N // 2
        wg, wu = w[:I].copy(), w[I:].copy()
        dirn = a[0] / np.linalg.norm(a[0]) ** 2
        wg[1], wg[2] = (100.0 * dirn).astype(np.float32), (-100.0 * dirn).astype(np.float32)
        wg[3], wg[4] = (30.0 * dirn).astype(np.float32), (-30.0 * dirn).astype(np.float32)
        w = interleave_gate_up(wg, wu)
    if nseg == 2:
        w = fp16_valued(w)
    c["A"], c["a_inv"] = act_planes(a, nseg)
    c["W"], c["w_inv"] = weight_planes(w, nseg)
    if epi == EPI_RESID:
        c["C0"] = (rng.standard_normal((M, N)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float32)
    if epi == EPI_QKV:
        c["hd"], c["n_rope"] = hd, (N - hd if n_rope is None else n_rope)
        c["cos"], c["sin"] = rope_tables(hd)
        c["pos"] = rng.permutation(MAX_POS)[:M].astype(np.int32)
        c["bias"] = (rng.standard_normal(N) * np.abs(w).max(axis=1) * np.sqrt(K0)).astype(np.float32) if bias else None
    if epi == EPI_SPLIT:
        # the row scale of the output as the encoder derives it: B = |row|^2 cmax 1.02 (in float64 here; the GPU test takes it from
        # the row-split hook as well)
        cm, _ = cmax_reference(c["W"], c["w_inv"], nseg)
        B = (planes_value(c["A"], c["a_inv"], nseg) ** 2).sum(axis=1) * cm * 1.001 * 1.02
        c["out_scale"] = row_scale_pow2(B.astype(np.float32))
        c["out_nseg"] = out_nseg
    return c


def _products(c, a_inv=None):
    """(T, d) of (G): float64 truth and the MFMA chain's bound, [M, N]."""
    A, W = c["A"].astype(np.float64), c["W"].astype(np.float64)
    sc = np.outer((c["a_inv"] if a_inv is None else a_inv).astype(np.float64), c["w_inv"].astype(np.float64))
    return (A @ W.T) * sc, c["K"] * E * (np.abs(A) @ np.abs(W).T) * sc


def _silu(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def _deinterleave(x):
    """[M, 2 I] accumulator columns in the interleaved row order -> (gate [M, I], up [M, I])."""
    M, N = x.shape
    b = x.reshape(M, N // 32, 2, 16)
    return b[:, :, 0].reshape(M, N // 2), b[:, :, 1].reshape(M, N // 2)


def _swiglu_ref(T, d):
    G, U = _deinterleave(T)
    dg, du = _deinterleave(d)
    s = _silu(G)
    es = 1.1 * dg + 4 * E * (np.abs(s) + 1.1 * dg) + 2.0 ** -121
    ep = es * (np.abs(U) + du) + np.abs(s) * du
    Y = s * U
    return Y, ep + E * (np.abs(Y) + ep) + 2.0 ** -149


_REFS = {}


def gemm_reference(c):
    """(ref, bound[, must_be_zero]) in float64, shaped like the decoded output (see decode); computed once per case."""
    if id(c) not in _REFS:
        while len(_REFS) >= 4:                        # a few cases at a time: the arrays are [M, N] float64 each
            _REFS.pop(next(iter(_REFS)))
        _REFS[id(c)] = (c, _gemm_reference(c))        # holds c, so that its id stays its own
    return _REFS[id(c)][1]


def _gemm_reference(c):
    epi = c["epi"]
    T, d = _products(c)
    if epi == EPI_RESID:
        ref = c["C0"].astype(np.float64) + T
        return ref, d + E * (np.abs(ref) + d)
    if epi == EPI_QKV:
        X, dx = T, d
        if c["bias"] is not None:
            X = T + c["bias"].astype(np.float64)
            dx = d + E * (np.abs(X) + d)
        hd, h2, nr = c["hd"], c["hd"] // 2, c["n_rope"]
        ref, bound = X.copy(), dx.copy()
        cs, sn = c["cos"].astype(np.float64)[c["pos"]], c["sin"].astype(np.float64)[c["pos"]]     # [M, hd / 2]
        for h0 in range(0, nr, hd):
            x1, x2, d1, d2 = X[:, h0:h0 + h2], X[:, h0 + h2:h0 + hd], dx[:, h0:h0 + h2], dx[:, h0 + h2:h0 + hd]
            for lo in (True, False):
                p, q, dp, dq = (x1, x2, d1, d2) if lo else (x2, x1, d2, d1)          # lo: x1 c - x2 s;  hi: x2 c + x1 s
                ea = np.abs(cs) * dp + E * (np.abs(p * cs) + np.abs(cs) * dp)
                eb = np.abs(sn) * dq + E * (np.abs(q * sn) + np.abs(sn) * dq)
                Y = p * cs - q * sn if lo else p * cs + q * sn
                sl = slice(h0, h0 + h2) if lo else slice(h0 + h2, h0 + hd)
                ref[:, sl], bound[:, sl] = Y, ea + eb + E * (np.abs(Y) + ea + eb)
        return ref, bound
    if epi == EPI_SWIGLU:
        return _swiglu_ref(T, d)
    if epi == EPI_SPLIT:
        Y, ey = _swiglu_ref(T, d)
        osc = c["out_scale"].astype(np.float64)[:, None]
        return Y, ey + np.maximum(2.0 ** -22 * (np.abs(Y) + ey), 2.0 ** -25 / osc)
    assert epi == EPI_SEGMAX
    ids, nq = c["seq_of"], c["n_seq"]
    ref, bound, zero = np.zeros((nq, c["N"])), np.zeros((nq, c["N"])), np.ones((nq, c["N"]), bool)
    for q in range(nq):
        rows = np.flatnonzero(ids == q)
        if not len(rows):
            continue
        Tq, dq = T[rows], d[rows]
        wi = Tq.argmax(axis=0)
        top, dtop = Tq.max(axis=0), np.take_along_axis(dq, wi[None], 0)[0]
        can_win = Tq + dq >= (top - dtop)[None]
        bq = np.where(can_win, dq, 0).max(axis=0)
        ref[q], bound[q] = np.maximum(top, 0.0), bq
        zero[q] = (Tq + dq < 0).all(axis=0)
    return ref, bound, zero


def decode(c, out):
    """A kernel's (or the ideal arithmetic's) output -> the float64 values gemm_reference speaks about."""
    if c["epi"] != EPI_SPLIT:
        return np.asarray(out, np.float64)
    I, ns = c["N"] // 2, c["out_nseg"]
    assert out.shape == (c["M"], ns * I) and out.dtype == np.float16
    p = out.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (p[:, :I] + p[:, I:2 * I]) / c["out_scale"].astype(np.float64)[:, None]


def check_gemm(c, out):
    """Failure strings of an output against the reference and its bound."""
    r = gemm_reference(c)
    ref, bound = r[0], r[1]
    bad = []
    if c["epi"] == EPI_SPLIT:
        I = c["N"] // 2
        if not np.isfinite(out.astype(np.float32)).all():
            bad.append("inf or NaN in a plane")
        if c["out_nseg"] == 3 and not np.array_equal(out[:, I:2 * I].view(np.uint16), out[:, 2 * I:].view(np.uint16)):
            bad.append("third segment != second segment")
    val = decode(c, out)
    if val.shape != ref.shape:
        return bad + [f"shape {val.shape} != {ref.shape}"]
    err = np.abs(val - ref)
    if not np.all(err <= bound):
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        bad.append(f"{int((err > bound).sum())} elements outside the bound, e.g. {i}: |{val[i]:.9g} - {ref[i]:.9g}| = {err[i]:.3g} > {bound[i]:.3g}")
    if c["epi"] == EPI_SEGMAX:
        z = r[2]
        if not np.all(np.asarray(out, np.float32).view(np.uint32)[z] == 0):
            bad.append("a column without a positive maximum is not exactly +0")
    return bad


def worst_ratio(c, out):
    r = gemm_reference(c)
    err = np.abs(decode(c, out) - r[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(r[1] > 0, err / r[1], np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


# ------------------------------------------------------------------------------------------ ideal arithmetic and defects
GEMM_DEFECTS = {
    "low_plane_dropped": (EPI_SPLIT,),                    # the split epilogue stores zeros for f1
    "third_from_low": (EPI_SPLIT,),                       # third output segment = f1 instead of f0
    "row0_scale": (EPI_RESID, EPI_QKV, EPI_SWIGLU, EPI_SEGMAX, EPI_SPLIT),     # rows >= 256 take a_scale[m - 256]
    "row0_out_scale": (EPI_SPLIT,),                       # rows >= 256 take out_scale[m - 256]
    "row0_pos": (EPI_QKV,),                               # rows >= 256 take pos[m - 256]
    "row0_seq": (EPI_SEGMAX,),                            # rows >= 256 take seq_of[m - 256]
    "bias_after_rotation": (EPI_QKV,),
    "gate_up_swapped": (EPI_SWIGLU, EPI_SPLIT),
    "masked_row_in_max": (EPI_SEGMAX,),
}


def _shift(v, row0=256):
    v = np.asarray(v).copy()
    v[row0:] = v[:len(v) - row0]
    return v


def gemm_ideal(c, defect=None):
    """float64 products rounded to fp32 once, then the kernel's epilogue in numpy fp32 - every operation rounded once, exactly the
    kernel's roundings; optionally with one defect of GEMM_DEFECTS."""
    f32 = np.float32
    epi = c["epi"]
    assert defect is None or epi in GEMM_DEFECTS[defect]
    a_inv = _shift(c["a_inv"]) if defect == "row0_scale" else c["a_inv"]
    A, W = c["A"].astype(np.float64), c["W"].astype(np.float64)
    t = (A @ W.T).astype(f32) * np.outer(a_inv, c["w_inv"]).astype(f32)
    if epi == EPI_RESID:
        return (c["C0"] + t).astype(f32)
    if epi == EPI_QKV:
        pos = _shift(c["pos"]) if defect == "row0_pos" else c["pos"]
        x = t if c["bias"] is None or defect == "bias_after_rotation" else (t + c["bias"]).astype(f32)
        out = x.copy()
        hd, h2 = c["hd"], c["hd"] // 2
        cs, sn = c["cos"][pos], c["sin"][pos]
        for h0 in range(0, c["n_rope"], hd):
            x1, x2 = x[:, h0:h0 + h2], x[:, h0 + h2:h0 + hd]
            out[:, h0:h0 + h2] = (x1 * cs).astype(f32) - (x2 * sn).astype(f32)
            out[:, h0 + h2:h0 + hd] = (x2 * cs).astype(f32) + (x1 * sn).astype(f32)
        if defect == "bias_after_rotation" and c["bias"] is not None:
            out = (out + c["bias"]).astype(f32)
        return out
    if epi in (EPI_SWIGLU, EPI_SPLIT):
        g, u = _deinterleave(t)
        if defect == "gate_up_swapped":
            g, u = u, g
        with np.errstate(over="ignore"):
            y = ((g / (f32(1) + np.exp(-g, dtype=f32))).astype(f32) * u).astype(f32)
        if epi == EPI_SWIGLU:
            return y
        osc = _shift(c["out_scale"]) if defect == "row0_out_scale" else c["out_scale"]
        with np.errstate(over="ignore", invalid="ignore"):        # a defect's wrong scale can overflow fp16
            f0, f1 = split_f16x2(y * osc[:, None])
        if defect == "low_plane_dropped":
            f1 = np.zeros_like(f1)
        return np.ascontiguousarray(np.concatenate([f1, f0, f1 if defect == "third_from_low" else f0][:c["out_nseg"]], axis=1))
    ids = _shift(c["seq_of"]) if defect == "row0_seq" else c["seq_of"].copy()
    if defect == "masked_row_in_max":
        for m in range(1, len(ids)):
            if ids[m] == -2:
                ids[m] = ids[m - 1]
    out = np.zeros((c["n_seq"], c["N"]), f32)
    for q in range(c["n_seq"]):
        rows = np.flatnonzero(ids == q)
        if len(rows):
            out[q] = np.maximum(t[rows].max(axis=0), f32(0))
    return out


# ------------------------------------------------------------------------------------------ the loose-bound case
LOOSE_LOG2 = {32: 15.0, 1024: 25.0}      # log2(B / r) beyond which a row of loose_case(factor) counts as loose (Gaussian weights: ~6)


@functools.lru_cache(maxsize=None)
def loose_case(factor, K0=256, I=512, T=16, seed=0):
    """Gate/up weights with ONE pair (j = 7) multiplied by `factor`, normalised inputs: the Cauchy-Schwarz bound B of every row is
    set by that pair, the row's real maximum r is not (half the rows have a negative gate there and silu silences it)."""
    rng = np.random.default_rng([factor, K0, I, T, seed])
    x = rng.standard_normal((T, K0)).astype(np.float32)
    wn = rng.uniform(0.5, 1.5, K0).astype(np.float32)
    wg = (rng.standard_normal((I, K0)) / np.sqrt(K0)).astype(np.float32)
    wu = (rng.standard_normal((I, K0)) / np.sqrt(K0)).astype(np.float32)
    wg[7] *= np.float32(factor)
    wu[7] *= np.float32(factor)
    W, w_inv = weight_planes(interleave_gate_up(wg, wu), 3)
    return dict(factor=factor, K0=K0, I=I, T=T, x=x, wn=wn, eps=1e-5, W=W, w_inv=w_inv)


def fused_looseness(wg, wu, hidden):
    """The criterion of sr_model_finalize in float64: hidden max_j p_j / median_j p_j over up to 256 evenly spaced pairs,
    p_j = |w_gate_j||w_up_j|; a layer runs the fused SwiGLU split while this is below 2^16."""
    p = np.linalg.norm(np.asarray(wg, np.float64), axis=1) * np.linalg.norm(np.asarray(wu, np.float64), axis=1)
    I = len(p)
    ns = min(I, 256)
    sample = np.sort(p[[k * I // ns for k in range(ns)]])
    return hidden * p.max() / sample[ns // 2]


def loose_reference(c):
    """float64: the normalised rows y, the SwiGLU output Y of the plane weights, each row's largest |Y| (rmax) and its bound B."""
    y, _ = norm_reference(c["x"], c["wn"], c["eps"])
    w = planes_value(c["W"], c["w_inv"], 3, activation=False)
    G, U = _deinterleave(y @ w.T)
    Y = _silu(G) * U
    cm, _ = cmax_reference(c["W"], c["w_inv"], 3)
    return dict(y=y, Y=Y, rmax=np.abs(Y).max(axis=1), B=(y * y).sum(axis=1) * cm * 1.001 * 1.02)


# ------------------------------------------------------------------------------------------ the GPU test's problems
QKV_VARIANTS = [  # (head_dim, N, n_rope, bias, K configs): n_rope a multiple of 128 and not, v features behind it
    (64, 128, 64, True, K_CONFIGS), (64, 320, 256, False, K_CONFIGS), (64, 320, 192, True, K_CONFIGS),
    (128, 256, 128, False, K_CONFIGS[::2]), (128, 384, 256, True, K_CONFIGS[1::2]),
]


def epilogue_cases(epi, Ms=None):
    """Every problem test_fp32_planes_gpu.py runs for an epilogue (test_fp32_planes_host.py walks the same list)."""
    out = []
    for M in (GEMM_M if Ms is None else Ms):
        if epi == EPI_QKV:
            for hd, N, nr, bias, kcs in QKV_VARIANTS:
                out += [gemm_case(epi, M, N, nseg, K0, hd=hd, bias=bias, n_rope=nr) for nseg, K0 in kcs]
            continue
        for ni, N in enumerate(GEMM_N):
            for ki, (nseg, K0) in enumerate(K_CONFIGS):
                out.append(gemm_case(epi, M, N, nseg, K0, out_nseg=2 + (ni + ki) % 2))
    return out
