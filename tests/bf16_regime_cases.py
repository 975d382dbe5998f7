"""CPU-only pieces shared by test_bf16_regime_host.py and test_bf16_regime_gpu.py: what the bf16 regime (fp32_planes = 0,
layer_bf16 in csrc/encoder.hip) and the two heads launch besides the attention - the RMSNorm with its gather and pending
residual, the bf16 GEMM with each of its epilogues, the dense head's pool, the sparse head's finish and the packing plan - as
seeded cases, numpy restatements of the format arithmetic, float64 references, and the element-wise error bound of every kernel.

Every bound is derived here from the operation count, never fitted and never computed from what a kernel returns.  e = 2^-24 is
the unit roundoff of fp32 (round to nearest even); hipcc's default keeps fp32 division and square root correctly rounded and fp32
denormals alive.  All bounds are first order in e, like those of fp32_plane_cases.py, whose (N) (9) (10) (12) are reused.

bf16 store (B).  bf16 has 8 significand bits: its numbers around v are hs(v) = 2^(floor(log2 |v|) - 7) apart, 2^-133 in the
subnormal range, and round to nearest even moves a value by at most half of that:

    h(v) = max(2^(floor(log2 |v|) - 8), 2^-134),  h(0) = 0;      2^-9 |v| < h(v) <= 2^-8 |v| for a normal v
    |o - Y| <= h(|Y| + dy) + dy        for o = bf16(y~), |y~ - Y| <= dy                                                    (B)

h is the whole of it: a store that truncates errs by up to 2 h and leaves (B), so nothing is added to it.  (The coefficient is not
2^-9: 1 + 2^-8 lies half way between the bf16 numbers 1 and 1 + 2^-7, so correct rounding itself errs by 2^-8 |v| there;
2^-9 |v| is h at the TOP of a binade.  test_bf16_regime_host.py shows both.)

Norm (N).  x' = fl(x + delta) is ONE rounding of two exactly known inputs (delta is a bf16 number), a gathered row is a copy: the
row the kernel writes back is compared bit for bit with numpy's fp32 sum.  y = (x' rs) w, rs = 1 / sqrt(ss / H + eps), ss = the
fp32 sum of H squares in an unspecified order: as (N) of fp32_plane_cases.py

    |y~ - y| <= RN |y|,  RN = (H / 2 + 5.5) e          (fp32 output);       |o - y| <= h(|y| (1 + RN)) + RN |y|   (bf16 output)

with y in float64 FROM x' (so the check of y does not depend on how x' came about).  A zero row gives zeros exactly.

GEMM (G).  The operands are bf16 numbers, their products exact in fp32, so float64 of the sum is the truth T, and the MFMA chain adds
K terms in fp32:

    |t~ - T| <= d = K e sum_k |a w|                                                                                        (G)

Epilogues on t~ (numbers: sr_gemm_bf16's epilogue argument; 5 / 6 are sr_gemm_qkv_rope_bias with fp32_out = 0 / 1):
  store bf16 (0)   (B) with dy = d.
  residual (1)     c = fl(c0 + t~):  |c - (c0 + T)| <= d + e (|c0 + T| + d).
  store fp32 (4)   d.
  QKV (5, 6)       x = fl(t~ + bias): dx = d + e (|T + bias| + d)  (no bias: dx = d, nothing is added).  Rotation of the halves x1, x2
                   of a head, products and sum rounded separately:  a = fl(x1 c), b = fl(x2 s), y = fl(a - b):
                   ea = |c| dx1 + e (|x1 c| + |c| dx1), eb likewise, |y~ - Y| <= ea + eb + e (|Y| + ea + eb); the second half
                   x2 c + x1 s likewise; v features: dx.  fp32_out = 1 stores y~; fp32_out = 0 stores bf16(y~): (B).
  SwiGLU (2)       y~ = fl(fl(g r) u), r = rcp(fl(1 + E~)), E~ = v_exp_f32(fl(-g L)), L = fl(log2 e) - the fast path __expf /
                   __builtin_amdgcn_rcpf.  With E = exp(-G), s = silu(G) = G / (1 + E) and sg = E / (1 + E) (the sensitivity of s
                   to a relative change of E):
                     argument   fl(-g L) carries e from the product and e from L: the exponent is off by 2 e |g| log2 e, that
                                is 2 e |g| relative in E;
                     v_exp_f32  1 ulp (AMD's CDNA ISA reference: "v_exp_f32 ... 1 ULP accuracy"), <= 2 e relative in E;
                     sum        e;   v_rcp_f32  1 ulp ("v_rcp_f32 ... 1 ULP accuracy"), <= 2 e;   product g r  e:
                   rel_s = ((2 (|G| + dg) + 2) sg + 4) e,   es = 1.1 dg + rel_s (|s| + 1.1 dg) + 2^-119     (|silu'| <= 1.1)
                   The floor: v_exp_f32 and v_rcp_f32 flush denormal results to zero.  E~ < 2^-126 -> 0 changes nothing
                   (1 + E rounds to 1 either way).  For g < -87.3, 1 + E >= 2^126 and r < 2^-126 may come back as 0 (below -88.7
                   E~ is inf and r IS 0): the kernel returns -0 where |s| <= 89 x 2^-126 < 2^-119.
                   ep = es (|U| + du) + |s| du,   |y~ - Y| <= ey = ep + e (|Y| + ep) + 2^-149,   then (B) with dy = ey.
  max (3)          out[q, n] = max(+0, max over the rows m of sequence q of t~[m, n]).  With w the true winner, a row can win in
                   the kernel only if T[m] + d[m] >= T[w] - d[w]; the bound is the largest d among those rows.  A column whose rows
                   all have T + d < 0 gives exactly +0.  Rows with seq_of = -2 take no part.

Dense head (P).  Per token rs as in (N): relative (H / 2 + 3.5) e.  y = (x rs) w: RN.  s2 = fp32 sum of y^2: 2 RN from y, e per
square, (H - 1) e from the sum: (2 RN + H) e; inv = 1 / max(sqrt(s2), 1e-12): half of that + e + e = (H + 7.5) e.  A term is three
products, ((x rs) w) inv: RT = (H / 2 + 3.5) + (H + 7.5) + 3 = (1.5 H + 14) e relative.  cnt terms are added in token order,
(cnt - 1) e sum |term|, and the mean's division adds e:

    |out - mean| <= (RT + (cnt - 1) e) sum |term| / cnt + e |mean|                                                          (P)

A sequence without a pooled token (cnt = 0) gives exactly +0.

Sparse finish (F).  out = logf(fl(max(fl(vb sc), 0) + 1)), vb = bf16(v) when asked (restated exactly).  With m = vb sc: the product's
rounding moves log(1 + m) by e m / (1 + m), the sum's by e; logf is within 1 ulp (HIP math API: logf, maximum error 1 ULP),
<= 2 e relative.  (hipcc's expansion of logf missed that - 1.99 ulps on MI355X - and the kernel now takes the logarithm in double;
the bound is the documented one and stays.)

    |out - log(1 + m)| <= 2 e log(1 + m) + e (1 + m / (1 + m))          m <= 0: exactly +0                                  (F)

Plan.  Integers: every array is compared bit for bit with plan_reference(), a plain restatement of the comments above
plan_rows_kernel / plan_tokens_kernel in csrc/encoder_kernels.hip."""
import functools

import numpy as np

import fp32_plane_cases as P

E = P.E
F32 = np.float32
EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_SEGMAX, EPI_STORE_F32, EPI_QKV, EPI_QKV_F32 = 0, 1, 2, 3, 4, 5, 6
EPILOGUES = {"store": EPI_STORE, "resid": EPI_RESID, "swiglu": EPI_SWIGLU, "segmax": EPI_SEGMAX, "store_f32": EPI_STORE_F32,
             "qkv": EPI_QKV, "qkv_f32": EPI_QKV_F32}
BF16_OUT = {EPI_STORE, EPI_SWIGLU, EPI_QKV}
STAGED_4W = {EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_STORE_F32, EPI_QKV}    # EpiTraits::STAGED_4W of csrc/gemm_bf16.hip
MAX_POS = P.MAX_POS

GEMM_M = [1, 17, 33, 65, 200, 300]
GEMM_N = [128, 320]
GEMM_K = [192, 256, 320, 768]           # 3, 4, 5, 12 k-steps of 64: below the pipelined loops, their minimum, odd, longer
LONG_K = (65, 128, 2048)                # + one long chain (M, N, K)


# ------------------------------------------------------------------------------------------ format arithmetic
def bf16_round(x):
    """fp32 -> the nearest bf16 number (ties to even) as fp32: the bit arithmetic of oracle/llama_bi.py:bf16_round."""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(np.uint32)
    r = ((u >> 16) & np.uint32(1)) + np.uint32(0x7FFF)
    y = ((u + r) & np.uint32(0xFFFF0000)).view(F32)
    return np.where(np.isnan(x), x, y)


def bf16_trunc(x):
    """The defect: the low 16 bits dropped."""
    x = np.ascontiguousarray(x, dtype=F32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def bf16_bits(x):
    """fp32 holding bf16 numbers -> their 16-bit words."""
    x = np.ascontiguousarray(x, dtype=F32)
    assert not (x.view(np.uint32) & np.uint32(0xFFFF)).any()
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def bf16_value(bits):
    """16-bit bf16 words -> fp32."""
    return (np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << 16).view(F32)


def half_spacing(v):
    """h(v) of (B), float64."""
    v = np.abs(np.asarray(v, np.float64))
    _, ex = np.frexp(v)                         # v = m 2^ex, m in [0.5, 1): floor(log2 v) = ex - 1
    return np.where(v == 0, 0.0, np.maximum(np.ldexp(1.0, ex - 9), 2.0 ** -134))      # an exact zero stays zero


def store_bound(Y, dy):
    return half_spacing(np.abs(Y) + dy) + dy


# ------------------------------------------------------------------------------------------ RMSNorm
NORM_H = [64, 320, 256, 512, 1024, 2048, 3072, 4096]        # rmsnorm_kernel<0> twice (H % 256 != 0), then <1> <2> <4> <8> <12> <16>
NORM_T = [1, 3, 4, 5, 9]                                     # a workgroup holds four rows
NORM_NCH = {64: 0, 320: 0, 256: 1, 512: 2, 1024: 4, 2048: 8, 3072: 12, 4096: 16}
VOCAB = 23
# what the encoder launches (launch_rmsnorm's call sites in csrc/encoder.hip: layer_bf16, model_forward, head_sparse, sr_model_last_hidden), + gather and residual together with both outputs
NORM_COMBOS = {
    "first_layer": dict(gather=True, delta=False, w=True, xn=True, f32=False),       # embedding gather + input_layernorm
    "layer": dict(gather=False, delta=True, w=True, xn=True, f32=False),             # pending residual + norm
    "fold": dict(gather=False, delta=True, w=False, xn=False, f32=False),            # residual add only (w == NULL)
    "head": dict(gather=False, delta=False, w=True, xn=True, f32=False),             # final norm of the sparse head
    "last_hidden": dict(gather=False, delta=False, w=True, xn=False, f32=True),      # sr_model_last_hidden
    "gather_delta": dict(gather=True, delta=True, w=True, xn=True, f32=True),
}


@functools.lru_cache(maxsize=None)
def norm_case(H, T, seed=0):
    """Rows [T, H] fp32 whose first rows are the edges (as many as T has room for), a pending residual in bf16, a norm weight, an
    embedding table with token ids out of order.  eps_row: mean(x^2) comparable with eps; zero: all zero (signs mixed); cancel:
    delta cancels x to a few ulps of x."""
    rng = np.random.default_rng(7000 * H + 10 * T + seed)
    eps = 1e-5
    x = (rng.standard_normal((T, H)) * np.exp(rng.uniform(-4, 4, (T, 1)))).astype(F32)
    delta = bf16_round((rng.standard_normal((T, H)) * np.exp(rng.uniform(-4, 2, (T, 1)))).astype(F32))
    edges = []
    e0 = (rng.standard_normal(H) * np.sqrt(eps)).astype(F32)
    edges.append(("eps_row", e0, bf16_round(e0 * F32(0.25))))
    z = np.zeros(H, F32); z[1::2] = -0.0                                                    # noqa: E702
    edges.append(("zero", z, np.zeros(H, F32)))
    dc = bf16_round(rng.standard_normal(H).astype(F32))
    xc = (-dc * (F32(1) + rng.integers(-3, 4, H).astype(F32) * F32(2.0 ** -23))).astype(F32)
    edges.append(("cancel", xc, dc))
    order = [0, 2, 1] if T >= 3 else [0]
    names = []
    for r, i in enumerate(order[:T]):
        x[r], delta[r] = edges[i][1], edges[i][2]
        names.append(edges[i][0])
    w = rng.uniform(0.5, 1.5, H).astype(F32)
    embed = (rng.standard_normal((VOCAB, H)) * np.exp(rng.uniform(-2, 2, (VOCAB, 1)))).astype(F32)
    embed[5] = e0
    tok = rng.permutation(VOCAB)[:T].astype(np.int32)
    if T >= 3:
        tok[1] = 5
    return dict(H=H, T=T, x=x, delta=delta, w=w, embed=embed, tok=tok, eps=eps, edge_names=names)


def norm_inputs(c, combo):
    """(source rows, delta or None, the row x' the kernel must leave in x - bit for bit) of a case under a combination."""
    k = NORM_COMBOS[combo]
    src = c["embed"][c["tok"]] if k["gather"] else c["x"]
    d = c["delta"] if k["delta"] else None
    xw = src if d is None else (src + d).astype(F32)            # one rounding
    return src, d, xw


def norm_reference(xw, w, eps):
    """float64 RMSNorm of the fp32 rows x' and RN."""
    return P.norm_reference(xw, w, eps)


def norm_ideal(src, delta, w, eps, defect=None, x_before=None):
    """The kernel in numpy fp32, every operation rounded once -> (x after the call, y fp32, y bf16 as fp32).  x_before: what x held
    (it differs from src under a gather; only the defect that leaves x alone needs it)."""
    src = np.asarray(src, F32)
    if delta is None:
        xw = src.copy()
    elif defect == "delta_after_bf16":             # the residual added to the bf16-rounded row
        xw = (bf16_round(src) + delta).astype(F32)
    else:
        xw = (src + delta).astype(F32)
    H = src.shape[1]
    ss = (xw * xw).sum(axis=1, dtype=F32)
    if defect == "eps_outside_root":
        with np.errstate(divide="ignore"):
            rs = (F32(1) / np.sqrt(ss / F32(H), dtype=F32) + F32(eps)).astype(F32)
        rs = np.where(np.isfinite(rs), rs, F32(0)).astype(F32)
    else:
        rs = (F32(1) / np.sqrt(ss / F32(H) + F32(eps), dtype=F32)).astype(F32)
    xr = (xw * rs[:, None]).astype(F32)
    if defect == "weight_on_bf16_row":
        xr = bf16_round(xr)
    y = (xr * np.asarray(w, F32)).astype(F32)
    back = (src if x_before is None else x_before).copy() if defect == "x_not_written_back" else xw
    return back, y, bf16_round(y)


def check_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return [f"{name}: {got.dtype}{got.shape} != {want.dtype}{want.shape}"]
    v = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    ne = got.view(v) != want.view(v)
    if ne.any():
        i = tuple(int(k) for k in np.argwhere(ne)[0])
        return [f"{name}: {int(ne.sum())} elements differ, e.g. {i}: {got[i]!r} != {want[i]!r}"]
    return []


def _outside(name, val, ref, bound):
    err = np.abs(np.asarray(val, np.float64) - ref)
    with np.errstate(invalid="ignore"):
        bad = ~(err <= bound)
    if not bad.any():
        return []
    i = np.unravel_index(np.argmax(np.where(bad, err - bound, -np.inf)), err.shape)
    return [f"{name}: {int(bad.sum())} elements outside the bound, e.g. {tuple(int(k) for k in i)}: "
            f"|{float(val[i]):.9g} - {ref[i]:.9g}| = {err[i]:.3g} > {bound[i]:.3g}"]


def ratio(val, ref, bound):
    """Worst error as a fraction of the bound (information only)."""
    err = np.abs(np.asarray(val, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(q.max()) if q.size else 0.0


def check_norm(c, combo, x_after, xn=None, xn_f32=None):
    """Failure strings of one rmsnorm launch: x after the call bit for bit, the outputs within (N) / (N) + (B)."""
    k = NORM_COMBOS[combo]
    _, _, xw = norm_inputs(c, combo)
    bad = check_bits("x after the call", x_after, xw)
    if not k["w"]:
        return bad
    y, rn = norm_reference(xw, c["w"], c["eps"])
    if k["f32"]:
        bad += _outside("xn_f32", xn_f32, y, rn * np.abs(y))
    if k["xn"]:
        bad += _outside("xn", xn, y, store_bound(y, rn * np.abs(y)))
    return bad


def norm_ratio(c, combo, xn=None, xn_f32=None):
    k = NORM_COMBOS[combo]
    if not k["w"]:
        return 0.0
    y, rn = norm_reference(norm_inputs(c, combo)[2], c["w"], c["eps"])
    r = 0.0
    if k["f32"]:
        r = max(r, ratio(xn_f32, y, rn * np.abs(y)))
    if k["xn"]:
        r = max(r, ratio(xn, y, store_bound(y, rn * np.abs(y))))
    return r


# ------------------------------------------------------------------------------------------ GEMM cases
@functools.lru_cache(maxsize=None)
def gemm_case(epi, M, N, K, seed=0, hd=64, bias=True, n_rope=None):
    """One bf16 GEMM problem as numpy arrays: A [M, K], W [N, K] fp32 holding bf16 numbers.  Rows carry distinct magnitudes (over
    e^+-3) and positions are shuffled, so that a wrong row offset of pos / seq_of / C changes the result."""
    rng = np.random.default_rng([epi % 5 if epi in (EPI_QKV, EPI_QKV_F32) else epi, M, N, K, seed, hd])
    a = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(F32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K) * np.exp(rng.uniform(-3, 3, (N, 1)))).astype(F32)
    c = dict(epi=epi, M=M, N=N, K=K)
    if epi == EPI_SEGMAX:
        # column 0 of the activations is large and positive in every row, feature 5 of W points against it: an all-negative column
        a[:, 0] = np.abs(a).max(axis=1) * 2
        w[5] = 0
        w[5, 0] = -1.0
        c["seq_of"], c["n_seq"] = P.seq_ids(M)
        a[c["seq_of"] == -2] *= 64.0              # masked rows carry the largest values
    a = bf16_round(a)
    if epi == EPI_SWIGLU:
        # large |g| of both signs: gate rows along / against activation row 0, scaled so that |g| reaches ~100 (__expf(-g) overflows
        # below -88.7) and ~30
        I = N // 2
        wg, wu = w[:I].copy(), w[I:].copy()
        dirn = a[0] / np.linalg.norm(a[0]) ** 2
        wg[1], wg[2] = (100.0 * dirn).astype(F32), (-100.0 * dirn).astype(F32)
        wg[3], wg[4] = (30.0 * dirn).astype(F32), (-30.0 * dirn).astype(F32)
        w = P.interleave_gate_up(wg, wu)
    c["A"], c["W"] = a, bf16_round(w)
    if epi == EPI_RESID:
        c["C0"] = (rng.standard_normal((M, N)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(F32)
    if epi in (EPI_QKV, EPI_QKV_F32):
        c["hd"], c["n_rope"] = hd, (N - hd if n_rope is None else n_rope)
        c["cos"], c["sin"] = P.rope_tables(hd)
        c["pos"] = rng.permutation(MAX_POS)[:M].astype(np.int32)
        # the bf16 regime hands the epilogue the bf16 roundings of the checkpoint's bias, held as fp32 (LayerW::bqkv_r)
        c["bias"] = bf16_round((rng.standard_normal(N) * np.abs(w).max(axis=1) * np.sqrt(K)).astype(F32)) if bias else None
    return c


def _products(c):
    """(T, d) of (G), [M, N] float64."""
    A, W = c["A"].astype(np.float64), c["W"].astype(np.float64)
    return A @ W.T, c["K"] * E * (np.abs(A) @ np.abs(W).T)


def _swiglu_ref(T, d):
    G, U = P._deinterleave(T)
    dg, du = P._deinterleave(d)
    s = P._silu(G)
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(G))                     # E / (1 + E), E = exp(-G)
    rel = ((2 * (np.abs(G) + dg) + 2) * sg + 4) * E
    es = 1.1 * dg + rel * (np.abs(s) + 1.1 * dg) + 2.0 ** -119
    ep = es * (np.abs(U) + du) + np.abs(s) * du
    Y = s * U
    return Y, ep + E * (np.abs(Y) + ep) + 2.0 ** -149


def _qkv_ref(c, T, d):
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


_REFS = {}


def gemm_reference(c):
    """(ref, bound[, must_be_zero]) in float64, shaped like the output; computed once per case."""
    if id(c) not in _REFS:
        while len(_REFS) >= 4:
            _REFS.pop(next(iter(_REFS)))
        _REFS[id(c)] = (c, _gemm_reference(c))        # holds c, so that its id stays its own
    return _REFS[id(c)][1]


def _gemm_reference(c):
    epi = c["epi"]
    T, d = _products(c)
    if epi == EPI_STORE:
        return T, store_bound(T, d)
    if epi == EPI_STORE_F32:
        return T, d
    if epi == EPI_RESID:
        ref = c["C0"].astype(np.float64) + T
        return ref, d + E * (np.abs(ref) + d)
    if epi in (EPI_QKV, EPI_QKV_F32):
        ref, b = _qkv_ref(c, T, d)
        return (ref, b) if epi == EPI_QKV_F32 else (ref, store_bound(ref, b))
    if epi == EPI_SWIGLU:
        Y, ey = _swiglu_ref(T, d)
        return Y, store_bound(Y, ey)
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
        ref[q], bound[q] = np.maximum(top, 0.0), np.where(can_win, dq, 0).max(axis=0)
        zero[q] = (Tq + dq < 0).all(axis=0)
    return ref, bound, zero


def out_shape(c):
    if c["epi"] == EPI_SEGMAX:
        return (c["n_seq"], c["N"])
    return (c["M"], c["N"] // 2 if c["epi"] == EPI_SWIGLU else c["N"])


def check_gemm(c, out):
    """Failure strings of an output (fp32 values; bf16 outputs decoded with bf16_value) against the reference and its bound."""
    r = gemm_reference(c)
    ref, bound = r[0], r[1]
    out = np.asarray(out, F32)
    if out.shape != ref.shape:
        return [f"shape {out.shape} != {ref.shape}"]
    bad = _outside("C", out, ref, bound)
    if c["epi"] == EPI_SEGMAX and not np.all(out.view(np.uint32)[r[2]] == 0):
        bad.append("a column without a positive maximum is not exactly +0")
    return bad


def worst_ratio(c, out):
    r = gemm_reference(c)
    return ratio(np.asarray(out, F32), r[0], r[1])


# ------------------------------------------------------------------------------------------ GEMM: ideal arithmetic and defects
GEMM_DEFECTS = {
    "store_truncates": (EPI_STORE, EPI_SWIGLU, EPI_QKV),
    "last_k_step_dropped": (EPI_STORE, EPI_RESID, EPI_SWIGLU, EPI_SEGMAX, EPI_STORE_F32, EPI_QKV, EPI_QKV_F32),
    "bias_after_rotation": (EPI_QKV, EPI_QKV_F32),
    "rotation_by_neighbour_row": (EPI_QKV, EPI_QKV_F32),
    "rotation_reaches_v": (EPI_QKV, EPI_QKV_F32),
    "rotation_misses_last_k_head": (EPI_QKV, EPI_QKV_F32),
    "silu_sign": (EPI_SWIGLU,),                       # g / (1 + exp(g))
    "masked_row_in_max": (EPI_SEGMAX,),
    "max_not_clamped": (EPI_SEGMAX,),
}
LOG2E = F32(1.4426950408889634)


def fast_silu(g):
    """g rcp(1 + __expf(-g)) with ideally rounded pieces: the argument product, exp2, sum, reciprocal and product each rounded to
    fp32 once, denormal results of exp2 and of the reciprocal flushed to zero as the hardware instructions do."""
    g = np.asarray(g, F32)
    tiny = np.finfo(F32).tiny
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        ex = np.exp2((-g * LOG2E).astype(F32).astype(np.float64)).astype(F32)
        ex = np.where(ex < tiny, F32(0), ex)
        r = (F32(1) / (F32(1) + ex).astype(F32)).astype(F32)
        r = np.where(np.abs(r) < tiny, F32(0), r)
    return (g * r).astype(F32)


def gemm_ideal(c, defect=None):
    """float64 products rounded to fp32 once, then the kernel's epilogue in numpy fp32 - every operation rounded once; optionally with
    one defect of GEMM_DEFECTS.  bf16 outputs come back as the fp32 values of the bf16 numbers."""
    epi = c["epi"]
    assert defect is None or epi in GEMM_DEFECTS[defect]
    A, W = c["A"].astype(np.float64), c["W"].astype(np.float64)
    if defect == "last_k_step_dropped":
        A, W = A[:, :-64], W[:, :-64]
    t = (A @ W.T).astype(F32)
    store = bf16_trunc if defect == "store_truncates" else bf16_round
    if epi == EPI_STORE:
        return store(t)
    if epi == EPI_STORE_F32:
        return t
    if epi == EPI_RESID:
        return (c["C0"] + t).astype(F32)
    if epi in (EPI_QKV, EPI_QKV_F32):
        pos = np.roll(c["pos"], 1) if defect == "rotation_by_neighbour_row" else c["pos"]
        x = t if c["bias"] is None or defect == "bias_after_rotation" else (t + c["bias"]).astype(F32)
        out = x.copy()
        hd, h2 = c["hd"], c["hd"] // 2
        nr = c["n_rope"] + (hd if defect == "rotation_reaches_v" else 0) - (hd if defect == "rotation_misses_last_k_head" else 0)
        cs, sn = c["cos"][pos], c["sin"][pos]
        for h0 in range(0, nr, hd):
            x1, x2 = x[:, h0:h0 + h2], x[:, h0 + h2:h0 + hd]
            out[:, h0:h0 + h2] = (x1 * cs).astype(F32) - (x2 * sn).astype(F32)
            out[:, h0 + h2:h0 + hd] = (x2 * cs).astype(F32) + (x1 * sn).astype(F32)
        if defect == "bias_after_rotation" and c["bias"] is not None:
            out = (out + c["bias"]).astype(F32)
        return out if epi == EPI_QKV_F32 else store(out)
    if epi == EPI_SWIGLU:
        g, u = P._deinterleave(t)
        if defect == "silu_sign":
            with np.errstate(over="ignore"):
                s = (g / (F32(1) + np.exp(g, dtype=F32))).astype(F32)
        else:
            s = fast_silu(g)
        return store((s * u).astype(F32))
    ids = c["seq_of"].copy()
    if defect == "masked_row_in_max":
        for m in range(1, len(ids)):
            if ids[m] == -2:
                ids[m] = ids[m - 1]
    out = np.zeros((c["n_seq"], c["N"]), F32)
    for q in range(c["n_seq"]):
        rows = np.flatnonzero(ids == q)
        if len(rows):
            out[q] = t[rows].max(axis=0) if defect == "max_not_clamped" else np.maximum(t[rows].max(axis=0), F32(0))
    return out


QKV_VARIANTS = [  # (head_dim, N, n_rope, bias, K list): n_rope a multiple of 128 and not, v features behind it
    (64, 128, 64, True, GEMM_K), (64, 320, 256, False, GEMM_K), (64, 320, 192, True, GEMM_K),
    (128, 256, 128, False, GEMM_K[::2]), (128, 384, 256, True, GEMM_K[1::2]),
]


def epilogue_cases(epi, Ms=None):
    """Every problem test_bf16_regime_gpu.py runs for an epilogue (test_bf16_regime_host.py walks the same list)."""
    out = []
    for M in (GEMM_M if Ms is None else Ms):
        if epi in (EPI_QKV, EPI_QKV_F32):
            for hd, N, nr, bias, ks in QKV_VARIANTS:
                out += [gemm_case(epi, M, N, K, hd=hd, bias=bias, n_rope=nr) for K in ks]
        else:
            out += [gemm_case(epi, M, N, K) for N in GEMM_N for K in GEMM_K]
        if M == LONG_K[0]:
            out.append(gemm_case(epi, M, LONG_K[1], LONG_K[2], n_rope=64) if epi in (EPI_QKV, EPI_QKV_F32) else gemm_case(epi, M, LONG_K[1], LONG_K[2]))
    return out


# ------------------------------------------------------------------------------------------ dense head
HEAD_H = [64, 320, 2048]
HEAD_LAYOUTS = {      # name -> per sequence (span start, tokens, pool_start, row_shift); span start / pool_start in unshifted columns
    "one_of_70": [(3, 70, 3, 0)],                                 # B = 1, pooled from the start of the span
    "one_of_1": [(9, 1, 9, 0)],
    "one_empty": [(0, 0, 0, 0)],                                  # T = 0: zeros without a launch
    "three": [(5, 2, 6, 0), (0, 0, 0, 0), (2, 70, 30, 0)],        # pool_start inside the span; a sequence of 0 tokens between others
    "three_shifted": [(12, 1, 12, 4), (7, 70, 7, 7), (20, 2, 25, 3)],   # row_shift; the last sequence pools nothing (count 0)
    "right_padded": [(0, 70, 0, 0), (0, 2, 0, 0), (0, 1, 0, 0)],  # pool_start at 0: pad positions behind the keys are pooled, by design
}


@functools.lru_cache(maxsize=None)
def head_case(H, layout, seed=0):
    rng = np.random.default_rng([H, sorted(HEAD_LAYOUTS).index(layout), seed])
    seqs = HEAD_LAYOUTS[layout]
    cu = np.concatenate([[0], np.cumsum([n for _, n, _, _ in seqs])]).astype(np.int32)
    T = int(cu[-1])
    pos = np.concatenate([np.arange(st, st + n) - sh for st, n, _, sh in seqs] + [np.zeros(0, int)]).astype(np.int32)
    ps = np.array([p - sh for _, _, p, sh in seqs], np.int32)
    x = (rng.standard_normal((T, H)) * np.exp(rng.uniform(-3, 3, (T, 1)))).astype(F32)
    w = rng.uniform(0.5, 1.5, H).astype(F32)
    return dict(H=H, B=len(seqs), T=T, cu=cu, pos=pos, pool_start=ps, x=x, w=w, eps=1e-5, span_len=np.diff(cu))


def head_reference(c):
    """(mean [B, H], bound [B, H], must_be_zero [B]) of (P)."""
    H, B = c["H"], c["B"]
    ref, bound, zero = np.zeros((B, H)), np.zeros((B, H)), np.zeros(B, bool)
    if c["T"]:
        y, _ = P.norm_reference(c["x"], c["w"], c["eps"])
        term = y / np.maximum(np.sqrt((y * y).sum(axis=1, keepdims=True)), float(F32(1e-12)))
    rt = (1.5 * H + 14) * E
    for b in range(B):
        t = np.arange(c["cu"][b], c["cu"][b + 1])
        t = t[c["pos"][t] >= c["pool_start"][b]]
        if not len(t):
            zero[b] = True
            continue
        sa = np.abs(term[t]).sum(axis=0)
        ref[b] = term[t].sum(axis=0) / len(t)
        bound[b] = (rt + (len(t) - 1) * E) * sa / len(t) + E * np.abs(ref[b])
    return ref, bound, zero


def head_ideal(c, defect=None):
    """The two kernels in numpy fp32 (numpy's own summation order inside a row; token order across rows)."""
    H, B = c["H"], c["B"]
    out = np.zeros((B, H), F32)
    if not c["T"]:
        return out
    x, w = c["x"], c["w"]
    rs = (F32(1) / np.sqrt((x * x).sum(axis=1, dtype=F32) / F32(H) + F32(c["eps"]), dtype=F32)).astype(F32)
    y = ((x * rs[:, None]).astype(F32) * w).astype(F32)
    inv = (F32(1) / np.maximum(np.sqrt((y * y).sum(axis=1, dtype=F32), dtype=F32), F32(1e-12))).astype(F32)
    for b in range(B):
        t0, t1 = c["cu"][b], c["cu"][b + 1]
        acc, cnt = np.zeros(H, F32), 0
        for t in range(t0, t1):
            if c["pos"][t] < c["pool_start"][b] and defect != "pool_before_start":
                continue
            acc = (acc + (y[t] * inv[t]).astype(F32)).astype(F32)
            cnt += 1
        n = (t1 - t0) if defect == "pool_by_span_len" else cnt
        out[b] = (acc / F32(n)).astype(F32) if cnt and n else F32(0)
    return out


def check_head(c, out):
    ref, bound, zero = head_reference(c)
    out = np.asarray(out, F32)
    if out.shape != ref.shape:
        return [f"shape {out.shape} != {ref.shape}"]
    bad = _outside("out", out, ref, bound)
    if not np.all(out.view(np.uint32)[zero] == 0):
        bad.append("a sequence without a pooled token is not exactly +0")
    return bad


# ------------------------------------------------------------------------------------------ sparse finish
FINISH_N = [1, 255, 257, 1000]


@functools.lru_cache(maxsize=None)
def finish_case(n, seed=0):
    """Maxima as EPI_SEGMAX leaves them (>= +0) over e^+-12, with the edges first: +0, -0, a negative value (the hook takes any
    float), values whose 1 + m rounds to 1, a bf16 tie, a large one."""
    rng = np.random.default_rng([n, seed])
    v = np.exp(rng.uniform(-12, 12, n)).astype(F32)
    edges = np.array([0.0, -0.0, -3.5, 2.0 ** -30, 1.0 + 2.0 ** -8, 3.0e4, 1.0 + 3 * 2.0 ** -8], F32)
    k = min(n, len(edges))
    v[:k] = np.roll(edges, -(n % 3))[:k] if n > 1 else edges[4:5]
    return dict(n=n, v=v, scale=F32(2048.0 ** -0.25))


def finish_reference(c, round_bf16):
    vb = bf16_round(c["v"]) if round_bf16 else c["v"]
    m = np.maximum(vb.astype(np.float64) * float(c["scale"]), 0.0)
    ref = np.log1p(m)
    return ref, 2 * E * ref + E * (1 + m / (1 + m)), m <= 0


def finish_ideal(c, round_bf16, defect=None):
    v = c["v"]
    if round_bf16 and defect != "no_bf16_rounding":
        v = bf16_round(v)
    if defect == "log_before_scale":
        return (np.log1p(np.maximum(v, F32(0)).astype(np.float64)).astype(F32) * c["scale"]).astype(F32)
    s = (np.maximum((v * c["scale"]).astype(F32), F32(0)) + F32(1)).astype(F32)
    return np.log(s.astype(np.float64)).astype(F32)


def check_finish(c, round_bf16, out):
    ref, bound, zero = finish_reference(c, round_bf16)
    out = np.asarray(out, F32)
    bad = _outside("out", out, ref, bound)
    if not np.all(out.view(np.uint32)[zero] == 0):
        bad.append("a value <= 0 does not give exactly +0")
    return bad


# ------------------------------------------------------------------------------------------ plan
PLAN_L = [1, 63, 64, 65, 130]
PLAN_B = [1, 5, 257]                     # 257: more rows than the scan's 256 partitions
PLAN_VOCAB = 1000
PLAN_KINDS = ["left", "right", "holes", "zero_rows"]


@functools.lru_cache(maxsize=None)
def plan_case(B, L, kind, shift, seed=0):
    """ids / mask [B, L] int64 (+ row_shift [B] int32 or None).  left / right: padded on that side with lengths 1 .. L; holes: random
    masks; zero_rows: left-padded with the first, the last and a middle row all zero.  ids reach below 0 and beyond the vocabulary.
    row_shift: up to a few columns, in row 0 beyond the span start."""
    rng = np.random.default_rng([B, L, PLAN_KINDS.index(kind), int(shift), seed])
    ids = rng.integers(-5, PLAN_VOCAB + 5, (B, L)).astype(np.int64)
    ids[0, 0], ids[-1, -1] = -7, PLAN_VOCAB
    lens = rng.integers(1, L + 1, B)
    lens[0] = L if kind != "left" else max(1, L // 2)
    col = np.arange(L)[None, :]
    if kind in ("left", "zero_rows"):
        mask = col >= (L - lens)[:, None]
    elif kind == "right":
        mask = col < lens[:, None]
    else:
        mask = rng.random((B, L)) < 0.6
        mask[0] = True
        if L > 2:
            mask[0, 1] = False
    mask = mask.astype(np.int64) * rng.integers(1, 3, (B, L))         # any nonzero value is a key
    if kind == "zero_rows":
        mask[[0, B // 2, B - 1]] = 0
    rs = None
    if shift:
        first = np.where(mask.any(axis=1), (mask != 0).argmax(axis=1), 0)
        rs = np.minimum(first, rng.integers(0, 4, B)).astype(np.int32)
        rs[0] = first[0] + 3                                           # beyond the span start: positions stay at 0
    return dict(B=B, L=L, kind=kind, ids=ids, mask=mask, row_shift=rs, vocab=PLAN_VOCAB)


def plan_reference(c, mode, defect=None):
    """The comments above plan_rows_kernel / plan_tokens_kernel, row by row.
    mode 0 (dense) and 2 (both): span = [min(first1, L - len), L), pool_start = L - len; mode 1 (sparse): span = [first1, last1 + 1),
    pool_start = first1; a row without a key: empty span, pool_start 0.  pool_start and the positions are counted row_shift[b]
    columns further left, positions never below 0.  Token ids are clamped into [0, vocab).  seq_of = b, or -2 for a masked
    position inside the span unless mode is 0."""
    B, L, ids, mask, rs = c["B"], c["L"], c["ids"], c["mask"], c["row_shift"]
    i32 = np.int32
    st, ln, ps, rl = (np.zeros(B, i32) for _ in range(4))
    tok, pos, kv, sq = [], [], [], []
    for b in range(B):
        keys = np.flatnonzero(mask[b])
        sh = 0 if rs is None else int(rs[b])
        rl[b] = len(keys)
        if len(keys):
            if mode != 1:
                p = L - len(keys)
                st[b] = min(keys[0], p)
                ln[b] = L - st[b]
            else:
                p = keys[0]
                st[b], ln[b] = keys[0], keys[-1] + 1 - keys[0]
            ps[b] = p - sh
        else:
            ps[b] = -sh
        cols = np.arange(st[b], st[b] + ln[b])
        tok.append(np.clip(ids[b, cols], 0, c["vocab"] - 1))
        pos.append(np.maximum(cols - sh, 0))
        valid = mask[b, cols] != 0
        kv.append(valid)
        sq.append(np.where((mode != 0) & ~valid, -2, b))
    cu = np.concatenate([[0], np.cumsum(ln)]).astype(i32)
    cat = lambda parts, dt: np.concatenate(parts + [np.zeros(0, dt)]).astype(dt)      # noqa: E731
    return dict(span_start=st, span_len=ln, pool_start=ps, row_len=rl, cu=cu, tok_id=cat(tok, i32), pos=cat(pos, i32),
                key_valid=cat(kv, np.uint8), seq_of=cat(sq, i32))


def check_plan(c, mode, got):
    ref = plan_reference(c, mode)
    bad = []
    for k, want in ref.items():
        bad += check_bits(k, got[k][:len(want)], want)
    return bad
