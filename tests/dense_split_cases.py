"""CPU-only pieces shared by test_dense_split_host.py and test_dense_split_gpu.py: the split-bf16 score modes of the dense search
(SR_PRECISION_BF16X3 / _BF16X6: split_bf16_kernel + dense_split_kernel<false, false>, csrc/dense_split.hip) as seeded cases, a numpy
restatement of the plane split, float64 references and the per-pair error bounds.

Every bound is derived here from the operation count and the number formats, never fitted and never computed from what a kernel
returns.  e = 2^-24 is the unit roundoff of fp32, f = 2^-134 half of bf16's smallest subnormal 2^-133 (bf16 has the exponent range of
fp32 and 8 significand bits).  All roundings are to nearest even.

Plane split (S).  For a finite fp32 v

    p0 = bf16(v),  r1 = fl(v - p0),  p1 = bf16(r1),  r2 = fl(r1 - p1),  p2 = bf16(r2);     rho1 = |r1|, rho2 = |r2|, rho3 = |r2 - p2|

with one exception at the very top: bf16(v) is infinite for |v| >= 0x7F7F8000 = (2 - 2^-8) 2^127, and there p0 is the largest finite
bf16 number P = (2 - 2^-7) 2^127 of v's sign (saturation; without it r1 = -inf and every score of the row is NaN).

  Both subtractions are exact in fp32.  Let E = floor(log2 |v|) >= -126.  v is a multiple of u = 2^(E - 23) and p0 a multiple of
  2^(E - 7) (also when it rounds up to 2^(E + 1)), so v - p0 is a multiple of u with |v - p0| <= 2^(E - 8) = 2^15 u: it has at most
  16 significant bits and fp32 holds it.  Saturated: v - P is a multiple of 2^104 in [2^119, 2^120 - 2^104], 16 bits again.  p1 is a
  multiple of u too and |r1 - p1| <= 2^-8 |r1| <= 2^7 u: 8 bits, exact.  A subnormal v (|v| < 2^-126) and all its planes are multiples
  of 2^-149 below 2^-126, where fp32 adds exactly.
  rho1 <= max(2^-8 |v|, f): half the spacing 2^(E - 7) of bf16 at v is 2^(E - 8) <= 2^-8 |v|; below 2^-126 the spacing is 2^-133.
      Saturated: v - P <= 2^-8 v  <=>  v <= P / (1 - 2^-8) = 2^128.
  rho2 <= max(2^-17 (1 + 2^-8) |v|, f): if |r1| = 2^(E - 8) it is a power of two, a bf16 number, and rho2 = 0; otherwise
      |r1| < 2^(E - 8), its exponent is at most E - 9 and half of bf16's spacing there is 2^(E - 17) <= 2^-17 |v|.  (Not 2^-16: the
      first residual cannot sit at the bottom of its binade, where a rounding errs most.)  Saturated: r1 in [2^119, 2^120), half
      spacing 2^111 <= 2^-17 (1 + 2^-8) |v| because |v| >= (2 - 2^-8) 2^127.
  rho3 = 0 whenever v is a multiple of 2^-133, in particular for every |v| >= 2^-110 (u >= 2^-133): r2 is then a multiple of 2^-133
      with at most 8 significant bits, a bf16 number.  So three planes reproduce v EXACTLY for |v| >= 2^-110, for +-0 and for
      every bf16 number (p1 = p2 = +0).  Below 2^-110 what lies under 2^-133 is lost: a residual below f vanishes, and rho3 <= f.
  |p0| <= (1 + 2^-8) |v| + f,   |p1| <= rho1 + rho2 <= 2^-8 (1 + 2^-8) |v| + 2 f.
  Non-finite v is outside the contract of the split modes.

Tier A, the kernel (bound (G) of bf16_regime_cases.py, reused through its _products).  A mode forms the plane products
(document plane, query plane) listed in dense_pass_16bit (csrc/dense_search.hip), in this order:

    bf16x3: (d1,q0) (d0,q1) (d0,q0)              bf16x6: (d2,q0) (d0,q2) (d1,q1) (d1,q0) (d0,q1) (d0,q0)

The truth for the device is T(q, j) = sum over the pairs (b, a) and over i of Qa[q, i] Db[j, i] in float64.  Products of two bf16
numbers have 16 significant bits and are exact in fp32 as long as they are multiples of 2^-149 (every case below is built that way:
the `tiny` kind keeps its queries on a 2^-16 grid in [0.5, 2)); v_mfma_f32_16x16x32_bf16 adds the K = n_pairs H terms of a pair in
fp32 in an unspecified order, and an fp32 sum of K terms errs by at most (K - 1) e sum |terms| to first order:

    |s~ - T| <= dA = K e sum_pairs sum_i |Qa_i Db_i|,    K = n_pairs H                                                          (A)

This is the GEMM [Q planes side by side] x [D planes side by side]^T with inner dimension K, which is how tier_a() hands it to (G).
(float64 itself adds K terms with 2^-53 each: 2^-29 of dA.)  A dropped or doubled k-slice of 64, a wrong plane pairing, a plane switch
one k-step early or late, a tile that read its neighbour's rows or a fragment carried over from the previous tile moves a score by
2^-8 sum |q d| or more for at least one data kind below, tens to hundreds of dA (test_dense_split_host.py::test_kernel_defects_leave_tier_a).
What (A) cannot see is a defect below K e sum |Qa Db| itself: bf16x6 without its (d2,q0) product is 2^-17 sum |q d| off, dA at H = 64 is
2^-15.4 sum |q d|.  A worst-case bound of an fp32 sum of K terms is that wide; the kernels sit at 1 % of it.

Tier B, the arithmetic (no kernel involved).  With q = q0 + rq1, rq1 = q1 + rq2, rq2 = q2 + eq (and d likewise), per element

    bf16x3:  q d - (q0 d0 + q0 d1 + q1 d0) = q0 rd2 + rq2 d0 + rq1 rd1
    bf16x6:  q d - (q0 d0 + q0 d1 + q1 d0 + q1 d1 + q0 d2 + q2 d0) = q0 ed + eq d0 + q1 rd2 + rq2 d1 + rq2 rd2

(multiply out (q0 + q1 + rq2)(d0 + d1 + rd2) and subtract).  The residual form bounds |T - sum q d| with the ACTUAL planes and residuals:

    bf16x3:  sum_i |q0| rho2(d) + rho2(q) |d0| + rho1(q) rho1(d)
    bf16x6:  sum_i |q0| rho3(d) + rho3(q) |d0| + |q1| rho2(d) + rho2(q) |d1| + rho2(q) rho2(d)                                   (B)

and with the bounds of (S) the closed form is cB(mode) sum_i |q_i d_i| + floor:

    bf16x3:  2 (1 + 2^-8) 2^-17 (1 + 2^-8) + 2^-16                            = ((1 + 2^-8)^2 + 1) 2^-16  <=  cB = (2 + 2^-6) 2^-16
    bf16x6:  2 2^-8 (1 + 2^-8) 2^-17 (1 + 2^-8) + (2^-17 (1 + 2^-8))^2       = (1 + 2^-8)^2 (1 + 2^-10) 2^-24  <=  cB = (1 + 2^-6) 2^-24
    floor = f (1.02 sum_i (|q_i| + |d_i|) + 7 H f)

(the floor collects every product that carries an f of (S): per element at most f (1 + 2^-8 + 2^-8 (1 + 2^-8) + 2^-15 + 2^-16)
(|q| + |d|) + 7 f^2).  Not 3 x 2^-16: by (S) the second residual is at most HALF of 2^-16 |v|.  The `aligned` kind - every element
(1 + 0.998 x 2^-8) 2^k with one sign, so that the roundings of p0 and of p1 are both at their maximum and all point the same way -
reaches 1.95 x 2^-16 sum |q d| for bf16x3 and 0.97 x 2^-24 for bf16x6: the closed forms are within a few per cent of attainable.
Gaussian data at H = 256 shows about a tenth of that relative to |q| |d| (errors of both signs cancel, and sum |q d| < |q| |d|).

The documented error of a mode against the true inner product is therefore dA + cB sum_i |q_i d_i| + floor per pair:
with dA <= K e (1 + 2^-5) sum |q d| (the planes of an operand add up to at most (1 + 2^-8) (1 + 2^-8 + 2^-16) of its magnitude) that is
(2.02 x 2^-16 + 3.1 H 2^-24) sum |q d| for bf16x3 and (1.02 + 6.2 H) 2^-24 sum |q d| for bf16x6, plus the floor."""
import functools

import numpy as np

import bf16_regime_cases as G

E = G.E
F32 = np.float32
F134 = 2.0 ** -134
MODES = ("bf16x3", "bf16x6")
N_PLANES = {"bf16x3": 2, "bf16x6": 3}
# (document plane, query plane) of every product, in the order dense_pass_16bit accumulates them
PAIRS = {"bf16x3": ((1, 0), (0, 1), (0, 0)), "bf16x6": ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))}
CB = {"bf16x3": (2 + 2.0 ** -6) * 2.0 ** -16, "bf16x6": (1 + 2.0 ** -6) * 2.0 ** -24}
FITTED_TOL = {"bf16x3": 2.5e-6, "bf16x6": 4e-7}          # x |q| max_j |d_j|: what tests/test_dense_bf16x3_gpu.py asserts on Gaussian data
BF16_MAX = F32(np.array([0x7F7F0000], np.uint32).view(F32)[0])      # (2 - 2^-7) 2^127
KINDS = ("gauss", "same_sign", "aligned", "wide", "tiny", "bf16_exact", "zeros")
HOST_H = (64, 192, 1024)


# ------------------------------------------------------------------------------------------ the plane split restated
def bf16_sat(v):
    """bf16(v), round to nearest even, as fp32; a finite v whose rounding is infinite takes the largest finite bf16 of its sign."""
    v = np.ascontiguousarray(v, dtype=F32)
    p = G.bf16_round(v)
    return np.where(np.isinf(p) & np.isfinite(v), np.copysign(BF16_MAX, v), p).astype(F32)


def split_planes(v, saturate=True):
    """(p0, p1, p2) of (S) as fp32 arrays holding bf16 numbers.  saturate=False: the split without the exception at the top."""
    v = np.ascontiguousarray(v, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        p0 = bf16_sat(v) if saturate else G.bf16_round(v)
        r1 = (v - p0).astype(F32)
        p1 = G.bf16_round(r1)
        r2 = (r1 - p1).astype(F32)
        p2 = G.bf16_round(r2)
    return p0, p1, p2


def plane_words(p):
    """fp32 holding bf16 numbers (inf and NaN included) -> uint16 words."""
    return (np.ascontiguousarray(p, dtype=F32).view(np.uint32) >> 16).astype(np.uint16)


def residuals(v):
    """(rho1, rho2, rho3) of (S) in float64, from the planes."""
    p0, p1, p2 = (p.astype(np.float64) for p in split_planes(v))
    x = np.asarray(v, np.float64)
    return np.abs(x - p0), np.abs(x - p0 - p1), np.abs(x - p0 - p1 - p2)


def specials():
    """The edges of (S): +-0, fp32 subnormals, bf16 subnormals, nextafter neighbours of rounding boundaries, ties, the top binade."""
    one = F32(1)
    tie_even, tie_odd = F32(1 + 2.0 ** -8), F32(1 + 3 * 2.0 ** -8)            # -> 1 (even) and 1 + 2^-6 (even)
    top = np.array([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7FFFFE, 0x7F7FFFFF, 0x7F000000, 0x7F000001, 0x7EFFFFFF],
                   np.uint32).view(F32)
    sub = np.array([1, 2, 3, 0x7FFF, 0x8000, 0x8001, 0x18000, 0x007FFFFF, 0x00800000, 0x00800001, 0x00FF8000], np.uint32).view(F32)
    vals = [F32(0), -F32(0), one, -one, tie_even, np.nextafter(tie_even, F32(0)), np.nextafter(tie_even, F32(2)),
            tie_odd, np.nextafter(tie_odd, F32(0)), np.nextafter(tie_odd, F32(2)), F32(1 + 2.0 ** -7), F32(2 - 2.0 ** -8),
            np.nextafter(F32(2), F32(0)), F32(1 + 2.0 ** -8 + 2.0 ** -16), F32(1 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23),
            F32((1 + 0.998 * 2.0 ** -8)), F32(2.0 ** -110), np.nextafter(F32(2.0 ** -110), F32(0)), F32(2.0 ** -126),
            F32(2.0 ** -133), F32(2.0 ** -134), F32(3 * 2.0 ** -135), F32(2.0 ** -134 + 2.0 ** -149), F32(1.5 * 2.0 ** -133)]
    pos = np.concatenate([np.array(vals, F32), top, sub])
    return np.concatenate([pos, -pos]).astype(F32)


@functools.lru_cache(maxsize=None)
def split_vector(n, seed=0):
    """n fp32 values (n % 4 == 0): the specials first (as many as fit), then every data kind, then magnitudes over the whole
    exponent range."""
    assert n % 4 == 0
    rng = np.random.default_rng([n, seed])
    parts = [specials()]
    for kind in KINDS:
        q, d = case(kind, 64, 24, 8, seed)
        parts += [q.ravel(), d.ravel()]
    v = np.concatenate(parts)
    if v.size < n:
        m = n - v.size
        with np.errstate(over="ignore"):
            body = (rng.standard_normal(m) * np.exp2(rng.uniform(-149, 127, m))).astype(F32)
        body = np.where(np.isfinite(body), body, F32(1))
        top = rng.integers(0x7F000000, 0x7F800000, m // 16 + 1, dtype=np.uint32).view(F32)          # the top binade, up to FLT_MAX
        body[:: 16][: top.size] = top[: body[:: 16].size] * rng.choice(np.array([-1, 1], F32), body[:: 16].size)
        v = np.concatenate([v, body])
    v = np.ascontiguousarray(v[:n], F32)
    assert np.isfinite(v).all()
    return v


# ------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=6)
def case(kind, H, N, nq, seed=0):
    """(Q [nq, H], D [N, H]) fp32.  Rows carry distinct magnitudes, so that a score read from a neighbouring row or tile is far off."""
    rng = np.random.default_rng([KINDS.index(kind), H, N, nq, seed])
    gq = rng.standard_normal((nq, H), dtype=F32)
    gd = rng.standard_normal((N, H), dtype=F32) * F32(0.5 / np.sqrt(H))
    sq = np.exp(rng.uniform(-1, 1, (nq, 1))).astype(F32)
    sd = np.exp(rng.uniform(-1, 1, (N, 1))).astype(F32)
    if kind == "gauss":
        Q, D = gq * sq, gd * sd
    elif kind == "same_sign":
        Q, D = np.abs(gq) * sq, np.abs(gd) * sd
    elif kind == "aligned":
        a = F32(1 + 0.998 * 2.0 ** -8)
        Q = a * np.exp2(rng.integers(-3, 4, (nq, H))).astype(F32)
        D = a * np.exp2(rng.integers(-6, 1, (N, H))).astype(F32)
    elif kind == "wide":
        Q = gq * sq * np.exp(rng.uniform(-np.log(1e3), np.log(1e3), (1, H))).astype(F32)
        D = gd * sd * np.exp(rng.uniform(-np.log(1e3), np.log(1e3), (1, H))).astype(F32)
    elif kind == "tiny":
        # documents scaled row by row down to where the lo planes are bf16-subnormal (2^-133 apart) or vanish, the last rows to where
        # p0 itself is; queries on a 2^-16 grid in [0.5, 2), so that every plane product is a multiple of 2^-149 (tier A's premise)
        Q = (rng.integers(1 << 15, 1 << 17, (nq, H)).astype(F32) * F32(2.0 ** -16)) * rng.choice(np.array([-1, 1], F32), (nq, H))
        ex = np.array([-100, -108, -112, -116, -118, -120, -122, -124, -126, -128, -130], np.float64)
        D = (gd * F32(np.sqrt(H))) * np.exp2(ex[rng.integers(0, ex.size, (N, 1))]).astype(F32)
    elif kind == "bf16_exact":
        Q, D = G.bf16_round(gq * sq), G.bf16_round(gd * sd)
    elif kind == "zeros":
        Q, D = gq * sq, gd * sd
        signed = np.where(np.arange(H) % 2 == 1, F32(-0.0), F32(0.0))          # zeros of both signs: still exactly +0
        Q[:: 7] = 0
        Q[nq - 1] = signed
        D[:: 5] = 0
        D[N - 1] = signed
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(Q, F32), np.ascontiguousarray(D, F32)


def zero_pairs(Q, D):
    """[nq, N] bool: pairs with a zero query or a zero document - their score is exactly +0."""
    return (~Q.any(axis=1))[:, None] | (~D.any(axis=1))[None, :]


# ------------------------------------------------------------------------------------------ tier A
def plane_operands(Qp, Dp, mode):
    """The plane products of a mode as ONE GEMM: (A [nq, K], W [N, K], K), the planes side by side in pair order.  numpy or torch."""
    cat = np.concatenate if isinstance(Qp[0], np.ndarray) else _torch().cat
    A = cat([Qp[a] for _, a in PAIRS[mode]], 1)
    W = cat([Dp[b] for b, _ in PAIRS[mode]], 1)
    return A, W, A.shape[1]


def _torch():
    import torch
    return torch


def tier_a(Qp, Dp, mode):
    """(T, dA) of (A), [nq, N] float64.  numpy planes: through (G) of bf16_regime_cases.py.  torch planes (the GPU tests' large
    cases): the same two products on the planes' device; test_dense_split_host.py holds the two routes against each other."""
    A, W, K = plane_operands(Qp, Dp, mode)
    assert K == len(PAIRS[mode]) * Qp[0].shape[1]
    if isinstance(A, np.ndarray):
        return G._products(dict(A=A, W=W, K=K))
    A, W = A.double(), W.double()
    return A @ W.T, (K * E) * (A.abs() @ W.abs().T)


# ------------------------------------------------------------------------------------------ tier B
def exact_product(Q, D):
    """(sum_i q_i d_i, sum_i |q_i d_i|), float64, numpy or torch.  (float64's own H 2^-53 is 2^-19 of the smallest bound here.)"""
    if isinstance(Q, np.ndarray):
        q, d = Q.astype(np.float64), D.astype(np.float64)
        return q @ d.T, np.abs(q) @ np.abs(d).T
    q, d = Q.double(), D.double()
    return q @ d.T, q.abs() @ d.abs().T


def tier_b_residual(Q, D, mode):
    """(B), residual form: [nq, N] float64 from the actual planes and residuals (numpy)."""
    qp, dp = [np.abs(p.astype(np.float64)) for p in split_planes(Q)], [np.abs(p.astype(np.float64)) for p in split_planes(D)]
    rq, rd = residuals(Q), residuals(D)
    if mode == "bf16x3":
        return qp[0] @ rd[1].T + rq[1] @ dp[0].T + rq[0] @ rd[0].T
    return qp[0] @ rd[2].T + rq[2] @ dp[0].T + qp[1] @ rd[1].T + rq[1] @ dp[1].T + rq[1] @ rd[1].T


def tier_b_floor(Q, D):
    """The subnormal floor of (B), [nq, N] float64, numpy or torch."""
    H = Q.shape[1]
    if isinstance(Q, np.ndarray):
        sq, sd = np.abs(Q.astype(np.float64)).sum(axis=1), np.abs(D.astype(np.float64)).sum(axis=1)
    else:
        sq, sd = Q.double().abs().sum(dim=1), D.double().abs().sum(dim=1)
    return F134 * (1.02 * (sq[:, None] + sd[None, :]) + 7 * H * F134)


def tier_b_closed(Q, D, mode):
    """(B), closed form cB sum |q d| + floor: [nq, N] float64, numpy or torch."""
    return CB[mode] * exact_product(Q, D)[1] + tier_b_floor(Q, D)


def ratio(val, ref, bound):
    """Worst error as a fraction of the bound (information; inf where a zero bound is missed), numpy or torch."""
    if isinstance(ref, np.ndarray):
        return G.ratio(val, ref, bound)
    torch = _torch()
    err = (val.double() - ref).abs()
    q = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(q.max()) if q.numel() else 0.0
