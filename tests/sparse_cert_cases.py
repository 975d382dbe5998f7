"""CPU-only pieces shared by test_sparse_cert_host.py, test_sparse_cert_kernels_gpu.py and test_sparse_cert_gpu.py: a numpy model of
the certified sparse scorer's stage 1 (csrc/sparse_cert.hip: cert_plan_kernel, cert_score_kernel; csrc/sparse_cert_build.hip: the index
side), a mirror of its certificate's cut, the documented two-sided bound and seeded cases.

Every constant below is derived here from the operations and the number formats; the tests import them and hold no copies.

Index side (index_model).  vscale = 2^(14 - ex) with vmax_all = m 2^ex, m in [0.5, 1): the largest value lands in [2^13, 2^14).  A
posting is kept as v16 = fp16(v * vscale) (the product is exact in fp32, the conversion rounds to nearest even and keeps fp16
subnormals), once in fragment order for the T dense terms (d16) and once packed with its place in the LDS tile (P).  Dense terms: the
lists with len * 1024 >= N by (length desc, term asc), at most SR_SPARSE_CERT_T rounded down to 16 (16 .. 128); T = their number
rounded up to 16, 48 promoted to 64.  S, E, the forward rows: see the functions.

Plan (plan_model), per query, in fp32 as the kernel's wave does it: lane l adds q_t * vmax_t of terms l, 64 + l, 128 + l, 192 + l with
fused multiply-adds (hipcc contracts `tot += v * vmx`), then the xor butterfly 32, 16 .. 1;
s_q = 0.98f / (tot * 1.0001f);  two_e = 2^(14 - ex) of dmax * s_q;  c_q = 1 / (two_e * vscale) (a power of two);  dense entry
b16 = fp16(q_t * s_q * two_e);  rare weight w16 = fp16(q_t * s_q * 65535 / vscale).  The division of s_q is the one operation whose last
bit a GPU may legitimately round differently from numpy: the GPU tests read s_q back, require the model's value within 1 ulp and
compute everything downstream from the GPU's.

Key (key_model), per (query, doc):   key = cvt(c_q * acc) + R

  R = sum over the rare postings of (uint32)(fp32(v16 * w16) + 1.0f).  v16 * w16 has 22 significant bits: exact in fp32; the + 1.0f rounds
      once, the conversion truncates.  Integer adds commute: R has exactly one value, whichever path (staged quads, overflow windows,
      single postings, extra groups) added a posting.  No tolerance.
  acc = sum over the T dense slots of a16 * b16, products exact (22 bits), added by v_mfma_f32_32x32x16_f16 in fp32 in an order the
      ISA does not specify: |acc - A| <= T 2^-24 A for A = the float64 sum (all terms >= 0).  c_q is a power of two: no cost.
  cvt = v_cvt_pknorm_u16_f32: 65535 x, to an integer.  Its rounding costs r key units.
  So with y = 65535 c_q A:      |key - (R + y)| <= r + y T 2^-24                                                                   (K)

  MEASURED on an MI355X (test_sparse_cert_kernels_gpu.py::test_conversion_rounding_and_subnormal_operands):
    r = 0.4998 on exact data (integer cases, 1.3 M pairs): v_cvt_pknorm_u16_f32 rounds to NEAREST, it does not truncate.  The tests
      hold r <= R_CVT = 0.5, the largest r for which the bound's 1.2 stands (next paragraph).
    v_mfma_f32_32x32x16_f16 KEEPS fp16 subnormal A operands: on all 148 docs of the subnormal case whose key tells (y with the 15
      subnormal products rounds to another integer than y without them, both 0.008 or more from the tie) the key is the one with
      them.  The bound does not need it - the plan's 0.1 budget covers a flush - but the model does: key_model multiplies them.
    Largest |key - (R + y)| seen on inexact data: 0.5057 (subnormal case) where (K) allows 0.5593; KS = 8: 0.5016 of 0.6473.

The documented bound (bound()).  tf = 65535 s_q (real-arithmetic score):
      tf (1 - dd) - 1.2 - 2.03 n_drop  <=  key  <=  tf (1 + dd) + 1.2 + 1.01 n_rare,     dd = 2 2^-11 + (T + 1) 2.4e-7 + 1e-5
  lower side, dense part: a16 b16 >= a b (1 - 2^-11)^2 for normal a16; a doc value whose v * vscale lies under 2^-14 errs by at most
      2^-25 absolutely (kept as a subnormal) or vanishes (flushed by the MFMA: at most 2^-14): 65535 c_q n_dense 2^-14 2^14 <= 0.1 is
      what the plan checks.  Accumulation (K): T 2^-24 relative.  Conversion: r <= 0.5.
  lower side, rare part: (uint)(x + 1) > x = v16 w16 >= v w (1 - 2^-11)^2 for normal v16; a subnormal v16 errs by 2^-25 w16 < 2^-25 6e4
      = 0.0018 per posting, 0.46 for 256 rare terms.  0.1 + 0.5 + 0.46 = 1.06 <= 1.2: the 1.2 has 0.14 to spare and NOTHING to spare for
      a truncating conversion (r up to 1).
  upper side: (uint)(x + 1) <= x + 1 + the rounding of the add (x < 2^16: 2^-8) <= x + 1.01 per rare posting, one per rare term.
  A dropped rare term (w16 < 6.2e-5 < 2^-13.9) is worth at most 2^14 2^-13.9 (1 + 2^-11) < 2.03 units.
  Saturation: tf <= 65535 * 0.98 / 1.0001 (s_q's 1.0001 covers the fp32 sum of tot), so key <= KEY_MAX < 65535 (saturation_limit()).

Seeded defects (test_sparse_cert_host.py): the model re-run with one posting of a run dropped, a posting in the other half of its LDS
word, table E read one tile late, the A ring one fragment ahead, a rare term of group 1 skipped, moves some key by more than (K)
allows on the cases below - a GPU failure of (K) therefore means the kernel, not the bound."""
import functools

import numpy as np

DT = 1024                 # docs per tile (SC_DT)
MAXR, MAXRT, MAXQT = 64, 256, 256
BAND = 1024
R_CVT = 0.5               # asserted on the GPU: the conversion rounds to nearest
# Findings of test_conversion_rounding_and_subnormal_operands on an MI355X (gfx950), see (K) above; the test asserts both
R_CVT_MEASURED = 0.4998
MFMA_FLUSHES_F16_SUBNORMALS = False
W_DROP, W_MAX, DENSE_MIN = np.float32(6.2e-5), np.float32(6.0e4), np.float32(6.2e-5)


def dd_of(T):
    return 2.0 * 4.8828125e-4 + 2.4e-7 + T * 2.4e-7 + 1.0e-5


def bound(tf, T, n_rare, n_drop):
    """(lowest, highest) key the documentation allows for tf = 65535 s_q (real-arithmetic score)."""
    dd = dd_of(T)
    return tf * (1 - dd) - 1.2 - 2.03 * n_drop, tf * (1 + dd) + 1.2 + 1.01 * n_rare


def saturation_limit(T, n_rare):
    return 65535.0 * 0.98 / 1.0001 * (1 + dd_of(T)) + 1.2 + 1.01 * n_rare


def cut_from_kth(Kk, T, n_rare, n_qt, n_drop):
    """Mirror of cert_cut_from_kth (double arithmetic, the same order of operations)."""
    dd = 2.0 * 4.8828125e-4 + 2.4e-7 + float(T) * 2.4e-7 + 1.0e-5
    gamma = (float(n_qt) + 2.0) * 6.0e-8 * 1.01
    lb = (float(Kk) - 1.2 - 1.01 * float(n_rare)) / (1.0 + dd)
    return float(np.floor((lb * (1.0 - gamma) / (1.0 + gamma) - 2.03 * float(n_drop)) * (1.0 - dd) - 1.2) - 1.0)


def key_tolerance(y, T):
    return R_CVT + y * T * 2.0 ** -24


def _f32(x):
    return np.float32(x)


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64, so one float64 add and one rounding to fp32 (a
    double rounding needs the float64 sum to land on an fp32 tie: not with the 48-bit products used here and 53 bits to hold them)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


# ------------------------------------------------------------------------------------------------------------- index model ---
def round_T(n_heavy_lists, t_cap=128):
    t_max = max(16, min(128, t_cap // 16 * 16))
    n_heavy = min(n_heavy_lists, t_max)
    T = max(16, (n_heavy + 15) // 16 * 16)
    if T == 48:
        T = 64
    return n_heavy, T


def index_model(indptr, ids, vals, N, t_cap=128):
    indptr = np.asarray(indptr, np.int64)
    ids = np.asarray(ids, np.int64)
    vals = np.asarray(vals, np.float32)
    V, nnz = len(indptr) - 1, len(ids)
    lens = np.diff(indptr)
    term_of = np.repeat(np.arange(V), lens)
    vmax = np.zeros(V, np.float32)
    np.maximum.at(vmax, term_of, vals)
    _, ex = np.frexp(np.float32(vmax.max()))
    vscale = np.float32(np.ldexp(np.float32(1.0), 14 - int(ex)))
    heavy = [t for t in range(V) if lens[t] > 0 and lens[t] * 1024 >= N]
    heavy.sort(key=lambda t: (-lens[t], t))
    n_heavy, T = round_T(len(heavy), t_cap)
    KS = T // 16
    slot_term = np.array(heavy[:n_heavy], np.int64)
    dslot = np.full(V, -1, np.int32)
    dslot[slot_term] = np.arange(n_heavy, dtype=np.int32)
    n_tiles = (N + DT - 1) // DT
    e_stride = (n_tiles + 3) // 4 * 4 + 4
    v16 = (vals * vscale).astype(np.float16)
    dl = (ids % DT).astype(np.uint32)
    P = np.zeros(nnz + 4, np.uint32)
    P[:nnz] = ((dl >> 1) << 2) | (dl & 1) | (v16.view(np.uint16).astype(np.uint32) << 16)
    tile_of = ids // DT
    cnt = np.zeros((V, n_tiles), np.int64)
    np.add.at(cnt, (term_of, tile_of), 1)
    S = (indptr[:-1, None] + np.concatenate([np.zeros((V, 1), np.int64), np.cumsum(cnt, axis=1)], axis=1)).astype(np.uint32)
    E = np.zeros((V, e_stride), np.uint32)
    E[:, :n_tiles] = np.where(cnt >= 2, 0xffff0000 | np.minimum(cnt, 0xffff), 0).astype(np.uint32)
    single = np.argwhere(cnt == 1)
    E[single[:, 0], single[:, 1]] = P[S[single[:, 0], single[:, 1]]] | 2
    d16 = np.zeros((n_tiles, DT // 32, KS, 64, 8), np.float16)
    A = np.zeros((n_tiles * DT, T), np.float16)                    # the same operand row-major, for the key model
    sl = dslot[term_of]
    m = sl >= 0
    kk, s = sl[m] & 15, sl[m] >> 4
    dlm = ids[m] % DT
    d16[tile_of[m], dlm >> 5, s, (dlm & 31) + 32 * (kk >> 3), kk & 7] = v16[m]
    A[ids[m], sl[m]] = v16[m]
    order = np.lexsort((term_of, ids))                              # forward rows: docs ascending, terms ascending inside a doc
    fwd_indptr = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=N))]).astype(np.int64)
    fwd_tv = (term_of[order].astype(np.uint64) << np.uint64(32)) | vals[order].view(np.uint32).astype(np.uint64)
    return dict(V=V, N=N, nnz=nnz, indptr=indptr, ids=ids, vals=vals, term_of=term_of, vmax=vmax, vscale=vscale, T=T, KS=KS,
                n_heavy=n_heavy, dslot=dslot, n_tiles=n_tiles, e_stride=e_stride, v16=v16, P=P, S=S, E=E, d16=d16, A=A,
                fwd_indptr=fwd_indptr, fwd_tv=fwd_tv, max_row=int(np.diff(fwd_indptr).max()))


# -------------------------------------------------------------------------------------------------------------- plan model ---
def plan_model(ix, qi, qc, qv, sq_from_gpu=None):
    """Per query what cert_plan_kernel writes.  reason[q]: "" = on the fast path, else why not.  sq_from_gpu [nq]: the GPU's s_q, used
    for everything downstream of it (sq_model keeps the model's own)."""
    nq = len(qi) - 1
    nq_pad = (nq + 31) // 32 * 32
    T, KS, vscale = ix["T"], ix["KS"], ix["vscale"]
    out = dict(bfrag=np.zeros((nq_pad // 32, KS, 64, 8), np.float16), B=np.zeros((nq_pad, T), np.float16),
               rare_term=np.full((nq_pad, MAXRT), -1, np.int32), rare_w=np.zeros((nq_pad, MAXRT), np.float32),
               cq=np.zeros(nq_pad, np.float32), sq=np.zeros(nq_pad, np.float32), sq_model=np.zeros(nq_pad, np.float32),
               n_rare=np.zeros(nq_pad, np.int32), n_qt=np.zeros(nq_pad, np.int32), n_drop=np.zeros(nq_pad, np.int32),
               elig=np.zeros(nq_pad, np.uint8), reason=["padding"] * nq_pad)
    lens = np.diff(ix["indptr"])
    for q in range(nq):
        cols, v = np.asarray(qc[qi[q]:qi[q + 1]], np.int64), np.asarray(qv[qi[q]:qi[q + 1]], np.float32)
        n = len(cols)
        if n <= 0 or n > MAXQT:
            out["reason"][q] = "length"
            continue
        ok = bool((np.diff(cols) > 0).all()) and bool(((v >= 0) & (v < np.float32(3.0e38))).all())
        live = (cols >= 0) & (cols < ix["V"]) & (v > 0)
        live[live] &= lens[cols[live]] > 0
        part = np.zeros(64, np.float32)
        for i in np.flatnonzero(live):                              # i = c * 64 + lane, ascending c per lane
            part[i % 64] = _fma32(v[i], ix["vmax"][cols[i]], part[i % 64])
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[np.arange(64) ^ off]
        tot = part[0]
        slot = np.where(live, ix["dslot"][np.clip(cols, 0, ix["V"] - 1)], -1)
        dense, rare = live & (slot >= 0), live & (slot < 0)
        if not ok:
            out["reason"][q] = "order or sign"
            continue
        if rare.sum() > MAXRT or not (tot > 0) or not (tot < np.float32(1.0e30)):
            out["reason"][q] = "no live term" if not (tot > 0) else "too many rare terms"
            continue
        sq_m = _f32(0.98) / (tot * _f32(1.0001))
        out["sq_model"][q] = sq_m
        sq = sq_m if sq_from_gpu is None or sq_from_gpu[q] == 0 else np.float32(sq_from_gpu[q])
        two_e = np.float32(1.0)
        if dense.any():
            _, ex = np.frexp(v[dense].max() * sq)
            two_e = np.float32(np.ldexp(np.float32(1.0), 14 - int(ex)))
            if not (v[dense].min() * sq * two_e >= DENSE_MIN):
                out["reason"][q] = "dense weight range"
                continue
        cq = _f32(1.0) / (two_e * vscale)
        if not (_f32(65535.0) * cq * _f32(int(dense.sum())) <= _f32(0.1)):
            out["reason"][q] = "subnormal budget"
            continue
        with np.errstate(over="ignore"):
            wr = (v * sq * _f32(65535.0) / vscale).astype(np.float16).astype(np.float32)
            b16 = (v * sq * two_e).astype(np.float16)
        if (rare & ~(wr < W_MAX)).any():
            out["reason"][q] = "rare weight too large"
            continue
        dropped = rare & (wr < W_DROP)
        kept = np.flatnonzero(rare & ~dropped)
        for i in np.flatnonzero(dense):
            s, kk = slot[i] >> 4, slot[i] & 15
            out["bfrag"][q // 32, s, q % 32 + 32 * (kk >> 3), kk & 7] = b16[i]
            out["B"][q, slot[i]] = b16[i]
        out["rare_term"][q, :len(kept)] = cols[kept]
        out["rare_w"][q, :len(kept)] = wr[kept]
        out["cq"][q], out["sq"][q], out["n_rare"][q], out["n_qt"][q] = cq, sq, len(kept), n
        out["n_drop"][q], out["elig"][q], out["reason"][q] = int(dropped.sum()), 1, ""
    return out


# --------------------------------------------------------------------------------------------------------------- key model ---
def rare_sums(ix, plan, q, defect=None):
    """R of (K) for query q and every doc: int64 [n_tiles * DT].  defect: one of the seeded kernel defects (docstring)."""
    R = np.zeros(ix["n_tiles"] * DT, np.int64)
    indptr, ids, v16 = ix["indptr"], ix["ids"], ix["v16"]
    for j in range(int(plan["n_rare"][q])):
        if defect == "skip_group1_term" and j == MAXR:
            continue
        t, w = int(plan["rare_term"][q, j]), np.float32(plan["rare_w"][q, j])
        sl = slice(indptr[t], indptr[t + 1])
        d = ids[sl].copy()
        c = (v16[sl].astype(np.float32) * w + np.float32(1.0)).astype(np.uint32).astype(np.int64)
        if defect == "drop_tail_posting":                           # the last posting of every run whose length is no multiple of 4
            tile = d // DT
            last = np.r_[tile[1:] != tile[:-1], True]
            run_len = np.bincount(tile, minlength=ix["n_tiles"])[tile]
            c = np.where(last & (run_len >= 2) & (run_len % 4 != 0), 0, c)
        elif defect == "other_half":                                # single postings of a (term, tile) land in the word's other half
            tile = d // DT
            run_len = np.bincount(tile, minlength=ix["n_tiles"])[tile]
            d = np.where(run_len == 1, d ^ 1, d)
        elif defect == "e_one_tile_late":                           # tile i adds what table E holds for tile i + 1 (same doc offsets)
            keep = d >= DT
            d, c = d[keep] - DT, c[keep]
        np.add.at(R, d, c)
    return R


def key_model(ix, plan, q, defect=None, flush_subnormals=False):
    """(R int64 [docs], y float64 [docs]) of (K) for one fast-path query; docs = n_tiles * DT (the padding of the last tile included)."""
    A = ix["A"]
    if flush_subnormals:
        A = np.where(np.abs(A) < np.float16(2.0 ** -14), np.float16(0), A)
    A = A.astype(np.float64)
    if defect == "ring_fragment_ahead":                             # every MFMA multiplies the fragment one place ahead in the wave's slice
        KS, nt = ix["KS"], ix["n_tiles"]                            # slice = 4 blocks x KS k-steps, fragment i = (block i / KS, k-step i % KS)
        F = A.reshape(nt, 8, 4, 32, KS, 16)                         # [tile][wave][block][doc][k-step][k]
        F = F.transpose(0, 1, 2, 4, 3, 5).reshape(nt * 8 * 4 * KS, 32, 16)
        F = np.roll(F, -1, axis=0)
        A = F.reshape(nt, 8, 4, KS, 32, 16).transpose(0, 1, 2, 4, 3, 5).reshape(nt * DT, KS * 16)
    acc = A @ plan["B"][q].astype(np.float64)
    y = 65535.0 * float(plan["cq"][q]) * acc
    return rare_sums(ix, plan, q, defect), y


def true_fix(ix, plan, qi, qc, qv, q):
    """65535 s_q (real-arithmetic score) in float64 for every doc."""
    s = np.zeros(ix["n_tiles"] * DT, np.float64)
    for t, w in zip(qc[qi[q]:qi[q + 1]], qv[qi[q]:qi[q + 1]]):
        if 0 <= t < ix["V"]:
            sl = slice(ix["indptr"][t], ix["indptr"][t + 1])
            np.add.at(s, ix["ids"][sl], float(w) * ix["vals"][sl].astype(np.float64))
    return 65535.0 * float(plan["sq"][q]) * s


# ------------------------------------------------------------------------------------------------------------------- cases ---
def _assemble(N, lists):
    """lists: {term: (docs, vals)} -> CSR by term with docs ascending; terms 0 .. max(term)."""
    V = max(lists) + 1
    indptr, ids, vals = [0], [], []
    for t in range(V):
        d, v = lists.get(t, (np.zeros(0, np.int64), np.zeros(0, np.float32)))
        d, v = np.asarray(d, np.int64), np.asarray(v, np.float32)
        o = np.argsort(d, kind="stable")
        assert len(np.unique(d)) == len(d) and (len(d) == 0 or (d.min() >= 0 and d.max() < N))
        ids.append(d[o]); vals.append(v[o]); indptr.append(indptr[-1] + len(d))
    return np.array(indptr, np.int64), np.concatenate(ids).astype(np.int32), np.concatenate(vals).astype(np.float32)


def _queries(qs):
    """qs: list of (cols, vals), cols ascending."""
    qi = np.concatenate([[0], np.cumsum([len(c) for c, _ in qs])]).astype(np.int64)
    return qi, np.concatenate([np.asarray(c, np.int32) for c, _ in qs]), np.concatenate([np.asarray(v, np.float32) for _, v in qs])


def _case(name, N, lists, qs, k, t_cap, **kw):
    indptr, ids, vals = _assemble(N, lists)
    qi, qc, qv = _queries(qs)
    return dict(name=name, N=N, indptr=indptr, ids=ids, vals=vals, qi=qi, qc=qc, qv=qv, k=k, t_cap=t_cap, nq=len(qs), **kw)


def _full_lists(N, n, value_of):
    """n terms present in every doc: with SR_SPARSE_CERT_T = n they are the dense ones (length N, lowest term ids)."""
    return {t: (np.arange(N), value_of(t)) for t in range(n)}


def _runs_lists(rng, N, first_term, integer):
    """Rare terms whose runs per (term, tile) have 0, 1, 2, 3, 4, 5, 8, 9 and 1 024 postings, runs that end on a tile's last doc and
    begin on the next tile's first, and a term living in the partial last tile only."""
    n_tiles = (N + DT - 1) // DT
    lens = [0, 1, 2, 3, 4, 5, 8, 9, 1024]
    lists, t = {}, first_term
    val = (lambda n: rng.choice([1.0, 2.0, 4.0, 8.0], size=n)) if integer else (lambda n: np.log1p(rng.uniform(0, 20, size=n)))
    for rot in range(len(lens)):                                    # term `rot`: tile i holds a run of lens[(i + rot) % 9]
        docs = []
        for i in range(n_tiles):
            room = min(DT, N - i * DT)
            n = min(lens[(i + rot) % len(lens)], room)
            docs.append(i * DT + np.sort(rng.choice(room, size=n, replace=False)))
        d = np.concatenate(docs)
        lists[t] = (d, val(len(d))); t += 1
    for i in range(n_tiles - 1):                                    # ... 1022, 1023 | 1024, 1025 ...: a run ends on the tile's last doc, the next begins on the first
        d = np.array([i * DT + 1021, i * DT + 1022, i * DT + 1023, (i + 1) * DT, (i + 1) * DT + 1])
        d = d[d < N]
        lists[t] = (d, val(len(d))); t += 1
    last0 = (n_tiles - 1) * DT
    for n in (1, 2, 5):                                             # only in the partial last tile, the last doc of the collection included
        d = np.unique(np.r_[N - 1, last0 + rng.choice(N - last0, size=min(n, N - last0), replace=False)])[-n:]
        lists[t] = (d, val(len(d))); t += 1
    return lists, t


def _mixed_queries(rng, dense_terms, rare_terms, nq, n_rare_of, integer, equal_dense=True):
    qs = []
    for q in range(nq):
        nr = min(n_rare_of(q), len(rare_terms))
        r = np.sort(rng.choice(rare_terms, size=nr, replace=False))
        d = np.zeros(0, np.int64) if nr + len(dense_terms) > MAXQT else np.array(dense_terms) if equal_dense else np.sort(rng.choice(dense_terms, size=max(1, len(dense_terms) // 2), replace=False))
        cols = np.sort(np.concatenate([d, r]))
        if integer:
            v = np.where(np.isin(cols, d), 1.0, rng.choice([1.0, 2.0, 4.0], size=len(cols)))
        else:
            v = np.log1p(rng.uniform(0.5, 20, size=len(cols)))
        qs.append((cols, v))
    return qs


@functools.lru_cache(maxsize=None)
def runs_case(n_tiles_mod4=1, integer=True):
    """N chosen so that n_tiles % 4 = n_tiles_mod4 and the last tile is partial; 40 queries = two blocks, the second ragged."""
    rng = np.random.default_rng(100 + n_tiles_mod4 + 10 * integer)
    n_tiles = {0: 12, 1: 9, 2: 10, 3: 11}[n_tiles_mod4]
    N = (n_tiles - 1) * DT + 517
    dense_val = (lambda t: rng.choice([1.0, 2.0, 4.0, 8.0], size=N)) if integer else (lambda t: np.log1p(rng.uniform(0, 20, size=N)))
    lists = _full_lists(N, 16, dense_val)
    rl, end = _runs_lists(rng, N, 16, integer)
    lists.update(rl)
    rare = np.arange(16, end)
    qs = _mixed_queries(rng, list(range(16)), rare, 40, lambda q: [len(rare), 9, 1, 20, 0][q % 5], integer)
    # 12 tiles with k + band >= 2 048: launches of 3, 6 tiles begin at the odd tiles 3 and 9; one tile per workgroup: odd tile0 in every case
    return _case(f"runs[{n_tiles} tiles,{'integer' if integer else 'real'}]", N, lists, qs, 1100 if n_tiles_mod4 == 0 else 10, 16, integer=integer)


@functools.lru_cache(maxsize=None)
def groups_case(integer=True):
    """64, 65, 128, 129 and 256 rare terms beside 16 dense ones; rare lists of ~250 postings per tile: the 4 items of a scatter wave
    stage 4 x 64 x 63 quads > 512 (cert_overflow_windows) and groups 1 - 3 walk runs of every tail length (cert_extra_groups)."""
    rng = np.random.default_rng(200 + integer)
    N = 3 * DT + 301
    val = (lambda n: rng.choice([1.0, 2.0, 4.0], size=n)) if integer else (lambda n: np.log1p(rng.uniform(0, 20, size=n)))
    lists = _full_lists(N, 16, lambda t: val(N))
    for t in range(16, 16 + 300):
        dens = [0.25, 0.02, 0.001][t % 3]
        d = np.flatnonzero(rng.random(N) < dens)
        if len(d) == 0:
            d = np.array([t % N])
        lists[t] = (d, val(len(d)))
    rare = np.arange(16, 316)
    counts = [64, 65, 128, 129, 256, 3, 70, 0]
    qs = _mixed_queries(rng, list(range(16)), rare, 36, lambda q: counts[q % len(counts)], integer)
    return _case(f"groups[{'integer' if integer else 'real'}]", N, lists, qs, 10, 16, integer=integer)


@functools.lru_cache(maxsize=None)
def saturation_case():
    """Doc 2049 (odd half of its LDS word, tile 2) holds every term of query 0 (256 rare terms) and of query 1 (16 dense + 240 rare) at
    the list's maximum; its neighbour 2048 in the same word holds one small posting of one rare term.  Weights spread over five binades."""
    rng = np.random.default_rng(300)
    N, star = 3 * DT + 77, 2 * DT + 1
    def lst(n_other):
        d = np.r_[star, rng.choice(np.setdiff1d(np.arange(N), [star, star - 1]), size=n_other, replace=False)]
        v = np.r_[16.0, rng.uniform(0.01, 15.9, size=n_other)]
        return d, v
    lists = _full_lists(N, 16, lambda t: np.where(np.arange(N) == star, 16.0, rng.uniform(0.01, 15.9, size=N)))
    for t in range(16, 16 + 256):
        lists[t] = lst(int(rng.integers(0, 40)))
    lists[16] = (np.r_[lists[16][0], star - 1], np.r_[lists[16][1], 0.37])
    w = lambda n: np.exp(rng.uniform(np.log(0.2), np.log(6.0), size=n))
    qs = [(np.arange(16, 272), w(256)), (np.arange(0, 256), np.r_[np.full(16, 3.0), w(240)]), (np.arange(0, 16), np.full(16, 1.0))]
    return _case("saturation", N, lists, qs, 5, 16, star=star)


@functools.lru_cache(maxsize=None)
def midpoints_case():
    """Values and weights on fp16 rounding ties: v * vscale = (2 m + 1) 2^-11 2^e (halfway between two fp16 numbers), query weights
    chosen likewise before the scaling; rare and dense."""
    rng = np.random.default_rng(400)
    N = 3 * DT + 5
    tie = lambda n: (2 * rng.integers(1024, 2048, size=n) + 1) * 2.0 ** -11 * 2.0 ** rng.integers(-6, 3, size=n)     # 12 significant bits, max < 8
    lists = _full_lists(N, 16, lambda t: tie(N))
    lists[0][1][7] = 8.0 - 2.0 ** -9                                # the index maximum: just under a power of two (vscale = 2^11)
    for t in range(16, 80):
        d = np.flatnonzero(rng.random(N) < [0.2, 0.004][t % 2])
        lists[t] = (d, tie(len(d)))
    qs = []
    for q in range(33):
        r = np.sort(rng.choice(np.arange(16, 80), size=int(rng.integers(1, 60)), replace=False))
        cols = np.r_[np.arange(16), r]
        qs.append((cols, tie(len(cols))))
    return _case("midpoints", N, lists, qs, 10, 16)


SUB_MAX = 1023 * 2.0 ** -37        # the largest fp16 subnormal after the scaling by vscale = 2^13 of the subnormal case


@functools.lru_cache(maxsize=None)
def subnormal_case():
    """The index maximum 1.0 belongs to a one-posting term outside the queries (vscale = 2^13).  Dense term 0: values on a 2^-13 grid in
    [2^-6, 2^-3]; dense terms 1 - 12: SUB_MAX (the largest fp16 subnormal once scaled), 13 - 15: 2^-28, 2^-29, 2^-30 of the maximum.
    Query 0 (16 equal dense weights) gets c_q = 2^-24, the largest the plan's subnormal budget allows: the 15 subnormal operands are
    worth ~0.033 key units together - docs whose key sits that close under a rounding tie tell whether the MFMA honours or flushes
    them.  Queries 1, 2 add 64 / 200 rare terms whose values are 2^-28 .. 2^-30 of the maximum under weights near 5.6e4; query 3 is turned
    down by the plan's subnormal budget."""
    rng = np.random.default_rng(500)
    N = 4 * DT + 9
    tiny = [2.0 ** -28, 2.0 ** -29, 2.0 ** -30]
    lists = {0: (np.arange(N), rng.integers(128, 1025, size=N) * 2.0 ** -13)}
    lists[0][1][11] = 2.0 ** -3
    for t in range(1, 13):
        lists[t] = (np.arange(N), np.full(N, SUB_MAX))
    for t in range(13, 16):
        lists[t] = (np.arange(N), np.full(N, tiny[t - 13]))
    for t in range(16, 216):
        d = np.flatnonzero(rng.random(N) < [0.3, 0.01][t % 2])
        lists[t] = (np.r_[d, N - 1] if len(d) == 0 else d, rng.choice(tiny + [SUB_MAX], size=max(1, len(d))))
    lists[216] = (np.array([5]), np.array([1.0]))
    dense = (np.arange(16), np.full(16, 1.0))
    qs = [dense,
          (np.arange(0, 80), np.r_[np.full(16, 1.0), np.full(64, 890.0)]),
          (np.arange(0, 216), np.r_[np.full(16, 1.0), rng.uniform(600.0, 890.0, size=200)]),
          (np.arange(1, 16), np.full(15, 1.0))]                      # only dense terms without a normal value: c_q = 2^-3, over the plan's budget
    return _case("subnormal", N, lists, qs, 5, 16, expect_reason={3: "subnormal budget"})


@functools.lru_cache(maxsize=None)
def drop_boundary_case():
    """Rare weights w16 on each side of 6.2e-5 (below: the term is left out of stage 1) and of 6.0e4 (at or above: exact kernels).  The
    dense terms carry tot, so s_q is known in advance up to the 1e-3 the rare terms add, far less than the steps between the targets;
    the 6e4 pair is a rare-only query whose second term (list maximum 2^-10 of the index's) is balanced against the first."""
    rng = np.random.default_rng(600)
    N = 3 * DT + 40
    lists = _full_lists(N, 16, lambda t: rng.uniform(0.5, 15.9, size=N))
    lists[0][1][3] = 16.0 - 2.0 ** -8                                # index maximum: vscale = 2^10
    for t in range(16, 40):
        d = np.flatnonzero(rng.random(N) < 0.05)
        lists[t] = (d, rng.uniform(2.0 ** -9, 2.0 ** -8, size=len(d)))
    d39 = lists[39][0]
    lists[39] = (d39, np.r_[2.0 ** -10, rng.uniform(2.0 ** -12, 2.0 ** -10, size=len(d39) - 1)])
    vscale, vmax16 = 2.0 ** 10, float(np.float32(lists[16][1].max()))
    tot_dense = sum(2.0 * float(np.float32(lists[t][1].max())) for t in range(16))
    per_w = 0.98 / (tot_dense * 1.0001) * 65535.0 / vscale          # w16 per unit of a rare query weight beside the 16 dense terms
    base = (np.arange(16), np.full(16, 2.0))
    qs = [base]
    for target in (6.0e-5, 6.15e-5, 6.25e-5, 6.4e-5):
        qs.append((np.arange(0, 20), np.r_[np.full(16, 2.0), np.full(4, target / per_w)]))
    qs.append((np.r_[np.arange(16), 20, 21, 22], np.r_[np.full(16, 2.0), 6.0e-5 / per_w, 6.4e-5 / per_w, 1.0]))
    qs.append((np.arange(16, 24), np.full(8, 1.0)))                 # rare terms only, ordinary weights
    for target in (5.9e4, 6.1e4):                                   # w16(term 39) = 0.98 * 65535 / (1.0001 vscale (x vmax16 + 2^-10)) for weights (x, 1)
        x = (0.98 * 65535.0 / (1.0001 * vscale * target) - 2.0 ** -10) / vmax16
        qs.append((np.array([16, 39]), np.array([x, 1.0])))
    return _case("drop boundary", N, lists, qs, 5, 16, expect_drop=[0, 4, 4, 0, 0, 1, 0, 0, None], expect_reason={8: "rare weight too large"})


@functools.lru_cache(maxsize=None)
def forward_rows_case(big=1024):
    """Docs with 0, 1, 2, 3 and `big` (1 024: the forward sort's limit; 1 025: over it) postings, each length beginning at an odd and at
    an even offset of fwd_tv (the re-score loads two postings per 16 bytes); queries of 64 and 65 terms (either side of the re-score's
    LDS-list / scalar-loop switch).  The short docs hold large values of terms 16 - 19, which every query weights heavily, and the
    dense lists cover half of the other docs with small values: the short docs rank among the k best, so they are candidates of
    the certificate and rows of the result."""
    rng = np.random.default_rng(700 + big)
    N = 3 * DT + 3
    n_post = {0: 0, 1: 1, 2: 2, 3: 3, 4: 0, 5: 1, 6: big, 7: 1, 8: 2, 9: 3, 10: big, 11: 2, 12: 1, 13: big}
    offs = np.concatenate([[0], np.cumsum([n_post[d] for d in sorted(n_post)])])
    assert big != 1024 or {(n_post[d], int(offs[d]) & 1) for d in n_post if n_post[d]} >= {(n, p) for n in (1, 2, 3, big) for p in (0, 1)}
    V = 20 + big + 40
    others = np.arange(len(n_post), N)
    lists, per_term = {}, {}
    for d, n in n_post.items():
        terms = rng.choice(np.arange(16, 20), size=n, replace=False) if n < big else np.r_[np.arange(16), 20 + np.arange(big - 16)]
        for t in terms:
            per_term.setdefault(int(t), []).append(d)
    for t in range(V):
        dens = 0.5 - 0.004 * t if t < 16 else (0.0 if t < 20 else 0.002)
        d = others[rng.random(len(others)) < dens]
        v = rng.uniform(0.1, 1.0, size=len(d))
        sp = np.array(per_term.get(t, []), np.int64)
        spv = np.full(len(sp), 15.0) if 16 <= t < 20 else rng.uniform(0.1, 1.0, size=len(sp))
        if len(d) + len(sp) == 0:
            d, v = np.array([others[t % len(others)]]), np.array([0.5])
        lists[t] = (np.r_[sp, d], np.r_[spv, v])
    lists[0][1][-1] = 16.0                                           # the index maximum, on an ordinary doc
    qs = []
    for n in (64, 65, 64, 65, 30, 200):
        cols = np.sort(np.r_[rng.choice(16, size=8, replace=False), np.arange(16, 20), rng.choice(np.arange(20, 4 + big), size=n - 12, replace=False)])
        qs.append((cols, np.where((cols >= 16) & (cols < 20), 3.0, np.log1p(rng.uniform(0.5, 3, size=n)))))
    return _case(f"forward rows[{big}]", N, lists, qs, 30, 16, special_docs=sorted(n_post), n_post=n_post)


@functools.lru_cache(maxsize=None)
def ks_case(t_cap):
    """An index with 130 lists long enough to be dense (lengths all distinct), forced to T = t_cap heavy terms; 300 rare terms; 40
    queries mixing both.  t_cap = 48 gives 48 dense slots in a T = 64 operand (16 all-zero columns)."""
    rng = np.random.default_rng(800)                                # the same index and queries for every t_cap
    N = 3 * DT + 5
    lists = {}
    for t in range(130):
        d = np.sort(rng.choice(N, size=1500 - 7 * t, replace=False))
        lists[t] = (d, np.log1p(rng.uniform(0, 20, size=len(d))))
    for t in range(130, 430):
        d = np.flatnonzero(rng.random(N) < [0.05, 0.0007][t % 2])
        lists[t] = (np.array([t % N]) if len(d) == 0 else d, np.log1p(rng.uniform(0, 20, size=max(1, len(d)))))
    qs = []
    for q in range(40):
        cols = np.sort(np.r_[rng.choice(130, size=int(rng.integers(1, 60)), replace=False), rng.choice(np.arange(130, 430), size=int(rng.integers(0, 40)), replace=False)])
        qs.append((cols, np.log1p(rng.uniform(0.5, 20, size=len(cols)))))
    return _case(f"KS[T cap {t_cap}]", N, lists, qs, 10, t_cap)


@functools.lru_cache(maxsize=None)
def off_path_case():
    """One query per way off the fast path (case["expect_reason"], "" = on it) over the index of ks_case(32)."""
    base = ks_case(32)
    V = len(base["indptr"]) - 1
    qs = [("", (np.array([1, 5, 200]), np.array([1.0, 2.0, 0.5]))),
          ("length", (np.arange(257), np.ones(257))),
          ("order or sign", (np.array([5, 1]), np.array([1.0, 1.0]))),                   # descending
          ("no live term", (np.array([V, V + 3]), np.array([1.0, 2.0]))),                # unknown terms only
          ("dense weight range", (np.array([0, 1]), np.array([1.0, 2.0 ** -28]))),       # a dense term 2^28 below the largest
          ("order or sign", (np.array([1, 5]), np.array([1.0, -1.0]))),                  # a negative weight
          ("order or sign", (np.array([1, 1]), np.array([1.0, 1.0]))),                   # a duplicate term
          ("length", (np.zeros(0, np.int64), np.zeros(0))),                              # empty
          ("", (np.array([1, 5]), np.array([0.0, 1.0]))),                                # a zero weight: one live term
          ("", (np.array([3, 140, V + 1]), np.array([1.0, 2.0, 3.0])))]                  # known + unknown
    qi, qc, qv = _queries([q for _, q in qs])
    return dict(base, name="off the fast path", qi=qi, qc=qc, qv=qv, nq=len(qs), k=5, expect_reason=[r for r, _ in qs])


@functools.lru_cache(maxsize=None)
def uncertifiable_case():
    """Query 0: every doc scores the same (16 dense terms of constant value): more ties than k + band keys.  Query 1: one rare term with
    3 postings, fewer than k non-zero keys.  Query 2: an ordinary query between them."""
    rng = np.random.default_rng(900)
    N = 4 * DT + 100
    lists = _full_lists(N, 16, lambda t: np.full(N, 1.0))
    lists[16] = (np.array([7, 1500, N - 1]), np.array([2.0, 1.0, 0.5]))
    for t in range(17, 60):
        d = np.flatnonzero(rng.random(N) < 0.08)
        lists[t] = (d, np.log1p(rng.uniform(0, 20, size=len(d))))
    qs = [(np.arange(16), np.full(16, 1.0)), (np.array([16]), np.array([1.5])), (np.arange(17, 60), np.log1p(rng.uniform(0.5, 20, size=43)))]
    return _case("uncertifiable", N, lists, qs, 10, 16, expect_uncert=[1, 1, 0])


KS_CAPS = (16, 32, 48, 64, 80, 96, 112, 128)
EXPECTED_T = {16: 16, 32: 32, 48: 64, 64: 64, 80: 80, 96: 96, 112: 112, 128: 128}


def host_cases():
    """Every case the CPU tests run the bound on."""
    return [runs_case(1, True), runs_case(2, False), groups_case(True), groups_case(False), saturation_case(), midpoints_case(),
            subnormal_case(), drop_boundary_case(), forward_rows_case(1024), ks_case(48), ks_case(128)]


def models(case, sq_from_gpu=None):
    ix = index_model(case["indptr"], case["ids"], case["vals"], case["N"], case["t_cap"])
    plan = plan_model(ix, case["qi"], case["qc"], case["qv"], sq_from_gpu)
    return ix, plan
