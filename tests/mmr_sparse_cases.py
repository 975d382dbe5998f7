"""The numpy model of sr_sparse_mmr (include/sr_hip.h): the document-document similarities restated literally - the
term-serial chain over the common terms in ascending term order, every product and every add rounded once to fp32 - and, for cosine,
np.sqrt and `/` on float32 (both correctly rounded).  The selection is tests/mmr_cases.py's `mmr`, imported unchanged.  Also the small
collections the tests search: doc-major rows with empty rows, one-term rows, rows of 63 / 64 / 65 / 130 / about 300 terms, pairs of
identical rows and disjoint rows.  Every comparison against the model is for equal bits."""
import numpy as np

from mmr_cases import FLT_MAX, bits, mmr  # noqa: F401  (re-exported: the selection and its helpers)

F32 = np.float32
V, N_DOCS = 512, 600
LONG_ROWS = {20: 63, 21: 64, 22: 65, 23: 130, 24: 300, 25: 130, 26: 300}      # document -> terms
EMPTY_ROWS = (3, 17, 40, 599)
ONE_TERM_ROWS = (4, 18, 41)
TWINS = 10                      # documents 50 .. 59 repeat documents 30 .. 39; 27 and 28 repeat the long rows 24 and 23
LOW_ONLY, HIGH_ONLY = (60, 61, 62), (63, 64, 65)      # terms below 100 only / from 400 only: disjoint rows


def dense_rows(rows, n_terms=V):
    """rows: a list of (terms int32 ascending, values fp32) -> (values fp32 [N, n_terms], present bool [N, n_terms])."""
    D = np.zeros((len(rows), n_terms), F32)
    P = np.zeros((len(rows), n_terms), bool)
    for i, (t, v) in enumerate(rows):
        D[i, t] = v
        P[i, t] = True
    return D, P


def ip_matrix(rows, n_terms=V):
    """ip[i, j] fp32 [N, N]: s = +0.0f, then for every term t that rows i and j both hold, in ascending t,
    s = f32(s + f32(v_i[t] * v_j[t])) - the chain run term by term, for all pairs at once."""
    D, P = dense_rows(rows, n_terms)
    S = np.zeros((len(rows), len(rows)), F32)
    for t in range(n_terms):
        both = P[:, t][:, None] & P[:, t][None, :]
        if both.any():
            prod = (D[:, t][:, None] * D[:, t][None, :]).astype(F32)
            S = np.where(both, (S + prod).astype(F32), S)
    return S


def ip_pair(a, b):
    """One pair, entry by entry: the definition without any array trick (the hand-worked tests check ip_matrix against it)."""
    s = F32(0.0)
    vb = {int(t): F32(v) for t, v in zip(*b)}
    for t, v in zip(*a):
        if int(t) in vb:
            s = F32(s + F32(F32(v) * vb[int(t)]))
    return s


def cosine_matrix(ip):
    """norm_i = f32(sqrt(ip(i, i))), den = f32(norm_i * norm_j), sim = den > 0 ? f32(ip / den) : +0.0f."""
    norm = np.sqrt(np.diagonal(ip).astype(F32)).astype(F32)
    den = (norm[:, None] * norm[None, :]).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (ip / den).astype(F32), F32(0.0)).astype(F32)


def sim_matrix(rows, sim, n_terms=V):
    ip = ip_matrix(rows, n_terms)
    return ip if sim == "ip" else cosine_matrix(ip)


def collection(seed=0, n_docs=N_DOCS, n_terms=V):
    """The documents of the GPU tests as a list of (terms, values): lengths 2 .. 40 by default, the special rows above, values in
    (0.05, 3) with full mantissas (a sum in another order has other bits)."""
    rng = np.random.default_rng(seed)
    rows = []
    for d in range(n_docs):
        if d in EMPTY_ROWS:
            L, lo, hi = 0, 0, n_terms
        elif d in ONE_TERM_ROWS:
            L, lo, hi = 1, 0, n_terms
        elif d in LONG_ROWS:
            L, lo, hi = LONG_ROWS[d], 0, n_terms
        elif d in LOW_ONLY:
            L, lo, hi = 30, 0, 100
        elif d in HIGH_ONLY:
            L, lo, hi = 30, 400, n_terms
        else:
            L, lo, hi = int(rng.integers(2, 41)), 0, n_terms
        t = np.sort(rng.choice(np.arange(lo, hi), size=L, replace=False)).astype(np.int32)
        v = rng.uniform(0.05, 3.0, size=L).astype(F32)
        rows.append((t, v))
    for i in range(TWINS):
        rows[50 + i] = rows[30 + i]
    rows[27], rows[28] = rows[24], rows[23]                         # long identical rows: 300 and 130 terms
    return rows


def doc_major_csr(rows):
    """(indptr int64 [N + 1], cols int32, vals fp32): what SparseIndexHIP.forward_rows() holds."""
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(t) for t, _ in rows])
    cols = np.concatenate([t for t, _ in rows]).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    vals = np.concatenate([v for _, v in rows]).astype(F32) if indptr[-1] else np.zeros(0, F32)
    return indptr, cols, vals


def term_major_csr(rows, n_terms=V):
    """(indptr int64 [V + 1], doc_ids int32 ascending inside a term, vals fp32): what SparseIndexHIP is built from."""
    indptr, cols, vals = doc_major_csr(rows)
    docs = np.repeat(np.arange(len(rows), dtype=np.int32), np.diff(indptr))
    order = np.lexsort((docs, cols))
    t_indptr = np.zeros(n_terms + 1, np.int64)
    t_indptr[1:] = np.cumsum(np.bincount(cols, minlength=n_terms))
    return t_indptr, docs[order], vals[order]


def candidates(n_docs, nq, n, seed, quantum=None):
    """ids int64 [nq, n] (documents repeat once n exceeds the collection), rel fp32 [nq, n]."""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.choice(n_docs, size=n, replace=n > n_docs) for _ in range(nq)]).astype(np.int64)
    rel = rng.uniform(0.0, 30.0, size=(nq, n)).astype(F32)
    if quantum:
        rel = (np.round(rel / quantum) * quantum).astype(F32)
    return ids, rel
