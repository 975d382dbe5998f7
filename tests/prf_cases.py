"""The numpy model of pseudo-relevance feedback (include/sr_hip.h sr_sparse_feedback / sr_dense_feedback): every output
bit of csrc/prf.hip is fixed here.  Shared by tests/test_prf_host.py (the model against a plain per-term loop and against float64) and
tests/test_prf_gpu.py (the kernels and the Python layers against the model).

Definition.  v = the entries i < counts[q] of fb_ids[q] with id >= 0, in list order; the positive set is the first p = min(n_pos, |v|),
the negative set the last g = min(n_neg, |v| - p), in list order; a document that appears twice counts twice.  cp = f32(beta) / f32(p) and
cn = f32(gamma) / f32(g), fp32 divisions.  Per coordinate t: P_t / N_t = the sets' values at t added in list order from +0.0f, one
rounded fp32 add each; w_t = f32(f32(alpha * q_t) + f32(cp * P_t)), then w_t = f32(w_t - f32(cn * N_t)); q_t absent starts from +0.0f,
p = 0 / g = 0 skips its step.  Dense: w over all columns.  Sparse: terms with w_t > 0, of those the max_terms largest by (w descending,
term ascending; 0 = no limit), emitted with terms ascending.

Error bound against exact arithmetic (test_prf_host.py): P_t carries p - 1 rounded adds, N_t g - 1, each product one rounding, the
two combining steps one each - with u = 2^-24 every partial result is within (1 + u)^n of its exact value over the absolute sums, so
|w_t - exact| <= (p + g + 3) u (alpha |q_t| + cp sum|d_t| + cn sum|d_t|) to first order; the tests use positive margins far from the
second-order term."""
import numpy as np

F32 = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def feedback_sets(row, count, n_pos, n_neg):
    """(positive ids, negative ids) of one feedback row, each in list order."""
    row = np.asarray(row, dtype=np.int64)
    count = len(row) if count is None else max(0, min(int(count), len(row)))
    v = [int(d) for d in row[:count] if d >= 0]
    p = min(int(n_pos), len(v))
    g = min(int(n_neg), len(v) - p)
    return v[:p], v[len(v) - g:] if g else []


def coefficients(beta, gamma, p, g):
    """(cp, cn) as fp32; 0 where the set is empty (never used)."""
    cp = F32(beta) / F32(p) if p else F32(0)
    cn = F32(gamma) / F32(g) if g else F32(0)
    return F32(cp), F32(cn)


def combine(q, P, N, p, g, alpha, beta, gamma):
    """The formula on fp32 arrays of one query (q: the query's values with +0.0 where absent)."""
    cp, cn = coefficients(beta, gamma, p, g)
    w = (F32(alpha) * q).astype(F32)
    if p:
        w = (w + (cp * P).astype(F32)).astype(F32)
    if g:
        w = (w - (cn * N).astype(F32)).astype(F32)
    return w


def rocchio_dense(queries, row_of, fb_ids, counts, n_pos, n_neg, alpha, beta, gamma):
    """fp32 [nq, dim]: the rebuilt dense queries.  row_of(id) -> the stored row as fp32 (fp16 rows widened), KeyError if unknown."""
    queries = np.asarray(queries, dtype=F32)
    out = np.empty_like(queries)
    for qi in range(queries.shape[0]):
        pos, neg = feedback_sets(fb_ids[qi], None if counts is None else counts[qi], n_pos, n_neg)
        P = np.zeros(queries.shape[1], dtype=F32)
        N = np.zeros(queries.shape[1], dtype=F32)
        for d in pos:
            P = (P + row_of(d)).astype(F32)
        for d in neg:
            N = (N + row_of(d)).astype(F32)
        out[qi] = combine(queries[qi], P, N, len(pos), len(neg), alpha, beta, gamma)
    return out


def rocchio_sparse(q_indptr, q_cols, q_vals, d_indptr, d_cols, d_vals, n_terms, fb_ids, counts, n_pos, n_neg, alpha, beta, gamma, max_terms):
    """(indptr int64 [nq + 1], cols int32, vals fp32): the rebuilt sparse queries, over dense scratch rows of n_terms entries (a term in
    no source has w = 0 there and is dropped, as a term the kernel never sees)."""
    nq = len(q_indptr) - 1
    indptr, cols, vals = [0], [], []
    for qi in range(nq):
        pos, neg = feedback_sets(fb_ids[qi], None if counts is None else counts[qi], n_pos, n_neg)
        q = np.zeros(n_terms, dtype=F32)
        a, b = int(q_indptr[qi]), int(q_indptr[qi + 1])
        q[np.asarray(q_cols[a:b], dtype=np.int64)] = q_vals[a:b]
        P = np.zeros(n_terms, dtype=F32)
        N = np.zeros(n_terms, dtype=F32)
        for acc, docs in ((P, pos), (N, neg)):
            for d in docs:
                a, b = int(d_indptr[d]), int(d_indptr[d + 1])
                c = np.asarray(d_cols[a:b], dtype=np.int64)
                acc[c] = (acc[c] + d_vals[a:b]).astype(F32)
        w = combine(q, P, N, len(pos), len(neg), alpha, beta, gamma)
        keep = np.flatnonzero(w > 0)
        if max_terms and keep.size > max_terms:
            order = np.lexsort((keep, -w[keep]))                # w descending, ties to the lower term
            keep = np.sort(keep[order[:max_terms]])
        cols.append(keep.astype(np.int32))
        vals.append(w[keep])
        indptr.append(indptr[-1] + keep.size)
    return (np.asarray(indptr, dtype=np.int64), np.concatenate(cols) if cols else np.zeros(0, np.int32),
            np.concatenate(vals).astype(F32) if vals else np.zeros(0, F32))


def entries(q_indptr, d_indptr, fb_ids, counts, n_pos, n_neg):
    """Per query the entry count sr_prf_max_entries() is compared with: the query's terms plus all terms of the documents used."""
    out = []
    for qi in range(len(q_indptr) - 1):
        pos, neg = feedback_sets(fb_ids[qi], None if counts is None else counts[qi], n_pos, n_neg)
        out.append(int(q_indptr[qi + 1] - q_indptr[qi]) + sum(int(d_indptr[d + 1] - d_indptr[d]) for d in pos + neg))
    return out


def transpose_csr(indptr, doc_ids, vals, n_docs):
    """CSR by term -> CSR by document (terms ascending inside a document): numpy's stable sort by document."""
    indptr = np.asarray(indptr, dtype=np.int64)
    terms = np.repeat(np.arange(len(indptr) - 1, dtype=np.int32), np.diff(indptr))
    order = np.argsort(np.asarray(doc_ids), kind="stable")
    d_indptr = np.zeros(n_docs + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(doc_ids), minlength=n_docs), out=d_indptr[1:])
    return d_indptr, terms[order], np.asarray(vals, dtype=F32)[order]


def small_collection(seed=0, V=97, n_docs=50, nq=6, doc_terms=12, q_terms=5, edge=True):
    """The collection of the sparse tests: a doc-major CSR (document 3 empty, document 4 one posting, document 5 holds a -0.0), queries
    as CSR (edge: query 2 without terms) - values in (0.1, 2), rounded to 2^-6 so that sums tie now and then."""
    rng = np.random.default_rng(seed)

    def rows(n, per):
        indptr, cols, vals = [0], [], []
        for r in range(n):
            k = int(rng.integers(1, per + 1))
            c = np.sort(rng.choice(V, size=k, replace=False)).astype(np.int32)
            v = (np.round(rng.uniform(0.1, 2.0, size=k) * 64) / 64).astype(F32)
            cols.append(c)
            vals.append(v)
            indptr.append(indptr[-1] + k)
        return indptr, cols, vals

    di, dc, dv = rows(n_docs, doc_terms)
    dc[3], dv[3] = dc[3][:0], dv[3][:0]
    dc[4], dv[4] = dc[4][:1], dv[4][:1]
    dv[5][0] = F32(-0.0)
    di = np.concatenate([[0], np.cumsum([len(c) for c in dc])]).astype(np.int64)
    qi, qc, qv = rows(nq, q_terms)
    if edge:
        qc[2], qv[2] = qc[2][:0], qv[2][:0]
    qi = np.concatenate([[0], np.cumsum([len(c) for c in qc])]).astype(np.int64)
    return (qi, np.concatenate(qc), np.concatenate(qv)), (di, np.concatenate(dc), np.concatenate(dv))
