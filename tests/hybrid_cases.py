"""Shared constructions of the exact hybrid search tests (numpy only): the fused score, the certificate and the d* bisection restated in
numpy float32 - the expected-route calculator of tests/test_hybrid_search_gpu.py, itself checked against a brute-force scan over every
float of a window by tests/test_hybrid_search_host.py - brute-force rankings, and the synthetic indexes of the end-to-end cases."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def f2ord(x):
    """Order-preserving uint32 image of float32 values (larger float -> larger integer; -0.0 just below +0.0)."""
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000).astype(np.uint64)


def ord2f(o):
    o = np.asarray(o, np.uint64)
    u = np.where(o & 0x80000000, o & 0x7FFFFFFF, 0xFFFFFFFF - o).astype(np.uint32)
    return u.view(F32)


def fuse(w, dense, sparse):
    """f32(f32(w_d * dense) + f32(w_s * sparse)): numpy float32 arithmetic rounds every operation."""
    with np.errstate(over="ignore", invalid="ignore"):
        a = (F32(w[0]) * np.asarray(dense, F32)).astype(F32)
        b = (F32(w[1]) * np.asarray(sparse, F32)).astype(F32)
        return (a + b).astype(F32)


def certified(w, Fk, D, S, complete=False):
    """The certificate: the candidates hold the true top-k when the dense list is complete or F_k > B = fused(D, S), strictly.  Fk None:
    fewer than k candidates."""
    return bool(complete) or (Fk is not None and bool(F32(Fk) > fuse(w, D, S)))


def range_threshold(w, Fk, S):
    """pred(d*), d* the smallest float32 with g(d*) = fuse(w, d*, S) >= Fk, by bisection over the ordered image; -inf when g(-FLT_MAX) >=
    Fk (or Fk is None), +inf when not even g(+inf) reaches Fk."""
    if Fk is None or fuse(w, -FLT_MAX, S) >= F32(Fk):
        return F32(-np.inf)
    if not fuse(w, np.inf, S) >= F32(Fk):
        return F32(np.inf)
    lo, hi = int(f2ord(-FLT_MAX)), int(f2ord(np.inf))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fuse(w, ord2f(mid), S) >= F32(Fk):
            hi = mid
        else:
            lo = mid
    return F32(ord2f(lo))


def tie_of(d2s, n_s2d):
    """retrieve_fused's tie rule over all dense positions: the sparse position, or len(s2d) + dense position without one."""
    d2s = np.asarray(d2s, np.int64)
    return np.where(d2s >= 0, d2s, n_s2d + np.arange(len(d2s), dtype=np.int64))


def rank_rows(fused, tie, k):
    """The first k of (fused descending, tie ascending) per row of fused [nq, n]: (positions [nq, k] padded with -1, scores padded with
    -FLT_MAX, counts)."""
    nq, n = fused.shape
    ids = np.full((nq, k), -1, np.int64)
    sc = np.full((nq, k), -FLT_MAX, F32)
    for q in range(nq):
        o = np.lexsort((tie, -fused[q].astype(np.float64)))[:k]
        ids[q, :len(o)], sc[q, :len(o)] = o, fused[q][o]
    return ids, sc, np.full(nq, min(k, n), np.int32)


def expected_routes(dense_all, sparse_all, d2s, n_s2d, w, k, depths):
    """What hybrid.search_fused must report for every query, from the brute-force pair scores dense_all / sparse_all [nq, N] (sparse 0.0
    where d2s < 0): (depth index at which the certificate holds, -1 = range route; candidates ranked; dense range hits)."""
    nq, N = dense_all.shape
    d2s = np.asarray(d2s, np.int64)
    tie = tie_of(d2s, n_s2d)
    fused = fuse(w, dense_all, sparse_all)
    n_sparse = int((d2s >= 0).sum())
    route, union_len, hits = np.full(nq, -1, np.int64), np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    for q in range(nq):
        d_order = np.lexsort((np.arange(N), -dense_all[q].astype(np.float64)))          # the dense search: score desc, position asc
        listed = np.flatnonzero((d2s >= 0) & (sparse_all[q] > 0))                       # the sparse search at threshold 0.0
        s_order = listed[np.lexsort((d2s[listed], -sparse_all[q][listed].astype(np.float64)))]
        for di, depth in enumerate(depths):
            kd, ks = min(depth, N), min(depth, max(1, n_sparse))
            A, B = d_order[:kd], s_order[:ks]
            D = dense_all[q][A[-1]]
            S = sparse_all[q][B[-1]] if len(B) == ks else F32(0)
            U = np.union1d(A, B)
            o = U[np.lexsort((tie[U], -fused[q][U].astype(np.float64)))]
            Fk = fused[q][o[k - 1]] if len(o) >= k else None
            if certified(w, Fk, D, S, complete=kd >= N):
                route[q], union_len[q] = di, len(U)
                break
        else:
            thr = range_threshold(w, Fk, S)
            H = np.flatnonzero(dense_all[q] > thr)
            hits[q], union_len[q] = len(H), len(np.union1d(H, B))
    return route, union_len, hits


def sparse_csr(postings, V):
    """{term: (doc positions ascending int32, values fp32)} -> CSR by term (indptr int64 [V + 1], doc_ids int32, vals fp32)."""
    indptr = np.zeros(V + 1, np.int64)
    for t, (d, _) in postings.items():
        indptr[t + 1] = len(d)
    np.cumsum(indptr, out=indptr)
    ids, vals = np.zeros(int(indptr[-1]), np.int32), np.zeros(int(indptr[-1]), F32)
    for t, (d, v) in postings.items():
        ids[indptr[t]:indptr[t + 1]], vals[indptr[t]:indptr[t + 1]] = d, v
    return indptr, ids, vals


def query_csr(queries):
    """[(cols int32 ascending, vals fp32)] -> (indptr int64, cols, vals)."""
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in queries])]).astype(np.int64)
    cols = np.concatenate([c for c, _ in queries]).astype(np.int32) if queries else np.zeros(0, np.int32)
    vals = np.concatenate([v for _, v in queries]).astype(F32) if queries else np.zeros(0, F32)
    return indptr, cols, vals


def family_case(seed=5, N=4096, dim=128, V=2000, per_family=8):
    """The end-to-end case: 3 x per_family queries, each with one dedicated term (term = query number) whose posting list covers every
    document with values built from that query's normalised dense scores a - correlated relu(a + 3 + 0.05 n), independent relu(n + 3),
    anti-correlated relu(3 - a + 0.05 n) - plus random background terms.  Sparse positions are a permutation of the dense ones.  Returns a
    dict: rows [N, dim], Q [nq, dim], postings CSR, the query CSR parts, d2s, s2d."""
    rng = np.random.default_rng(seed)
    nq = 3 * per_family
    rows = rng.standard_normal((N, dim), dtype=F32)
    Q = rng.standard_normal((nq, dim), dtype=F32)
    a = Q.astype(np.float64) @ rows.astype(np.float64).T
    Q = (Q / a.std(1, keepdims=True)).astype(F32)                 # dense scores of unit spread: the two heads weigh alike
    a = (a - a.mean(1, keepdims=True)) / a.std(1, keepdims=True)
    s2d = rng.permutation(N).astype(np.int64)
    d2s = np.empty(N, np.int64)
    d2s[s2d] = np.arange(N)
    postings = {}
    for q in range(nq):
        n = rng.standard_normal(N)
        v = [a[q] + 3 + 0.05 * n, n + 3, 3 - a[q] + 0.05 * n][q // per_family]
        postings[q] = (np.arange(N, dtype=np.int32), np.maximum(v, 0).astype(F32)[s2d])      # value of sparse position p: its document s2d[p]
    background = np.arange(nq, V)
    for t in rng.choice(background, 400, replace=False):
        d = np.sort(rng.choice(N, int(rng.integers(1, 60)), replace=False)).astype(np.int32)
        postings[int(t)] = (d, rng.uniform(0.0, 0.3, len(d)).astype(F32))
    terms = np.array(sorted(t for t in postings if t >= nq), np.int32)
    queries = []
    for q in range(nq):
        extra = np.sort(rng.choice(terms, 6, replace=False)).astype(np.int32)
        queries.append((np.concatenate([[q], extra]).astype(np.int32), np.concatenate([[1.0], rng.uniform(0.1, 1.0, 6)]).astype(F32)))
    return dict(rows=rows, Q=Q, index=sparse_csr(postings, V), queries=queries, d2s=d2s, s2d=s2d, N=N, V=V)


def integer_case(seed=6, N=600, dim=64, V=40, nq=16):
    """Rows and queries in {-1, 0, 1}, posting values in {1, 2}: every score is a small integer, ties are everywhere.  About a fifth of
    the documents have no posting (d2s = -1); the others' sparse positions are a random order."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-1, 2, (N, dim)).astype(F32)
    Q = rng.integers(-1, 2, (nq, dim)).astype(F32)
    has = rng.random(N) < 0.8
    s2d = rng.permutation(np.flatnonzero(has)).astype(np.int64)
    d2s = np.full(N, -1, np.int64)
    d2s[s2d] = np.arange(len(s2d))
    postings = {}
    for t in range(V):
        d = np.sort(rng.choice(len(s2d), int(rng.integers(5, len(s2d) // 3)), replace=False)).astype(np.int32)
        postings[t] = (d, rng.integers(1, 3, len(d)).astype(F32))
    for p in range(len(s2d)):                      # every sparse position has a posting
        if not any(p in postings[t][0] for t in range(V)):
            d, v = postings[0]
            i = int(np.searchsorted(d, p))
            postings[0] = (np.insert(d, i, p).astype(np.int32), np.insert(v, i, F32(1)))
    queries = []
    for q in range(nq):
        c = np.sort(rng.choice(V, int(rng.integers(1, 6)), replace=False)).astype(np.int32)
        queries.append((c, rng.integers(1, 3, len(c)).astype(F32)))
    return dict(rows=rows, Q=Q, index=sparse_csr(postings, V), queries=queries, d2s=d2s, s2d=s2d, N=N, V=V)
