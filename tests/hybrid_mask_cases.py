"""The expected-route calculator of tests/hybrid_cases.py restated for an allowed set of documents (numpy only): what
hybrid.search_fused(mask=) must report and return when only the documents with allowed[p] take part.  The lists are those of the allowed
documents, the dense list is complete when it holds all m of them (kd >= m; D = -FLT_MAX when m < kd: the list ends in padding), and
range hits are counted over allowed documents only."""
import numpy as np

import hybrid_cases as H

F32 = np.float32


def expected_routes(dense_all, sparse_all, d2s, n_s2d, w, k, depths, allowed):
    """(depth index at which the certificate holds, -1 = range route; candidates ranked; dense range hits) per query, from the brute-force
    pair scores dense_all / sparse_all [nq, N] (sparse 0.0 where d2s < 0) and allowed bool [N]."""
    nq, N = dense_all.shape
    d2s = np.asarray(d2s, np.int64)
    allowed = np.asarray(allowed, bool)
    tie = H.tie_of(d2s, n_s2d)
    fused = H.fuse(w, dense_all, sparse_all)
    n_sparse = int((d2s >= 0).sum())
    pool = np.flatnonzero(allowed)
    m = len(pool)
    route, union_len, hits = np.full(nq, -1, np.int64), np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    if m == 0:
        route[:] = 0
        return route, union_len, hits
    for q in range(nq):
        d_order = pool[np.lexsort((pool, -dense_all[q][pool].astype(np.float64)))]      # the masked dense search: score desc, position asc
        listed = np.flatnonzero(allowed & (d2s >= 0) & (sparse_all[q] > 0))             # the masked sparse search at threshold 0.0
        s_order = listed[np.lexsort((d2s[listed], -sparse_all[q][listed].astype(np.float64)))]
        for di, depth in enumerate(depths):
            kd, ks = min(depth, N), min(depth, max(1, n_sparse))
            A, B = d_order[:kd], s_order[:ks]
            D = dense_all[q][A[-1]] if len(A) == kd else F32(-H.FLT_MAX)
            S = sparse_all[q][B[-1]] if len(B) == ks else F32(0)
            U = np.union1d(A, B)
            o = U[np.lexsort((tie[U], -fused[q][U].astype(np.float64)))]
            Fk = fused[q][o[k - 1]] if len(o) >= k else None
            if H.certified(w, Fk, D, S, complete=kd >= m):
                route[q], union_len[q] = di, len(U)
                break
        else:
            thr = H.range_threshold(w, Fk, S)
            R = np.flatnonzero((dense_all[q] > thr) & allowed)
            hits[q], union_len[q] = len(R), len(np.union1d(R, B))
    return route, union_len, hits


def rank_rows(fused, tie, k, allowed):
    """hybrid_cases.rank_rows over the allowed documents only, positions given back in the numbering of all documents."""
    pool = np.flatnonzero(np.asarray(allowed, bool))
    ids, sc, counts = H.rank_rows(np.ascontiguousarray(fused[:, pool]), np.asarray(tie)[pool], k)
    return np.where(ids >= 0, pool[np.clip(ids, 0, None)] if len(pool) else -1, -1), sc, counts
