"""Collapsed search (scaling_retriever_amd/collapse.py, csrc/topk_collapse.hip): a plain model and the shared inputs of
tests/test_collapse_host.py and tests/test_collapse_gpu.py.

The model is a loop over a row that keeps first occurrences.  All dense rows and queries here are small INTEGERS (|x| <= 3), so every
fp32 inner product is exact in any summation order; sparse weights are small positive integers.  The full ranking (score descending,
id ascending) is therefore computed in numpy on the CPU and is the GPU's bit for bit, whatever route served a query - and which route
serves a query is decided here, not on the device."""
import functools

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def collapse_model(scores, ids, keys, k, counts=None, exhaustive=False):
    """sr_topk_collapse in plain Python: (scores [nq, k], ids [nq, k], keys [nq, k], counts [nq], complete [nq])."""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.int64)
    nq, row_len = scores.shape
    out_s = np.full((nq, k), -FLT_MAX, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    out_k = np.full((nq, k), -1, np.int32)
    out_c = np.zeros(nq, np.int32)
    done = np.zeros(nq, np.int32)
    for q in range(nq):
        if counts is not None:
            n = min(max(int(counts[q]), 0), row_len)
        else:
            neg = np.flatnonzero(ids[q] < 0)
            n = int(neg[0]) if len(neg) else row_len
        seen, m = set(), 0
        for p in range(n):
            g = int(keys[ids[q, p]])
            if g in seen:
                continue
            seen.add(g)
            out_s[q, m], out_i[q, m], out_k[q, m] = scores[q, p], ids[q, p], g
            m += 1
            if m == k:
                break
        out_c[q] = m
        done[q] = 1 if (m == k or n < row_len or exhaustive) else 0
    return out_s, out_i, out_k, out_c, done


def full_ranking(S, ids=None, keep=None):
    """Per query of the score matrix S [nq, N] the full ranking as (scores, ids) lists: score descending, ties by ascending id; ids
    (default the column numbers) name the columns, keep [nq, N] or [N] bool leaves columns out."""
    nq, N = S.shape
    ids = np.arange(N, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    out = []
    for q in range(nq):
        cols = np.arange(N) if keep is None else np.flatnonzero(keep if keep.ndim == 1 else keep[q])
        order = cols[np.lexsort((ids[cols], -S[q, cols].astype(np.float64)))]
        out.append((S[q, order].astype(np.float32), ids[order]))
    return out


def collapsed_ranking(ranking, keys, k):
    """The definition applied to full rankings [(scores, ids)]: (scores [nq, k], ids, keys, counts) with padding."""
    nq = len(ranking)
    width = max(1, max(len(r[1]) for r in ranking))
    S = np.zeros((nq, width), np.float32)
    I = np.full((nq, width), -1, np.int64)
    for q, (s, i) in enumerate(ranking):
        S[q, :len(i)], I[q, :len(i)] = s, i
    counts = np.array([len(r[1]) for r in ranking], np.int32)
    return collapse_model(S, I, keys, k, counts=counts, exhaustive=True)[:4]


def first_complete_depth(ranking, keys, k, depths, n_docs):
    """Per query the index of the first depth d at which the device can prove the row: the prefix of d entries holds k distinct keys, or
    the ranking is shorter than d (the row ends in padding), or d >= n_docs, the number of documents the search ranks by construction
    (the driver then states that rows are whole rankings); -1: none (the full-ranking route)."""
    out = np.full(len(ranking), -1, np.int64)
    for q, (_, ids) in enumerate(ranking):
        for j, d in enumerate(depths):
            if len(ids) < d or d >= n_docs or len(set(keys[ids[:d]].tolist())) >= k:
                out[q] = j
                break
    return out


# ------------------------------------------------------------------------------------------------------------------ dense inputs
N_DOCS, DIM, N_GROUPS = 3000, 128, 400


@functools.lru_cache(maxsize=None)
def dense_case():
    """(D int-valued fp32 [3000, 128], Q [200, 128], keys int32 [3000], S = Q D^T exactly).  Random groups of mean size 7.5; queries
    0 - 19 point at a planted group of 500 passages (key 0) that outranks everything else for them: their top-k groups need the whole
    ranking behind depths (16, 64); queries 20 - 39 point half as strongly at a group of 40, which depth 16 cannot get past."""
    rng = np.random.default_rng(2024)
    D = rng.integers(-3, 4, size=(N_DOCS, DIM)).astype(np.float32)
    Q = rng.integers(-3, 4, size=(200, DIM)).astype(np.float32)
    keys = rng.integers(2, N_GROUPS, size=N_DOCS).astype(np.int32)
    big = rng.choice(N_DOCS, 540, replace=False)
    keys[big[:500]], keys[big[500:]] = 0, 1
    # the planted passages carry +3 on the first 64 / 32 dimensions, as do their queries: 576 / 288 above the noise (std ~ 45)
    D[big[:500], :64] = 3
    Q[:20, :64] = 3
    D[big[500:], 64:96] = 3
    Q[20:40, 64:96] = 3
    S = (Q.astype(np.float64) @ D.astype(np.float64).T).astype(np.float32)
    assert np.abs(S).max() < 2 ** 24
    return D, Q, keys, S


# ----------------------------------------------------------------------------------------------------------------- sparse inputs
S_DOCS, S_TERMS = 3000, 64


@functools.lru_cache(maxsize=None)
def sparse_case():
    """A 3000-document, 64-term index as CSR by term (indptr, doc_ids, vals), 40 queries as CSR (qi, qc, qv), keys int32 [3000] and the
    exact score matrix S [40, 3000] (small positive integer weights).  Terms 0 and 1 belong to two planted groups: 500 documents of key
    0 carry term 0 and 40 documents of key 1 carry term 1, both with a large weight; queries 0 - 7 ask for term 0 (their top-k groups
    need the whole ranking behind depths (16, 64)), queries 8 - 15 for term 1 (depth 16 cannot get past that group)."""
    rng = np.random.default_rng(77)
    W = np.zeros((S_DOCS, S_TERMS), np.float32)
    for d in range(S_DOCS):
        t = rng.choice(np.arange(2, S_TERMS), size=rng.integers(2, 7), replace=False)
        W[d, t] = rng.integers(1, 5, size=len(t))
    keys = rng.integers(2, N_GROUPS, size=S_DOCS).astype(np.int32)
    big = rng.choice(S_DOCS, 540, replace=False)
    keys[big[:500]], keys[big[500:]] = 0, 1
    W[big[:500], 0] = 50
    W[big[500:], 1] = 50
    nq = 40
    Qw = np.zeros((nq, S_TERMS), np.float32)
    for q in range(nq):
        t = rng.choice(np.arange(2, S_TERMS), size=rng.integers(2, 9), replace=False)
        Qw[q, t] = rng.integers(1, 4, size=len(t))
    Qw[:8, 0] = 3
    Qw[8:16, 1] = 3
    indptr, doc_ids, vals = [0], [], []
    for t in range(S_TERMS):
        rows = np.flatnonzero(W[:, t])
        doc_ids.extend(rows.tolist())
        vals.extend(W[rows, t].tolist())
        indptr.append(len(doc_ids))
    qi, qc, qv = [0], [], []
    for q in range(nq):
        cols = np.flatnonzero(Qw[q])
        qc.extend(cols.tolist())
        qv.extend(Qw[q, cols].tolist())
        qi.append(len(qc))
    S = (Qw.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    return (np.array(indptr, np.int64), np.array(doc_ids, np.int32), np.array(vals, np.float32), np.array(qi, np.int64),
            np.array(qc, np.int32), np.array(qv, np.float32), keys, S)
