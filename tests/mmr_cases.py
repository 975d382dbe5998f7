"""The numpy model of sr_dense_mmr (include/sr_hip.h): a direct restatement of its definition, one query and one pick at
a time over np.float32 arrays (every operation rounds once, to fp32).  Similarities come from oracle.scoring.dense_scores_fma over the stored rows in the exact kernel's k order
(mfma_korder), fp16-stored rows rounded first.  Every comparison against it is for equal bits."""
import numpy as np

from oracle.scoring import dense_scores_fma, mfma_korder

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def stored(rows, row_dtype="fp32"):
    """The rows as the index holds them, widened to fp32."""
    rows = np.ascontiguousarray(rows, F32)
    return rows.astype(np.float16).astype(F32) if row_dtype == "fp16" else rows


def similarities(rows, korder=None):
    """sim[i, j] fp32 [N, N]: the fmaf chain from +0.0f over rows i and j, k visited in `korder` (None: the exact kernel's order)."""
    rows = np.ascontiguousarray(rows, F32)
    return dense_scores_fma(rows, rows, mfma_korder(rows.shape[1]) if korder is None else korder)


def mmr(sim, row_of, ids, rel, k, lam, counts=None, info=None):
    """ids int64 [nq, n], rel fp32 [nq, n], counts [nq] or None -> (ids int64 [nq, k], rel fp32 [nq, k], mmr fp32 [nq, k],
    pos int32 [nq, k], counts int32 [nq]).  row_of(id) -> the row of sim that holds document id (KeyError / None: not in the index ->
    ValueError).  info (a dict): gains "ties" = the picks t >= 1 at which another live candidate had an equal marginal value, and
    "below_first" = the queries whose pick 1 lies above pick 0."""
    ids = np.asarray(ids, np.int64)
    rel = np.ascontiguousarray(rel, F32)
    nq, n = ids.shape
    lam32 = F32(lam)
    mu = F32(F32(1.0) - lam32)
    out_i = np.full((nq, k), -1, np.int64)
    out_r = np.full((nq, k), -FLT_MAX, F32)
    out_m = np.full((nq, k), -FLT_MAX, F32)
    out_p = np.full((nq, k), -1, np.int32)
    out_c = np.zeros(nq, np.int32)
    ties = below = 0
    for q in range(nq):
        cnt = n if counts is None else max(0, min(n, int(counts[q])))
        alive = [i for i in range(cnt) if ids[q, i] >= 0]
        row = {}
        for i in alive:
            r = row_of(int(ids[q, i]))
            if r is None:
                raise ValueError(f"candidate id {int(ids[q, i])} (query {q}, entry {i}) is not in the index")
            row[i] = r
        alive = np.array(alive, np.int64)
        rows = np.array([row[i] for i in alive], np.int64)
        lr = (lam32 * rel[q, alive]).astype(F32)                  # float32 arrays: every operation below rounds once, to fp32
        m = np.full(alive.size, -np.inf, F32)
        cid = ids[q, alive]
        last = None
        for t in range(min(k, n)):
            if alive.size == 0:
                break
            if t == 0:
                value, key = lr, rel[q, alive]
            else:
                s = sim[rows, last]
                m = np.where(s > m, s, m)
                value = key = (lr - (mu * m).astype(F32)).astype(F32)
            order = np.lexsort((alive, cid, -key.astype(np.float64)))      # -0.0 and +0.0 compare equal: then id, then position
            b = order[0]
            ties += bool(t >= 1 and alive.size >= 2 and key[order[1]] == key[b])
            out_i[q, t], out_r[q, t], out_m[q, t], out_p[q, t] = cid[b], rel[q, alive[b]], value[b], alive[b]
            out_c[q] = t + 1
            last = rows[b]
            keep = np.arange(alive.size) != b
            alive, rows, lr, m, cid = alive[keep], rows[keep], lr[keep], m[keep], cid[keep]
        below += bool(out_c[q] >= 2 and out_m[q, 1] > out_m[q, 0])
    if info is not None:
        info["ties"], info["below_first"] = ties, below
    return out_i, out_r, out_m, out_p, out_c
