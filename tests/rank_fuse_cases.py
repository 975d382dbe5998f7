"""The numpy model of sr_rank_fuse (include/sr_hip.h): a direct restatement of its semantics with Python loops over
np.float32 scalars, a dict per query and sorted(key=(-fused, id)).  Every comparison against it is for equal bits."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max


def valid_entries(ids, counts, l, q):
    """[(rank0, id)] of the valid entries of row (l, q): r < counts[l, q] (or depth) and id >= 0; the rank is the slot's place."""
    depth = ids.shape[2]
    n = depth if counts is None else max(0, min(depth, int(counts[l, q])))
    return [(r, int(ids[l, q, r])) for r in range(n) if ids[l, q, r] >= 0]


def contributions(ids, counts, scores, method, weights, c, l, q):
    """{id: (contribution as np.float32, 1-based rank)} of list l for query q."""
    ent = valid_entries(ids, counts, l, q)
    w = F32(weights[l])
    out = {}
    if method == "rrf":
        for r, d in ent:
            out[d] = (F32(w / F32(F32(c) + F32(r + 1))), r + 1)
        return out
    assert method == "minmax"
    if not ent:
        return out
    s = [F32(scores[l, q, r]) for r, _ in ent]
    mn, mx = min(s), max(s)
    with np.errstate(over="ignore", invalid="ignore"):
        span = F32(mx - mn)
        for (r, d), x in zip(ent, s):
            norm = F32(F32(x - mn) / span) if span > 0 else F32(1.0)
            out[d] = (F32(w * norm), r + 1)
    return out


def rank_fuse(ids, k, counts=None, scores=None, method="rrf", weights=None, c=60.0, order=None):
    """ids int64 [L, nq, depth] ... -> (scores fp32 [nq, k], ids int64 [nq, k], counts int32 [nq], ranks int32 [nq, k, L]).
    order (None: ascending l): the order in which the lists' contributions are added - the contract is ascending; the tests use
    another order to show that their inputs can tell the difference."""
    ids = np.asarray(ids)
    L, nq, depth = ids.shape
    weights = [1.0] * L if weights is None else weights
    out_s = np.full((nq, k), -FLT_MAX, F32)
    out_i = np.full((nq, k), -1, np.int64)
    out_c = np.zeros(nq, np.int32)
    out_r = np.zeros((nq, k, L), np.int32)
    for q in range(nq):
        fused, ranks = {}, {}
        for l in (range(L) if order is None else order):
            for d, (contrib, rank) in contributions(ids, counts, scores, method, weights, c, l, q).items():
                with np.errstate(over="ignore", invalid="ignore"):
                    fused[d] = F32(fused.get(d, F32(0.0)) + contrib)
                ranks.setdefault(d, {})[l] = rank
        best = sorted(fused, key=lambda d: (-fused[d], d))[:k]
        out_c[q] = len(best)
        for i, d in enumerate(best):
            out_s[q, i], out_i[q, i] = fused[d], d
            for l, rank in ranks[d].items():
                out_r[q, i, l] = rank
    return out_s, out_i, out_c, out_r


def rank_fuse_f64(ids, k, counts=None, scores=None, method="rrf", weights=None, c=60.0):
    """The same contributions summed in float64 and rounded once: what a contracted prev + w * norm would drift towards.  Scores only,
    as {(q, id): np.float32}."""
    ids = np.asarray(ids)
    L, nq, _ = ids.shape
    weights = [1.0] * L if weights is None else weights
    out = {}
    for q in range(nq):
        acc = {}
        for l in range(L):
            ent = valid_entries(ids, counts, l, q)
            if method == "minmax" and ent:
                s = [F32(scores[l, q, r]) for r, _ in ent]
                mn, mx = min(s), max(s)
                span = F32(mx - mn)
            for r, d in ent:
                if method == "rrf":
                    x = float(F32(weights[l])) / float(F32(F32(c) + F32(r + 1)))
                else:
                    norm = F32(F32(F32(scores[l, q, r]) - mn) / span) if span > 0 else F32(1.0)
                    x = float(F32(weights[l])) * float(norm)
                acc[d] = acc.get(d, 0.0) + x
        for d, v in acc.items():
            out[(q, d)] = F32(v)
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)
