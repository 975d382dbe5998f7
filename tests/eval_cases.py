"""The model of sr_eval_ranked and sr_eval_randomization (include/sr_hip.h) and the case generators of their tests.

The metric model is loops over Python floats - `+` and `/` on a Python float are the rounded double operations the contract names - and
`sorted` with the kernel's 64-bit key; the randomization model mixes in uint64 arrays (numpy wraps) and adds along the queries with
np.cumsum, which is a sequential loop."""
import math
import struct

import numpy as np

ORDER_SCORE, ORDER_LIST = 0, 1
MASK64 = (1 << 64) - 1


def f2ord(x):
    """The order-preserving uint32 of a float32 (csrc/common.h sr_f2ord): -0.0 is read as +0.0."""
    u = struct.unpack("<I", struct.pack("<f", float(x)))[0]
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def rank_key(score, tie, slot):
    return (f2ord(score) << 32) | (int(tie) << 16) | (0xFFFF - slot)


# ------------------------------------------------------------------------------------------------------- judgement tables ---
def qrel_tables(rows, cuts, depth):
    """rows: per query (ids ascending, grades).  -> indptr int64, ids int64, grades int32, n_rel int32, idcg float64 [nq, n_cuts],
    log2 float64 [depth], as the contract defines them."""
    indptr = np.zeros(len(rows) + 1, np.int64)
    ids, grades = [], []
    n_rel = np.zeros(len(rows), np.int32)
    idcg = np.zeros((len(rows), len(cuts)), np.float64)
    for q, (ri, rg) in enumerate(rows):
        ids.extend(int(x) for x in ri)
        grades.extend(int(x) for x in rg)
        indptr[q + 1] = len(ids)
        pos = sorted((int(g) for g in rg if g > 0), reverse=True)
        n_rel[q] = len(pos)
        for j, c in enumerate(cuts):
            s = 0.0
            for i, g in enumerate(pos[:c]):
                s = s + float(g) / math.log2(i + 2)
            idcg[q, j] = s
    log2 = np.array([math.log2(i + 2) for i in range(depth)], np.float64)
    return indptr, np.array(ids, np.int64), np.array(grades, np.int32), n_rel, idcg, log2


# ------------------------------------------------------------------------------------------------------------ the metrics ---
class EvalError(ValueError):
    pass


def eval_ranked(scores, ids, counts, tie, exclude, indptr, qrel_ids, qrel_grades, n_rel, idcg, log2, cuts, order=ORDER_SCORE, rr_depth=0):
    """-> (out float64 [nq, 1 + 4 n_cuts], flags int32 [nq], mean float64 [1 + 4 n_cuts], n evaluated).  Raises EvalError with the text
    the library's message holds for the conditions it finds on the device."""
    nq, depth = ids.shape
    nc = len(cuts)
    out = np.zeros((nq, 1 + 4 * nc), np.float64)
    flags = np.zeros(nq, np.int32)
    bad_qrel, bad_tie, bad_dup = None, None, None
    for q in range(nq):
        lo, hi = int(indptr[q]), int(indptr[q + 1])
        row_ids = [int(x) for x in qrel_ids[lo:hi]]
        if any(a >= b for a, b in zip(row_ids, row_ids[1:])) and bad_qrel is None:
            bad_qrel = q
        grade_of = dict(zip(row_ids, (int(g) for g in qrel_grades[lo:hi])))
        cnt = depth if counts is None else max(0, min(depth, int(counts[q])))
        ex = -1 if exclude is None else int(exclude[q])
        valid = [r for r in range(cnt) if ids[q, r] >= 0 and int(ids[q, r]) != ex]
        seen = set()
        for r in valid:
            d = int(ids[q, r])
            if d in grade_of:
                if d in seen and bad_dup is None:
                    bad_dup = (q, r, d)
                seen.add(d)
            if tie is not None and not 0 <= int(tie[q, r]) < 65536 and bad_tie is None:
                bad_tie = (q, r)

        def ranking(entries):
            if order == ORDER_LIST:
                return list(entries)
            return sorted(entries, key=lambda r: rank_key(scores[q, r], 0 if tie is None else int(tie[q, r]) & 0xFFFF, r), reverse=True)

        nr = int(n_rel[q])
        evaluated = hi > lo and len(valid) > 0
        flags[q] = (1 if evaluated else 0) | (2 if nr <= 0 else 0)
        if not evaluated:
            continue
        rr = 0.0
        for rank, r in enumerate(ranking(valid[:rr_depth] if rr_depth > 0 else valid), start=1):
            if grade_of.get(int(ids[q, r]), 0) > 0:
                rr = 1.0 / rank
                break
        out[q, 0] = rr
        ranked = ranking(valid)
        for j, c in enumerate(cuts):
            h, dcg, ap = 0, 0.0, 0.0
            for i, r in enumerate(ranked[:c]):
                g = grade_of.get(int(ids[q, r]), 0)
                dcg = dcg + float(max(g, 0)) / float(log2[i])
                if g > 0:
                    h += 1
                    ap = ap + float(h) / float(i + 1)
            out[q, 1 + j] = float(h) / float(nr) if nr > 0 else 0.0
            out[q, 1 + nc + j] = dcg / float(idcg[q, j]) if idcg[q, j] > 0 else 0.0
            out[q, 1 + 2 * nc + j] = float(h) / float(min(nr, c)) if nr > 0 else 0.0
            out[q, 1 + 3 * nc + j] = ap / float(nr) if nr > 0 else 0.0
    if bad_qrel is not None:
        raise EvalError(f"the judged ids of query {bad_qrel} are not strictly ascending")
    if bad_tie is not None:
        raise EvalError(f"(query {bad_tie[0]}, entry {bad_tie[1]}) is outside [0, 65536)")
    if bad_dup is not None:
        raise EvalError(f"judged id {bad_dup[2]} (query {bad_dup[0]}, entry {bad_dup[1]}) occurs twice")
    mean = np.zeros(1 + 4 * nc, np.float64)
    n = int((flags & 1).sum())
    for col in range(1 + 4 * nc):
        s = 0.0
        for q in range(nq):
            if flags[q] & 1:
                s = s + float(out[q, col])
        mean[col] = s / n if n else 0.0
    return out, flags, mean, n


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ----------------------------------------------------------------------------------------------------- randomization test ---
def mix(z):
    """The splitmix64 step on a uint64 array."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def flips(n, b0, b1, seed):
    """bool [b1 - b0, n]: the signs of permutations b0 .. b1 - 1."""
    W = (n + 63) // 64
    b = np.arange(b0, b1, dtype=np.uint64)[:, None]
    with np.errstate(over="ignore"):
        words = mix(np.uint64(seed & MASK64) + b * np.uint64(W) + np.arange(W, dtype=np.uint64)[None, :])        # [B, W]
    q = np.arange(n)
    return ((words[:, q >> 6] >> (q & 63).astype(np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def randomization(diff, n_perm, seed, chunk=1024):
    """diff float64 [n_cols, n] -> (t_obs float64 [n_cols], count_ge int64 [n_cols]).  np.cumsum adds along the queries one rounded
    add at a time, starting with the first term itself: that is +0.0 + term for every term but -0.0, and a sum that is -0.0 here is
    +0.0 on the device - the same absolute value; t_obs is normalised by `+ 0.0`."""
    diff = np.ascontiguousarray(diff, dtype=np.float64)
    n_cols, n = diff.shape
    if n == 0:
        return np.zeros(n_cols, np.float64), np.full(n_cols, n_perm, np.int64)
    t_obs = np.cumsum(diff, axis=1)[:, -1] + 0.0
    count = np.zeros(n_cols, np.int64)
    for b0 in range(0, n_perm, chunk):
        f = flips(n, b0, min(n_perm, b0 + chunk), seed)
        for c in range(n_cols):
            t = np.cumsum(np.where(f, -diff[c][None, :], diff[c][None, :]), axis=1)[:, -1]
            count[c] += int((np.abs(t) >= abs(t_obs[c])).sum())
    return t_obs, count


# ------------------------------------------------------------------------------------------------------------- generators ---
def tied_case(rng, nq, depth, n_docs, max_judged=12, ragged=True, decimals=1, neg_zero=False):
    """A run with heavy score ties (scores rounded to `decimals`), ragged lists, padding, grades in -1 .. 3, and judgement rows that
    hold documents outside the index (ids from n_docs up).  -> dict of arrays; ids are positions, drawn without replacement per row."""
    ids = np.stack([rng.choice(n_docs, size=depth, replace=False) for _ in range(nq)]).astype(np.int64) if nq else np.zeros((0, depth), np.int64)
    scores = np.round(rng.standard_normal((nq, depth)) * 0.6, decimals).astype(np.float32)
    scores = -np.sort(-scores, axis=1)
    if neg_zero and nq:
        z = scores == 0
        scores[z & (rng.random(scores.shape) < 0.5)] = np.float32(-0.0)
    counts = np.full(nq, depth, np.int32)
    if ragged and nq:
        counts = rng.integers(0, depth + 1, size=nq).astype(np.int32)
        counts[rng.integers(0, nq)] = depth
        pad = rng.random((nq, depth)) < 0.05
        ids[pad] = -1
    rows = []
    for q in range(nq):
        m = int(rng.integers(0, max_judged + 1))
        in_list = [int(x) for x in rng.permutation(ids[q][ids[q] >= 0])[:m]]
        extra = [int(x) for x in rng.choice(n_docs + 50, size=int(rng.integers(0, 4)), replace=False)]
        row = sorted(set(in_list + extra))
        rows.append((row, [int(g) for g in rng.integers(-1, 4, size=len(row))]))
    return dict(scores=scores, ids=ids, counts=counts, rows=rows)


def str_tie_keys(scores, ids, doc_key=str):
    """tie_key int32 [nq, depth]: the rank of doc_key(id) among the documents of the row that share its score (0 where none does) -
    trec_eval's docid-descending tie rule as the kernel's key takes it."""
    nq, depth = ids.shape
    tie = np.zeros((nq, depth), np.int32)
    for q in range(nq):
        groups = {}
        for r in range(depth):
            if ids[q, r] >= 0:
                groups.setdefault(float(scores[q, r]) + 0.0, []).append(r)
        for rs in groups.values():
            if len(rs) > 1:
                for rank, r in enumerate(sorted(rs, key=lambda r: doc_key(int(ids[q, r])))):
                    tie[q, r] = rank
    return tie


def run_dict(case, qid=lambda q: f"q{q}", doc_key=str):
    """{qid: {doc: score}} of a generated case in LIST order, as RunResult.to_dict() gives it (queries without a hit are absent)."""
    run = {}
    for q in range(case["ids"].shape[0]):
        docs = {doc_key(int(d)): float(s) for r, (d, s) in enumerate(zip(case["ids"][q], case["scores"][q])) if r < case["counts"][q] and d >= 0}
        if docs:
            run[qid(q)] = docs
    return run


def qrel_dict(case, qid=lambda q: f"q{q}", doc_key=str):
    return {qid(q): {doc_key(d): g for d, g in zip(*row)} for q, row in enumerate(case["rows"]) if row[0]}
