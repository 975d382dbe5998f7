"""Hits inside the groups of a collapsed search (scaling_retriever_amd/collapse.py group_hits, csrc/group_hits.hip): plain models of
the two device steps and of the definition, shared by tests/test_group_hits_host.py and tests/test_group_hits_gpu.py.

As in tests/collapse_cases.py every score here is a small integer (or one of a few special values that are compared, never added), so
what numpy computes on the CPU is the device's result bit for bit."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def member_table_model(keys):
    """collapse.member_table in numpy: (uniq_keys int32 [G] ascending, member_indptr int64 [G + 1], member_ids int64 [n]); a negative key
    belongs to no group."""
    keys = np.asarray(keys, np.int32)
    ids = np.flatnonzero(keys >= 0).astype(np.int64)
    order = np.argsort(keys[ids], kind="stable")
    uniq, sizes = np.unique(keys[ids], return_counts=True)
    indptr = np.zeros(len(uniq) + 1, np.int64)
    indptr[1:] = np.cumsum(sizes)
    return uniq.astype(np.int32), indptr, ids[order]


def members_model(slot_keys, table, keep=None):
    """sr_group_members_count / _fill in plain Python: (indptr int64 [nq * kg + 1], ids int64 [total]).  table = member_table_model(...);
    keep: None, bool [n_bits] (one mask) or bool [nq, n_bits] (the mask of every query's group)."""
    uniq, mptr, mids = table
    slot_keys = np.asarray(slot_keys, np.int32)
    nq, kg = slot_keys.shape
    indptr, out = [0], []
    for q in range(nq):
        allowed = None if keep is None else (keep if keep.ndim == 1 else keep[q])
        for j in range(kg):
            key = int(slot_keys[q, j])
            if key >= 0:
                g = int(np.searchsorted(uniq, key))
                assert g < len(uniq) and uniq[g] == key, (q, j, key)
                ids = mids[mptr[g]:mptr[g + 1]]
                out.extend(int(d) for d in ids if allowed is None or allowed[d])
            indptr.append(len(out))
    return np.array(indptr, np.int64), np.array(out, np.int64)


def ranked(scores, ids):
    """The library's top-k order of a list: score descending compared as floats (-0.0 = +0.0), then id ascending.  Returns the order."""
    return np.lexsort((np.asarray(ids, np.int64), -np.asarray(scores, np.float64)))


def segment_topm_model(scores, ids, indptr, m, threshold=None, pad_score=-FLT_MAX):
    """sr_segment_topm in plain Python: (scores fp32 [n_segs, m], ids int64 [n_segs, m], counts int32 [n_segs])."""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids, np.int64)
    n = len(indptr) - 1
    out_s = np.full((n, m), pad_score, np.float32)
    out_i = np.full((n, m), -1, np.int64)
    out_c = np.zeros(n, np.int32)
    for s in range(n):
        sc, di = scores[indptr[s]:indptr[s + 1]], ids[indptr[s]:indptr[s + 1]]
        if threshold is not None:
            take = sc > np.float32(threshold)
            sc, di = sc[take], di[take]
        order = ranked(sc, di)[:m]
        out_s[s, :len(order)] = sc[order] + np.float32(0.0)            # -0.0 reads back as +0.0
        out_i[s, :len(order)] = di[order]
        out_c[s] = len(sc)
    return out_s, out_i, out_c


def hits_model(S, keys, collapsed_keys, keep, threshold, m, pad_score=-FLT_MAX):
    """The definition applied to an exact score matrix S [nq, N]: keys int32 [N] the group key of every document, collapsed_keys int32
    [nq, k] the keys a collapsed search returned (-1: padding), keep None / bool [N] / bool [nq, N] the documents the filter allows,
    threshold None (dense) or the sparse head's.  Returns (hit_scores fp32 [nq, k, m], hit_ids int64 [nq, k, m], hit_counts int32
    [nq, k]): per slot the allowed members (with score > threshold) by (score descending, id ascending), cut to m, then padding;
    hit_counts = their number before the cut."""
    S, keys = np.asarray(S, np.float32), np.asarray(keys)
    nq, k = collapsed_keys.shape
    out_s = np.full((nq, k, m), pad_score, np.float32)
    out_i = np.full((nq, k, m), -1, np.int64)
    out_c = np.zeros((nq, k), np.int32)
    by_key = {}
    for d, g in enumerate(keys.tolist()):
        if g >= 0:
            by_key.setdefault(g, []).append(d)
    for q in range(nq):
        allowed = None if keep is None else (keep if keep.ndim == 1 else keep[q])
        for j in range(k):
            g = int(collapsed_keys[q, j])
            if g < 0:
                continue
            ids = np.array(by_key[g], np.int64)
            if allowed is not None:
                ids = ids[allowed[ids]]
            if threshold is not None:
                ids = ids[S[q, ids] > np.float32(threshold)]
            order = ids[ranked(S[q, ids], ids)][:m]
            out_s[q, j, :len(order)] = S[q, order] + np.float32(0.0)
            out_i[q, j, :len(order)] = order
            out_c[q, j] = len(ids)
    return out_s, out_i, out_c
