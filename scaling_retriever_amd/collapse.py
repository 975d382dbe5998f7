"""Collapsed search: the top-k distinct GROUPS of a ranking, each represented and scored by its best passage ("MaxP", field collapsing).

`keys` (int32) maps a document index - what a search returns as an id - to a group key >= 0.  For a query, take the row the search
returns with k = the number of (allowed) documents: the full ranking, score descending, ties by ascending document index (on the sparse
head only documents with score > threshold).  Remove every entry whose key occurred earlier in the row and cut to k: the top-k groups,
each represented by its best passage (among equal scores the lowest index), ordered by (best score descending, best passage's index
ascending); unused slots are padding (-FLT_MAX, -1, key -1) and counts[q] is the number of groups.

Exactness needs no margin argument, because the order on (score, id) is total: when a prefix of the full ranking already holds k
distinct keys - or is the whole ranking - its first-occurrence row equals that of the full ranking in the first k entries, since every
passage outside the prefix ranks behind everything inside it.  The device step (sr_topk_collapse, csrc/topk_collapse.hip) computes the
first-occurrence row of a prefix and that flag; the driver here deepens until every query is proven, like
hybrid.search_fused:

  rounds          the still-pending queries are searched at depths[0], depths[1], ... (default hybrid.default_depths: 4k, 16k, ...; a depth
                  may exceed sr_max_topk() - the searches take any k - and is clipped to the number of documents), the rows collapsed,
                  the completed ones copied out.
  full ranking    queries still pending after the last depth are searched with k = the number of documents, in sub-batches sized from
                  fallback_bytes, and collapsed with exhaustive=True.  Always terminates.

Collapsing post-processes rows the existing searches return, so it composes with every filter (subset=, mask=, masks= + query_group=).
All arithmetic is in the HIP kernels; the host only moves rows between rounds.  Not offered: the fused hybrid searches and the range
searches under collapse, doc-sharded indexes, k > sr_max_topk()."""
import numpy as np
import torch

from . import _lib
from .hybrid import FLT_MAX, default_depths

# device bytes the full-ranking route holds per entry of a row: the result (score 4 + id 8) and the large select's running set and
# buffers (20, include/sr_hip.h sr_dense_search / sr_sparse_search) - rounded up
ENTRY_BYTES = 40


def group_keys(labels):
    """Group labels (any hashables, one per document, in index order) -> (keys np.int32 [n], table): keys[i] is the position of
    labels[i] in `table`, the list of distinct labels in order of first appearance.  The one place where labels become the int32 keys
    of the device step; built once, on the host."""
    table, index = [], {}
    keys = np.empty(len(labels), dtype=np.int32)
    for i, label in enumerate(labels):
        g = index.get(label)
        if g is None:
            g = index[label] = len(table)
            table.append(label)
        keys[i] = g
    return keys, table


def labels_of(group_of, db_ids):
    """The group label of every document of an index whose database ids are `db_ids` (in index order): group_of is a dict on the id, a
    callable on the id, or a sequence aligned with index order (its length is checked).  A dict without an id: ValueError naming it."""
    if isinstance(group_of, dict):
        out = []
        for d in db_ids:
            if d not in group_of:
                raise ValueError(f"collapse: document id {d!r} has no group")
            out.append(group_of[d])
        return out
    if callable(group_of):
        return [group_of(d) for d in db_ids]
    labels = list(group_of)
    if len(labels) != len(db_ids):
        raise ValueError(f"collapse: a sequence of group labels is aligned with the index ({len(db_ids)} documents), got {len(labels)}")
    return labels


def key_table(group_of, db_ids):
    """(keys np.int32 [n], table) for an index whose documents, in index order, have the database ids `db_ids`: labels_of, then
    group_keys.  An entry None of db_ids is a position without a document id (the inverted index: a document without a posting); it
    gets a group of its own and is skipped when group_of is a dict or a callable (a sequence is aligned with every position)."""
    if isinstance(group_of, dict) or callable(group_of):
        known = iter(labels_of(group_of, [d for d in db_ids if d is not None]))
        labels = [next(known) if d is not None else ("\x00no-id", p) for p, d in enumerate(db_ids)]
    else:
        labels = labels_of(group_of, db_ids)
    return group_keys(labels)


def route_stats(stats):
    """The route statistics of a collapsed search as plain Python (q_stats.json): the schedule, how many queries each depth proved, how
    many took the full-ranking route, the mean number of groups returned."""
    depth = stats["depth"]
    return {"depths": [int(d) for d in stats["depths"]],
            "queries_per_depth": [int((depth == i).sum()) for i in range(len(stats["depths"]))],
            "full_ranking_queries": int((depth < 0).sum()),
            "mean_groups": float(stats["groups_seen"].mean()) if len(depth) else 0.0}


def not_under_collapse(who, collapse):
    """The searches that are not offered under collapse say so."""
    if collapse is not None:
        raise NotImplementedError(f"{who}: not offered under collapse (top-k distinct groups); collapsed search is search_collapsed / "
                                  "retrieve(collapse=) of the two heads")


def read_collapse_file(path):
    """A TSV of passage_id<TAB>group_id (empty lines ignored) -> dict passage id -> group id, both str."""
    out = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line.strip():
                continue
            parts = line.split("\t")
            if len(parts) != 2:
                raise ValueError(f"{path}:{n}: expected passage_id<TAB>group_id, got {line!r}")
            out[parts[0].strip()] = parts[1].strip()
    return out


def check_arguments(who, k, keys, depths, n_ids, clip=None):
    """(k, depths) of a collapsed search, or ValueError - before anything is uploaded: k an integer in [1, sr_max_topk()], keys a 1-D
    int32 tensor / array of n_ids() entries (asked last), every depth an integer >= k (clip: an upper limit depths are cut to)."""
    from .scoring import collapse_keys_argument
    try:
        kk = int(k)
        if kk != k:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{who}: k must be an integer >= 1, got {k!r}") from None
    if kk < 1:
        raise ValueError(f"{who}: k must be an integer >= 1, got {k!r}")
    max_topk = int(_lib.load().sr_max_topk())
    if kk > max_topk:
        raise ValueError(f"{who}: k = {kk} is beyond sr_max_topk() = {max_topk} (the groups met so far are kept in LDS)")
    collapse_keys_argument(keys)
    if depths is None:
        depths = default_depths(kk, max_topk)
    else:
        try:
            depths = tuple(int(d) for d in depths)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: depths must be a sequence of integers, got {depths!r}") from None
        if not depths or any(d < kk for d in depths):
            raise ValueError(f"{who}: every depth must be at least k = {kk}, got {depths!r}")
    if clip is not None:
        depths = tuple(min(d, clip) for d in depths)
    n = int(n_ids())
    if keys.shape[0] != n:
        raise ValueError(f"{who}: keys must hold one group key per document index ({n}), got {keys.shape[0]}")
    return kk, depths


def collapse_rounds(who, nq, k, keys, depths, device, search, full_parts, fallback_bytes):
    """The driver both heads use.  search(rows, depth) -> (scores [n, d], ids [n, d], counts [n] or None, exhaustive) for the pending
    queries `rows` (an int64 device tensor); full_parts(rows) -> [(rows of a part, n_full, fn)] with fn(rows) -> (scores, ids, counts or
    None) the whole rankings (n_full entries) of a part's queries.  Returns (scores fp32 [nq, k], ids int64 [nq, k], keys int32 [nq, k],
    counts int32 [nq]) on the device and stats."""
    from .scoring import topk_collapse
    scores = torch.full((nq, k), -FLT_MAX, dtype=torch.float32, device=device)
    ids = torch.full((nq, k), -1, dtype=torch.int64, device=device)
    gkeys = torch.full((nq, k), -1, dtype=torch.int32, device=device)
    counts = torch.zeros((nq,), dtype=torch.int32, device=device)
    stats = {"depth": np.full(nq, -1, np.int64), "groups_seen": np.zeros(nq, np.int64), "depths": depths}
    if nq == 0:
        return scores, ids, gkeys, counts, stats

    def store(rows, keep, out):
        scores[rows], ids[rows], gkeys[rows], counts[rows] = out[0][keep], out[1][keep], out[2][keep], out[3][keep]
        stats["groups_seen"][rows.cpu().numpy()] = out[3][keep].cpu().numpy()

    pending = torch.arange(nq, device=device)
    for depth_i, depth in enumerate(depths):
        if pending.numel() == 0:
            break
        s, i, c, exhaustive = search(pending, depth)
        out = topk_collapse(s, i, keys, k, counts=c, exhaustive=exhaustive)
        done = out[4] != 0
        rows = pending[done]
        store(rows, done, out)
        stats["depth"][rows.cpu().numpy()] = depth_i
        pending = pending[~done]
    if pending.numel():
        for rows, n_full, fn in full_parts(pending):
            per_query = max(1, int(n_full)) * ENTRY_BYTES
            step = int(fallback_bytes) // per_query
            if step < 1:
                raise MemoryError(f"{who}: query {int(rows[0])} alone needs {per_query} bytes on the full-ranking route ({int(n_full)} "
                                  f"documents), fallback_bytes is {int(fallback_bytes)}")
            for a in range(0, rows.numel(), step):
                sub = rows[a:a + step]
                s, i, c = fn(sub)
                store(sub, slice(None), topk_collapse(s, i, keys, k, counts=c, exhaustive=True))
    return scores, ids, gkeys, counts, stats


def dense_search_collapsed(dense, queries, k, keys, depths=None, fallback_bytes=1 << 30, subset=None, mask=None, masks=None, query_group=None):
    """DenseIndexHIP.search_collapsed (see there)."""
    from .doc_filter import _subset, doc_list_from_mask, mask_on_device, one_filter, query_group_argument
    who = "search_collapsed"
    if dense.precision not in ("fp32", "fp32_filtered"):
        raise ValueError(f"{who} needs a dense index whose search returns the exact kernel's bits (precision 'fp32' or 'fp32_filtered'), "
                         f"this one is in {dense.precision!r}")
    one_filter(who, masks, query_group, subset=subset, mask=mask)
    grouped = masks is not None
    k, depths = check_arguments(who, k, keys, depths, lambda: dense.id_end, clip=int(_lib.load().sr_max_topk()) if grouped else None)
    if mask is not None:
        mask = dense._mask(mask)
    if grouped:
        masks = dense._mask(masks, ndim=2)
        query_group = query_group_argument(query_group, dense._check_queries(queries))
    q = dense._queries(queries)
    dev, nq, N = dense.device, q.shape[0], dense.ntotal
    keys = keys if torch.is_tensor(keys) else torch.from_numpy(np.ascontiguousarray(keys))
    keys = keys.to(dev).contiguous()
    # everything a filter needs on the device, once per call: later rounds carry the pending queries' rows, nothing is re-uploaded
    n_allowed, how = N, {}
    if subset is not None:
        subset, n_allowed = _subset(subset, dev)
        subset = subset[:n_allowed]
        how = dict(subset=subset)
    elif mask is not None:
        words, n_bits = mask_on_device(*mask, dev)
        if n_bits != dense.id_end:
            raise ValueError(f"a mask of this index holds {dense.id_end} flags (id_end), got {n_bits}")
        words = words[:(n_bits + 31) // 32]
        n_allowed = doc_list_from_mask(words, n_bits, capacity=0)[1]
        how = dict(mask=words)
    elif grouped:
        n_groups = int(masks[0].shape[0])
        words, n_bits = mask_on_device(*masks, dev)
        if n_bits != dense.id_end:
            raise ValueError(f"masks of this index hold {dense.id_end} flags per group (id_end), got {n_bits}")
        words = words.reshape(-1)[:n_groups * ((n_bits + 31) // 32)].reshape(n_groups, (n_bits + 31) // 32)
        groups = (query_group if torch.is_tensor(query_group) else torch.from_numpy(np.ascontiguousarray(query_group))).to(device=dev, dtype=torch.int64)
        bad = torch.nonzero((groups < 0) | (groups >= n_groups))
        if bad.numel():
            raise ValueError(f"{who}: query {int(bad[0])} is in group {int(groups[int(bad[0])])}, outside [0, {n_groups})")

    def search(rows, depth):
        qs = q[rows].contiguous()
        if grouped:
            d = max(1, min(depth, N))
            return (*dense.search_grouped(qs, d, words, groups[rows]), None, False)       # a group's shorter ranking shows as padding
        d = max(1, min(depth, n_allowed))
        return (*dense.search(qs, d, **how), None, d >= n_allowed)

    def full_parts(rows):
        if not grouped:
            return [(rows, n_allowed, lambda sub: (*dense.search(q[sub].contiguous(), max(1, n_allowed), **how), None))]
        parts, pg = [], groups[rows]
        for g in torch.unique(pg).tolist():                                               # group by group, under that group's bitmap
            m = doc_list_from_mask(words[g], n_bits, capacity=0)[1]
            parts.append((rows[pg == g], m, lambda sub, g=g, m=m: (*dense.search(q[sub].contiguous(), max(1, m), mask=words[g]), None)))
        return parts

    if N == 0:                                  # nothing to rank: padding rows, count 0, depth 0
        out = collapse_rounds(who, nq, k, keys, (), dev, search, lambda rows: [], fallback_bytes)
        out[4]["depth"][:], out[4]["depths"] = 0, depths
        return out
    was_invariant = dense.batch_invariant
    if not was_invariant:
        dense.set_batch_invariant(True)
    try:
        return collapse_rounds(who, nq, k, keys, depths, dev, search, full_parts, fallback_bytes)
    finally:
        if not was_invariant:
            dense.set_batch_invariant(False)


def sparse_search_collapsed(sparse, q_indptr, q_cols, q_vals, k, keys, threshold=0.0, id_base=0, id_stride=1, depths=None,
                            fallback_bytes=1 << 30, subset=None, mask=None, masks=None, query_group=None):
    """SparseIndexHIP.search_collapsed (see there)."""
    from .doc_filter import _subset, mask_argument, mask_on_device, one_filter, query_group_argument
    from .hybrid import _csr_rows
    who = "search_collapsed"
    one_filter(who, masks, query_group, subset=subset, mask=mask)
    grouped = masks is not None
    N = sparse.n_docs
    id_base, id_stride = int(id_base), int(id_stride)
    k, depths = check_arguments(who, k, keys, depths, lambda: (id_base + (N - 1) * id_stride + 1) if N > 0 else 0)
    if mask is not None:
        mask = sparse._mask(mask)
    if grouped:
        masks = mask_argument(masks, lambda: N, "n_docs", ndim=2)
        query_group = query_group_argument(query_group, len(q_indptr) - 1)
    dev = sparse.device
    (row_ptr, cols, vals), nq = sparse._query_csr(q_indptr, q_cols, q_vals)
    keys = keys if torch.is_tensor(keys) else torch.from_numpy(np.ascontiguousarray(keys))
    keys = keys.to(dev).contiguous()
    how = {}
    if subset is not None:
        subset, m = _subset(subset, dev)
        how = dict(subset=subset[:m])
    elif mask is not None:
        words, n_bits = mask_on_device(*mask, dev)
        if n_bits != N:
            raise ValueError(f"a mask of this index holds {N} flags (n_docs), got {n_bits}")
        how = dict(mask=words[:(n_bits + 31) // 32])
    elif grouped:
        n_groups = int(masks[0].shape[0])
        words, n_bits = mask_on_device(*masks, dev)
        if n_bits != N:
            raise ValueError(f"masks of this index hold {N} flags per group (n_docs), got {n_bits}")
        words = words.reshape(-1)[:n_groups * ((n_bits + 31) // 32)].reshape(n_groups, (n_bits + 31) // 32)
        groups = (query_group if torch.is_tensor(query_group) else torch.from_numpy(np.ascontiguousarray(query_group))).to(device=dev, dtype=torch.int64)
    ids_kw = dict(threshold=float(threshold), id_base=id_base, id_stride=id_stride)

    def run(rows, d):
        csr = _csr_rows(row_ptr, cols, vals, rows)
        if grouped:
            return sparse.search_grouped(csr[0], csr[1], csr[2], d, words, groups[rows], **ids_kw)
        return sparse.search(csr[0], csr[1], csr[2], d, **ids_kw, **how)

    def search(rows, depth):
        d = max(1, min(depth, N))
        return (*run(rows, d), d >= N)

    def full_parts(rows):
        return [(rows, N, lambda sub: run(sub, max(1, N)))]

    return collapse_rounds(who, nq, k, keys, depths, dev, search, full_parts, fallback_bytes)
