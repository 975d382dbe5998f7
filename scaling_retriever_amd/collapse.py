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
searches under collapse, doc-sharded indexes, k > sr_max_topk().

Hits inside the groups (hits=m of the two drivers): for every returned group its up to m best passages - the members
of the group that the call's filter allows for the query, on the sparse head with score > threshold, in the same (score, id) order,
scored by the head's pair scorer.  member_table inverts `keys` once (torch's stable sort on the device); group_hits runs
sr_group_members_count -> _fill -> score_pairs -> sr_segment_topm (csrc/group_hits.hip) in query sub-batches sized from fallback_bytes
by the count pass's totals (PAIR_BYTES per pair); pack_hits turns the ragged [k, m] block into the left-aligned rows the run writer
takes.  Without hits= nothing here runs and every call returns what it returned before."""
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


def member_table(keys, device=None):
    """The inverse of a key table, the input of group_hits: (uniq_keys int32 [G] strictly ascending, member_indptr int64 [G + 1],
    member_ids int64 [n]) on `device` (None: where keys live) - the documents of group uniq_keys[g] are member_ids[member_indptr[g] :
    member_indptr[g + 1]], ascending.  keys (int32 tensor / array) is indexed in the numbering the head's bitmaps and pair scorer use:
    the dense head's global document index (what its search returns), the sparse head's document POSITION (for a sparse search with
    id_base / id_stride: keys[id_base + id_stride * arange(n_docs)]).  A negative key is an index without a document and belongs to
    no group.  Built with torch's stable sort where the keys are - plumbing, no arithmetic; build it once per key table and pass it as
    members= when many calls share it."""
    from .scoring import collapse_keys_argument
    keys = collapse_keys_argument(keys)
    keys = keys if torch.is_tensor(keys) else torch.from_numpy(np.ascontiguousarray(keys))
    if device is not None:
        keys = keys.to(device)
    ids = torch.nonzero(keys >= 0).reshape(-1)                      # ascending
    by_key, order = torch.sort(keys[ids], stable=True)              # stable: ids stay ascending inside a group
    uniq, sizes = torch.unique_consecutive(by_key, return_counts=True)
    indptr = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=keys.device)
    indptr[1:] = torch.cumsum(sizes, 0)
    return uniq.to(torch.int32).contiguous(), indptr, ids[order].contiguous()


# device bytes group_hits holds per (query, member) pair of a sub-batch: the member's id in the head's numbering (8) and its score (4) -
# the materialised pair list - and the id in the caller's numbering where a strided sparse search renames it (8); rounded up for the
# per-slot offsets (8 per slot) and the [slots, m] result, which do not grow with the group sizes
PAIR_BYTES = 24


def hits_stats(stats, hit_counts, gkeys, m):
    """stats of a collapsed search + "mean_hits": the mean number of hits RETURNED (at most m) per returned group."""
    valid = gkeys >= 0
    n = int(valid.sum())
    stats["mean_hits"] = float(hit_counts.clamp(max=m)[valid].sum()) / n if n else 0.0
    return stats


def group_hits(head, queries, slot_keys, members, m, filt=None, threshold=None, id_base=0, id_stride=1, fallback_bytes=1 << 30,
               who="group_hits"):
    """The top-m passages inside every group of a collapsed result ("inner hits") - the driver both heads share.
    head: a DenseIndexHIP (queries: its contiguous fp32 cuda [nq, dim] tensor) or a SparseIndexHIP (queries: the (indptr, cols, vals) CSR
    on its device); slot_keys int32 cuda [nq, kg], the keys search_collapsed returned (-1: padding); members: member_table(...) in the
    head's numbering; filt: None, (words int32 [W], n_bits) or (words int32 [G, W], n_bits, query_group [nq]) - the call's filter as
    bitmaps in that numbering.

    The hits of (q, slot j) are the members of the slot's group that the filter allows for q - on the sparse head (threshold given) only
    those with score > threshold - ordered by (score descending as floats, id ascending) and cut to m.  Returns (hit_scores fp32
    [nq, kg, m], hit_ids int64 [nq, kg, m], hit_counts int32 [nq, kg]): min(hit_counts, m) entries of a list are hits, the rest the
    head's padding (dense (-FLT_MAX, -1), sparse (0, -1)); hit_counts is the number of hits before the cut, 0 for a padding slot.
    Every score is the head's score_pairs of that pair, bit for bit.

    Steps, all on the device: sr_group_members_count over all queries; then per sub-batch of queries sr_group_members_fill, the head's
    score_pairs, sr_segment_topm.  A sub-batch is as many consecutive queries as have at most fallback_bytes / PAIR_BYTES pairs by the
    count's totals; a list is selected whole inside its sub-batch, so the bytes do not depend on the cut.  A query whose pairs alone do not
    fit: MemoryError naming it."""
    from .hybrid import _csr_rows
    from .scoring import SparseIndexHIP, group_members_count, group_members_fill, hits_argument, segment_topm
    m = hits_argument(who, m)
    sparse = isinstance(head, SparseIndexHIP)
    dev = slot_keys.device
    nq, kg = slot_keys.shape
    pad = 0.0 if sparse else -FLT_MAX
    out_s = torch.full((nq, kg, m), pad, dtype=torch.float32, device=dev)
    out_i = torch.full((nq, kg, m), -1, dtype=torch.int64, device=dev)
    out_c = torch.zeros((nq, kg), dtype=torch.int32, device=dev)
    if nq * kg == 0:
        return out_s, out_i, out_c
    slot_keys = slot_keys.contiguous()
    indptr, _ = group_members_count(slot_keys, members, filt)
    per_query = (indptr[kg::kg] - indptr[:-1:kg]).cpu().numpy()             # pairs of every query: nq words to the host
    budget = int(fallback_bytes) // PAIR_BYTES
    q0 = 0
    while q0 < nq:
        if per_query[q0] > budget:
            raise MemoryError(f"{who}: query {q0} alone needs {int(per_query[q0]) * PAIR_BYTES} bytes for its {int(per_query[q0])} (query, "
                              f"group member) pairs, fallback_bytes is {int(fallback_bytes)}")
        q1, pairs = q0, 0
        while q1 < nq and pairs + per_query[q1] <= budget:
            pairs += int(per_query[q1])
            q1 += 1
        sub_ptr = indptr[q0 * kg:q1 * kg + 1] - indptr[q0 * kg]
        sub_filt = filt if filt is None or len(filt) < 3 or filt[2] is None else (filt[0], filt[1], filt[2][q0:q1])
        ids = group_members_fill(slot_keys[q0:q1], members, sub_ptr, pairs, sub_filt)
        cand_ptr = sub_ptr[::kg].contiguous()
        if sparse:
            csr = _csr_rows(*queries, torch.arange(q0, q1, device=dev))
            scores = head.score_pairs(csr[0], csr[1], csr[2], cand_ptr, ids)
        else:
            scores = head.score_pairs(queries[q0:q1], cand_ptr, ids)
        s, i, c = segment_topm(scores, ids, sub_ptr, m, threshold=threshold, pad_score=pad)
        out_s[q0:q1], out_i[q0:q1], out_c[q0:q1] = s.view(-1, kg, m), i.view(-1, kg, m), c.view(-1, kg)
        q0 = q1
    if sparse and (int(id_base) != 0 or int(id_stride) != 1):
        out_i = torch.where(out_i >= 0, int(id_base) + out_i * int(id_stride), out_i)
    return out_s, out_i, out_c


def pack_hits(hit_scores, hit_ids, hit_counts):
    """The ragged [nq, k, m] block of a hits result as left-aligned rows, on the device: (scores fp32 [nq, k * m], ids int64 [nq, k * m],
    counts int32 [nq]) - per query the hits of its groups in (group rank, hit rank) order, counts[q] of them, the rest (0, -1).  What the
    run writer takes for the passage-level run of a collapsed retrieval."""
    nq, k, m = hit_scores.shape
    dev = hit_scores.device
    valid = (torch.arange(m, device=dev)[None, None, :] < hit_counts.clamp(max=m)[:, :, None]).reshape(nq, k * m)
    order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)          # the hits first, in their order
    scores = torch.gather(hit_scores.reshape(nq, k * m), 1, order)
    ids = torch.gather(hit_ids.reshape(nq, k * m), 1, order)
    counts = valid.sum(1).to(torch.int32)
    rest = torch.arange(k * m, device=dev)[None, :] >= counts[:, None]
    return scores.masked_fill(rest, 0.0), ids.masked_fill(rest, -1), counts


def hits_of_no_collapse(who, hits, collapse):
    """hits= asks for the passages inside the groups of a collapsed search: without collapse= there are none."""
    if hits is not None and collapse is None:
        raise ValueError(f"{who}: hits= are the passages inside the groups of a collapsed search; pass collapse= as well")


def _with_hits(out, hits):
    """(scores, ids, keys, counts, stats) of a collapsed search + the hits tuple and its statistic."""
    hits_stats(out[4], hits[2], out[2], hits[0].shape[2])
    return (*out, hits)


def dense_search_collapsed(dense, queries, k, keys, depths=None, fallback_bytes=1 << 30, subset=None, mask=None, masks=None, query_group=None,
                           hits=None, members=None):
    """DenseIndexHIP.search_collapsed (see there)."""
    from .doc_filter import _subset, check_group_ids, doc_list_from_mask, doc_mask_from_list, mask_on_device, one_filter, query_group_argument
    from .scoring import hits_argument, member_table_argument
    who = "search_collapsed"
    if dense.precision not in ("fp32", "fp32_filtered"):
        raise ValueError(f"{who} needs a dense index whose search returns the exact kernel's bits (precision 'fp32' or 'fp32_filtered'), "
                         f"this one is in {dense.precision!r}")
    one_filter(who, masks, query_group, subset=subset, mask=mask)
    if hits is not None:
        hits = hits_argument(who, hits)
    if members is not None:
        members = member_table_argument(members)
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
        check_group_ids(who, groups, n_groups)

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

    def with_hits(out):
        """The hits of the groups just returned, under the call's filter as a bitmap over [0, id_end)."""
        if hits is None:
            return out
        filt = None
        if subset is not None:
            filt = (doc_mask_from_list(subset, dense.id_end, dev), dense.id_end)
        elif mask is not None:
            filt = (words, n_bits)
        elif grouped:
            filt = (words, n_bits, groups)
        table = member_table(keys) if members is None else members
        return _with_hits(out, group_hits(dense, q, out[2], table, hits, filt=filt, fallback_bytes=fallback_bytes, who=who))

    if N == 0:                                  # nothing to rank: padding rows, count 0, depth 0
        out = collapse_rounds(who, nq, k, keys, (), dev, search, lambda rows: [], fallback_bytes)
        out[4]["depth"][:], out[4]["depths"] = 0, depths
        return with_hits(out)
    was_invariant = dense.batch_invariant
    if not was_invariant:
        dense.set_batch_invariant(True)
    try:
        return with_hits(collapse_rounds(who, nq, k, keys, depths, dev, search, full_parts, fallback_bytes))
    finally:
        if not was_invariant:
            dense.set_batch_invariant(False)


def sparse_search_collapsed(sparse, q_indptr, q_cols, q_vals, k, keys, threshold=0.0, id_base=0, id_stride=1, depths=None,
                            fallback_bytes=1 << 30, subset=None, mask=None, masks=None, query_group=None, hits=None, members=None):
    """SparseIndexHIP.search_collapsed (see there)."""
    from .doc_filter import _subset, doc_mask_from_list, mask_argument, mask_on_device, one_filter, query_group_argument
    from .hybrid import _csr_rows
    from .scoring import hits_argument, member_table_argument
    who = "search_collapsed"
    one_filter(who, masks, query_group, subset=subset, mask=mask)
    if hits is not None:
        hits = hits_argument(who, hits)
    if members is not None:
        members = member_table_argument(members)
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

    out = collapse_rounds(who, nq, k, keys, depths, dev, search, full_parts, fallback_bytes)
    if hits is None:
        return out
    # the hits of the groups just returned: members, bitmaps and the pair scorer number documents by POSITION; ids go out renamed
    filt = None
    if subset is not None:
        filt = (doc_mask_from_list(how["subset"], N, dev), N)
    elif mask is not None:
        filt = (how["mask"], N)
    elif grouped:
        filt = (words, N, groups)
    table = members
    if table is None:
        table = member_table(keys[id_base + id_stride * torch.arange(N, device=dev)] if (id_base, id_stride) != (0, 1) else keys)
    return _with_hits(out, group_hits(sparse, (row_ptr, cols, vals), out[2], table, hits, filt=filt, threshold=float(threshold), id_base=id_base,
                                      id_stride=id_stride, fallback_bytes=fallback_bytes, who=who))
