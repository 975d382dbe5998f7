"""Exact hybrid search: the certified top-k of the fused dense + sparse score over EVERY document of the dense index.

    fused(p) = f32( f32(w_d * dense(p)) + f32(w_s * sparse(p)) )        (rerank.fused_scores: two roundings, one add)

dense(p) are the bits of DenseIndexHIP.score_pairs, sparse(p) those of SparseIndexHIP.score_pairs at d2s[p] (0.0 for a document without
a posting); order: fused descending, then tie ascending (tie = sparse position, or len(s2d) + dense position without one) - the rule of
HybridRetriever.retrieve_fused.  The reference's HybridRetriever (scaling_retriever/indexer.py:859-1019) dumps the two heads' runs and
fuses nothing; retrieve_fused ranks the union of the two top-k lists, which is not the top-k of the fused score.  This module returns
that top-k exactly, for every query, by three routes (the argument is in DESIGN.md 4.17):

  first depth    both heads are searched at depths[0] >= k, the union of the two lists (sr_hybrid_union) is re-scored by both pair
                 scorers and ranked (sr_hybrid_rank).  Every document outside both lists has dense <= D and sparse <= S (the last scores
                 of the two lists), hence fused <= B = fused(D, S): the union holds the true top-k when its k-th fused score F_k > B.
  deepening      queries without that certificate are searched again, those alone, at depths[1], depths[2], ...
  range          queries still open after the last depth: the dense range search above pred(d*), d* the smallest dense score that can
                 reach F_k next to the sparse bound S, returns every outside document that could enter; those and the sparse list are
                 re-scored and ranked.  Always terminates; runs in query sub-batches under a byte budget.

Under a document bitmap (mask=, one for all queries) the same three routes run over the allowed documents alone: both heads search
under the mask (the sparse head under the bitmap carried over to its own positions, sr_doc_mask_remap), the range route is the masked
dense range search, and a dense list that holds every allowed document (depth >= their number m) is complete.  The argument holds for
the allowed set word for word: every allowed document outside both lists has dense <= D and sparse <= S.

Under per-query masks (masks= + query_group=: a bitmap per filter group and a group id per query) every query runs the
three routes over ITS group's allowed documents: both heads search under groups (search_grouped; the stacked bitmaps are carried over to
sparse positions once per call), the allowed documents are counted per group once per call and a dense list is complete when its depth
reaches the count of the query's own group, later rounds carry the pending queries' group ids, and the range route is the grouped dense
range search.  The argument holds per query: every allowed document of that query outside both of its lists has dense <= D and sparse
<= S.  For every group the rows, counts and stats are those of search_fused(mask=masks[g]) for its queries alone.

All arithmetic is in the HIP kernels; the host only moves rows between rounds.  Not offered: doc-sharded indexes, allow-lists given as
ids (build the bitmap: HybridRetriever.allowed_mask), k > sr_max_topk()."""
import contextlib

import numpy as np
import torch

from . import _lib

FLT_MAX = float(np.finfo(np.float32).max)
# device bytes the range route holds per candidate entry of a sub-batch: the hit (score 4 + id 8), the union's three int64 columns, the
# clamped sparse positions, the two pair scores - rounded up
CANDIDATE_BYTES = 64


def check_arguments(topk, weights):
    """(k, (w_d, w_s)) of a fused search, or ValueError: topk an integer >= 1, weights two finite numbers >= 0 (as fp32 too).  Touches no
    device and does not load the library."""
    try:
        k = int(topk)
        if k != topk:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"topk must be an integer >= 1, got {topk!r}") from None
    if k < 1:
        raise ValueError(f"topk must be an integer >= 1, got {topk!r}")
    try:
        with np.errstate(over="ignore"):                       # a weight beyond float32 becomes inf and is refused below
            w = tuple(float(np.float32(float(x))) for x in weights)
    except (TypeError, ValueError):
        raise ValueError(f"weights must be two numbers, got {weights!r}") from None
    if len(w) != 2 or not all(np.isfinite(x) and x >= 0.0 for x in w):
        raise ValueError(f"weights must be two finite numbers >= 0 (in float32), got {weights!r}")
    return k, w


def default_depths(k, max_topk):
    """4k, 16k, ... while <= max_topk; (k,) when even 4k is beyond it."""
    out, d = [], 4 * k
    while d <= max_topk:
        out.append(d)
        d *= 4
    return tuple(out) if out else (k,)


def _check_depths(depths, k, max_topk):
    try:
        depths = tuple(int(d) for d in depths)
    except (TypeError, ValueError):
        raise ValueError(f"depths must be a sequence of integers, got {depths!r}") from None
    if not depths or any(d < k or d > max_topk for d in depths):
        raise ValueError(f"every depth must lie in [topk, sr_max_topk()] = [{k}, {max_topk}] (the union is sorted in LDS), got {depths!r}")
    return depths


@contextlib.contextmanager
def _pair_order(dense, nq):
    """A dense search whose scores are pair-score bits (include/sr_hip.h sr_dense_score_pairs): batches of <= 64 queries with dim % 256
    == 0 accumulate in the pair scorer's order only under set_batch_invariant(True), switched on here and put back afterwards."""
    if nq <= 64 and dense.dim % 256 == 0 and not dense.batch_invariant:
        dense.set_batch_invariant(True)
        try:
            yield
        finally:
            dense.set_batch_invariant(False)
    else:
        yield


def _csr_rows(row_ptr, cols, vals, rows):
    """The CSR of the given rows (an int64 device tensor), in that order."""
    starts, lens = row_ptr[rows], row_ptr[rows + 1] - row_ptr[rows]
    out_ptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=row_ptr.device)
    out_ptr[1:] = torch.cumsum(lens, 0)
    total = int(out_ptr[-1])
    take = torch.repeat_interleave(starts - out_ptr[:-1], lens, output_size=total) + torch.arange(total, device=row_ptr.device)
    return out_ptr, cols[take], vals[take]


def _rescore_and_rank(dense, sparse, q, csr, indptr, dpos, spos, tie, w, k, D, S, complete, n_s2d):
    dense_s = dense.score_pairs(q, indptr, dpos)
    if sparse.n_docs > 0:
        sparse_s = sparse.score_pairs(csr[0], csr[1], csr[2], indptr, torch.clamp(spos, min=0))
    else:
        sparse_s = torch.zeros_like(dense_s)
    from .scoring import hybrid_rank
    return hybrid_rank(indptr, dpos, spos, tie, dense_s, sparse_s, w, k, D, S, complete, n_s2d, dense.id_end)


def search_fused(dense, sparse, d2s, s2d, dense_queries, q_row_ptr, q_cols, q_vals, topk, weights=(1.0, 1.0), depths=None,
                 fallback_bytes=1 << 30, mask=None, masks=None, query_group=None):
    """dense: DenseIndexHIP in precision "fp32" or "fp32_filtered" (ValueError otherwise: the k'-th dense score must be comparable with
    pair scores); sparse: SparseIndexHIP; d2s int64 [dense.id_end] / s2d int64 the two position maps on the device (-1: none); queries
    fp32 [nq, dim] and a CSR over the vocabulary, on the device.  depths (default 4k, 16k, ... <= sr_max_topk()): the search depths of
    the rounds, each in [topk, sr_max_topk()]; fallback_bytes: the device bytes a sub-batch of the range route may hold (a single query
    whose candidates alone exceed it: MemoryError naming it).  mask (None: every document): packed int32 / uint32 words over dense
    positions [0, dense.id_end) (scoring.pack_doc_mask), one bitmap for all queries - only documents whose bit is set are ranked; a set
    bit that names no document is a ValueError (DenseIndexHIP.search); with fewer than k allowed documents a row ends in padding and its
    count says so.  masks + query_group (not together with mask): packed words [G, W] over dense positions (scoring.pack_doc_masks), one
    bitmap per filter group, and one group id per query - query q is ranked over the documents of masks[query_group[q]] alone; a group
    without an allowed document gives padding rows with count 0 at depth 0; a group id outside [0, G) is a ValueError naming the query.
    Returns (scores fp32 [nq, k] padded with -FLT_MAX, dense positions int64
    [nq, k] padded with -1, counts int32 [nq]) as numpy arrays and stats = {"depth": int64 [nq] the index into depths at which the
    query was certified, -1 = range route; "union": int64 [nq] candidates ranked for it; "range_hits": int64 [nq]; "depths": the
    schedule} - the exact top-k of the fused score for every query, whatever route served it."""
    k, w = check_arguments(topk, weights)
    if dense.precision not in ("fp32", "fp32_filtered"):
        raise ValueError(f"search_fused needs a dense index whose search returns the exact kernel's bits (precision 'fp32' or 'fp32_filtered'), "
                         f"this one is in {dense.precision!r}")
    max_topk = int(_lib.load().sr_max_topk())
    if k > max_topk:
        raise ValueError(f"search_fused: topk = {k} is beyond sr_max_topk() = {max_topk}")
    depths = default_depths(k, max_topk) if depths is None else _check_depths(depths, k, max_topk)
    from .doc_filter import check_group_ids, mask_argument, mask_on_device, one_filter, query_group_argument
    from .scoring import doc_list_from_mask, doc_mask_remap, hybrid_union
    dev = dense.device
    one_filter("search_fused", masks, query_group, mask=mask)
    if masks is not None:
        masks, n_bits = mask_argument(masks, lambda: dense.id_end, "id_end", ndim=2)
        if n_bits is None:
            raise ValueError("search_fused takes its masks as packed int32 / uint32 words (scoring.pack_doc_masks), not as flags")
        query_group = query_group_argument(query_group, dense_queries.shape[0])
        n_groups = int(masks.shape[0])
        n_words = (n_bits + 31) // 32
        masks = mask_on_device(masks, n_bits, dev)[0].reshape(-1)[:n_groups * n_words].reshape(n_groups, n_words)      # on the device, uploaded once
        groups = (query_group if torch.is_tensor(query_group) else torch.from_numpy(np.ascontiguousarray(query_group))).to(device=dev, dtype=torch.int64)
    if mask is not None:
        mask, n_bits = mask_argument(mask, lambda: dense.id_end, "id_end")
        if n_bits is None:
            raise ValueError("search_fused takes its mask as packed int32 / uint32 words (scoring.pack_doc_mask), not as flags")
        # the words themselves on the device: the searches below resolve them again, without a copy
        mask = mask_on_device(mask, n_bits, dev)[0][:(n_bits + 31) // 32]
    q = dense_queries.to(device=dev, dtype=torch.float32).contiguous()
    row_ptr, cols, vals = (q_row_ptr.to(device=dev, dtype=torch.int64), q_cols.to(device=dev, dtype=torch.int32),
                           q_vals.to(device=dev, dtype=torch.float32))
    nq, N = q.shape[0], dense.ntotal
    if row_ptr.numel() != nq + 1:
        raise ValueError(f"{nq} dense queries, {row_ptr.numel() - 1} sparse queries")
    d2s, s2d = d2s.to(device=dev, dtype=torch.int64).contiguous(), s2d.to(device=dev, dtype=torch.int64).contiguous()
    if d2s.numel() != dense.id_end:
        raise ValueError(f"d2s holds {d2s.numel()} entries, the dense index numbers its documents in [0, {dense.id_end})")
    n_s2d = s2d.numel()
    scores = torch.full((nq, k), -FLT_MAX, dtype=torch.float32, device=dev)
    ids = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    counts = torch.zeros((nq,), dtype=torch.int32, device=dev)
    stats = {"depth": np.full(nq, -1, np.int64), "union": np.zeros(nq, np.int64), "range_hits": np.zeros(nq, np.int64), "depths": depths}

    def result():
        return scores.cpu().numpy(), ids.cpu().numpy(), counts.cpu().numpy(), stats
    if nq == 0 or N == 0:
        stats["depth"][:] = 0
        return result()
    n_allowed, sparse_mask = N, None
    if masks is not None:
        check_group_ids("search_fused", groups, n_groups)
        # m_g: counted once per call; the same filters over sparse positions, built once per call
        n_allowed = torch.tensor([doc_list_from_mask(masks[g], dense.id_end, capacity=0)[1] for g in range(n_groups)], dtype=torch.int64, device=dev)
        if sparse.n_docs > 0:
            sparse_mask = torch.stack([doc_mask_remap(masks[g], dense.id_end, s2d[:sparse.n_docs], sparse.n_docs) for g in range(n_groups)])
    if mask is not None:
        n_allowed = doc_list_from_mask(mask, dense.id_end, capacity=0)[1]      # m: counted once per call
        if n_allowed == 0:
            stats["depth"][:] = 0
            return result()
        if sparse.n_docs > 0:                                                  # the same filter over sparse positions, built once per call
            sparse_mask = doc_mask_remap(mask, dense.id_end, s2d[:sparse.n_docs], sparse.n_docs)      # an s2d shorter than n_docs: ValueError

    def store(rows, keep, out):
        scores[rows], ids[rows], counts[rows] = out[0][keep], out[1][keep], out[2][keep]

    pending = torch.arange(nq, device=dev)
    if masks is not None:                       # a group without an allowed document: padding rows, count 0, depth 0 - nothing to search
        empty = n_allowed[groups] == 0
        stats["depth"][empty.cpu().numpy()] = 0
        pending = pending[~empty]
    open_lists = None
    for depth_i, depth in enumerate(depths):
        n = pending.numel()
        if n == 0:
            break
        qs, csr = q[pending].contiguous(), _csr_rows(row_ptr, cols, vals, pending)
        kd, ks = min(depth, N), min(depth, max(1, sparse.n_docs))
        if masks is not None:
            pg = groups[pending]                                           # later rounds carry the pending queries' groups, no mask is re-uploaded
            ds, di = dense.search_grouped(qs, kd, masks, pg)               # each group's rows are those of search(mask=masks[g])
            if sparse_mask is not None:
                ss, si, sc = sparse.search_grouped(csr[0], csr[1], csr[2], ks, sparse_mask, pg, threshold=0.0)
            else:
                ss, si, sc = sparse.search(csr[0], csr[1], csr[2], ks, threshold=0.0)
            complete = kd >= n_allowed[pg]
        else:
            if mask is None:
                with _pair_order(dense, n):
                    ds, di = dense.search(qs, kd)
            else:
                ds, di = dense.search(qs, kd, mask=mask)                   # pair-score bits for every nq; padded (-FLT_MAX, -1) when m < kd
            ss, si, sc = sparse.search(csr[0], csr[1], csr[2], ks, threshold=0.0, mask=sparse_mask)
            complete = torch.full((n,), kd >= n_allowed, dtype=torch.bool, device=dev)
        D = ds[:, kd - 1].contiguous()
        S = torch.where(sc == ks, ss[:, ks - 1], torch.zeros_like(D))      # a shorter list: every document outside it scores <= 0
        indptr, dpos, spos, tie = hybrid_union(di, si, sc, s2d, d2s)
        out = _rescore_and_rank(dense, sparse, qs, csr, indptr, dpos, spos, tie, w, k, D, S, complete, n_s2d)
        certified = out[3] != 0
        rows = pending[certified]
        store(rows, certified, out)
        rows_h, lens = rows.cpu().numpy(), (indptr[1:] - indptr[:-1])[certified].cpu().numpy()
        stats["depth"][rows_h], stats["union"][rows_h] = depth_i, lens
        still = ~certified
        open_lists = (out[4][still].contiguous(), si[still].contiguous(), sc[still].contiguous())
        pending = pending[still]

    if pending.numel():
        # the range route.  Uncertified means g(D) >= F_k, so d* <= D: the dense list of the last depth lies inside the hits.
        thr, si, sc = open_lists
        qs = q[pending].contiguous()
        pg = groups[pending] if masks is not None else None
        how = (lambda a, b: dict(masks=masks, query_group=pg[a:b])) if masks is not None else (lambda a, b: dict(mask=mask))
        qs, thr, lims, total = dense.range_count(qs, thr, **how(0, pending.numel()))
        lens = (lims[1:] - lims[:-1]).cpu().numpy()
        pend_h = pending.cpu().numpy()
        need = (lens + si.shape[1]) * CANDIDATE_BYTES
        groups, g0, held = [], 0, 0
        for i in range(len(need)):
            if need[i] > fallback_bytes:
                raise MemoryError(f"search_fused: query {int(pend_h[i])} alone needs {int(need[i])} bytes on the range route ({int(lens[i])} dense "
                                  f"range hits), fallback_bytes is {int(fallback_bytes)}")
            if held + need[i] > fallback_bytes:
                groups.append((g0, i))
                g0, held = i, 0
            held += need[i]
        groups.append((g0, len(need)))
        for g0, g1 in groups:
            if len(groups) == 1:
                gq, glims = qs, lims
                _, hit_ids = dense.range_fill(qs, thr, lims, total, **how(0, pending.numel()))
            else:
                gq, gthr, glims, gtotal = dense.range_count(qs[g0:g1], thr[g0:g1], **how(g0, g1))
                _, hit_ids = dense.range_fill(gq, gthr, glims, gtotal, **how(g0, g1))
            rows = pending[g0:g1]
            csr = _csr_rows(row_ptr, cols, vals, rows)
            indptr, dpos, spos, tie = hybrid_union(hit_ids, si[g0:g1], sc[g0:g1], s2d, d2s, a_indptr=glims)
            n = g1 - g0
            zero = torch.zeros((n,), dtype=torch.float32, device=dev)
            out = _rescore_and_rank(dense, sparse, gq, csr, indptr, dpos, spos, tie, w, k, zero, zero,
                                    torch.ones((n,), dtype=torch.bool, device=dev), n_s2d)      # no certificate is needed here
            store(rows, slice(None), out)
            stats["union"][pend_h[g0:g1]] = (indptr[1:] - indptr[:-1]).cpu().numpy()
            stats["range_hits"][pend_h[g0:g1]] = lens[g0:g1]
    return result()
