"""Pseudo-relevance feedback: the argument rules of the Rocchio entry points, and the per-step compositions of what
the library offered before sr_sparse_feedback / sr_dense_feedback - the baselines tools/bench_prf.py measures the kernels against and
tests/test_prf_gpu.py proves bit-identical to them.  The kernels are csrc/prf.hip; scoring.sparse_feedback, SparseIndexHIP.feedback /
search_prf and DenseIndexHIP.feedback / search_prf (scoring.py) call them.

The definition (include/sr_hip.h): v = the valid, non-padding entries of a feedback row in list order, the positive set its first
p = min(n_pos, |v|), the negative set its last g = min(n_neg, |v| - p); cp = f32(beta / f32(p)), cn = f32(gamma / f32(g));
w_t = f32(f32(alpha * q_t) + f32(cp * P_t)), then f32(w_t - f32(cn * N_t)), P_t / N_t summed in list order from +0.0f."""
import numpy as np
import torch

from . import _lib
from .doc_filter import _to_dev, one_filter

MAX_SET = 64            # n_pos, n_neg: the coefficient tables of csrc/prf.hip


def prf_arguments(who, n_pos, n_neg, alpha, beta, gamma, max_terms=0, depth=None, first_round=False, fb_depth=None, allowed_masks=None,
                  query_group=None, **filters):
    """The one place that checks a feedback call, before anything is uploaded: 1 <= n_pos <= 64, 0 <= n_neg <= 64, alpha / beta / gamma
    finite and >= 0, max_terms >= 0 (0 = no limit), depth (the length of a feedback row) in [1, sr_max_topk()]; first_round (search_prf):
    fb_depth, the depth of the first round (None = n_pos), obeys the rule of depth and must hold n_pos + n_neg entries when there is a
    negative set; the filters of a search (doc_filter.one_filter).  ValueError names the limit.  Returns the depth of the first round
    (None without first_round)."""
    n_pos, n_neg = int(n_pos), int(n_neg)
    if not 1 <= n_pos <= MAX_SET:
        raise ValueError(f"{who}: n_pos = {n_pos} must lie in [1, {MAX_SET}]: the positive set is the head of the feedback list")
    if not 0 <= n_neg <= MAX_SET:
        raise ValueError(f"{who}: n_neg = {n_neg} must lie in [0, {MAX_SET}] (0 = no negative set)")
    for name, value in (("alpha", alpha), ("beta", beta), ("gamma", gamma)):
        if not 0.0 <= float(value) <= float(np.finfo(np.float32).max):        # NaN fails both comparisons; the kernels take fp32
            raise ValueError(f"{who}: {name} = {value} must be finite and >= 0")
    if int(max_terms) < 0:
        raise ValueError(f"{who}: max_terms = {max_terms} must be >= 0 (0 = no limit)")
    cap = int(_lib.load().sr_max_topk())
    first = None
    if first_round:
        first = n_pos if fb_depth is None else int(fb_depth)
        if n_neg > 0 and first < n_pos + n_neg:
            raise ValueError(f"{who}: fb_depth = {first} must be >= n_pos + n_neg = {n_pos + n_neg}: the negative set is the tail of "
                             "the first round")
    for name, value in (("depth", depth), ("fb_depth", first)):
        if value is not None and not 1 <= int(value) <= cap:
            raise ValueError(f"{who}: {name} = {value} must lie in [1, sr_max_topk() = {cap}]")
    one_filter(who, allowed_masks, query_group, **filters)
    return first


def feedback_depth(fb_ids):
    """The depth of a feedback argument (tensor, array or nested list [nq, depth]) without moving it; ValueError unless it is 2-D."""
    shape = tuple(fb_ids.shape) if hasattr(fb_ids, "shape") else np.shape(fb_ids)
    if len(shape) != 2:
        raise ValueError(f"expected fb_ids int64 [nq, depth], got {shape}")
    return int(shape[1])


def coefficient_tables(beta, gamma):
    """(cp, cn) fp32 [64]: cp[p - 1] = f32(beta) / f32(p), cn[g - 1] = f32(gamma) / f32(g) as fp32 divisions - the tables sr_sparse_feedback
    and sr_dense_feedback compute on the host."""
    n = np.arange(1, MAX_SET + 1, dtype=np.float32)
    return np.float32(beta) / n, np.float32(gamma) / n


def _feedback_lists(fb_ids, counts, n_pos, n_neg, dev):
    """(vlist int64 [nq, depth]: the valid entries of every row first, in list order; p, g, nv int64 [nq])."""
    ids = _to_dev(fb_ids, torch.int64, dev)
    if ids.dim() != 2:
        raise ValueError(f"expected fb_ids int64 [nq, depth], got {tuple(ids.shape)}")
    nq, depth = ids.shape
    cnt = torch.full((nq,), depth, dtype=torch.int64, device=dev) if counts is None else _to_dev(counts, torch.int64, dev).clamp(0, depth)
    if cnt.dim() != 1 or cnt.numel() != nq:
        raise ValueError(f"expected {nq} counts, got {tuple(cnt.shape)}")
    valid = (torch.arange(depth, device=dev).expand(nq, depth) < cnt[:, None]) & (ids >= 0)
    order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)
    vlist = torch.where(torch.gather(valid, 1, order), torch.gather(ids, 1, order), torch.full_like(ids, -1))
    nv = valid.sum(dim=1)
    p = nv.clamp(max=int(n_pos))
    g = (nv - p).clamp(max=int(n_neg))
    return vlist, p, g, nv


def _apply(q, P, N, p, g, alpha, beta, gamma):
    """The formula on dense fp32 buffers [rows, width], one rounded operation per torch call (eager torch contracts nothing)."""
    dev = q.device
    cp_tab, cn_tab = (torch.from_numpy(t).to(dev) for t in coefficient_tables(beta, gamma))
    w = torch.tensor(float(alpha), dtype=torch.float32, device=dev) * q
    cp = cp_tab[(p - 1).clamp(min=0)][:, None]
    w = torch.where((p > 0)[:, None], w + cp * P, w)
    if N is not None:
        cn = cn_tab[(g - 1).clamp(min=0)][:, None]
        w = torch.where((g > 0)[:, None], w - cn * N, w)
    return w


def sparse_feedback_by_steps(q_indptr, q_cols, q_vals, doc_indptr, doc_cols, doc_vals, n_terms, fb_ids, counts=None, n_pos=10, n_neg=0,
                             alpha=1.0, beta=0.75, gamma=0.0, max_terms=128, fallback_bytes=1 << 30):
    """scoring.sparse_feedback composed from what the library had without its kernel: per document rank one gather-add of that rank's
    rows into dense [rows, V] P / N buffers (the (row, term) pairs of one rank are distinct, so the add is one rounded fp32 add in list
    order), in query sub-batches whose three buffers fit fallback_bytes; then the formula in torch, the clamp to w > 0 and
    sparse_reps_to_csr(., max_terms).  Same arguments, the same three tensors, the same bits."""
    from .indexer import sparse_reps_to_csr
    dev = doc_vals.device
    V = int(n_terms)
    q_indptr = _to_dev(q_indptr, torch.int64, dev)
    q_cols = _to_dev(q_cols, torch.int32, dev).long()
    q_vals = _to_dev(q_vals, torch.float32, dev)
    nq = q_indptr.numel() - 1
    vlist, p, g, nv = _feedback_lists(fb_ids, counts, n_pos, n_neg, dev)
    depth = vlist.shape[1]
    prf_arguments("sparse_feedback_by_steps", n_pos, n_neg, alpha, beta, gamma, max_terms, depth=vlist.shape[1])
    n_docs = doc_indptr.numel() - 1
    if bool((vlist >= n_docs).any()):
        raise ValueError(f"sparse_feedback_by_steps: a feedback id is not a position in [0, {n_docs})")
    q_rows = torch.repeat_interleave(torch.arange(nq, device=dev), q_indptr[1:] - q_indptr[:-1], output_size=q_cols.numel())
    if q_cols.numel():
        same_row = q_rows[1:] == q_rows[:-1]
        if bool((same_row & (q_cols[1:] <= q_cols[:-1])).any()) or bool(((q_cols < 0) | (q_cols >= V)).any()):
            raise ValueError(f"sparse_feedback_by_steps: query columns must be strictly ascending inside [0, {V})")

    def gather_add(buf, docs, use):
        docs = torch.where(use, docs, torch.zeros_like(docs))
        start = doc_indptr[docs]
        lens = torch.where(use, doc_indptr[docs + 1] - start, torch.zeros_like(start))
        total = int(lens.sum())
        if total == 0:
            return
        rows = torch.repeat_interleave(torch.arange(docs.numel(), device=dev), lens, output_size=total)
        first = torch.cumsum(lens, 0) - lens
        src = start[rows] + (torch.arange(total, device=dev) - first[rows])
        buf.index_put_((rows, doc_cols[src].long()), doc_vals[src], accumulate=True)

    step = max(1, int(fallback_bytes) // (3 * 4 * V))
    parts = []
    for r0 in range(0, nq, step):
        r1 = min(nq, r0 + step)
        n = r1 - r0
        Q = torch.zeros((n, V), dtype=torch.float32, device=dev)
        a, b = int(q_indptr[r0]), int(q_indptr[r1])
        Q[q_rows[a:b] - r0, q_cols[a:b]] = q_vals[a:b]
        P = torch.zeros((n, V), dtype=torch.float32, device=dev)
        for j in range(min(int(n_pos), depth)):
            gather_add(P, vlist[r0:r1, j], j < p[r0:r1])
        N = None
        if int(n_neg) > 0:
            N = torch.zeros((n, V), dtype=torch.float32, device=dev)
            for j in range(min(int(n_neg), depth)):
                at = ((nv - g)[r0:r1] + j).clamp(max=depth - 1)            # the negative set starts at entry |v| - g of v
                gather_add(N, torch.gather(vlist[r0:r1], 1, at[:, None])[:, 0], j < g[r0:r1])
        w = _apply(Q, P, N, p[r0:r1], g[r0:r1], alpha, beta, gamma)
        w = torch.where(w > 0, w, torch.zeros_like(w))
        parts.append(sparse_reps_to_csr(w, max_terms))
    if not parts:
        return (torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev))
    indptr, base = [parts[0][0][:1]], 0
    for rp, _, _ in parts:
        indptr.append(rp[1:] + base)
        base += int(rp[-1])
    return torch.cat(indptr), torch.cat([c for _, c, _ in parts]), torch.cat([v for _, _, v in parts])


def dense_feedback_by_steps(index, queries, fb_ids, counts=None, n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0):
    """DenseIndexHIP.feedback composed from what the library had without its kernel: per document rank the stored rows of that rank
    (mmr.stored_rows, widened to fp32) added to dense [nq, dim] P / N buffers in list order, then the formula in torch.  The same
    tensor, the same bits.  An id the index does not hold is not found here (its row reads as zero)."""
    from .mmr import stored_rows
    dev = index.device
    vlist, p, g, nv = _feedback_lists(fb_ids, counts, n_pos, n_neg, dev)
    prf_arguments("dense_feedback_by_steps", n_pos, n_neg, alpha, beta, gamma, depth=vlist.shape[1])
    queries = index._queries(queries)
    depth = vlist.shape[1]
    P = torch.zeros_like(queries)
    for j in range(min(int(n_pos), depth)):
        use = j < p
        P = torch.where(use[:, None], P + stored_rows(index, torch.where(use, vlist[:, j], torch.full_like(p, -1))), P)
    N = None
    if int(n_neg) > 0:
        N = torch.zeros_like(queries)
        for j in range(min(int(n_neg), depth)):
            use = j < g
            at = (nv - g + j).clamp(max=depth - 1)
            docs = torch.gather(vlist, 1, at[:, None])[:, 0]
            N = torch.where(use[:, None], N + stored_rows(index, torch.where(use, docs, torch.full_like(p, -1))), N)
    return _apply(queries, P, N, p, g, alpha, beta, gamma)
