"""Diversified search: the argument rules of the MMR entry points, and the per-step compositions of what the
library offered before sr_dense_mmr / sr_sparse_mmr - the baselines tools/bench_mmr.py and tools/bench_mmr_sparse.py measure the kernels
against and tests/test_mmr_gpu.py / tests/test_mmr_sparse_gpu.py prove bit-identical to them.  The selection itself is
csrc/dense_mmr.hip and csrc/sparse_mmr.hip; DenseIndexHIP / SparseIndexHIP .mmr / .search_mmr (scoring.py) call it."""
import torch

from . import _lib
from .doc_filter import _to_dev, one_filter


SIM_MODES = {"ip": _lib.SR_MMR_SIM_IP, "cosine": _lib.SR_MMR_SIM_COSINE}     # the sparse head's similarities (sr_sparse_mmr)


def mmr_arguments(who, k, fetch_k, lam, allowed_masks=None, query_group=None, sim=None, **filters):
    """The one place that checks an MMR call, before anything is uploaded: 1 <= k <= fetch_k <= sr_mmr_max_candidates() (fetch_k = the
    length of a candidate row), lam in [0, 1], sim (the sparse head; None: the call has none) one of "ip" / "cosine", and the filters of
    a search (doc_filter.one_filter: one for all queries at most, or the per-group pair).  ValueError names the limit."""
    cap = int(_lib.load().sr_mmr_max_candidates())
    k, fetch_k = int(k), int(fetch_k)
    if not 1 <= k <= fetch_k:
        raise ValueError(f"{who}: k = {k} must lie in [1, fetch_k = {fetch_k}]: MMR selects among the candidates it is given")
    if fetch_k > cap:
        raise ValueError(f"{who}: fetch_k = {fetch_k} candidates per query exceed sr_mmr_max_candidates() = {cap}")
    if not 0.0 <= float(lam) <= 1.0:                 # NaN fails both comparisons
        raise ValueError(f"{who}: lambda = {lam} must lie in [0, 1]")
    if sim is not None and sim not in SIM_MODES:
        raise ValueError(f"{who}: sim = {sim!r} must be one of {sorted(SIM_MODES)}")
    one_filter(who, allowed_masks, query_group, **filters)


def _ordered_bits(x):
    """int64 image of fp32 values that orders like the floats, -0.0 equal to +0.0 (sr_f2ord of csrc/common.h)."""
    bits = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    bits = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
    return torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)


def stored_rows(index, ids):
    """Helper of the baseline below: the stored rows of the documents `ids` (int64 cuda tensor, any shape; the ids `search` returns) of a
    DenseIndexHIP, widened to fp32: [*ids.shape, dim].  A row of an id that is in no segment (padding) is zero.  One pass per segment."""
    flat = ids.reshape(-1)
    out = torch.zeros((flat.numel(), index.dim), dtype=torch.float32, device=index.device)
    for rows, (base, stride) in zip(index._segments, index._segment_ids):
        if rows.shape[0] == 0:
            continue
        r = torch.div(flat - base, stride, rounding_mode="floor")
        here = (flat >= base) & (r * stride == flat - base) & (r < rows.shape[0])
        out = torch.where(here[:, None], rows[r.clamp(0, rows.shape[0] - 1)].float(), out)      # no size comes back to the host
    return out.reshape(*ids.shape, index.dim)


def mmr_by_steps(index, cand_ids, cand_rel, k, lam=0.5, counts=None):
    """DenseIndexHIP.mmr composed from what the library had without its kernel: per pick one score_pairs call (the rows picked last as
    queries, every valid candidate as a pair) and torch operations for the maximum, the marginal value and the selection - k launches of
    the pair scorer, each with score_pairs' one host round trip, plus one synchronisation in the set-up (the positions of the valid
    entries).  Same arguments, same five tensors, the same bits."""
    dev = index.device
    ids = _to_dev(cand_ids, torch.int64, dev)
    rel = _to_dev(cand_rel, torch.float32, dev)
    nq, n = ids.shape
    mmr_arguments("mmr_by_steps", k, n, lam)
    cnt = torch.full((nq,), n, dtype=torch.int64, device=dev) if counts is None else _to_dev(counts, torch.int64, dev).clamp(0, n)
    arange = torch.arange(n, device=dev).expand(nq, n)
    valid = (arange < cnt[:, None]) & (ids >= 0)
    alive = valid
    indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    indptr[1:] = valid.sum(dim=1).cumsum(0)
    valid_at = valid.reshape(-1).nonzero().squeeze(1)
    flat_ids = ids.reshape(-1)[valid_at]
    fmax = torch.finfo(torch.float32).max
    lam_t = torch.tensor(float(lam), dtype=torch.float32, device=dev)
    mu = torch.tensor(1.0, dtype=torch.float32, device=dev) - lam_t
    lr = lam_t * rel
    m = torch.full((nq, n), float("-inf"), dtype=torch.float32, device=dev)
    out_ids = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    out_rel = torch.full((nq, k), -fmax, dtype=torch.float32, device=dev)
    out_mmr = torch.full((nq, k), -fmax, dtype=torch.float32, device=dev)
    out_pos = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    out_counts = torch.zeros(nq, dtype=torch.int32, device=dev)
    rows_q = torch.arange(nq, device=dev)
    big = torch.iinfo(torch.int64).max
    value, key = lr, rel                                        # pick 0: ordered by rel, reported as f32(lam * rel)
    for t in range(k):
        order = torch.where(alive, _ordered_bits(key), torch.full_like(ids, -1))
        first = alive & (order == order.max(dim=1, keepdim=True).values)
        first &= ids == torch.where(first, ids, torch.full_like(ids, big)).min(dim=1, keepdim=True).values
        pos = torch.where(first, arange, torch.full_like(arange, n)).min(dim=1).values
        has = pos < n
        pos = pos.clamp(max=n - 1)
        out_ids[:, t] = torch.where(has, ids[rows_q, pos], out_ids[:, t])
        out_rel[:, t] = torch.where(has, rel[rows_q, pos], out_rel[:, t])
        out_mmr[:, t] = torch.where(has, value[rows_q, pos], out_mmr[:, t])
        out_pos[:, t] = torch.where(has, pos.to(torch.int32), out_pos[:, t])
        out_counts += has.to(torch.int32)
        alive = alive & ~((arange == pos[:, None]) & has[:, None])
        if t + 1 == k:
            break
        picked = stored_rows(index, torch.where(has, ids[rows_q, pos], torch.full_like(pos, -1)))
        sim = torch.zeros(nq * n, dtype=torch.float32, device=dev)
        sim[valid_at] = index.score_pairs(picked, indptr, flat_ids)
        sim = sim.view(nq, n)
        m = torch.where(sim > m, sim, m)
        value = key = lr - mu * m
    return out_ids, out_rel, out_mmr, out_pos, out_counts


def forward_rows_of(index, docs):
    """Helper of the baseline below: the forward rows of the documents `docs` (int64 cuda [m] positions; < 0: an empty row) of a
    SparseIndexHIP as one CSR (indptr int64 [m + 1], cols int32, vals fp32), gathered with torch; one size comes back to the host."""
    indptr, cols, vals = index.forward_rows()
    at = docs.clamp(min=0)
    lens = torch.where(docs >= 0, indptr[at + 1] - indptr[at], torch.zeros_like(docs))
    out = torch.zeros(docs.numel() + 1, dtype=torch.int64, device=docs.device)
    out[1:] = lens.cumsum(0)
    total = int(out[-1])
    row = torch.repeat_interleave(torch.arange(docs.numel(), device=docs.device), lens, output_size=total)
    src = indptr[at][row] + (torch.arange(total, device=docs.device) - out[row])
    return out, cols[src], vals[src]


def sparse_mmr_by_steps(index, cand_ids, cand_rel, k, lam=0.5, counts=None, sim="cosine"):
    """SparseIndexHIP.mmr composed from what the library had without its kernel, as mmr_by_steps above: per pick the picked documents'
    forward rows are gathered into a query CSR (forward_rows_of), one score_pairs call scores every valid candidate against it, and
    torch operations take the maximum, the marginal value and the selection.  sim = "cosine": the norms are one more score_pairs call
    (every candidate with itself) and torch's fp32 sqrt / multiply / divide.  Same arguments, same five tensors, the same bits."""
    dev = index.device
    ids = _to_dev(cand_ids, torch.int64, dev)
    rel = _to_dev(cand_rel, torch.float32, dev)
    nq, n = ids.shape
    mmr_arguments("sparse_mmr_by_steps", k, n, lam, sim=sim)
    cnt = torch.full((nq,), n, dtype=torch.int64, device=dev) if counts is None else _to_dev(counts, torch.int64, dev).clamp(0, n)
    arange = torch.arange(n, device=dev).expand(nq, n)
    valid = (arange < cnt[:, None]) & (ids >= 0)
    alive = valid
    indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    indptr[1:] = valid.sum(dim=1).cumsum(0)
    valid_at = valid.reshape(-1).nonzero().squeeze(1)
    flat_ids = ids.reshape(-1)[valid_at]
    norm = torch.zeros(nq * n, dtype=torch.float32, device=dev)
    if sim == "cosine":
        own = torch.arange(flat_ids.numel() + 1, dtype=torch.int64, device=dev)
        norm[valid_at] = torch.sqrt(index.score_pairs(*forward_rows_of(index, flat_ids), own, flat_ids))
    norm = norm.view(nq, n)
    fmax = torch.finfo(torch.float32).max
    lam_t = torch.tensor(float(lam), dtype=torch.float32, device=dev)
    mu = torch.tensor(1.0, dtype=torch.float32, device=dev) - lam_t
    lr = lam_t * rel
    m = torch.full((nq, n), float("-inf"), dtype=torch.float32, device=dev)
    out_ids = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    out_rel = torch.full((nq, k), -fmax, dtype=torch.float32, device=dev)
    out_mmr = torch.full((nq, k), -fmax, dtype=torch.float32, device=dev)
    out_pos = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    out_counts = torch.zeros(nq, dtype=torch.int32, device=dev)
    rows_q = torch.arange(nq, device=dev)
    big = torch.iinfo(torch.int64).max
    value, key = lr, rel                                        # pick 0: ordered by rel, reported as f32(lam * rel)
    for t in range(k):
        order = torch.where(alive, _ordered_bits(key), torch.full_like(ids, -1))
        first = alive & (order == order.max(dim=1, keepdim=True).values)
        first &= ids == torch.where(first, ids, torch.full_like(ids, big)).min(dim=1, keepdim=True).values
        pos = torch.where(first, arange, torch.full_like(arange, n)).min(dim=1).values
        has = pos < n
        pos = pos.clamp(max=n - 1)
        out_ids[:, t] = torch.where(has, ids[rows_q, pos], out_ids[:, t])
        out_rel[:, t] = torch.where(has, rel[rows_q, pos], out_rel[:, t])
        out_mmr[:, t] = torch.where(has, value[rows_q, pos], out_mmr[:, t])
        out_pos[:, t] = torch.where(has, pos.to(torch.int32), out_pos[:, t])
        out_counts += has.to(torch.int32)
        alive = alive & ~((arange == pos[:, None]) & has[:, None])
        if t + 1 == k:
            break
        picked = forward_rows_of(index, torch.where(has, ids[rows_q, pos], torch.full_like(pos, -1)))
        s = torch.zeros(nq * n, dtype=torch.float32, device=dev)
        s[valid_at] = index.score_pairs(*picked, indptr, flat_ids)
        s = s.view(nq, n)
        if sim == "cosine":
            den = norm * norm[rows_q, pos][:, None]
            s = torch.where(den > 0, s / den, torch.zeros_like(s))
        m = torch.where(s > m, s, m)
        value = key = lr - mu * m
    return out_ids, out_rel, out_mmr, out_pos, out_counts
