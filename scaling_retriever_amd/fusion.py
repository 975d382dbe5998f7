"""Rank fusion of the hybrid retriever's two lists: the one place that knows its tie space.

The two indexes number documents independently, and `retrieve_fused` breaks ties at equal fused score by the SPARSE position, a
document without a posting after every indexed one.  scoring.rank_fuse breaks ties by id ascending, so both lists are mapped to
one id space whose order is that tie rule:

    tie = spos                   for a document with a posting (spos = d2s[dpos] >= 0)
    tie = len(s2d) + dpos        for a document without one

fused there, and mapped back to dense positions.  The maps are plain tensor code: they run on whatever device holds their inputs.
"""
import torch

from . import scoring


def dense_to_tie(dense_pos, d2s, n_s2d):
    """Dense positions (negative = padding) -> tie values; pads stay -1."""
    valid = dense_pos >= 0
    dp = torch.clamp(dense_pos, min=0)
    sp = d2s[dp]
    return torch.where(valid, torch.where(sp >= 0, sp, n_s2d + dp), torch.full_like(dense_pos, -1))


def sparse_to_tie(sparse_pos, sparse_counts, s2d):
    """Sparse positions [nq, ks] with their valid prefix per row -> tie values (a sparse position is its own tie); entries beyond the
    prefix and negative ones become -1.  A valid position that maps to no dense document: KeyError, retrieve_fused's."""
    valid = sparse_pos >= 0
    if sparse_counts is not None:
        cols = torch.arange(sparse_pos.shape[1], device=sparse_pos.device)[None, :]
        valid = valid & (cols < sparse_counts.to(device=sparse_pos.device, dtype=torch.int64)[:, None])
    sp = sparse_pos[valid]
    if bool((sp >= s2d.numel()).any()) or bool((s2d[torch.clamp(sp, max=max(0, s2d.numel() - 1))] < 0).any()):
        raise KeyError("retrieve_fused: the inverted index holds a document the dense index does not")
    return torch.where(valid, sparse_pos, torch.full_like(sparse_pos, -1))


def tie_to_dense(tie, s2d):
    """The inverse of the two maps: tie values (negative = padding) -> dense positions."""
    n_s2d = s2d.numel()
    with_posting = s2d[torch.clamp(tie, min=0, max=max(0, n_s2d - 1))]
    return torch.where(tie < 0, torch.full_like(tie, -1), torch.where(tie < n_s2d, with_posting, tie - n_s2d))


def _widen(t, width, fill):
    if t.shape[1] == width:
        return t
    return torch.cat([t, t.new_full((t.shape[0], width - t.shape[1]), fill)], 1)


def fuse_hybrid_lists(dense_pos, sparse_pos, sparse_counts, d2s, s2d, k, method="rrf", weights=(1.0, 1.0), c=60.0, dense_scores=None,
                      sparse_scores=None, return_ranks=False):
    """The two top-k lists of a hybrid retrieval, fused by rank on the device: dense_pos int64 [nq, kd] dense positions (negative =
    padding), sparse_pos int64 [nq, ks] SPARSE positions with sparse_counts [nq] valid entries per row (None: every non-negative one),
    d2s / s2d the two position maps (int64, -1 = none), all on one cuda device.  weights = (w_dense, w_sparse): the dense list is list 0.
    method "minmax" reads dense_scores / sparse_scores (fp32, shaped like the positions).  Returns what scoring.rank_fuse returns, its
    ids mapped back to DENSE positions (padding -1): ties at equal fused score break as in retrieve_fused, by sparse position, documents
    without a posting last."""
    k, _, weights, c = scoring.rank_fuse_arguments(2, k, method, weights, c)
    if method == "minmax" and (dense_scores is None or sparse_scores is None):
        raise ValueError("fuse_hybrid_lists: method 'minmax' needs dense_scores and sparse_scores")
    if dense_pos.dim() != 2 or sparse_pos.dim() != 2 or dense_pos.shape[0] != sparse_pos.shape[0]:
        raise ValueError(f"fuse_hybrid_lists: expected positions [nq, kd] and [nq, ks], got {tuple(dense_pos.shape)} and {tuple(sparse_pos.shape)}")
    dev = dense_pos.device
    d2s, s2d = d2s.to(device=dev, dtype=torch.int64), s2d.to(device=dev, dtype=torch.int64)
    tie_d = dense_to_tie(dense_pos.to(torch.int64), d2s, s2d.numel())
    tie_s = sparse_to_tie(sparse_pos.to(device=dev, dtype=torch.int64), sparse_counts, s2d)
    depth = max(tie_d.shape[1], tie_s.shape[1])
    ids = torch.stack([_widen(tie_d, depth, -1), _widen(tie_s, depth, -1)])
    scores = None
    if method == "minmax":
        scores = torch.stack([_widen(dense_scores.to(device=dev, dtype=torch.float32), depth, 0.0),
                              _widen(sparse_scores.to(device=dev, dtype=torch.float32), depth, 0.0)])
    out = scoring.rank_fuse(ids, k, scores=scores, method=method, weights=weights, c=c, return_ranks=return_ranks)
    return (out[0], tie_to_dense(out[1], s2d)) + tuple(out[2:])
