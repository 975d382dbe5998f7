"""Plumbing of pair scoring: candidate lists of a run.json / jsonl file -> CSR over index positions, fused scores, ranking.

The reference re-scores a run in eval_reranker.py (input :91-105 a run.json or `{"qid", "docids"}` lines, output a run.json) by
encoding both sides of every pair again (DecoderOnlyBiDense / DecoderOnlyBiSparse .rerank_forward, modeling/llm_encoder.py:593-615).
Here the documents' vectors are read from the resident indexes (scoring.py score_pairs); this module holds what surrounds those
calls.  Nothing here touches the GPU by itself: the functions take torch tensors on whatever device they live on.
"""
import json

import numpy as np
import torch

from .utils.run_file import RunResult


def candidates_from_run(run):
    """run.json content {qid: {docid: score}} -> (qids, [docid lists]) in the file's order."""
    qids = list(run.keys())
    return qids, [list(run[q].keys()) for q in qids]


def candidates_from_jsonl(lines):
    """Lines `{"qid": ..., "docids": [...]}` (eval_reranker.py:91-105) -> (qids, [docid lists]): qids in order of first appearance,
    a qid that comes back appends to its list; duplicates inside a list and empty lists are kept."""
    qids, lists, row = [], [], {}
    for line in lines:
        if isinstance(line, (str, bytes)):
            if not line.strip():
                continue
            line = json.loads(line)
        q = str(line["qid"])
        if q not in row:
            row[q] = len(qids)
            qids.append(q)
            lists.append([])
        lists[row[q]].extend(line["docids"])
    return qids, lists


def read_candidates(run_path=None, jsonl_path=None):
    if (run_path is None) == (jsonl_path is None):
        raise ValueError("give exactly one of run_path and jsonl_path")            # eval_reranker.py:81
    if run_path is not None:
        with open(run_path) as f:
            return candidates_from_run(json.load(f))
    with open(jsonl_path) as f:
        return candidates_from_jsonl(f)


class InverseIdMap:
    """str(database id) -> index position, built once per index from its position -> id table (ids that repeat keep their first
    position)."""

    def __init__(self, ids):
        self.pos = {}
        for p, d in (ids.items() if isinstance(ids, dict) else enumerate(ids)):       # a dict: position -> id (doc_ids.pkl)
            self.pos.setdefault(str(d), p)

    def __len__(self):
        return len(self.pos)

    def get(self, doc_id, default=-1):
        return self.pos.get(str(doc_id), default)

    def positions(self, doc_id_lists):
        """[docid lists] -> (cand_indptr int64 [nq + 1], positions int64 [total]); an id the index does not hold: KeyError naming it."""
        indptr = np.zeros(len(doc_id_lists) + 1, np.int64)
        np.cumsum([len(l) for l in doc_id_lists], out=indptr[1:])
        out = np.empty(int(indptr[-1]), np.int64)
        i, pos = 0, self.pos
        for l in doc_id_lists:
            for d in l:
                p = pos.get(str(d))
                if p is None:
                    raise KeyError(f"document id {d!r} is not in the index")
                out[i] = p
                i += 1
        return indptr, out


def fused_scores(dense, sparse, weights=(1.0, 1.0)):
    """float32(w_d * dense) + float32(w_s * sparse): two fp32 roundings, then one fp32 add (fp32 tensors on any device; the
    products and the sum are separate element-wise kernels, nothing is contracted)."""
    w_d = torch.tensor(float(weights[0]), dtype=torch.float32, device=dense.device)
    w_s = torch.tensor(float(weights[1]), dtype=torch.float32, device=sparse.device)
    a = dense.to(torch.float32) * w_d
    b = sparse.to(torch.float32) * w_s
    return a + b


def rank_candidates(scores, tie_positions, cand_indptr, topk=None):
    """Rows of ragged candidates sorted by (score descending, tie position ascending), cut to topk: returns (order int64 [kept]
    = indices into the flat candidate arrays, row-major in rank order, counts int64 [nq]).  Three stable sorts, least significant
    key first."""
    dev = scores.device
    cand_indptr = cand_indptr.to(device=dev, dtype=torch.int64)
    nq = cand_indptr.numel() - 1
    lens = cand_indptr[1:] - cand_indptr[:-1]
    row = torch.repeat_interleave(torch.arange(nq, device=dev), lens)
    order = torch.sort(tie_positions.to(dev), stable=True).indices
    order = order[torch.sort(scores[order], descending=True, stable=True).indices]
    order = order[torch.sort(row[order], stable=True).indices]
    if topk is not None:
        rank = torch.arange(order.numel(), device=dev) - cand_indptr[:-1][row[order]]
        order = order[rank < int(topk)]
        lens = torch.clamp(lens, max=int(topk))
    return order, lens


def padded_rows(values, counts, pad):
    """Flat row-major values + counts [nq] -> [nq, max(count)] (numpy), `pad` in the unused slots."""
    counts = np.asarray(counts, np.int64)
    k = int(counts.max()) if counts.size else 0
    out = np.full((len(counts), k), pad, dtype=values.dtype)
    if k:
        out[np.arange(k)[None, :] < counts[:, None]] = values
    return out


def drop_repeats(scores, positions, tie_positions, cand_indptr):
    """A candidate list may name a document twice (the kernels score both, to equal bits); a run.json object holds a key once.
    Keeps one entry per (row, position): returns (scores, positions, tie_positions, cand_indptr) of the reduced lists, each row
    in ascending position order."""
    dev = scores.device
    cand_indptr = cand_indptr.to(device=dev, dtype=torch.int64)
    nq = cand_indptr.numel() - 1
    if scores.numel() == 0:
        return scores, positions, tie_positions, cand_indptr
    positions, tie_positions = positions.to(dev), tie_positions.to(dev)
    row = torch.repeat_interleave(torch.arange(nq, device=dev), cand_indptr[1:] - cand_indptr[:-1])
    span = int(positions.max()) + 1
    key, inverse = torch.unique(row * span + positions, return_inverse=True)            # sorted: by row, then position
    first = torch.full((key.numel(),), scores.numel(), dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inverse, torch.arange(scores.numel(), device=dev), reduce="amin")
    indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(torch.div(key, span, rounding_mode="floor"), minlength=nq), 0)
    return scores[first], positions[first], tie_positions[first], indptr


def ranked_run(qids, scores, positions, tie_positions, cand_indptr, doc_table, topk=None):
    """RunResult (per-query counts; `.dump()` writes the run.json) of ragged candidates: scores fp32 [total], positions int64 [total]
    into doc_table, each row sorted by (score desc, tie position asc); a document a list repeats appears once."""
    scores, positions, tie_positions, cand_indptr = drop_repeats(scores, positions, tie_positions, cand_indptr)
    order, counts = rank_candidates(scores, tie_positions, cand_indptr, topk)
    counts = counts.cpu().numpy()
    s = padded_rows(scores[order].cpu().numpy(), counts, np.float32(0))
    p = padded_rows(positions.to(scores.device)[order].cpu().numpy(), counts, np.int64(-1))
    return RunResult(qids, s, p, doc_table, counts.astype(np.int32))
