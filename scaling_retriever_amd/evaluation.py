"""Evaluation from the result arrays: trec-style ranking metrics and the paired randomization test on the device.

utils/metrics.py works on {qid: {docid: score}} dicts and sorts every query's hits once per cutoff; behind a Dev-sized search that is the
longest step of a run.  Here the judgements become arrays once (`Qrels`), a run is evaluated from the arrays its search returned
(`evaluate_arrays`, sr_eval_ranked in csrc/eval_metrics.hip: one workgroup per query, every cutoff in one pass), and two runs are
compared with a two-sided paired randomization test (`compare`, sr_eval_randomization).  `evaluate_by_steps` computes the same bytes
from torch operations alone - the baseline a caller could have written, and the second witness of the tests.

The values are those of utils/metrics.py bit for bit (tests/test_eval_host.py): recip_rank, recall_k, ndcg_cut_k as trec_eval defines
them (ties by document id descending), r_cap_k with the same ranking, map_cut_k.  A query counts iff the judgements hold it with at
least one document and its list has a valid entry.

Not offered: lists longer than sr_max_topk(), alpha-nDCG and subtopic metrics, bpref and other condensed-list metrics, bootstrap
intervals and the t-test, the doc-sharded classes.
"""
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib
from .doc_filter import _call, _cuda_device, _ptr, _to_dev, _valid
from .utils.run_file import id_table

DEFAULT_CUTS = (5, 10, 15, 20, 30, 100, 200, 500, 1000)
MAX_CUTS = 16                           # sr_eval_max_cuts()
MAX_DEPTH = 4096                        # sr_max_topk()
MAX_COLS = 8                            # columns of one sr_eval_randomization call
FAMILIES = ("recall", "ndcg_cut", "r_cap", "map_cut")
ORDERS = {"score": _lib.SR_EVAL_ORDER_SCORE, "list": _lib.SR_EVAL_ORDER_LIST}


def cuts_argument(cuts):
    cuts = tuple(int(c) for c in cuts)
    if len(cuts) > MAX_CUTS or any(c < 1 for c in cuts) or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"evaluation: the cuts must be at most {MAX_CUTS}, each >= 1 and strictly ascending, got {cuts}")
    return cuts


def column_names(cuts):
    """The columns of a per-query row: recip_rank, then every family over the cuts."""
    return ["recip_rank"] + [f"{fam}_{c}" for fam in FAMILIES for c in cuts]


class QrelRows:
    """The judgement tables aligned with one run's query order: what sr_eval_ranked reads.  numpy arrays; device copies are kept."""

    def __init__(self, indptr, ids, grades, n_rel, idcg, log2, cuts, present):
        self.indptr, self.ids, self.grades, self.n_rel, self.idcg, self.log2 = indptr, ids, grades, n_rel, idcg, log2
        self.cuts, self.present = cuts, present
        self.nq = len(n_rel)
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(_to_dev(a, dt, device) for a, dt in (
                (self.indptr, torch.int64), (self.ids, torch.int64), (self.grades, torch.int32), (self.n_rel, torch.int32),
                (self.idcg, torch.float64), (self.log2, torch.float64)))
        return self._dev[key]


class Qrels:
    """Judgements {qid: {doc id: grade}} as arrays, built once per judgement file.  Judged ids are mapped to positions in `doc_table`
    (by str(), as run.json writes them); a judged document the table does not hold is numbered from len(table) up, an id no list can
    hold.  Per query: the row of (position ascending, grade), n_rel = the grades > 0, and for every cut the ideal DCG - the positive
    grades sorted descending, the first `cut` of them, summed from 0.0 as float(g) / math.log2(i + 2)."""

    def __init__(self, qrels_dict, doc_table, cuts=DEFAULT_CUTS):
        self.cuts = cuts_argument(cuts)
        self.docs = id_table(doc_table)
        self.n_docs = self.docs.n
        self.position_of = {k: i for i, k in enumerate(self.docs.keys_of(np.arange(self.n_docs)))}
        self.unknown = {}
        self.qids = [str(q) for q in qrels_dict]
        self.row_of = {q: i for i, q in enumerate(self.qids)}
        indptr, ids, grades = np.zeros(len(self.qids) + 1, np.int64), [], []
        self.n_rel = np.zeros(len(self.qids), np.int32)
        self.idcg = np.zeros((len(self.qids), len(self.cuts)), np.float64)
        for i, docs in enumerate(qrels_dict.values()):
            row = []
            for d, g in docs.items():
                d = str(d)
                p = self.position_of.get(d)
                if p is None:
                    p = self.unknown.setdefault(d, self.n_docs + len(self.unknown))
                row.append((p, int(g)))
            row.sort()
            ids.extend(p for p, _ in row)
            grades.extend(g for _, g in row)
            indptr[i + 1] = len(ids)
            pos = sorted((g for _, g in row if g > 0), reverse=True)
            self.n_rel[i] = len(pos)
            s, j = 0.0, 0
            for n, g in enumerate(pos[:self.cuts[-1]] if self.cuts else []):
                while n >= self.cuts[j]:
                    self.idcg[i, j] = s
                    j += 1
                s = s + float(g) / math.log2(n + 2)
            self.idcg[i, j:] = s
        self.indptr, self.ids, self.grades = indptr, np.asarray(ids, np.int64), np.asarray(grades, np.int32)
        self.log2 = np.array([math.log2(i + 2) for i in range(MAX_DEPTH)], np.float64)

    def rows_for(self, qids):
        """QrelRows in the order of `qids` (any keys; compared by str()).  A query outside the judgements gets an empty row."""
        if isinstance(qids, QrelRows):
            return qids
        qt = id_table(qids)
        keys = qt.keys_of(np.arange(qt.n)) if qt.n else []
        src = np.array([self.row_of.get(k, -1) for k in keys], np.int64)
        present = src >= 0
        s = np.where(present, src, 0)
        lens = np.where(present, self.indptr[s + 1] - self.indptr[s], 0) if len(src) else np.zeros(0, np.int64)
        indptr = np.zeros(len(src) + 1, np.int64)
        np.cumsum(lens, out=indptr[1:])
        take = np.repeat(self.indptr[s] - indptr[:-1], lens) + np.arange(indptr[-1]) if len(src) else np.zeros(0, np.int64)
        n_rel = np.where(present, self.n_rel[s], 0).astype(np.int32) if len(src) else np.zeros(0, np.int32)
        idcg = np.where(present[:, None], self.idcg[s], 0.0) if len(src) else np.zeros((0, len(self.cuts)), np.float64)
        return QrelRows(indptr, self.ids[take], self.grades[take], n_rel, np.ascontiguousarray(idcg), self.log2, self.cuts, present)

    def positions_of(self, keys):
        """int64 [n]: the table position of str(key), -1 where the table does not hold it (BEIR's exclude = the query's own id)."""
        return np.array([self.position_of.get(str(k), -1) for k in keys], np.int64)


class EvalResult:
    """per_query float64 [nq, 1 + 4 n_cuts] and flags int32 [nq] (bit 0: evaluated, bit 1: no relevant document) on the device, `means`
    {trec-style key: float} over the n_evaluated queries, `columns` the keys in column order, `qids` the run's query keys as given."""

    def __init__(self, per_query, flags, mean, n_evaluated, cuts, qids):
        self.per_query, self.flags, self.mean, self.n_evaluated, self.cuts, self.qids = per_query, flags, mean, int(n_evaluated), cuts, qids
        self.columns = column_names(cuts)
        self.means = dict(zip(self.columns, mean.tolist()))

    def column(self, name):
        return self.per_query[:, self.columns.index(name)]


def _list_arguments(scores, ids, counts, exclude, order, rr_depth):
    """The host checks both evaluators share; touches no device.  -> (order id, rr_depth)."""
    if order not in ORDERS:
        raise ValueError(f"evaluation: order must be 'score' or 'list', got {order!r}")
    rr_depth = int(rr_depth)
    if rr_depth < 0:
        raise ValueError(f"evaluation: rr_depth = {rr_depth} must be >= 0")
    if ids.ndim != 2:
        raise ValueError(f"evaluation: expected ids [nq, depth], got {tuple(ids.shape)}")
    nq, depth = ids.shape
    if depth < 1 or depth > MAX_DEPTH:
        raise ValueError(f"evaluation: depth = {depth}, lists of 1 to {MAX_DEPTH} entries are evaluated")
    if order == "score" and (scores is None or tuple(scores.shape) != (nq, depth)):
        raise ValueError(f"evaluation: the score order needs scores shaped like ids {(nq, depth)}")
    for name, a in (("counts", counts), ("exclude", exclude)):
        if a is not None and tuple(a.shape) != (nq,):
            raise ValueError(f"evaluation: expected {name} [{nq}], got {tuple(a.shape)}")
    return ORDERS[order], rr_depth


def _tensor(x):
    return x if x is None or torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _valid_mask(ids, counts, exclude):
    depth = ids.shape[1]
    valid = ids >= 0
    if counts is not None:
        valid &= torch.arange(depth, device=ids.device)[None, :] < counts.to(torch.int64)[:, None]
    if exclude is not None:
        valid &= ids != exclude[:, None]
    return valid


_INT_KEY_DIGITS = 17                    # decimal ids below 10^17: the left-aligned digits * 32 + their number fit an int64


def _int_table_on(docs, device):
    """The document ids of an all-integer table on `device` if str() order can be computed there (0 <= id < 10^17), else None.  Kept on
    the table."""
    if docs.kind != "i64" or docs.n == 0:
        return None
    cache = docs.__dict__.setdefault("_eval_dev", {})
    if "ok" not in cache:
        cache["ok"] = bool(docs.i64.min() >= 0 and docs.i64.max() < 10 ** _INT_KEY_DIGITS)
    if not cache["ok"]:
        return None
    if str(device) not in cache:
        cache[str(device)] = torch.from_numpy(docs.i64).to(device)
    return cache[str(device)]


def _int_tie_ranks(s, doc):
    """int32 [m, depth]: the rank of str(doc) among the entries of the row that share the score s (NaN shares with nothing), on the
    device.  str() order of non-negative integers is the order of their decimal digits left-aligned, a prefix first: one integer key."""
    depth = s.shape[1]
    pw = 10 ** torch.arange(0, _INT_KEY_DIGITS + 1, dtype=torch.int64, device=s.device)
    nd = torch.bucketize(doc, pw[1:], right=True) + 1                       # decimal digits; 0 has one
    key = doc * pw[_INT_KEY_DIGITS - nd] * 32 + nd
    perm = torch.sort(key, dim=1, stable=True).indices
    perm = torch.gather(perm, 1, torch.sort(torch.gather(s, 1, perm), dim=1, stable=True).indices)
    ss = torch.gather(s, 1, perm)
    idx = torch.arange(depth, device=s.device)[None, :].expand_as(ss)
    start = torch.ones_like(ss, dtype=torch.bool)
    start[:, 1:] = ss[:, 1:] != ss[:, :-1]
    rank = idx - torch.where(start, idx, torch.zeros_like(idx)).cummax(1).values
    return torch.zeros_like(rank, dtype=torch.int32).scatter_(1, perm, rank.to(torch.int32))


def tie_keys(scores, ids, valid, doc_table):
    """tie_key int32 [nq, depth] on the device, or None when no row holds two valid entries of one score.  Neighbouring scores are
    compared on the device after a sort; only the rows with equal neighbours are ranked (trec_eval breaks ties by document id
    descending: the larger string gets the larger key) - on the device when the table holds integers in [0, 10^17), whose str() order
    is an integer key; else those rows come to the host, where str() of the tied documents is sorted."""
    nq, depth = ids.shape
    if nq == 0 or depth < 2:
        return None
    s = torch.where(valid, scores + 0.0, torch.full_like(scores, float("nan")))      # -0.0 + 0.0 = +0.0; NaN equals nothing
    ss = torch.sort(s, dim=1).values
    rows = torch.nonzero((ss[:, 1:] == ss[:, :-1]).any(1)).flatten()
    if rows.numel() == 0:
        return None
    docs = id_table(doc_table)
    table = _int_table_on(docs, ids.device)
    if table is not None:
        out = torch.zeros((nq, depth), dtype=torch.int32, device=ids.device)
        out[rows] = _int_tie_ranks(s[rows], table[ids[rows].clamp(min=0)])
        return out
    tie = np.zeros((rows.numel(), depth), np.int32)
    h_s, h_i = s[rows].cpu().numpy(), ids[rows].cpu().numpy()
    for n in range(rows.numel()):
        vals, inv, cnt = np.unique(h_s[n], return_inverse=True, return_counts=True)      # NaNs: one group or many, never read
        for g in np.nonzero((cnt > 1) & ~np.isnan(vals))[0]:
            at = np.nonzero(inv == g)[0]
            keys = docs.keys_of(h_i[n][at])
            for rank, j in enumerate(sorted(range(len(at)), key=keys.__getitem__)):
                tie[n, at[j]] = rank
    out = torch.zeros((nq, depth), dtype=torch.int32, device=ids.device)
    out[rows] = torch.from_numpy(tie).to(ids.device)
    return out


def _prepare(scores, ids, counts, qrels, qids, order, rr_depth, exclude, doc_table, tie_key):
    no_ties = tie_key is False                                  # the caller wants none built: equal scores keep their list order
    scores, ids, counts, exclude, tie_key = (_tensor(x) for x in (scores, ids, counts, exclude, None if no_ties else tie_key))
    order_id, rr_depth = _list_arguments(scores, ids, counts, exclude, order, rr_depth)
    rows = qrels if isinstance(qrels, QrelRows) else qrels.rows_for(qids)      # a caller with tables of its own brings its tie keys too
    if rows.nq != ids.shape[0]:
        raise ValueError(f"evaluation: {ids.shape[0]} lists, {rows.nq} queries")
    _lib.require_gpu()
    dev = _cuda_device(ids)
    ids = ids.to(device=dev, dtype=torch.int64).contiguous()
    scores = None if scores is None else scores.to(device=dev, dtype=torch.float32).contiguous()
    counts = None if counts is None else counts.to(device=dev, dtype=torch.int32).contiguous()
    exclude = None if exclude is None else exclude.to(device=dev, dtype=torch.int64).contiguous()
    if tie_key is not None:
        tie_key = tie_key.to(device=dev, dtype=torch.int32).contiguous()
    elif order == "score" and not no_ties:
        if doc_table is None and isinstance(qrels, QrelRows):
            raise ValueError("evaluation: judgement tables without a Qrels need tie_key (or tie_key=False) or a doc_table")
        tie_key = tie_keys(scores, ids, _valid_mask(ids, counts, exclude), qrels.docs if doc_table is None else doc_table)
    return scores, ids, counts, exclude, tie_key, rows, order_id, rr_depth, dev


def evaluate_arrays(scores, ids, counts, qrels, qids, order="score", rr_depth=0, exclude=None, doc_table=None, tie_key=None):
    """The metrics of a run from its arrays (torch or numpy): scores fp32 [nq, depth], ids int64 [nq, depth] positions in the document
    table (negative = padding), counts [nq] or None, `qrels` a Qrels, `qids` the run's query keys (or a QrelRows from rows_for).
    order "score" ranks by (score descending, document id as a string descending), "list" takes the entries as they stand.  rr_depth = 10
    gives MRR@10 as mrr_k computes it.  exclude int64 [nq]: a position to drop from each list (-1: none).  tie_key: the caller's own tie
    ranks; by default they are built from doc_table (the Qrels' table) where scores tie.  Returns an EvalResult."""
    scores, ids, counts, exclude, tie_key, rows, order_id, rr_depth, dev = _prepare(scores, ids, counts, qrels, qids, order, rr_depth, exclude,
                                                                                  doc_table, tie_key)
    nq, depth = ids.shape
    cuts = rows.cuts
    ncol = 1 + 4 * len(cuts)
    indptr, q_ids, q_grades, n_rel, idcg, log2 = rows.on(dev)
    out = torch.empty((nq, ncol), dtype=torch.float64, device=dev)
    flags = torch.empty((nq,), dtype=torch.int32, device=dev)
    mean = torch.empty((ncol,), dtype=torch.float64, device=dev)
    n_eval = torch.zeros((1,), dtype=torch.int64, device=dev)
    keep = [_valid(t) for t in (ids, out, flags, q_ids, q_grades, n_rel, idcg)]
    opt = [None if t is None else _valid(t) for t in (scores, counts, tie_key, exclude)]
    _call(dev, "sr_eval_ranked", _ptr(opt[0]), _ptr(keep[0]), _ptr(opt[1]), _ptr(opt[2]), _ptr(opt[3]), nq, depth, _ptr(indptr), _ptr(keep[3]),
          _ptr(keep[4]), q_ids.numel(), _ptr(keep[5]), _ptr(keep[6]), _ptr(log2), (ctypes.c_int32 * max(1, len(cuts)))(*cuts), len(cuts),
          order_id, rr_depth, _ptr(keep[1]), _ptr(keep[2]), _ptr(mean), _ptr(n_eval))
    return EvalResult(out, flags, mean.cpu().numpy(), int(n_eval.item()), cuts, qids)


def evaluate_by_steps(scores, ids, counts, qrels, qids, order="score", rr_depth=0, exclude=None, doc_table=None, tie_key=None):
    """The same EvalResult, byte for byte, from torch operations alone: searchsorted for the grades, stable sorts for the ranking, and the
    rounded sums in the kernel's order.  A device cumsum or sum is a tree, not that order, so the float64 sums run as one vectorised
    add per relevant entry (adding 0.0 changes no bit: only the relevant entries matter), and the column means are taken with a
    sequential cumsum on the host."""
    scores, ids, counts, exclude, tie_key, rows, _, rr_depth, dev = _prepare(scores, ids, counts, qrels, qids, order, rr_depth, exclude, doc_table,
                                                                           tie_key)
    nq, depth = ids.shape
    cuts = rows.cuts
    nc = len(cuts)
    indptr, q_ids, q_grades, n_rel, idcg, log2 = rows.on(dev)
    out = torch.zeros((nq, 1 + 4 * nc), dtype=torch.float64, device=dev)
    if nq == 0:
        return EvalResult(out, torch.zeros((0,), dtype=torch.int32, device=dev), np.zeros(1 + 4 * nc), 0, cuts, qids)
    valid = _valid_mask(ids, counts, exclude)
    # the grade of every entry: one searchsorted over (query, id) keys, ascending because every row ascends
    span = int(max(int(ids.max().item()), int(q_ids.max().item()) if q_ids.numel() else 0, 0)) + 1
    row_of = torch.repeat_interleave(torch.arange(nq, device=dev), indptr[1:] - indptr[:-1])
    q_keys = row_of * span + q_ids
    e_keys = torch.arange(nq, device=dev)[:, None] * span + ids.clamp(min=0)
    grade = torch.zeros((nq, depth), dtype=torch.int64, device=dev)
    if q_keys.numel():
        at = torch.searchsorted(q_keys, e_keys.contiguous()).clamp(max=q_keys.numel() - 1)
        grade = torch.where(valid & (q_keys[at] == e_keys), q_grades[at].to(torch.int64), grade)
    # the ranking: stable sorts, least significant key first - position is the order the entries stand in
    perm = torch.arange(depth, device=dev)[None, :].expand(nq, depth)
    if order == "score":
        if tie_key is not None:
            perm = torch.gather(perm, 1, torch.sort(tie_key, dim=1, descending=True, stable=True).indices)
        s = torch.gather(scores + 0.0, 1, perm)
        perm = torch.gather(perm, 1, torch.sort(s, dim=1, descending=True, stable=True).indices)
    perm = torch.gather(perm, 1, torch.sort((~torch.gather(valid, 1, perm)).to(torch.int8), dim=1, stable=True).indices)
    g = torch.gather(grade, 1, perm)                            # the invalid entries stand last with grade 0
    rel = g > 0
    rank = torch.arange(1, depth + 1, device=dev)[None, :]
    # recip_rank: the entries in front of the cut keep their order; the rank counts them alone
    in_cut = torch.gather(valid, 1, perm)
    if rr_depth > 0:
        in_cut = in_cut & torch.gather(torch.cumsum(valid.to(torch.int64), 1) <= rr_depth, 1, perm)
    cut_rank = torch.cumsum(in_cut.to(torch.int64), 1)
    first = torch.where(rel & in_cut, cut_rank, torch.full_like(cut_rank, depth + 1)).min(1).values
    out[:, 0] = torch.where(first <= depth, 1.0 / first.to(torch.float64), torch.zeros_like(first, dtype=torch.float64))
    # the relevant entries in rank order, then one rounded add per entry and cut
    n_hit = rel.sum(1)
    R = int(n_hit.max().item())
    front = torch.sort((~rel).to(torch.int8), dim=1, stable=True).indices[:, :R]
    r_rank = torch.gather(rank.expand(nq, depth), 1, front)
    r_gain = torch.gather(g, 1, front).to(torch.float64) / log2[(r_rank - 1).clamp(min=0)]
    cut_t = torch.tensor(cuts, dtype=torch.int64, device=dev)[None, :]
    dcg = torch.zeros((nq, nc), dtype=torch.float64, device=dev)
    ap = torch.zeros((nq, nc), dtype=torch.float64, device=dev)
    hits = torch.zeros((nq, nc), dtype=torch.int64, device=dev)
    for i in range(R if nc else 0):
        on = ((i < n_hit)[:, None]) & (r_rank[:, i:i + 1] <= cut_t)
        dcg = torch.where(on, dcg + r_gain[:, i:i + 1], dcg)
        r = r_rank[:, i:i + 1].to(torch.float64)
        ap = torch.where(on, ap + torch.full_like(r, float(i + 1)) / r, ap)     # tensor / tensor: `scalar / tensor` is reciprocal() * scalar, two roundings
        hits = hits + on.to(torch.int64)
    nr = n_rel.to(torch.float64)[:, None]
    has = (n_rel > 0)[:, None]
    zero = torch.zeros((nq, nc), dtype=torch.float64, device=dev)
    h = hits.to(torch.float64)
    out[:, 1:1 + nc] = torch.where(has, h / nr, zero)
    out[:, 1 + nc:1 + 2 * nc] = torch.where(idcg > 0, dcg / idcg, zero)
    out[:, 1 + 2 * nc:1 + 3 * nc] = torch.where(has, h / torch.minimum(n_rel.to(torch.int64)[:, None], cut_t).to(torch.float64), zero)
    out[:, 1 + 3 * nc:] = torch.where(has, ap / nr, zero)
    evaluated = ((indptr[1:] > indptr[:-1]) & valid.any(1))
    out = torch.where(evaluated[:, None], out, torch.zeros_like(out))
    flags = evaluated.to(torch.int32) | ((n_rel <= 0).to(torch.int32) << 1)
    kept = out[evaluated].cpu().numpy()
    n = kept.shape[0]
    mean = np.cumsum(kept, axis=0)[-1] / n if n else np.zeros(1 + 4 * nc)
    return EvalResult(out, flags, mean + 0.0, n, cuts, qids)


# ------------------------------------------------------------------------------------------------------ comparing two runs ---
def randomization_arguments(n_cols, n_perm, seed):
    """The host checks of the randomization test; touches no device."""
    n_perm, seed = int(n_perm), int(seed)
    if not 1 <= n_perm < (1 << 31):
        raise ValueError(f"randomization test: n_perm = {n_perm}, 1 to 2^31 - 1 permutations are drawn")
    if n_cols < 1:
        raise ValueError("randomization test: no metric column")
    return n_perm, seed & ((1 << 64) - 1)


def randomization_test(diff, n_perm=100000, seed=0):
    """diff float64 [n_cols, n] (torch or numpy): per-query differences of up to 8 columns per call (more are taken 8 at a time with the
    same signs).  -> (t_obs float64 [n_cols], count_ge int64 [n_cols]) on the host; p = (count_ge + 1) / (n_perm + 1)."""
    diff = _tensor(diff)
    if diff.ndim != 2:
        raise ValueError(f"randomization test: expected differences [n_cols, n], got {tuple(diff.shape)}")
    n_cols, n = diff.shape
    n_perm, seed = randomization_arguments(n_cols, n_perm, seed)
    _lib.require_gpu()
    dev = _cuda_device(diff)
    diff = diff.to(device=dev, dtype=torch.float64).contiguous()
    t_obs = torch.empty((n_cols,), dtype=torch.float64, device=dev)
    count = torch.empty((n_cols,), dtype=torch.int64, device=dev)
    for c0 in range(0, n_cols, MAX_COLS):
        m = min(MAX_COLS, n_cols - c0)
        part = _valid(diff[c0:c0 + m].contiguous())
        _call(dev, "sr_eval_randomization", _ptr(part), m, n, n_perm, seed, _ptr(t_obs[c0:]), _ptr(count[c0:]))
    return t_obs.cpu().numpy(), count.cpu().numpy()


def compare(result_a, result_b, metrics, n_perm=100000, seed=0):
    """Two EvalResults over the same queries in the same order -> {metric: {"mean_a", "mean_b", "diff", "n", "count_ge", "p"}}: the
    runs' own means and their difference, and the two-sided paired randomization test over the n queries evaluated in both:
    count_ge permutations of n_perm had |T| >= |T observed|, p = (count_ge + 1) / (n_perm + 1)."""
    metrics = list(metrics)
    if result_a.columns != result_b.columns or tuple(result_a.per_query.shape) != tuple(result_b.per_query.shape):
        raise ValueError("compare: the two results must hold the same queries and cuts")
    cols = []
    for m in metrics:
        if m not in result_a.columns:
            raise ValueError(f"compare: unknown metric {m!r}; the results hold {result_a.columns}")
        cols.append(result_a.columns.index(m))
    n_perm, seed = randomization_arguments(len(cols), n_perm, seed)
    both = ((result_a.flags & 1) != 0) & ((result_b.flags.to(result_a.flags.device) & 1) != 0)
    idx = torch.tensor(cols, dtype=torch.int64, device=result_a.per_query.device)
    diff = (result_a.per_query[both][:, idx] - result_b.per_query.to(result_a.per_query.device)[both][:, idx]).t().contiguous()
    _, count = randomization_test(diff, n_perm, seed)
    out = {}
    for j, m in enumerate(metrics):
        out[m] = {"mean_a": result_a.means[m], "mean_b": result_b.means[m], "diff": result_a.means[m] - result_b.means[m],
                  "n": int(diff.shape[1]), "count_ge": int(count[j]), "p": (int(count[j]) + 1) / (n_perm + 1)}
    return out


# ------------------------------------------------------------------------------------------------------------------ run files ---
def load_run_arrays(path_or_dict, doc_table=None):
    """A run.json ({qid: {doc id: score}}, or the loaded dict) as arrays: (qids [str], scores fp32 [nq, depth], positions int64
    [nq, depth], counts int32 [nq], doc table).  Each row is ordered by score descending with a STABLE sort, file order among equals -
    truncate_run's first step, so rr_depth cuts what mrr_k cuts.  Scores become fp32, what the project's runs hold.  Without a
    doc_table the table is the sorted set of the file's document ids; with one, a document outside it is a KeyError."""
    run = path_or_dict
    if not isinstance(run, dict):
        with open(path_or_dict) as f:
            run = json.load(f)
    if doc_table is None:
        doc_table = sorted({str(d) for docs in run.values() for d in docs})
    table = id_table(doc_table)
    pos_of = {k: i for i, k in enumerate(table.keys_of(np.arange(table.n)))}
    depth = max([len(docs) for docs in run.values()] + [1])
    if depth > MAX_DEPTH:
        raise ValueError(f"load_run_arrays: a list of {depth} entries; lists of up to {MAX_DEPTH} are evaluated")
    qids = [str(q) for q in run]
    scores = np.zeros((len(qids), depth), np.float32)
    pos = np.full((len(qids), depth), -1, np.int64)
    counts = np.zeros(len(qids), np.int32)
    for i, docs in enumerate(run.values()):
        ranked = sorted(docs.items(), key=lambda item: item[1], reverse=True)
        counts[i] = len(ranked)
        scores[i, :len(ranked)] = [s for _, s in ranked]
        pos[i, :len(ranked)] = [pos_of[str(d)] for d, _ in ranked]
    return qids, scores, pos, counts, table


def evaluate_run_file(qrel_path, run_path, metric):
    """utils.metrics.load_and_evaluate through the device: the same dict for metric in {"mrr_10", "recall", "ndcg_cut", "recip_rank"}."""
    if metric not in MSMARCO_METRICS:
        raise ValueError("provide valid metric")
    with open(qrel_path) as f:
        qrel = json.load(f)
    qids, scores, pos, counts, table = load_run_arrays(run_path)
    qrels = Qrels(qrel, table)
    out = perf_from_arrays([metric], qrels, qids, scores, pos, counts, n=int(qrels.rows_for(qids).present.sum()))[metric]
    print("MRR@10:" if metric == "mrr_10" else metric + " ==>", out["mrr_10"] if metric == "mrr_10" else out)
    return out


def beir_metrics(result):
    """perf.json of evaluate_beir from an EvalResult whose cuts hold 10 and 100."""
    return {"NDCG@10": round(result.means["ndcg_cut_10"], 5), "Recall@100": round(result.means["recall_100"], 5),
            "R_cap@100": round(result.means["r_cap_100"], 5)}


# ------------------------------------------------------------------------------------------------------ the drivers' tasks ---
MSMARCO_METRICS = ("mrr_10", "recall", "ndcg_cut", "recip_rank")


def dict_means(result, n):
    """The means as utils/metrics.py takes them over a run DICT: Python's sum() over the per-query values in query order, divided by
    max(1, n) - n the queries that dict code counts, which the caller knows (a query whose list is empty after a filter still counts
    there).  The columns of a query that is not evaluated are 0.0, and adding 0.0 changes no bit."""
    per_q = result.per_query.cpu().numpy()
    return {name: sum(per_q[:, j].tolist()) / max(1, n) for j, name in enumerate(result.columns)}


def metric_dict(means, metric, cuts=DEFAULT_CUTS):
    """What load_and_evaluate returns for `metric`, from a means dict (recip_rank already cut for "mrr_10")."""
    if metric == "mrr_10":
        return {"mrr_10": means["recip_rank"]}
    if metric == "recip_rank":
        return {"recip_rank": means["recip_rank"]}
    if metric in ("recall", "ndcg_cut"):
        return {f"{metric}_{c}": means[f"{metric}_{c}"] for c in cuts}
    raise ValueError("provide valid metric")


def perf_from_arrays(metrics, qrels, qids, scores, positions, counts, n=None):
    """{metric: load_and_evaluate's dict} for a run held as arrays; n = the queries a dict of this run would count (default: those the
    judgements hold whose list has a hit - RunResult's dict has no other)."""
    for m in metrics:
        metric_dict({"recip_rank": 0.0, **{f"{f}_{c}": 0.0 for f in ("recall", "ndcg_cut") for c in DEFAULT_CUTS}}, m)    # ValueError first
    rows = qrels.rows_for(qids)
    if n is None:
        pos = np.asarray(positions.cpu() if torch.is_tensor(positions) else positions)
        has = pos >= 0
        if counts is not None:
            has &= np.arange(pos.shape[1])[None, :] < np.asarray(counts.cpu() if torch.is_tensor(counts) else counts)[:, None]
        n = int((rows.present & has.any(1)).sum())
    out, cache = {}, {}
    for m in metrics:
        rr = 10 if m == "mrr_10" else 0
        if rr not in cache:
            cache[rr] = dict_means(evaluate_arrays(scores, positions, counts, qrels, rows, rr_depth=rr), n)
        out[m] = metric_dict(cache[rr], m, qrels.cuts)
    return out


def device_eval_msmarco(args):
    """The evaluate_msmarco task through the device: the same perf.json content."""
    import os
    with open(args.eval_qrel_path) as f:
        qrel = json.load(f)
    qids, scores, pos, counts, table = load_run_arrays(args.eval_run_path)
    qrels = Qrels(qrel, table)
    res = perf_from_arrays(args.eval_metric, qrels, qids, scores, pos, counts, n=int(qrels.rows_for(qids).present.sum()))
    for metric, vals in res.items():
        print("MRR@10:" if metric == "mrr_10" else metric + " ==>", vals["mrr_10"] if metric == "mrr_10" else vals)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "perf.json"), "w") as fout:
        json.dump(res, fout, indent=4)
    return res


def device_eval_beir(args, qrels):
    """The evaluate_beir task through the device: {out_dir}/run.json without the hit whose id is the query's, NDCG@10 and Recall@100
    under trec_eval's order, R_cap@100 under beir's (score descending, file order among equals), rounded to 5 places.  As
    recall_cap_k: a query of the run outside the judgements is a KeyError, one without a relevant document a ZeroDivisionError -
    both before any launch."""
    import os
    with open(os.path.join(args.out_dir, "run.json")) as reader:
        run = json.load(reader)
    print("Removing query id from document list")
    qrels = {str(q): {str(d): int(r) for d, r in docs.items()} for q, docs in qrels.items()}
    for q in run:
        if not any(r > 0 for r in qrels[q].values()):          # qrels[q]: the KeyError
            raise ZeroDivisionError("division by zero")
    qids, scores, pos, counts, table = load_run_arrays(run)
    Q = Qrels(qrels, table, cuts=(10, 100))
    exclude = Q.positions_of(qids)
    rows = Q.rows_for(qids)
    trec = dict_means(evaluate_arrays(scores, pos, counts, Q, rows, exclude=exclude), len(run))
    beir = dict_means(evaluate_arrays(scores, pos, counts, Q, rows, exclude=exclude, tie_key=False), len(run))
    res = {"NDCG@10": round(trec["ndcg_cut_10"], 5), "Recall@100": round(trec["recall_100"], 5), "R_cap@100": round(beir["r_cap_100"], 5)}
    with open(os.path.join(args.out_dir, "perf.json"), "w") as writer:
        json.dump(res, writer, indent=4)
    return res


def write_run_perf(path, metrics, qrels, res):
    """perf.json beside a run the retrieval task wrote, from the RunResult's arrays."""
    perf = perf_from_arrays(metrics or MSMARCO_METRICS[:3], qrels, res.qids, res.scores, res.positions, res.counts)
    with open(path, "w") as fout:
        json.dump(perf, fout, indent=4)
    return perf
