"""BM25 on the device: a lexical index and search from token ids, without a model.

  Bm25Indexer     token rows of a collection loader -> term frequencies (sr_token_counts) -> one sr_sparse_csr_build; the artefacts of
                  SparseIndexer with the raw frequencies as values, plus doc_len.npy and bm25_stats.json.
  Bm25Retrieval   a SparseRetrieval whose postings are weighted on the device (sr_bm25_weights) with its own (k1, b) when the index is
                  opened - the frequencies are what is stored, so a parameter sweep needs no re-indexing - and whose queries are the
                  token counts of the query rows.  Everything SparseRetrieval does with a SparseIndexHIP works on it unchanged.

The weight of posting (t, d) with frequency tf:  idf[t] * (tf * numer) / (tf + a + s * doc_len[d]),  numer = k1 + 1 (1 for Lucene's
rank-equivalent form), a = k1 (1 - b), s = k1 b / avgdl, idf[t] = log1p((N - df + 0.5) / (df + 0.5)) - Lucene's always-positive idf.
bm25_scalars / idf_table hold the host side of that to the bit (the kernel runs no logarithm); *_by_steps are the compositions of
torch calls a caller has without the two kernels: baselines of tools/bench_bm25.py and cross-checks of the tests.
"""
import json
import os
import pickle

import numpy as np
import torch

from .indexer import QueryCSR, SparseRetrieval, _csr_sorted_by_doc
from .scoring import SparseIndexHIP, bm25_weights, sparse_csr_build, token_counts
from .utils.inverted_index import IndexDictOfArray
from .utils.utils import get_rank, get_world_size, to_list

_SHARDED = ("BM25 is not implemented for world_size > 1: document frequencies and the average document length are statistics of the "
            "whole collection, a sharded index would need a reduction of both across ranks - build and search on one process")


# ------------------------------------------------------------------------------------------------------------------- host formulas
def bm25_scalars(k1, b, avgdl, lucene=False):
    """(numer, a, s) of sr_bm25_weights as Python floats holding fp32 values, every step one rounded fp32 operation:
    numer = f32(f32(k1) + 1), or 1.0 with lucene=True (Lucene drops the constant factor k1 + 1: the same ranking);
    a = f32(f32(k1) * f32(1 - f32(b)));  s = f32(f32(f32(k1) * f32(b)) / f32(avgdl)), 0 when avgdl == 0 (no counted token at all)."""
    k1f, bf, one = np.float32(k1), np.float32(b), np.float32(1)
    if not (np.isfinite(k1f) and k1f >= 0 and 0 <= bf <= 1):
        raise ValueError(f"BM25 needs a finite k1 >= 0 and b in [0, 1], got k1 = {k1}, b = {b}")
    numer = one if lucene else np.float32(k1f + one)
    a = np.float32(k1f * np.float32(one - bf))
    s = np.float32(np.float32(k1f * bf) / np.float32(avgdl)) if avgdl else np.float32(0)
    return float(numer), float(a), float(s)


def idf_table(df, n_docs):
    """idf[t] = f32(log1p((N - df[t] + 0.5) / (df[t] + 0.5))) computed in float64 (np.float32 [n_terms]): positive for every df in
    [0, N]; df = the posting list sizes, indptr[1:] - indptr[:-1]."""
    df = np.asarray(df, dtype=np.float64)
    return np.log1p((float(n_docs) - df + 0.5) / (df + 0.5)).astype(np.float32)


def average_length(total_len, n_docs):
    """avgdl in double from the int64 sum of the document lengths; 0.0 for an empty collection."""
    return float(int(total_len)) / float(int(n_docs)) if n_docs else 0.0


# ------------------------------------------------------------------------------------------------------------------- compositions
def token_counts_by_steps(input_ids, attention_mask=None, skip_ids=(), n_terms=None):
    """scoring.token_counts as torch calls: a sort of every row's keys (the id, n_terms for a slot that does not count), then
    unique_consecutive over (row, key).  The same four tensors, the same bytes."""
    ids = input_ids.to(torch.int64)
    B, L = ids.shape
    dev = ids.device
    counted = torch.ones_like(ids, dtype=torch.bool) if attention_mask is None else attention_mask.to(dev) != 0
    for sid in skip_ids:
        counted &= ids != int(sid)
    bad = counted & ((ids < 0) | (ids >= int(n_terms)))
    if bool(bad.any()):
        r, p = [int(x) for x in torch.nonzero(bad)[0]]
        raise ValueError(f"token id {int(ids[r, p])} (row {r}, position {p}) is outside [0, {int(n_terms)})")
    M = int(n_terms) + 1
    keys = torch.sort(torch.where(counted, ids, torch.full_like(ids, M - 1)), dim=1).values
    flat = (keys + torch.arange(B, device=dev, dtype=torch.int64)[:, None] * M).reshape(-1)
    uniq, cnt = torch.unique_consecutive(flat, return_counts=True)
    keep = uniq % M != M - 1
    uniq, cnt = uniq[keep], cnt[keep]
    row_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(torch.bincount(uniq // M, minlength=B), 0)
    return row_ptr, (uniq % M).to(torch.int32), cnt.to(torch.float32), counted.sum(1).to(torch.int32)


def bm25_weights_by_steps(indptr, doc_ids, tf, doc_len, idf, numer, a, s):
    """scoring.bm25_weights as torch calls: the term of every posting by repeat_interleave, then one element-wise fp32 op per rounding
    of the formula.  The same bytes."""
    dev = tf.device
    n_terms = indptr.numel() - 1
    term = torch.repeat_interleave(torch.arange(n_terms, device=dev), indptr[1:] - indptr[:-1])
    f = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)      # noqa: E731
    dl = doc_len.to(dev)[doc_ids.long()].to(torch.float32)
    K = torch.add(torch.mul(dl, f(s)), f(a))
    q = torch.div(torch.mul(tf, f(numer)), torch.add(tf, K))
    return torch.mul(idf.to(dev)[term], q)


# ---------------------------------------------------------------------------------------------------------------------- indexing
def _stats(n_docs, total_len, k1, b, lucene, skip_ids, dim_voc):
    return {"n_docs": int(n_docs), "total_len": int(total_len), "avgdl": average_length(total_len, n_docs), "k1": float(k1), "b": float(b),
            "lucene": bool(lucene), "skip_ids": [int(x) for x in skip_ids], "dim_voc": int(dim_voc)}


class Bm25Indexer:
    """SparseIndexer without a model: the postings of a document are the counts of its tokens.  skip_ids: the special ids that are no
    terms (BOS, EOS, pad; at most 16).  k1, b, lucene are only recorded (bm25_stats.json: the defaults of a Bm25Retrieval over this
    index); the stored values are the raw frequencies."""

    def __init__(self, index_dir, device, dim_voc, skip_ids, k1=0.9, b=0.4, lucene=False, force_new=True, filename="array_index.h5py"):
        self.world_size = get_world_size()
        if self.world_size > 1:
            raise NotImplementedError(_SHARDED)
        bm25_scalars(k1, b, 1.0, lucene)                     # the argument check
        self.index_dir, self.device, self.dim_voc = index_dir, device, int(dim_voc)
        self.skip_ids = sorted({int(x) for x in skip_ids})
        self.k1, self.b, self.lucene = float(k1), float(b), bool(lucene)
        self.sparse_index = IndexDictOfArray(index_dir, dim_voc=self.dim_voc, force_new=force_new, filename=filename)
        self.local_rank = get_rank()

    def index(self, collection_loader, id_dict=None):
        """SparseIndexer.index: per batch the term frequencies stay on the device as COO triples, one sr_sparse_csr_build at the end.  A
        document without a counted token gets no doc_ids entry but counts in N and in the average length.  With an index_dir the files
        of SparseIndexer (index_stats.json: L0_d, the distinct terms per document) plus doc_len.npy (int32 [N]) and bm25_stats.json; without
        one the in-memory dict of SparseIndexer plus "doc_len" (int32 [N] on the device) and "bm25_stats"."""
        if self.sparse_index.nb_docs() != 0 or len(self.sparse_index.doc_ids) != 0:
            raise ValueError("Bm25Indexer.index builds a new index; this container already holds documents (use force_new=True)")
        dev = torch.device(self.device if not isinstance(self.device, int) else f"cuda:{self.device}")
        doc_ids, count = {}, 0
        dev_rows, dev_cols, dev_vals, dev_len = [], [], [], []
        for batch in collection_loader:
            batch_ids = to_list(batch["ids"]) if isinstance(batch["ids"], torch.Tensor) else batch["ids"]
            if id_dict:
                batch_ids = [id_dict[x] for x in batch_ids]
            mask = batch.get("attention_mask")
            row_ptr, col, tf, lengths = token_counts(batch["input_ids"].to(dev), None if mask is None else mask.to(dev), self.skip_ids,
                                                     self.dim_voc)
            nnz_per_row = row_ptr[1:] - row_ptr[:-1]
            if count + len(batch_ids) >= 2 ** 31:
                raise OverflowError("document index exceeds int32 (the posting lists hold int32 doc ids)")
            dev_rows.append((torch.repeat_interleave(torch.arange(len(nnz_per_row), device=dev), nnz_per_row) + count).to(torch.int32))
            dev_cols.append(col)
            dev_vals.append(tf)
            dev_len.append(lengths)
            has_posting = np.nonzero((nnz_per_row > 0).cpu().numpy())[0]
            doc_ids.update(zip((count + has_posting).tolist(), (batch_ids[i] for i in has_posting.tolist())))
            count += len(batch_ids)
        doc_len = torch.cat(dev_len) if dev_len else torch.zeros(0, dtype=torch.int32, device=dev)
        self.stats = _stats(count, int(doc_len.sum(dtype=torch.int64)) if count else 0, self.k1, self.b, self.lucene, self.skip_ids, self.dim_voc)
        self.device_csr = None
        # SparseIndexer's index statistics: distinct terms per document, over all N documents
        index_stats = {"L0_d": float(sum(int(c.numel()) for c in dev_cols)) / max(1, count)}
        if dev_rows:
            indptr, rows_t, tf_t = sparse_csr_build(torch.cat(dev_rows), torch.cat(dev_cols), torch.cat(dev_vals), self.dim_voc)
            del dev_rows, dev_cols, dev_vals
            if self.index_dir is not None:
                self.sparse_index.set_csr(indptr.cpu().numpy(), rows_t.cpu().numpy(), tf_t.cpu().numpy(), count)
            else:
                self.sparse_index.set_device_csr(indptr, rows_t, tf_t, count)
                self.device_csr = (indptr, rows_t, tf_t, count)
        if self.index_dir is None:
            return {"index": self.sparse_index, "ids_mapping": doc_ids, "device_csr": self.device_csr, "doc_len": doc_len,
                    "bm25_stats": self.stats, "stats": index_stats}
        self.sparse_index.save()
        with open(os.path.join(self.index_dir, "doc_ids.pkl"), "wb") as f:
            pickle.dump(doc_ids, f)
        np.save(os.path.join(self.index_dir, "doc_len.npy"), doc_len.cpu().numpy())
        with open(os.path.join(self.index_dir, "bm25_stats.json"), "w") as f:
            json.dump(self.stats, f)
        with open(os.path.join(self.index_dir, "index_stats.json"), "w") as f:
            json.dump(index_stats, f)
        print("index contains {} posting lists".format(len(self.sparse_index)))
        print("index contains {} documents, {} with a term".format(count, len(doc_ids)))


# --------------------------------------------------------------------------------------------------------------------- retrieval
class Bm25Retrieval(SparseRetrieval):
    """SparseRetrieval over a Bm25Indexer's index.  config / index_d as SparseRetrieval ({"index_dir", "out_dir"}, or {"out_dir"} with
    the dict Bm25Indexer.index returned).  skip_ids, k1, b, lucene: None = what bm25_stats.json records.  query_tf: a query term's
    weight is its number of occurrences in the query; False: 1.0.  No k3 saturation."""

    QUERY_GROUP_ROWS = 1 << 62          # retrieve(): one search of the whole query set - token counts need no [rows, V] buffer

    def __init__(self, config, dim_voc, device, skip_ids=None, index_d=None, k1=None, b=None, lucene=None, query_tf=True, **kw):
        if get_world_size() > 1:
            raise NotImplementedError(_SHARDED)
        if index_d is not None:
            stats, doc_len = index_d["bm25_stats"], index_d["doc_len"]
            self._dcsr, index_d = index_d.get("device_csr"), dict(index_d, device_csr=None)     # weighted below, not adopted as it is
        else:
            with open(os.path.join(config["index_dir"], "bm25_stats.json")) as f:
                stats = json.load(f)
            doc_len, self._dcsr = np.load(os.path.join(config["index_dir"], "doc_len.npy")), None
        self.bm25_stats = dict(stats)
        self.k1 = float(stats["k1"] if k1 is None else k1)
        self.b = float(stats["b"] if b is None else b)
        self.lucene = bool(stats["lucene"] if lucene is None else lucene)
        self.skip_ids = sorted({int(x) for x in (stats["skip_ids"] if skip_ids is None else skip_ids)})
        self.query_tf = bool(query_tf)
        self.dim_voc = int(dim_voc if dim_voc is not None else stats["dim_voc"])
        bm25_scalars(self.k1, self.b, 1.0, self.lucene)      # the argument check, before anything is loaded
        self._doc_len_src = doc_len
        super().__init__(None, config, self.dim_voc, device, index_d=index_d, **kw)

    def _build_hip_index(self, dim_voc, dev):
        n_docs = int(self.bm25_stats["n_docs"])
        if self._dcsr is not None:
            indptr_t, ids_t, tf_t, _ = self._dcsr
            if indptr_t.numel() - 1 < dim_voc:
                indptr_t = torch.cat([indptr_t, indptr_t[-1:].expand(dim_voc + 1 - indptr_t.numel())])
        else:
            indptr_t, ids_t, tf_t = _csr_sorted_by_doc(*self.sparse_index.csr(dim_voc), dev)
        self._dcsr = None
        self.sparse_index.n = max(self.sparse_index.nb_docs(), n_docs)      # trailing documents without a term count too
        self._postings = (indptr_t.to(torch.int64).contiguous(), ids_t, tf_t)
        self._doc_len = torch.as_tensor(self._doc_len_src).to(device=dev, dtype=torch.int32).contiguous()
        if self._doc_len.numel() != n_docs:
            raise ValueError(f"doc_len holds {self._doc_len.numel()} lengths, bm25_stats.json counts {n_docs} documents")
        df = (self._postings[0][1:] - self._postings[0][:-1]).cpu().numpy()
        self._idf = torch.from_numpy(idf_table(df, n_docs)).to(dev)
        return self._weighted_index()

    def _weighted_index(self):
        """A SparseIndexHIP over the kept postings with the weights of the current (k1, b, lucene)."""
        indptr_t, ids_t, tf_t = self._postings
        numer, a, s = bm25_scalars(self.k1, self.b, float(self.bm25_stats["avgdl"]), self.lucene)
        weights = bm25_weights(indptr_t, ids_t, tf_t, self._doc_len, self._idf, numer, a, s)
        return SparseIndexHIP(indptr_t, ids_t, weights, max(1, int(self.bm25_stats["n_docs"])), device=self._dev)

    def set_params(self, k1, b, lucene=None):
        """Re-weight from the kept frequencies: the index of a fresh Bm25Retrieval with these parameters."""
        bm25_scalars(k1, b, 1.0, self.lucene if lucene is None else lucene)
        self.k1, self.b = float(k1), float(b)
        if lucene is not None:
            self.lucene = bool(lucene)
        self.hip_index.close()
        with torch.cuda.device(self._dev):
            self.hip_index = self._weighted_index()

    def _generate_query_vecs(self, q_loader):
        """The query CSR of a loader's batches: per query its distinct counted tokens with their counts (query_tf) or 1.0."""
        parts, qids = [], []
        dev = self._dev
        for batch in q_loader:
            qids.extend(batch["ids"] if isinstance(batch["ids"], list) else to_list(batch["ids"]))
            mask = batch.get("attention_mask")
            row_ptr, cols, vals, _ = token_counts(batch["input_ids"].to(dev), None if mask is None else mask.to(dev), self.skip_ids, self.dim_voc)
            parts.append(QueryCSR(row_ptr, cols, vals if self.query_tf else torch.ones_like(vals)))
        if not parts:
            return QueryCSR(torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                            torch.zeros(0, dtype=torch.float32, device=dev)), qids
        return QueryCSR.cat(parts), qids
