"""Retrieval / indexing layer: host-side mirror of
/root/reference/scaling_retriever/indexer.py for the eval path -
store_embs (:26-97), DenseIndexer / DenseFlatIndexer (:127-217), SparseIndexer (:220-308),
SparseRetrieval (:311-540) - with every arithmetic step on the MI355X:

  reference (CPU)                                   here (HIP, via libsr_hip.so)
  faiss.IndexFlatIP.add / .search                   DenseIndexHIP: D resident in HBM, fp32 MFMA + fused top-k
  numba_score_float + select_topk, 4 threads        SparseIndexHIP: LDS-tiled posting scan + fused top-k, batched
  torch.nonzero + python per-posting append         sr_sparse_compact (device CSR) + one sort by term
  model.encode under torch.autocast(bf16)           LlamaBiDense/LlamaBiSparse.encode (HIP Llama forward)

Same class / method names, arguments, artefact files (embs_{rank}_{chunk}.npy, ids_*.npy,
plan.json, doc_ids.pkl, index_dist.json, index_stats.json, run.json, q_stats.json).
"""
import ctypes
import json
import logging
import os
import pickle
from collections import defaultdict
from typing import List

import numpy as np
import torch
from tqdm import tqdm

from . import _lib
from .doc_filter import Filter, FilterKeywords, allowed_positions_on, doc_mask_remap, one_filter, range_filter_kwargs
from .scoring import DenseIndexHIP, SparseIndexHIP, sparse_csr_build, sparse_csr_expand_terms
from .utils.inverted_index import IndexDictOfArray
from .utils.run_file import IdTable, PiecewiseRunWriter, RunResult, id_table, to_host, write_run_json
from .utils.utils import get_rank, get_world_size, is_first_worker, to_list

logger = logging.getLogger()


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def _dense_queries(query_reps, device):
    """Query vectors as given (a tensor on any device, or an array) -> fp32 on the index's device."""
    if isinstance(query_reps, torch.Tensor):
        return query_reps.to(device=device, dtype=torch.float32)
    return torch.from_numpy(np.ascontiguousarray(query_reps, dtype=np.float32)).to(device)


def _search_filter(filt):
    """The subset= / mask= keyword of the index classes' `search` for a resolved doc_filter.Filter (None: none)."""
    return {} if filt is None else {filt.kind: filt.data}


def _collapse_filter(filt):
    """The filter keywords of the index classes' `search_collapsed` for a resolved doc_filter.Filter (None: none)."""
    if filt is not None and filt.kind == "groups":
        return dict(masks=filt.data, query_group=filt.groups)
    return _search_filter(filt)


def _collapse_stats(route):
    """collapse.route_stats plus, where the search computed hits, their mean number per returned group (q_stats.json)."""
    from .collapse import route_stats
    out = route_stats(route)
    if "mean_hits" in route:
        out["mean_hits"] = float(route["mean_hits"])
    return out


def _hits_run(qids, hits, table):
    """The passage-level run of a collapsed search's hits (scores [nq, k, m], ids [nq, k, m], counts [nq, k] on the device): packed to
    left-aligned rows there (collapse.pack_hits), a RunResult over the id table of the head."""
    from .collapse import pack_hits
    scores, ids, counts = pack_hits(*hits)
    return RunResult(qids, to_host(scores), to_host(ids), table, to_host(counts))


def _dump_hits_run(hits_res, out_dir):
    """{out_dir}/hits/run.json through the run writer."""
    os.makedirs(os.path.join(out_dir, "hits"), exist_ok=True)
    hits_res.dump(os.path.join(out_dir, "hits", "run.json"))


def batch_groups(loader, max_rows=16384):
    """Consecutive collator batches of `loader`, grouped until `max_rows` rows: one LlamaBi*.encode_batches call per group.
    The reference's query loaders yield eval_batch_size (128) rows at a time (eval_dense.py:219-220, eval_sparse.py:125-127);
    the engine wants tens of thousands of tokens per pass."""
    group, rows = [], 0
    for batch in loader:
        n = len(batch["ids"])
        if group and rows + n > max_rows:
            yield group
            group, rows = [], 0
        group.append(batch)
        rows += n
    if group:
        yield group


def encode_group(model, group, device, which="encode"):
    """Encode one group of collator batches: encode_batches when the model has it (bit-identical rows, one engine pass),
    else batch by batch like the reference."""
    inputs = [{k: v.to(device) for k, v in batch.items() if k != "ids"} for batch in group]
    if len(inputs) > 1 and hasattr(model, "encode_batches"):
        return model.encode_batches(inputs)
    outs = [getattr(model, which)(**i) for i in inputs]
    if isinstance(outs[0], tuple):
        return tuple(torch.cat(o) for o in zip(*outs))
    return torch.cat(outs) if len(outs) > 1 else outs[0]


STORE_GROUP_ROWS = 512          # store_embs: fixed-size loader batches encoded per engine pass (4 batches of 128)


# =============================================================== dense: corpus encode
def store_embs(model, collection_loader, local_rank, index_dir, device, chunk_size=2_000_000, use_fp16=False,
               is_query=False, idx_to_id=None):
    """indexer.py:26-97.  Encodes this rank's shard and writes embs_{rank}_{chunk}.npy (fp32 [n, H]),
    ids_{rank}_{chunk}.npy and (rank 0) plan.json.  Embeddings stay on the device until a chunk is full,
    so there is one D2H copy per chunk instead of one per batch (indexer.py:56)."""
    if is_query:
        raise NotImplementedError
    batch_size = getattr(collection_loader, "batch_size", None)
    if is_first_worker():
        print("batch_size: {}, chunk_size: {}".format(batch_size if batch_size else "token budget", chunk_size))
    os.makedirs(index_dir, exist_ok=True)
    enc = _unwrap(model)
    embeddings, embeddings_ids = [], []
    chunk_idx = 0
    # a chunk is closed after `chunk_size` passages; with fixed-size batches that is every chunk_size // batch_size
    # batches, exactly the reference's write_freq (indexer.py:32-33, :60)
    chunk_docs = max(1, chunk_size // batch_size) * batch_size if batch_size else chunk_size

    # A full chunk leaves the device on a side stream and is written by ONE background thread while the next chunk is being
    # encoded: at MS MARCO scale a chunk is 2 M x H fp32 = 16 GB - a third of a second of PCIe and several seconds of np.save
    # during which the GPU would otherwise idle.  One chunk in flight; files appear in chunk order.
    from concurrent.futures import ThreadPoolExecutor
    writer = ThreadPoolExecutor(max_workers=1)
    pending = []
    on_gpu = torch.cuda.is_available() and torch.device(device).type == "cuda"
    side = torch.cuda.Stream(device=device) if on_gpu else None

    def flush():
        nonlocal embeddings, embeddings_ids, chunk_idx
        embs_dev = torch.cat(embeddings).float()
        ids = embeddings_ids
        if isinstance(ids[0], int):
            ids = np.array(ids, dtype=np.int64)
        assert len(embs_dev) == len(ids), (len(embs_dev), len(ids))
        while pending:                          # at most one chunk in flight (host and device memory stay bounded)
            pending.pop().result()
        if on_gpu:
            host = torch.empty(embs_dev.shape, dtype=torch.float32, pin_memory=True)
            side.wait_stream(torch.cuda.current_stream(embs_dev.device))
            with torch.cuda.stream(side):
                host.copy_(embs_dev, non_blocking=True)
                done = torch.cuda.Event()
                done.record(side)
            embs_dev.record_stream(side)
        else:
            host, done = embs_dev, None

        def write(host=host, ids=ids, done=done, ci=chunk_idx):
            if done is not None:
                done.synchronize()
            np.save(os.path.join(index_dir, "embs_{}_{}.npy".format(local_rank, ci)), host.numpy())
            np.save(os.path.join(index_dir, "ids_{}_{}.npy".format(local_rank, ci)), ids)
        pending.append(writer.submit(write))
        embeddings, embeddings_ids = [], []
        chunk_idx += 1

    try:
        total = len(collection_loader)
    except TypeError:
        total = None              # token-budget loaders do not know their batch count up front
    # The reference's loader yields fixed batches of per_device_eval_batch_size passages (128: ~9 600 real tokens), less than the
    # engine wants per pass.  Fixed-size batches are therefore encoded a few at a time in ONE engine pass (encode_batches: every row
    # keeps the positions of its own batch, so the vectors are those of batch-by-batch doc_encode calls, bit for bit); a
    # token-budget loader's batches are already sized for the engine and go one by one.  Chunk files keep the reference's row
    # counts: a group's rows are appended batch by batch, with the flush check in between.
    group_rows = STORE_GROUP_ROWS if (batch_size and hasattr(enc, "encode_batches")) else 0
    progress = tqdm(disable=not is_first_worker(), desc="encode # {} seqs".format(total if total is not None else "?"), total=total)
    for group in (batch_groups(collection_loader, group_rows) if group_rows else ([b] for b in collection_loader)):
        with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):      # indexer.py:46-52
            if len(group) > 1:
                reps_g = encode_group(enc, group, device, which="doc_encode")
            else:
                inputs = {k: v.to(device, non_blocking=True) for k, v in group[0].items() if k != "ids"}
                reps_g = enc.doc_encode(**inputs)
        r0 = 0
        for batch in group:
            text_ids = batch["ids"]
            assert isinstance(text_ids, list)
            embeddings.append(reps_g[r0:r0 + len(text_ids)])
            r0 += len(text_ids)
            embeddings_ids.extend(text_ids)
            progress.update(1)
            if len(embeddings_ids) >= chunk_docs:
                flush()
        assert r0 == len(reps_g), (r0, len(reps_g))
    progress.close()
    if len(embeddings) != 0:
        print("last embedddings shape = {}".format((sum(len(e) for e in embeddings), embeddings[0].shape[1])))
        flush()
    while pending:
        pending.pop().result()                  # the last chunk is on disk (an exception of the writer surfaces here)
    writer.shutdown()

    plan = {"nranks": get_world_size(), "num_chunks": chunk_idx, "index_path": os.path.join(index_dir, "model.index")}
    print("plan: ", plan)
    if is_first_worker():
        with open(os.path.join(index_dir, "plan.json"), "w") as fout:
            json.dump(plan, fout)


# ================================================================ dense: flat index
class DenseIndexer(object):
    """indexer.py:127-188."""

    def __init__(self, buffer_size: int = 50000):
        self.buffer_size = buffer_size
        self.index_id_to_db_id = []
        self.index = None

    def init_index(self, vector_sz: int):
        raise NotImplementedError

    def index_data(self, doc_reps, doc_ids):
        raise NotImplementedError

    def get_index_name(self):
        raise NotImplementedError

    def search_knn(self, query_vectors, top_docs: int):
        raise NotImplementedError

    def get_files(self, path: str):
        if os.path.isdir(path):
            return os.path.join(path, "index.dpr"), os.path.join(path, "index_meta.dpr")
        return path + ".{}.dpr".format(self.get_index_name()), path + ".{}_meta.dpr".format(self.get_index_name())

    def index_exists(self, path: str):
        index_file, meta_file = self.get_files(path)
        return os.path.isfile(index_file) and os.path.isfile(meta_file)

    def _update_id_mapping(self, db_ids: List):
        self.index_id_to_db_id.extend(db_ids)
        self._id_table = self._run_table = None
        return len(self.index_id_to_db_id)

    def id_table(self):
        """index_id_to_db_id as one object array (+ a trailing None for faiss' label -1), rebuilt when the list grew: the id
        mapping of search_knn is ONE numpy take instead of a Python loop over every hit (indexer.py:212-213)."""
        ids = self.index_id_to_db_id
        n = len(ids)
        # the reference lets callers assign or edit index_id_to_db_id directly (deserialize, :189): the cache is tied to the list object,
        # its length and its first / last entries, so a re-assigned or re-loaded list of the same length is not served stale ids
        stamp = (id(ids), n, ids[0] if n else None, ids[-1] if n else None)
        cached = getattr(self, "_id_table", None)
        if cached is None or getattr(self, "_id_table_stamp", None) != stamp:
            cached = np.empty(n + 1, dtype=object)
            cached[:n] = ids
            cached[n] = None
            self._id_table = cached
            self._id_table_stamp = stamp
            self._run_table = None
        return cached

    def run_table(self):
        """The same ids as an IdTable (typed keys of run.json)."""
        self.id_table()
        if getattr(self, "_run_table", None) is None:
            self._run_table = IdTable(self.index_id_to_db_id)
        return self._run_table


class DenseFlatIndexer(FilterKeywords, DenseIndexer):
    """indexer.py:191-217 over a flat inner-product index resident in HBM."""

    def __init__(self, buffer_size: int = 50000):
        super().__init__(buffer_size)
        self.hidden_dim = None

    def init_index(self, hidden_dim, storage="fp32"):
        """storage="fp16": the rows are kept as float16 (fp32 input is rounded once, at ingest; half the HBM, and every result is bit
        for bit that of an fp32 index over the rounded rows: DenseIndexHIP).  float16 input is stored as it is under either setting."""
        self.hidden_dim = int(hidden_dim)
        self.storage = storage
        self.index = DenseIndexHIP(self.hidden_dim, row_dtype=storage)
        # IndexFlatIP's exact results (bit-identical to the exact fp32 kernel) through the certified bf16 filter + exact
        # re-score; the library uses the exact kernel by itself when HBM has no room for the filter's bf16 planes
        if self.hidden_dim % 64 == 0:
            self.index.set_precision("fp32_filtered")

    def index_data(self, doc_reps, doc_ids):
        assert len(doc_reps) == len(doc_ids)
        n = len(doc_reps)
        if isinstance(doc_reps, torch.Tensor) and doc_reps.is_cuda:
            self.index.add_device_rows(doc_reps if doc_reps.dtype == torch.float16 else doc_reps.float())
        else:
            self.index.add_host_rows(doc_reps if isinstance(doc_reps, np.ndarray) else np.asarray(doc_reps), buffer_size=self.buffer_size)
        n_total = self._update_id_mapping(list(doc_ids))
        logger.info("total data indexed %d", n_total)
        assert self.index.ntotal == n_total, (self.index.ntotal, n_total)
        return n

    def id_lists(self, positions):
        """[[db id of p for p in row] for row in positions] (indexer.py:212-213) for a C-contiguous int64 [nq, k] array of index
        positions; -1 -> None.  csrc/host_lists.c visits the id objects in index order instead of hit order (7 M references over a
        500 MB object heap: a TLB miss each in hit order); the lists hold the index's own id objects, as the reference's do."""
        from . import _host_lists
        table = self.id_table()
        positions = np.ascontiguousarray(positions, dtype=np.int64)
        return _host_lists.take_rows(table.ctypes.data, len(table) - 1, positions.ctypes.data, positions.shape[0], positions.shape[1])

    def range_search(self, query_reps, thresholds, sort=True, allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None):
        """Every document scoring above a threshold (faiss's IndexFlatIP.range_search; the dense counterpart of the threshold of
        numba_score_float, indexer.py:315-344): (list of db-id lists, list of fp32 score arrays), one pair per query, of the documents
        with score > thresholds (a float, or one value per query).  sort=True: best first, ties by index position, so a list is a
        prefix of what search_knn ranks; False: index order.  The ids go through id_table in one numpy take (the ragged counterpart
        of id_lists).  allowed_ids / allowed_mask (one of them at most) as for search_knn: only these documents are returned - the
        lists are the unrestricted ones with every other document removed (DenseIndexHIP.range_search, mask; faiss's range_search with
        an IDSelector).  allowed_masks bool [G, index positions] with query_group int [nq], as for search_knn: a filter per query - the
        lists of query q hold documents of allowed_masks[query_group[q]] only (DenseIndexHIP.range_search, masks / query_group); not
        together with a filter for all queries."""
        filt = self._resolve("range_search", allowed_ids, allowed_mask, allowed_masks, query_group)
        q = _dense_queries(query_reps, self.index.device)
        how = range_filter_kwargs(filt, q.shape[0], self.index.id_end, self.index.device)
        lims, scores, positions = self.index.range_search(q, thresholds, sort=sort, **how)
        lims, scores = lims.cpu().numpy(), scores.cpu().numpy()
        flat = self.id_table()[positions.cpu().numpy()]
        return ([flat[a:b].tolist() for a, b in zip(lims[:-1], lims[1:])],
                [scores[a:b] for a, b in zip(lims[:-1], lims[1:])])

    KNN_CHUNKS = 2          # search_knn pipelines the query set in this many pieces when it is large (>= 1 024 queries)

    def _filter_space(self):
        return self.index.device, self.index.id_end, "index position"

    def search_knn(self, query_reps, top_docs: int, allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None):
        """indexer.py:210-214: (list of db-id lists, fp32 scores [nq, k]); label -1 (fewer than k vectors) -> None.  allowed_ids (None:
        the whole index): database ids, any order, duplicates allowed - only these documents are ranked (DenseIndexHIP.search, subset).
        allowed_mask: the same filter as a boolean array over index positions (DenseIndexHIP.search, mask); one of the two at most.
        allowed_masks bool [G, index positions] with query_group int [nq]: a filter per query - query q is ranked within the documents of
        allowed_masks[query_group[q]] (DenseIndexHIP.search_grouped); not together with a filter for all queries.
        The lists come
        from id_lists (csrc/host_lists.c).  A large query set is searched in KNN_CHUNKS pieces, the GPU working on piece c + 1 (in a
        worker thread: the C call releases the GIL) while this thread builds the lists of piece c - the exact results do not depend
        on how the queries are batched (pieces stay above 64 queries: one kernel family, one k order)."""
        filt = self._resolve("search_knn", allowed_ids, allowed_mask, allowed_masks, query_group)
        q = _dense_queries(query_reps, self.index.device)
        nq = q.shape[0]
        if filt is not None and filt.kind == "groups" and filt.groups.numel() != nq:
            raise ValueError(f"search_knn: query_group must hold one group id per query ({nq}), got {filt.groups.numel()}")
        n_chunks = self.KNN_CHUNKS if nq >= 1024 else 1
        if n_chunks == 1:
            scores, indexes = self.search_arrays(q, top_docs, _filter=filt)
            return self.id_lists(indexes), scores
        from concurrent.futures import ThreadPoolExecutor
        per = (nq + n_chunks - 1) // n_chunks
        bounds = [(c0, min(nq, c0 + per)) for c0 in range(0, nq, per)]
        dev = self.index.device
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))          # q may come from a side stream of the caller
        grouped = filt is not None and filt.kind == "groups"

        def gpu(c):
            with torch.cuda.device(dev):
                torch.cuda.current_stream(dev).wait_event(ready)          # the worker thread's current stream is the default one
                part = filt._replace(groups=filt.groups[bounds[c][0]:bounds[c][1]]) if grouped else filt
                return self.search_arrays(q[bounds[c][0]:bounds[c][1]], top_docs, _filter=part)
        top_doc_ids, score_parts = [], []
        with ThreadPoolExecutor(max_workers=1) as pool:
            fut = pool.submit(gpu, 0)
            for c in range(len(bounds)):
                scores, indexes = fut.result()
                if c + 1 < len(bounds):
                    fut = pool.submit(gpu, c + 1)
                top_doc_ids.extend(self.id_lists(indexes))
                score_parts.append(scores)
        return top_doc_ids, np.concatenate(score_parts)

    def search_arrays(self, query_reps, top_docs: int, allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None, _filter=None):
        """(scores fp32 [nq, k], index positions int64 [nq, k]; -1 = fewer than k vectors) as host arrays: what search_knn maps
        to db ids, and what the run.json writer takes as they are (utils/run_file.py).  allowed_ids / allowed_mask / allowed_masks with
        query_group as for search_knn (_filter: such a filter already resolved and on the device, doc_filter.Filter)."""
        filt = self._resolve("search_arrays", allowed_ids, allowed_mask, allowed_masks, query_group) or _filter
        q = _dense_queries(query_reps, self.index.device)
        if filt is not None and filt.kind == "groups":
            scores, indexes = self.index.search_grouped(q, top_docs, filt.data, filt.groups)
        else:
            scores, indexes = self.index.search(q, top_docs, **_search_filter(filt))
        return to_host(scores), to_host(indexes)

    def collapse_keys(self, group_of):
        """(keys np.int32 [index positions], table of group labels) of a `group_of` - a dict on the database id, a callable on it, or a
        sequence aligned with index order (collapse.key_table: built once, on the host)."""
        from .collapse import key_table
        return key_table(group_of, self.index_id_to_db_id)

    def search_collapsed(self, query_reps, top_docs: int, group_of, depths=None, fallback_bytes=1 << 30, allowed_ids=None, allowed_mask=None,
                         allowed_masks=None, query_group=None, return_stats=False, hits=None):
        """The top_docs best GROUPS of every query, each represented and scored by its best passage (MaxP; DenseIndexHIP.search_collapsed,
        collapse.py): group_of gives each passage's group label - a dict on the database id, a callable on it, or a sequence aligned with
        index order.  Returns one (group_labels, scores fp32, passage_db_ids) triple per query, best group first (fewer than top_docs
        groups: shorter lists); return_stats=True: also the route statistics of the driver.  Filters as for search_knn.
        hits=m (1 <= m <= 64; None: off): every triple gains a fourth element, per group its (passage_db_ids, scores fp32) - the up to m
        best passages of the group that the filter allows, best first (collapse.group_hits); the first is the group's passage above."""
        filt = self._resolve("search_collapsed", allowed_ids, allowed_mask, allowed_masks, query_group)
        keys, table = self.collapse_keys(group_of)
        q = _dense_queries(query_reps, self.index.device)
        found = self.index.search_collapsed(q, top_docs, keys, depths=depths, fallback_bytes=fallback_bytes, hits=hits, **_collapse_filter(filt))
        scores, positions, gkeys, counts = (to_host(t) for t in found[:4])
        stats = found[4]
        ids = self.id_lists(positions)
        out = [([table[g] for g in gkeys[i, :c].tolist()], scores[i, :c].copy(), ids[i][:c]) for i, c in enumerate(counts.tolist())]
        if hits is not None:
            h_scores, h_pos, h_counts = (to_host(t) for t in found[5])
            m = h_scores.shape[2]
            h_ids = self.id_lists(h_pos.reshape(h_pos.shape[0], -1))
            h_n = np.minimum(h_counts, m)
            out = [row + ([(h_ids[i][j * m:j * m + n], h_scores[i, j, :n].copy()) for j, n in enumerate(h_n[i, :len(row[0])].tolist())],)
                   for i, row in enumerate(out)]
        return (out, stats) if return_stats else out

    def search_mmr(self, query_reps, top_docs: int, fetch_k: int, lam=0.5, allowed_ids=None, allowed_mask=None, allowed_masks=None,
                   query_group=None):
        """Diversified search_knn (DenseIndexHIP.search_mmr): the top fetch_k of every query, then top_docs picks by exact
        greedy MMR with lambda = lam over the stored rows.  Returns (list of db-id lists in selection order, relevance fp32 [nq, top_docs] =
        the picks' search scores, marginal values fp32 [nq, top_docs]); a query with fewer picks has a shorter list and -FLT_MAX padding.
        top_docs <= fetch_k <= sr_mmr_max_candidates(), lam in [0, 1]; filters as for search_knn."""
        from .mmr import mmr_arguments
        mmr_arguments("search_mmr", top_docs, fetch_k, lam, allowed_masks, query_group, allowed_ids=allowed_ids, allowed_mask=allowed_mask)
        filt = self._resolve("search_mmr", allowed_ids, allowed_mask, allowed_masks, query_group)
        q = _dense_queries(query_reps, self.index.device)
        ids, rel, mmr, _, counts = self.index.search_mmr(q, top_docs, fetch_k, lam, **_collapse_filter(filt))
        lists = self.id_lists(to_host(ids))
        return [row[:c] for row, c in zip(lists, to_host(counts).tolist())], to_host(rel), to_host(mmr)

    def search_prf(self, query_reps, top_docs: int, n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, fb_depth=None, allowed_ids=None,
                   allowed_mask=None, allowed_masks=None, query_group=None):
        """search_knn with pseudo-relevance feedback (DenseIndexHIP.search_prf): the top fb_depth (default n_pos) of every
        query, Rocchio's rebuilt query from the first n_pos (and, with n_neg > 0, the last n_neg) of them, then the search at top_docs
        with the new queries under the same filter.  Returns (list of db-id lists, fp32 scores [nq, top_docs], the new queries fp32
        [nq, dim]) as host values; filters as for search_knn."""
        from .prf import prf_arguments
        prf_arguments("search_prf", n_pos, n_neg, alpha, beta, gamma, first_round=True, fb_depth=fb_depth, allowed_masks=allowed_masks,
                      query_group=query_group, allowed_ids=allowed_ids, allowed_mask=allowed_mask)
        filt = self._resolve("search_prf", allowed_ids, allowed_mask, allowed_masks, query_group)
        q = _dense_queries(query_reps, self.index.device)
        scores, ids, new = self.index.search_prf(q, top_docs, n_pos, n_neg, alpha, beta, gamma, fb_depth=fb_depth, **_collapse_filter(filt))
        return self.id_lists(to_host(ids)), to_host(scores), to_host(new)

    def inverse_id_map(self):
        """str(db id) -> index position, cached with the id table (rebuilt when the list grew)."""
        from .rerank import InverseIdMap
        self.id_table()                                   # refreshes the stamp; a changed list drops the cache below
        stamp = self._id_table_stamp
        if getattr(self, "_inverse", None) is None or self._inverse[0] != stamp:
            self._inverse = (stamp, InverseIdMap(self.index_id_to_db_id))
        return self._inverse[1]

    def score_candidates(self, query_reps, doc_id_lists, qids=None):
        """Exact scores of given candidates (what eval_reranker.py computes by re-encoding every pair): query_reps [nq, dim],
        doc_id_lists = nq lists of database ids (what run.json holds); an id the index does not hold raises KeyError naming it.
        Returns a RunResult (rows sorted by score descending, ties by index position ascending; `.dump(path)` writes run.json).
        The scores are DenseIndexHIP.score_pairs's: the bits a search of more than 64 queries returns for the pair."""
        from .rerank import ranked_run
        q = _dense_queries(query_reps, self.index.device)
        assert len(doc_id_lists) == q.shape[0], (len(doc_id_lists), q.shape[0])
        indptr, positions = self.inverse_id_map().positions(doc_id_lists)
        pos_t = torch.from_numpy(positions).to(self.index.device)
        indptr_t = torch.from_numpy(indptr).to(self.index.device)
        scores = self.index.score_pairs(q, indptr, pos_t)       # index positions are the global doc indices (segments are added in order)
        return ranked_run(list(range(q.shape[0])) if qids is None else qids, scores, pos_t, pos_t, indptr_t, self.run_table())

    def get_index_name(self):
        return "flat_index"

    def serialize(self, file: str):
        """indexer.py:145-159 writes a faiss file; here the same two files hold the raw rows as they are stored (an fp32 or a
        float16 npy) + the pickled id map (faiss' binary format is not reproduced)."""
        if os.path.isdir(file):
            index_file, meta_file = os.path.join(file, "index.dpr"), os.path.join(file, "index_meta.dpr")
        else:
            index_file, meta_file = file + ".index.dpr", file + ".index_meta.dpr"
        rows = torch.cat([s for s in self.index._segments]).cpu().numpy()
        with open(index_file, "wb") as f:
            np.save(f, rows)
        with open(meta_file, mode="wb") as f:
            pickle.dump(self.index_id_to_db_id, f)

    def deserialize(self, path: str):
        index_file, meta_file = self.get_files(path)
        if not os.path.isfile(index_file):   # the reference's serialize() naming (".index.dpr")
            index_file, meta_file = path + ".index.dpr", path + ".index_meta.dpr"
        with open(index_file, "rb") as f:
            rows = np.load(f)
        self.init_index(rows.shape[1], storage="fp16" if rows.dtype == np.float16 else "fp32")
        self.index.add_host_rows(rows, buffer_size=self.buffer_size)
        with open(meta_file, "rb") as reader:
            self.index_id_to_db_id = pickle.load(reader)
        assert len(self.index_id_to_db_id) == self.index.ntotal, \
            "Deserialized index_id_to_db_id should match faiss index size"


# ======================================================================= sparse reps
def sparse_reps_to_csr(reps, max_terms=0):
    """[B, V] fp32 cuda tensor -> (row_ptr int64 [B+1], cols int32 [nnz], vals fp32 [nnz]) cuda tensors in
    torch.nonzero order (indexer.py:259-260, :393-399), via sr_sparse_compact.
    max_terms > 0 (no reference counterpart): a row keeps only its max_terms largest non-zeros - value descending, ties to the
    lower column, still emitted with cols ascending and values unchanged (sr_sparse_compact_topm); 0 = every non-zero."""
    lib = _lib.load()
    reps = reps.contiguous().float()
    B, V = reps.shape
    row_ptr = torch.empty(B + 1, dtype=torch.int64, device=reps.device)
    max_terms = int(max_terms)
    if max_terms != 0:
        if max_terms < 0:
            raise ValueError(f"max_terms must be >= 0 (0 = no limit), got {max_terms}")
        cap = max(1, min(B * V, B * max_terms))          # the budget bounds the output: no retry
        n = ctypes.c_int64(0)
        with torch.cuda.device(reps.device):
            cols = torch.empty(cap, dtype=torch.int32, device=reps.device)
            vals = torch.empty(cap, dtype=torch.float32, device=reps.device)
            _lib.check(lib.sr_sparse_compact_topm(reps.data_ptr(), B, V, max_terms, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(),
                                                  cap, ctypes.byref(n), _lib.stream_ptr()), "sr_sparse_compact_topm")
        return row_ptr, cols[:n.value], vals[:n.value]
    cap = max(1, min(B * V, 1 << 22))
    n = ctypes.c_int64(0)
    with torch.cuda.device(reps.device):
        while True:
            cols = torch.empty(cap, dtype=torch.int32, device=reps.device)
            vals = torch.empty(cap, dtype=torch.float32, device=reps.device)
            rc = lib.sr_sparse_compact(reps.data_ptr(), B, V, row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), cap,
                                       ctypes.byref(n), _lib.stream_ptr())
            if rc == _lib.SR_ERR_NOMEM and n.value > cap:
                cap = n.value
                continue
            _lib.check(rc, "sr_sparse_compact")
            break
    return row_ptr, cols[:n.value], vals[:n.value]


class L0:
    """losses/regulariaztion.py:9-14 (index statistics only)."""

    def __call__(self, batch_rep):
        return torch.count_nonzero(batch_rep, dim=-1).float().mean()


# ===================================================================== sparse: indexing
class SparseIndexer:
    """indexer.py:220-308.  The per-batch nonzero extraction runs on the device; postings are appended
    as arrays (no per-posting Python loop)."""

    def __init__(self, model, index_dir, device, compute_stats=False, dim_voc=None, force_new=True,
                 filename="array_index.h5py", doc_max_terms=0, **kwargs):
        self.model = model
        self.model.eval()
        self.index_dir = index_dir
        # per-document term budget (no reference counterpart): only the doc_max_terms largest terms of a document are indexed
        # (sparse_reps_to_csr); 0 = all of them, the reference's behaviour
        self.doc_max_terms = int(doc_max_terms)
        if self.doc_max_terms < 0:
            raise ValueError(f"doc_max_terms must be >= 0 (0 = no limit), got {doc_max_terms}")
        self.sparse_index = IndexDictOfArray(self.index_dir, dim_voc=dim_voc, force_new=force_new, filename=filename)
        self.compute_stats = compute_stats
        self.device = device
        if self.compute_stats:
            self.l0 = L0()
        self.model.to(self.device)
        self.local_rank = get_rank()
        self.world_size = get_world_size()
        print("world_size: {}, local_rank: {}".format(self.world_size, self.local_rank))

    GROUP_ROWS = 256          # index(): fixed-size loader batches encoded per engine pass (4 batches of 64)

    def _encode_batch(self, inputs, batch_ids):
        return self.model.encode(**inputs)

    def index(self, collection_loader, id_dict=None):
        doc_ids = {}
        stats = defaultdict(float)
        count = 0
        # index() builds a whole index: postings are adopted with set_csr, so a container that already holds postings
        # (a second index() call, or force_new=False over an existing file) would lose them while keeping their doc count
        if self.sparse_index.nb_docs() != 0 or len(self.sparse_index.doc_ids) != 0:
            raise ValueError("SparseIndexer.index builds a new index; this container already holds documents "
                             "(use force_new=True, or IndexDictOfArray.add_batch_document to append)")
        # COO triples stay on the device; ONE stable sort by term at the end builds the CSR (the reference appends
        # posting by posting in Python, inverted_index.py:74-76).  12 B per posting: 13.5 GB for MS MARCO at L0_d = 128.
        dev_rows, dev_cols, dev_vals = [], [], []
        n_batches = 0
        # The reference's loader yields fixed batches (64 passages: ~4 800 real tokens, a fraction of what the engine wants per
        # pass): fixed-size batches are encoded a few at a time in ONE engine pass (encode_batches: rows bit-identical to
        # batch-by-batch encode calls), then handled batch by batch exactly as before - statistics, postings and doc ids do not
        # change.  Token-budget loaders and subclasses with their own _encode_batch (HybridIndexer) go batch by batch.
        group_rows = (self.GROUP_ROWS if getattr(collection_loader, "batch_size", None) and hasattr(self.model, "encode_batches")
                      and type(self)._encode_batch is SparseIndexer._encode_batch else 0)

        def encoded_batches():
            for group in (batch_groups(collection_loader, group_rows) if group_rows else ([b] for b in collection_loader)):
                if len(group) > 1:
                    with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):  # indexer.py:255-256
                        reps_g = encode_group(self.model, group, self.device)
                    r0 = 0
                    for b in group:
                        n = len(b["ids"])
                        yield b, reps_g[r0:r0 + n]
                        r0 += n
                else:
                    yield group[0], None

        for t, (batch, batch_documents) in enumerate(tqdm(encoded_batches(), disable=not is_first_worker())):
            n_batches += 1
            batch_ids = to_list(batch["ids"]) if isinstance(batch["ids"], torch.Tensor) else batch["ids"]
            assert isinstance(batch_ids, list)
            if id_dict:
                batch_ids = [id_dict[x] for x in batch_ids]
            if batch_documents is None:
                inputs = {k: v.to(self.device) for k, v in batch.items() if k not in {"ids"}}
                with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):  # indexer.py:255-256
                    batch_documents = self._encode_batch(inputs, batch_ids)      # [bz, vocab_size] fp32 on device
            if self.compute_stats:
                stats["L0_d"] += self.l0(batch_documents).item()
            row_ptr, col, data = sparse_reps_to_csr(batch_documents, self.doc_max_terms)
            nnz_per_row = (row_ptr[1:] - row_ptr[:-1])
            if self.compute_stats and self.doc_max_terms:
                stats["L0_d_kept"] += float(col.numel()) / max(1, len(nnz_per_row))      # L0_d stays the full representation's
            row = torch.repeat_interleave(torch.arange(len(nnz_per_row), device=row_ptr.device), nnz_per_row) + count
            if (count + len(nnz_per_row)) * self.world_size + self.local_rank >= 2 ** 31:
                raise OverflowError("global document index exceeds int32 (the posting lists hold int32 doc ids, inverted_index.py:22-55)")
            dev_rows.append((row * self.world_size + self.local_rank).to(torch.int32))   # g_row = (row + count) * W + rank
            dev_cols.append(col.clone())
            dev_vals.append(data.clone())
            has_posting = np.nonzero((nnz_per_row > 0).cpu().numpy())[0]       # docs without any posting get no entry (:271-283)
            all_idxes = (count + has_posting) * self.world_size + self.local_rank
            doc_ids.update(zip(all_idxes.tolist(), (batch_ids[_i] for _i in has_posting.tolist())))
            count += len(batch_ids)
        if dev_rows:
            rows_t, cols_t, vals_t = torch.cat(dev_rows), torch.cat(dev_cols), torch.cat(dev_vals)
            del dev_rows, dev_cols, dev_vals
            V = max(int(self.sparse_index.dim_voc or 0), int(cols_t.max().item()) + 1 if cols_t.numel() else 0)
            # sr_sparse_csr_build (csrc/sparse_build.hip): this library's stable radix sort by term - insertion order kept inside a
            # term, i.e. the posting lists add_batch_document's appends would hold (inverted_index.py:67-76)
            indptr, rows_t, vals_t = sparse_csr_build(rows_t, cols_t, vals_t, V)
            del cols_t
            n_docs = (count - 1) * self.world_size + self.local_rank + 1 if self.world_size > 1 else count   # nb_docs() = max g_row + 1
            if self.index_dir is not None:       # the host copy is needed to write the files; the 12 B per posting in HBM are released
                self.sparse_index.set_csr(indptr.cpu().numpy(), rows_t.cpu().numpy(), vals_t.cpu().numpy(), n_docs)
                self.device_csr = None
            else:
                # the container carries the postings like the reference's in-memory index_d (host copy made on first use);
                # an immediately following SparseRetrieval(index_d=...) scores from the device arrays: no 13 GB round trip
                self.sparse_index.set_device_csr(indptr, rows_t, vals_t, n_docs)
                self.device_csr = (indptr, rows_t, vals_t, int(n_docs))

        if self.compute_stats:
            stats = {key: value / max(1, n_batches) for key, value in stats.items()}     # mean over batches, as the reference
        if self.index_dir is not None:
            self.sparse_index.save()
            pickle.dump(doc_ids, open(os.path.join(self.index_dir, "doc_ids.pkl"), "wb"))
            print("done iterating over the corpus...")
            print("index contains {} posting lists".format(len(self.sparse_index)))
            print("index contains {} documents".format(len(doc_ids)))
            if self.compute_stats:
                with open(os.path.join(self.index_dir, "index_stats.json"), "w") as handler:
                    json.dump(stats, handler)
        else:
            out = {"index": self.sparse_index, "ids_mapping": doc_ids, "device_csr": getattr(self, "device_csr", None)}
            if self.compute_stats:
                out["stats"] = stats
            return out


# ==================================================================== sparse: retrieval
def _csr_sorted_by_doc(indptr, doc_ids, vals, device):
    """Sort every posting list by doc id on the device (a merged multi-rank index is rank-major inside
    a term, inverted_index.py:139-146; per-doc sums do not depend on the order inside a list)."""
    indptr_t = torch.from_numpy(np.ascontiguousarray(indptr)).to(device)
    ids_t = torch.from_numpy(np.ascontiguousarray(doc_ids)).to(device)
    vals_t = torch.from_numpy(np.ascontiguousarray(vals)).to(device)
    if ids_t.numel():
        # sr_sparse_csr_build with sort_docs: stable radix passes over the doc rows, then over the terms (csrc/sparse_build.hip)
        term = sparse_csr_expand_terms(indptr_t, ids_t.numel())
        indptr2, ids_t, vals_t = sparse_csr_build(ids_t, term, vals_t, len(indptr) - 1, n_docs=int(ids_t.max().item()) + 1, sort_docs=True)
        assert torch.equal(indptr2, indptr_t.to(torch.int64))
    return indptr_t, ids_t, vals_t


class QueryCSR:
    """What _generate_query_vecs returns as `sparse_query_vecs`: the reference's list of (cols int32, vals fp32) pairs per query
    (indexer.py:393-401), held as ONE CSR on the device (row_ptr int64 [nq + 1], cols int32, vals fp32) - the form
    sr_sparse_search takes.  It still reads like the list (len, indexing, iteration give the per-query numpy pairs, from a host
    copy made on first use), so callers of the reference's interface keep working; the HIP scorer never leaves the device."""

    def __init__(self, row_ptr, cols, vals):
        self.row_ptr, self.cols, self.vals = row_ptr, cols, vals
        self._host = None

    @classmethod
    def cat(cls, parts):
        if len(parts) == 1:
            return parts[0]
        ptrs, base = [parts[0].row_ptr], int(parts[0].row_ptr[-1])
        for p_ in parts[1:]:
            ptrs.append(p_.row_ptr[1:] + base)
            base += int(p_.row_ptr[-1])
        return cls(torch.cat(ptrs), torch.cat([p_.cols for p_ in parts]), torch.cat([p_.vals for p_ in parts]))

    def host(self):
        if self._host is None:
            self._host = (self.row_ptr.cpu().numpy(), self.cols.cpu().numpy().astype(np.int32), self.vals.cpu().numpy().astype(np.float32))
        return self._host

    def __len__(self):
        return int(self.row_ptr.numel()) - 1

    def __getitem__(self, q):
        ptr, cols, vals = self.host()
        if isinstance(q, slice):
            return [self[i] for i in range(*q.indices(len(self)))]
        if q < 0:
            q += len(self)
        return cols[ptr[q]:ptr[q + 1]], vals[ptr[q]:ptr[q + 1]]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def mean_l0(self):
        n = len(self)
        return float(self.cols.numel()) / n if n else 0.0


def _as_query_csr(sparse_query_vecs, device):
    if isinstance(sparse_query_vecs, QueryCSR):
        return sparse_query_vecs
    counts = [len(c) for c, _ in sparse_query_vecs]
    row_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(device)
    cols = torch.from_numpy(np.concatenate([np.asarray(c, np.int32) for c, _ in sparse_query_vecs]) if counts else np.zeros(0, np.int32)).to(device)
    vals = torch.from_numpy(np.concatenate([np.asarray(v, np.float32) for _, v in sparse_query_vecs]) if counts else np.zeros(0, np.float32)).to(device)
    return QueryCSR(row_ptr, cols, vals)


def _doc_id_table(doc_ids, n_docs):
    """doc_ids.pkl (dict: global doc index -> collection id, docs without a posting absent; indexer.py:271-283) as an array over
    [0, n_docs): one vectorised look-up per result instead of a dict access per hit."""
    n = max(int(n_docs), (max(doc_ids) + 1) if len(doc_ids) else 0)
    keys = np.fromiter(doc_ids.keys(), dtype=np.int64, count=len(doc_ids))
    vals = list(doc_ids.values())
    # Docs without a posting have no id (they can never be hits); their slots get DISTINCT placeholders, so that a few empty documents
    # in a real collection do not make the id table look like it held duplicates (which sends run.json through the dict path)
    holes = np.ones(n, dtype=bool)
    holes[keys] = False
    hole_pos = np.nonzero(holes)[0]
    if vals and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in vals):
        table = np.full(n, -1, dtype=np.int64)
        table[keys] = np.asarray(vals, dtype=np.int64)
        if len(hole_pos):
            lo = min(int(table[keys].min()) if len(keys) else 0, 0)
            table[hole_pos] = lo - 1 - np.arange(len(hole_pos), dtype=np.int64)       # below every real id
        return table
    table = np.empty(n, dtype=object)
    table[keys] = np.asarray(vals, dtype=object)
    for j, pos in enumerate(hole_pos.tolist()):
        table[pos] = f"\x00no-posting-{j}"
    return table


class SparseRetrieval(FilterKeywords):
    """indexer.py:311-540."""

    _static_cache = None      # (the caller's dict - held, so its id cannot be recycled -, device index, n_terms)

    def __init__(self, model, config, dim_voc, device, dataset_name=None, index_d=None, compute_stats=False,
                 is_beir=False, query_max_terms=0, **kwargs):
        self.model = model
        if self.model is not None:       # None: a retriever whose queries need no encoder (bm25.Bm25Retrieval)
            self.model.eval()
        # per-query term budget (no reference counterpart): a query is searched with its query_max_terms largest terms only
        # (sparse_reps_to_csr); 0 = all of them, the reference's behaviour
        self.query_max_terms = int(query_max_terms)
        if self.query_max_terms < 0:
            raise ValueError(f"query_max_terms must be >= 0 (0 = no limit), got {query_max_terms}")
        assert ("index_dir" in config and index_d is None) or ("index_dir" not in config and index_d is not None)
        if "index_dir" in config:
            self.sparse_index, self.doc_ids = self._open_index(config["index_dir"], dim_voc)
        else:
            self.sparse_index = index_d["index"]
            self.doc_ids = index_d["ids_mapping"]
        self.device = device
        if self.model is not None:
            self.model.to(device)
        dev = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self._dev = dev
        dcsr = index_d.get("device_csr") if index_d is not None else None
        with torch.cuda.device(dev):
            if dcsr is not None and get_world_size() == 1:
                # built by SparseIndexer.index in this process: term-major, doc-ascending inside a term, already in HBM
                indptr_t, ids_t, vals_t, n_docs = dcsr
                if dim_voc is not None and indptr_t.numel() - 1 < dim_voc:
                    indptr_t = torch.cat([indptr_t, indptr_t[-1:].expand(dim_voc + 1 - indptr_t.numel())])
                self.hip_index = SparseIndexHIP(indptr_t, ids_t, vals_t, max(1, n_docs), device=dev)
            else:
                self.hip_index = self._build_hip_index(dim_voc, dev)
        self.out_dir = os.path.join(config["out_dir"], dataset_name) if (dataset_name is not None and not is_beir) \
            else config["out_dir"]
        self.doc_stats = index_d["stats"] if (index_d is not None and compute_stats) else None
        self.compute_stats = compute_stats
        if self.compute_stats:
            self.l0 = L0()

    def _open_index(self, index_dir, dim_voc):
        with open(os.path.join(index_dir, "doc_ids.pkl"), "rb") as f:
            return IndexDictOfArray(index_dir, dim_voc=dim_voc), pickle.load(f)

    def _build_hip_index(self, dim_voc, dev):
        indptr, ids, vals = self.sparse_index.csr(dim_voc)
        indptr_t, ids_t, vals_t = _csr_sorted_by_doc(indptr, ids, vals, dev)
        return SparseIndexHIP(indptr_t, ids_t, vals_t, max(1, self.sparse_index.nb_docs()), device=dev)

    # -- kept for callers of the reference's static helpers (indexer.py:315-344) ------------
    @staticmethod
    def select_topk(filtered_indexes, scores, k):
        if len(filtered_indexes) > k:
            order = np.lexsort((filtered_indexes, scores))[:k]      # scores are negated: ascending = best first
            return filtered_indexes[order], -scores[order]
        return filtered_indexes, -scores

    @staticmethod
    def numba_score_float(inverted_index_ids, inverted_index_floats, indexes_to_retrieve, query_values, threshold,
                          size_collection):
        """Same signature/returns as the reference: (doc indexes with score > threshold ascending int64,
        NEGATED scores fp32), every such document - documents without a common term included when the threshold is negative, as in
        the reference, whose score array starts at zero.  The list is one range search on the HIP index (SparseIndexHIP.range_search:
        count, scan, fill), which already comes in document order; use SparseRetrieval.retrieve or range_search for bulk work, this
        entry point exists for drop-in callers."""
        cache = SparseRetrieval._static_cache
        if cache is not None and cache[0] is inverted_index_ids and cache[3] == size_collection:
            hit = cache[1]
        else:
            terms = sorted(t for t in inverted_index_ids.keys() if len(inverted_index_ids[t]))
            V = (max(terms) + 1) if terms else 1
            counts = np.zeros(V, np.int64)
            for t in terms:
                counts[t] = len(inverted_index_ids[t])
            indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            ids = np.concatenate([np.asarray(inverted_index_ids[t], np.int32) for t in terms]) if terms else np.zeros(0, np.int32)
            vals = np.concatenate([np.asarray(inverted_index_floats[t], np.float32) for t in terms]) if terms else np.zeros(0, np.float32)
            dev = torch.device("cuda", torch.cuda.current_device())
            hit = SparseIndexHIP(*_csr_sorted_by_doc(indptr, ids, vals, dev), size_collection, device=dev)
            SparseRetrieval._static_cache = (inverted_index_ids, hit, V, size_collection)
        cols = np.asarray(indexes_to_retrieve, np.int32)
        _, sc, idx = hit.range_search(np.array([0, len(cols)], np.int64), cols, np.asarray(query_values, np.float32), float(threshold))
        return idx.cpu().numpy(), -sc.cpu().numpy()

    QUERY_GROUP_ROWS = 2048      # rows per encode_batches call: the [rows, V] fp32 reps of a group live in HBM (1 GB at V = 128 256)

    def _generate_query_vecs(self, q_loader):
        """indexer.py:382-403: encode queries, keep the nonzero (col, value) pairs per query.  The loader's batches are encoded
        group-wise in one engine pass each (encode_batches: same bits as batch by batch) and the pairs stay on the device as ONE
        CSR (QueryCSR) - no per-batch .cpu(), no per-query slicing."""
        parts, qids = [], []
        for group in tqdm(batch_groups(q_loader, self.QUERY_GROUP_ROWS), desc="generate query vecs", disable=not is_first_worker()):
            with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):  # indexer.py:390-391
                reps = encode_group(self.model, group, self.device)
            for batch in group:
                qids.extend(batch["ids"] if isinstance(batch["ids"], list) else to_list(batch["ids"]))
            parts.append(QueryCSR(*sparse_reps_to_csr(reps, self.query_max_terms)))
            del reps
        if not parts:
            dev = self._dev
            return QueryCSR(torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                            torch.zeros(0, dtype=torch.float32, device=dev)), qids
        return QueryCSR.cat(parts), qids

    def inverse_id_map(self):
        """str(collection id) -> document position of the inverted index, built once."""
        if getattr(self, "_inverse", None) is None:
            from .rerank import InverseIdMap
            self._inverse = InverseIdMap(self.doc_ids)
        return self._inverse

    def score_candidates(self, sparse_query_vecs, qids, doc_id_lists):
        """Exact scores of given candidates: sparse_query_vecs as _generate_query_vecs returns them (QueryCSR or the reference's list
        of (cols, vals) pairs), doc_id_lists = one list of collection ids per query; an unknown id raises KeyError naming it (the
        inverted index knows the documents that have a posting, doc_ids.pkl: one without any is unknown to it - HybridRetriever,
        which also has the dense index's id table, scores such a document 0.0 instead).  No threshold: a candidate that shares no term with its query is kept with score 0.0.  Returns a RunResult sorted by (score
        descending, document position ascending)."""
        from .rerank import ranked_run
        q = _as_query_csr(sparse_query_vecs, self._dev)
        assert len(doc_id_lists) == len(q) == len(qids), (len(doc_id_lists), len(q), len(qids))
        indptr, positions = self.inverse_id_map().positions(doc_id_lists)
        pos_t = torch.from_numpy(positions).to(self._dev)
        scores = self.hip_index.score_pairs(q.row_ptr, q.cols, q.vals, indptr, pos_t)
        return ranked_run(qids, scores, pos_t, pos_t, torch.from_numpy(indptr).to(self._dev), self.doc_id_table())

    def doc_id_table(self):
        if getattr(self, "_doc_table", None) is None:
            self._doc_table = IdTable(_doc_id_table(self.doc_ids, self.sparse_index.nb_docs()))
        return self._doc_table

    def range_search(self, sparse_query_vecs, thresholds=0., sort=True, allowed_ids=None, allowed_mask=None, allowed_masks=None,
                     query_group=None, _filter=None):
        """Every document scoring above a threshold - the full list of numba_score_float (indexer.py:324-344) for a whole query set,
        the counterpart of DenseFlatIndexer.range_search: (list of collection-id lists, list of fp32 score arrays), one pair per query,
        of the documents with score > thresholds (a float, or one value per query).  sparse_query_vecs as _generate_query_vecs returns
        them (QueryCSR) or the reference's list of (cols, vals) pairs.  sort=True: best first, ties by document position, so a list is
        a prefix of what retrieve ranks; False: document order.  The ids go through doc_id_table in one numpy take.
        A document without any posting has no collection id (doc_ids.pkl does not list it; the reference's doc_ids[id_] raises
        KeyError for it).  It scores 0.0 and so passes a negative threshold: such documents are left out of the lists here, their
        placeholders of doc_id_table never come back.  SparseIndexHIP.range_search returns them, by position.
        allowed_ids / allowed_mask (one of them at most) as for retrieve: only these documents are returned - the unrestricted lists
        with every other document removed (SparseIndexHIP.range_search, mask).  allowed_masks bool [G, document positions] with
        query_group int [number of queries], as for retrieve: a filter per query - the lists of query q hold documents of
        allowed_masks[query_group[q]] only (SparseIndexHIP.range_search, masks / query_group); not together with a filter for all queries
        (_filter: such a filter already resolved and on the device, doc_filter.Filter)."""
        filt = self._resolve("range_search", allowed_ids, allowed_mask, allowed_masks, query_group) or _filter
        q = _as_query_csr(sparse_query_vecs, self._dev)
        how = range_filter_kwargs(filt, len(q), self.hip_index.n_docs, self._dev)
        lims, scores, positions = self.hip_index.range_search(q.row_ptr, q.cols, q.vals, thresholds, sort=sort, **how)
        lims, scores, positions = lims.cpu().numpy(), scores.cpu().numpy(), positions.cpu().numpy()
        table = self.doc_id_table()
        if len(self.doc_ids) < table.n:                      # some document has no id: drop its entries, list by list
            has_id = np.zeros(table.n, dtype=bool)
            has_id[np.fromiter(self.doc_ids.keys(), dtype=np.int64, count=len(self.doc_ids))] = True
            keep = has_id[positions]
            lims = np.concatenate([[0], np.cumsum(keep)])[lims]
            scores, positions = scores[keep], positions[keep]
        flat = table.take(positions)
        return ([flat[a:b].tolist() for a, b in zip(lims[:-1], lims[1:])],
                [scores[a:b] for a, b in zip(lims[:-1], lims[1:])])

    def _filter_space(self):
        return self._dev, self.hip_index.n_docs, "document position"

    def _search(self, q, topk, threshold, filt, row0=0):
        """One search of the query CSR `q` under a resolved filter (None: none).  Under groups the queries are rows row0 .. of the query
        set the filter's group ids were given for (SparseIndexHIP.search_grouped)."""
        if filt is not None and filt.kind == "groups":
            if row0 + len(q) > filt.groups.numel():
                raise ValueError(f"query_group must hold one group id per query, got {filt.groups.numel()} for at least {row0 + len(q)} queries")
            return self.hip_index.search_grouped(q.row_ptr, q.cols, q.vals, topk, filt.data, filt.groups[row0:row0 + len(q)], threshold=threshold)
        return self.hip_index.search(q.row_ptr, q.cols, q.vals, topk, threshold=threshold, **_search_filter(filt))

    def _sparse_retrieve_multithreaded(self, sparse_query_vecs, qids, threshold=0., topk=1000, allowed_ids=None, allowed_mask=None,
                                       allowed_masks=None, query_group=None, _filter=None):
        """allowed_ids (None: every document): collection ids - only these documents are ranked.  allowed_mask: the same filter as a
        boolean array over document positions; one of the two at most.  allowed_masks bool [G, document positions] with query_group int
        [number of queries]: a filter per query - query q is ranked within the documents of allowed_masks[query_group[q]]
        (SparseIndexHIP.search_grouped); not together with a filter for all queries (_filter: such a filter already resolved and on the
        device, doc_filter.Filter).  indexer.py:405-474 runs 4 Python threads x numba and fills res[str(qid)][str(doc_ids[id_])] hit by hit; here the
        whole query set is one batched HIP search (the doc space is tiled across workgroups instead) and `res` is a RunResult
        over the result arrays: the same mapping, without 7 M dict insertions."""
        filt = self._resolve("_sparse_retrieve_multithreaded", allowed_ids, allowed_mask, allowed_masks, query_group) or _filter
        q = _as_query_csr(sparse_query_vecs, self._dev)
        if filt is not None and filt.kind == "groups" and filt.groups.numel() != len(q):
            raise ValueError(f"query_group must hold one group id per query ({len(q)}), got {filt.groups.numel()}")
        scores, ids, counts = self._search(q, topk, threshold, filt)
        res = RunResult(qids, to_host(scores), to_host(ids), self.doc_id_table(), to_host(counts))
        stats = defaultdict(float)
        stats["L0_q"] = q.mean_l0()
        return res, stats

    def collapse_keys(self, group_of):
        """(keys np.int32 [document positions], table of group labels) of a `group_of` - a dict on the collection id, a callable on it,
        or a sequence aligned with document positions (collapse.key_table); a document without a posting has no collection id and gets a
        group of its own."""
        from .collapse import key_table
        return key_table(group_of, [self.doc_ids.get(p) for p in range(self.hip_index.n_docs)])

    def _retrieve_collapsed(self, sparse_query_vecs, qids, group_of, threshold, topk, filt, depths=None, fallback_bytes=1 << 30, hits=None):
        """One collapsed search of the whole query set (SparseIndexHIP.search_collapsed): a RunResult keyed by group label - its
        "positions" are the group keys, its id table the labels - and the stats of q_stats.json with the route statistics.  hits=m: a
        third value, the passage-level RunResult of the groups' hits (collapse.pack_hits), and "mean_hits" in the statistics."""
        q =_as_query_csr(sparse_query_vecs, self._dev)
        if filt is not None and filt.kind == "groups" and filt.groups.numel() != len(q):
            raise ValueError(f"query_group must hold one group id per query ({len(q)}), got {filt.groups.numel()}")
        keys, table = self.collapse_keys(group_of)
        found = self.hip_index.search_collapsed(q.row_ptr, q.cols, q.vals, topk, keys, threshold=threshold, depths=depths,
                                                fallback_bytes=fallback_bytes, hits=hits, **_collapse_filter(filt))
        scores, _, gkeys, counts, route = found[:5]
        res = RunResult(qids, to_host(scores), to_host(gkeys.to(torch.int64)), IdTable(table), to_host(counts))
        stats = defaultdict(float)
        stats["L0_q"] = q.mean_l0()
        stats["collapse"] = _collapse_stats(route)
        if hits is None:
            return res, stats
        return res, stats, _hits_run(qids, found[5], self.doc_id_table())

    def _write_outputs(self, res, stats, hits_res=None):
        os.makedirs(self.out_dir, exist_ok=True)
        if self.compute_stats:
            with open(os.path.join(self.out_dir, "q_stats.json"), "w") as handler:
                json.dump(stats, handler)
        res.dump(os.path.join(self.out_dir, "run.json"))        # sr_write_run_json: the bytes json.dump(res) writes
        if hits_res is not None:
            _dump_hits_run(hits_res, self.out_dir)

    def retrieve(self, q_loader, topk, threshold=0., allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None, collapse=None,
                 hits=None):
        """collapse (None: rank passages): a `group_of` - dict on the collection id, callable on it, or a sequence aligned with document
        positions - makes this the collapsed search: the topk best GROUPS per query, each scored by its best passage
        (SparseIndexHIP.search_collapsed); run.json is then keyed by group label instead of passage id, and q_stats.json gains the route
        statistics ("collapse").  The query set is searched in one call.
        hits=m (with collapse only, else ValueError; 1 <= m <= 64): also the up to m best passages inside every returned group
        (collapse.group_hits).  run.json stays the group-keyed file, byte for byte; a second, passage-level run goes to hits/run.json -
        qid -> {passage id: score}, per query the hits of its topk groups ordered by group rank, then hit rank - through the same run
        writer; q_stats.json's "collapse" gains "mean_hits"; the return value becomes (group run, hits run).
        allowed_ids (None: every document): collection ids, any order, duplicates allowed - only these documents are ranked; an unknown
        id raises ValueError before anything is encoded.  allowed_mask: the same filter as a boolean array over the document positions
        of the inverted index (SparseIndexHIP.search, mask); one of the two at most.  allowed_masks bool [G, document positions] with
        query_group int [number of queries, in loader order]: a filter per query (SparseIndexHIP.search_grouped), not together with a
        filter for all queries; the query set is searched in pieces and every piece takes its own slice of query_group.  run.json and
        q_stats.json keep their format.
        indexer.py:530-540.  Query groups of QUERY_GROUP_ROWS rows go through encode -> search one after the other while a worker
        thread writes the previous group's piece of run.json (sr_write_run_json_part): formatting and the page-cache copy of a Dev-sized
        file take as long as the encode, and nothing in them needs the GPU.  A query's rows do not depend on the batch it is searched in
        (certified or exact: the same bits), and the file is the one-call file byte for byte (tests/test_boundary_gpu.py)."""
        from .collapse import hits_of_no_collapse
        hits_of_no_collapse("retrieve", hits, collapse)
        filt = self._resolve("retrieve", allowed_ids, allowed_mask, allowed_masks, query_group)
        groups = list(batch_groups(q_loader, self.QUERY_GROUP_ROWS))
        group_qids = [[x for batch in g for x in (batch["ids"] if isinstance(batch["ids"], list) else to_list(batch["ids"]))] for g in groups]
        qids = [x for g in group_qids for x in g]
        if filt is not None and filt.kind == "groups" and filt.groups.numel() != len(qids):
            raise ValueError(f"retrieve: query_group must hold one group id per query ({len(qids)}), got {filt.groups.numel()}")
        if collapse is not None:
            sparse_query_vecs, qids = self._generate_query_vecs([batch for g in groups for batch in g])
            res, stats, *hits_res = self._retrieve_collapsed(sparse_query_vecs, qids, collapse, threshold, topk, filt, hits=hits)
            self._write_outputs(res, stats, *hits_res)
            return (res, hits_res[0]) if hits_res else res
        table = self.doc_id_table()
        if len(groups) < 2 or not (id_table(qids).distinct and id_table(table).distinct):
            sparse_query_vecs, qids = self._generate_query_vecs([batch for g in groups for batch in g])
            res, stats = self._sparse_retrieve_multithreaded(sparse_query_vecs, qids, threshold=threshold, topk=topk, _filter=filt)
            self._write_outputs(res, stats)
            return res
        os.makedirs(self.out_dir, exist_ok=True)
        path = os.path.join(self.out_dir, "run.json")
        pieces, nnz, row0 = [], 0, 0
        with PiecewiseRunWriter(path) as writer:                       # run.json appears only when its last piece is written
            for gi, group in enumerate(groups):
                with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):  # indexer.py:390-391
                    reps = encode_group(self.model, group, self.device)
                q = QueryCSR(*sparse_reps_to_csr(reps, self.query_max_terms))
                del reps
                nnz += int(q.cols.numel())
                scores, ids, counts = self._search(q, topk, threshold, filt, row0)
                row0 += len(q)
                piece = (to_host(scores), to_host(ids), to_host(counts))
                pieces.append(piece)
                writer.add(group_qids[gi], piece[0], piece[1], table, piece[2], last=gi + 1 == len(groups))
            writer.finish()
        res = RunResult(qids, np.concatenate([p_[0] for p_ in pieces]), np.concatenate([p_[1] for p_ in pieces]), table,
                        np.concatenate([p_[2] for p_ in pieces]))
        if self.compute_stats:
            stats = defaultdict(float)
            stats["L0_q"] = float(nnz) / len(qids) if qids else 0.0
            with open(os.path.join(self.out_dir, "q_stats.json"), "w") as handler:
                json.dump(stats, handler)
        return res


    def retrieve_prf(self, q_loader, topk, threshold=0., n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=128, fb_depth=None,
                     allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None):
        """`retrieve` with pseudo-relevance feedback (SparseIndexHIP.search_prf): the whole query set is encoded and
        searched at fb_depth (default n_pos), every query is rebuilt by Rocchio from the first n_pos (and, with n_neg > 0, the last n_neg)
        documents of its list and cut to its max_terms largest terms, and searched again at topk - all under the same filter and
        threshold.  Writes prf/run.json and prf/q_stats.json (L0_q of the expanded queries) under the output directory; the run.json /
        q_stats.json of a plain `retrieve` are not touched.  Returns the RunResult.  Filters as for `retrieve`; no collapse."""
        from .prf import prf_arguments
        prf_arguments("retrieve_prf", n_pos, n_neg, alpha, beta, gamma, max_terms, first_round=True, fb_depth=fb_depth,
                      allowed_masks=allowed_masks, query_group=query_group, allowed_ids=allowed_ids, allowed_mask=allowed_mask)
        filt = self._resolve("retrieve_prf", allowed_ids, allowed_mask, allowed_masks, query_group)
        q, qids = self._generate_query_vecs(q_loader)
        if filt is not None and filt.kind == "groups" and filt.groups.numel() != len(q):
            raise ValueError(f"retrieve_prf: query_group must hold one group id per query ({len(q)}), got {filt.groups.numel()}")
        scores, ids, counts, new = self.hip_index.search_prf(q.row_ptr, q.cols, q.vals, topk, n_pos, n_neg, alpha, beta, gamma, max_terms,
                                                             fb_depth=fb_depth, threshold=threshold, **_collapse_filter(filt))
        res = RunResult(qids, to_host(scores), to_host(ids), self.doc_id_table(), to_host(counts))
        out_dir = os.path.join(self.out_dir, "prf")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "q_stats.json"), "w") as handler:
            json.dump({"L0_q": QueryCSR(*new).mean_l0()}, handler)
        res.dump(os.path.join(out_dir, "run.json"))
        return res

    def retrieve_mmr(self, q_loader, topk, fetch_k, lam=0.5, sim="cosine", threshold=0., allowed_ids=None, allowed_mask=None, allowed_masks=None,
                     query_group=None):
        """`retrieve` diversified (SparseIndexHIP.search_mmr): the whole query set is encoded and searched at fetch_k, and
        exact greedy MMR with `lam` and the document-document similarity `sim` ("ip" / "cosine") selects topk of every query's rows -
        under the same filter and threshold.  Writes mmr/run.json and mmr/q_stats.json under the output directory; the run.json /
        q_stats.json of a plain `retrieve` are not touched.  A marginal value is no ranking score (pick 0's may lie below pick 1's), so
        pick t of a query with n picks carries float(n - t), eval_dense.py's convention; q_stats.json holds per query the number of
        picks, the mean marginal value and how many picks are not among the plain topk.  Returns the RunResult.  Filters as for
        `retrieve`; no collapse."""
        from .mmr import mmr_arguments
        mmr_arguments("retrieve_mmr", topk, fetch_k, lam, allowed_masks, query_group, sim=sim, allowed_ids=allowed_ids, allowed_mask=allowed_mask)
        filt = self._resolve("retrieve_mmr", allowed_ids, allowed_mask, allowed_masks, query_group)
        q, qids = self._generate_query_vecs(q_loader)
        if filt is not None and filt.kind == "groups" and filt.groups.numel() != len(q):
            raise ValueError(f"retrieve_mmr: query_group must hold one group id per query ({len(q)}), got {filt.groups.numel()}")
        ids, _, mmr, pos, counts = self.hip_index.search_mmr(q.row_ptr, q.cols, q.vals, topk, fetch_k, lam, sim=sim, threshold=threshold,
                                                             **_collapse_filter(filt))
        ids, mmr, pos, counts = to_host(ids), to_host(mmr), to_host(pos), to_host(counts)
        ranks = np.arange(topk)[None, :]
        order_scores = np.where(ranks < counts[:, None], counts[:, None] - ranks, 0).astype(np.float32)
        res = RunResult(qids, order_scores, ids, self.doc_id_table(), counts)
        out_dir = os.path.join(self.out_dir, "mmr")
        os.makedirs(out_dir, exist_ok=True)
        stats = {}
        for r, qid in enumerate(qids):
            n = int(counts[r])
            stats[str(qid)] = {"picks": n, "mean_mmr": float(mmr[r, :n].astype(np.float64).mean()) if n else None,
                               "picks_outside_top_k": int((pos[r, :n] >= topk).sum())}
        with open(os.path.join(out_dir, "q_stats.json"), "w") as handler:
            json.dump(stats, handler, indent=4)
        res.dump(os.path.join(out_dir, "run.json"))
        return res


class ShardedSparseRetrieval(SparseRetrieval):
    """Doc-sharded SparseRetrieval for world_size > 1 (the reference asserts world_size == 1, eval_sparse.py:114, and
    needs a merge_indexes pass first, scripts/eval_sparse.sh:19): rank r opens the directory `{index_dir}_{r}` the indexing
    task wrote (eval_sparse.py:98-100), scores its own documents and the per-shard top-k meet in ONE gather
    (distributed.ShardedSparseRetriever).  Every rank encodes only its block of the queries; the query CSR is
    all-gathered (distributed.all_gather_query_csr).  run.json / q_stats.json are written by rank 0."""

    def __init__(self, model, config, dim_voc, device, rank=None, world_size=None, **kwargs):
        from .distributed import ShardedSparseRetriever
        self.rank = get_rank() if rank is None else rank
        self.world_size = get_world_size() if world_size is None else world_size
        base = config["index_dir"][:-1] if config["index_dir"].endswith("/") else config["index_dir"]
        self.shard_dir = f"{base}_{self.rank}"
        self._base_dir = base
        self._shard_factory = ShardedSparseRetriever
        super().__init__(model, dict(config, index_dir=self.shard_dir), dim_voc, device, **kwargs)

    def _open_index(self, index_dir, dim_voc):
        # a shard's doc_ids.pkl holds only the global rows r, r + W, ...: count them here, not with the single-index rule
        # (IndexDictOfArray: min key == 0, inverted_index.py:44-55)
        with open(os.path.join(index_dir, "doc_ids.pkl"), "rb") as f:
            doc_ids = pickle.load(f)
        index = IndexDictOfArray(index_dir, dim_voc=dim_voc, _count_docs=False)
        index.n = (max(doc_ids) + 1) if len(doc_ids) else 0      # max g_row + 1 of THIS shard
        return index, doc_ids

    def _build_hip_index(self, dim_voc, dev):
        indptr, ids, vals = self.sparse_index.csr(dim_voc)
        self.sharded = self._shard_factory(indptr, ids, vals, self.sparse_index.nb_docs(), rank=self.rank,
                                           world_size=self.world_size, device=dev)
        return self.sharded.index

    def _all_doc_ids(self):
        ids = {}
        for r in range(self.world_size):
            with open(os.path.join(f"{self._base_dir}_{r}", "doc_ids.pkl"), "rb") as f:
                ids.update(pickle.load(f))
        return ids

    def range_search(self, sparse_query_vecs, thresholds=0., sort=True, allowed_ids=None, allowed_mask=None, allowed_masks=None,
                     query_group=None):
        if allowed_masks is not None or query_group is not None:
            raise NotImplementedError("ShardedSparseRetrieval.range_search: filter groups (allowed_masks / query_group) are not supported on "
                                      "a doc-sharded index, and neither is a range search; search one merged index with SparseRetrieval instead")
        raise NotImplementedError("ShardedSparseRetrieval.range_search: a range search is not offered on a doc-sharded index; "
                                  "search one merged index with SparseRetrieval instead")

    def search_fused(self, *args, **kwargs):
        if kwargs.get("allowed_masks") is not None or kwargs.get("query_group") is not None:
            raise NotImplementedError("ShardedSparseRetrieval.search_fused: filter groups (allowed_masks / query_group) are not supported on "
                                      "a doc-sharded index, and neither is the exact fused search; use HybridRetriever over one merged index")
        raise NotImplementedError("ShardedSparseRetrieval.search_fused: the exact fused search is not offered on a doc-sharded index; "
                                  "use HybridRetriever over one merged index")

    def retrieve_rank_fused(self, *args, **kwargs):
        raise NotImplementedError("ShardedSparseRetrieval.retrieve_rank_fused: rank fusion of the two heads' lists is not offered on a "
                                  "doc-sharded index; use HybridRetriever over one merged index, or eval_fuse.py on the run files")

    def retrieve_prf(self, *args, **kwargs):
        raise NotImplementedError("ShardedSparseRetrieval.retrieve_prf: pseudo-relevance feedback needs the rows of every feedback document "
                                  "on one device and is not offered on a doc-sharded index; search one merged index with SparseRetrieval")

    def retrieve_mmr(self, *args, **kwargs):
        raise NotImplementedError("ShardedSparseRetrieval.retrieve_mmr: the diversified search needs the forward rows of every candidate "
                                  "on one device and is not offered on a doc-sharded index; search one merged index with SparseRetrieval")

    def retrieve(self, q_loader, topk, threshold=0., allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None, collapse=None):
        """q_loader yields THIS rank's block of the queries (distributed.query_slice order) or all of them when
        `q_loader.replicated` is set."""
        if collapse is not None:
            raise NotImplementedError("ShardedSparseRetrieval.retrieve: the collapsed search (collapse=) is not supported on a doc-sharded "
                                      "index; search one merged index with SparseRetrieval instead")
        if allowed_masks is not None or query_group is not None:
            raise NotImplementedError("ShardedSparseRetrieval.retrieve: filter groups (allowed_masks / query_group) are not supported on a "
                                      "doc-sharded index; search one merged index with SparseRetrieval instead")
        if allowed_ids is not None:
            raise NotImplementedError("ShardedSparseRetrieval.retrieve: an allow-list (allowed_ids) is not supported on a doc-sharded "
                                      "index; search one merged index with SparseRetrieval instead")
        if allowed_mask is not None:
            raise NotImplementedError("ShardedSparseRetrieval.retrieve: a document bitmap (allowed_mask) is not supported on a doc-sharded "
                                      "index; search one merged index with SparseRetrieval instead")
        from .distributed import all_gather_query_csr
        import torch.distributed as dist
        q, qids = self._generate_query_vecs(q_loader)
        row_ptr, cols, vals = q.row_ptr, q.cols, q.vals
        if self.world_size > 1 and not getattr(q_loader, "replicated", False):
            all_qids = [None] * self.world_size
            dist.all_gather_object(all_qids, qids)
            qids = [q_ for part in all_qids for q_ in part]
            row_ptr, cols, vals = all_gather_query_csr(row_ptr, cols, vals, len(qids))
        scores, ids, counts_t = self.sharded.search(row_ptr, cols, vals, topk, threshold=threshold)
        if scores is None:
            return None
        doc_ids = self._all_doc_ids()
        n_docs = (max(doc_ids) + 1) if len(doc_ids) else 0
        res = RunResult(qids, to_host(scores), to_host(ids), IdTable(_doc_id_table(doc_ids, n_docs)), to_host(counts_t))
        nnz = (row_ptr[1:] - row_ptr[:-1])
        stats = {"L0_q": float(nnz.float().mean().item()) if nnz.numel() else 0.0}
        self._write_outputs(res, stats)
        return res


# ============================================================================== hybrid
class HybridIndexer(SparseIndexer):
    """indexer.py:710-857: ONE pass over the collection writes both the inverted index (sparse_index_dir) and the dense
    shard files embs_{rank}_{chunk}.npy / ids_*.npy / plan.json (dense_index_dir).  model.encode returns
    (sparse reps [B, V], dense reps [B, H]) from one backbone pass (LlamaBiHybrid -> sr_encode_both)."""

    def __init__(self, model, sparse_index_dir, dense_index_dir, device, chunk_size=2_000_000, compute_stats=False,
                 dim_voc=None, force_new=True, filename="array_index.h5py", doc_max_terms=0, **kwargs):
        super().__init__(model, sparse_index_dir, device, compute_stats=compute_stats, dim_voc=dim_voc, force_new=force_new,
                         filename=filename, doc_max_terms=doc_max_terms)
        self.sparse_index_dir, self.dense_index_dir, self.chunk_size = sparse_index_dir, dense_index_dir, chunk_size
        os.makedirs(dense_index_dir, exist_ok=True)
        self._dense, self._dense_ids, self._chunk_idx = [], [], 0

    def _flush_dense(self):
        embs = torch.cat(self._dense).numpy()
        ids = self._dense_ids
        if isinstance(ids[0], int):
            ids = np.array(ids, dtype=np.int64)
        assert len(embs) == len(ids), (len(embs), len(ids))
        np.save(os.path.join(self.dense_index_dir, "embs_{}_{}.npy".format(self.local_rank, self._chunk_idx)), embs)
        np.save(os.path.join(self.dense_index_dir, "ids_{}_{}.npy".format(self.local_rank, self._chunk_idx)), ids)
        self._dense, self._dense_ids = [], []
        self._chunk_idx += 1

    def _encode_batch(self, inputs, batch_ids):
        sparse, dense = self.model.encode(**inputs)
        # to the host batch by batch, as store_embs does (indexer.py:56): a whole chunk of 2 M x H fp32 rows (16 GB at H = 2048,
        # 32 GB at 4096) would otherwise sit in HBM next to the COO triples of the sparse index
        self._dense.append(dense.float().cpu())
        self._dense_ids.extend(batch_ids)
        if len(self._dense_ids) >= self.chunk_size:
            self._flush_dense()
        return sparse

    def index(self, collection_loader, id_dict=None):
        out = super().index(collection_loader, id_dict=id_dict)
        if self._dense:
            print("last embedddings shape = {}".format((len(self._dense_ids), self._dense[0].shape[1])))
            self._flush_dense()
        plan = {"nranks": get_world_size(), "num_chunks": self._chunk_idx, "index_path": os.path.join(self.dense_index_dir, "model.index")}
        print("plan: ", plan)
        if is_first_worker():
            with open(os.path.join(self.dense_index_dir, "plan.json"), "w") as fout:
                json.dump(plan, fout)
        return out


class HybridRetriever(SparseRetrieval):
    """indexer.py:859-1019: queries are encoded once (both heads), scored against the inverted index and against the flat
    dense index; writes {out_dir}/sparse/run.json + q_stats.json and {out_dir}/dense/run.json."""

    def __init__(self, model, sparse_index_dir, dense_index_dir, out_dir, dim_voc, device, query_max_terms=0, **kwargs):
        from .utils.utils import obtain_doc_vec_dir_files
        super().__init__(model, {"index_dir": sparse_index_dir, "out_dir": out_dir}, dim_voc, device, compute_stats=True,
                         query_max_terms=query_max_terms)
        self.sparse_out_dir, self.dense_out_dir = os.path.join(out_dir, "sparse"), os.path.join(out_dir, "dense")
        if is_first_worker():
            os.makedirs(self.sparse_out_dir, exist_ok=True)
            os.makedirs(self.dense_out_dir, exist_ok=True)
        self.dense_index = DenseFlatIndexer()
        self.dense_index.init_index(self.model.hidden_size)
        self._index_encoded_data(*obtain_doc_vec_dir_files(dense_index_dir))

    def _index_encoded_data(self, doc_vec_files, doc_id_files):
        total = 0
        for doc_file, id_file in zip(doc_vec_files, doc_id_files):       # one HBM segment per shard file
            total += self.dense_index.index_data(np.load(doc_file, mmap_mode="r"), np.load(id_file).tolist())
        print("size of doc reps to index: ", total)

    def _generate_query_vecs(self, q_loader):
        parts, dense_query_vecs, qids = [], [], []
        for group in tqdm(batch_groups(q_loader, self.QUERY_GROUP_ROWS), desc="generate query vecs", disable=not is_first_worker()):
            with torch.inference_mode(), torch.autocast("cuda", dtype=torch.bfloat16):      # indexer.py:938-939
                batch_sparse_reps, batch_dense_reps = encode_group(self.model, group, self.device)
            for batch in group:
                qids.extend(batch["ids"] if isinstance(batch["ids"], list) else to_list(batch["ids"]))
            dense_query_vecs.append(batch_dense_reps)
            parts.append(QueryCSR(*sparse_reps_to_csr(batch_sparse_reps, self.query_max_terms)))
            del batch_sparse_reps
        sparse_query_vecs = QueryCSR.cat(parts)
        dense_query_vecs = torch.cat(dense_query_vecs)
        assert len(sparse_query_vecs) == len(dense_query_vecs) == len(qids)
        return sparse_query_vecs, dense_query_vecs, qids

    def _dense_retrieve(self, query_reps, qids, topk=1000, _filter=None):
        """indexer.py:973-982, as a RunResult over the result arrays (label -1 rows = fewer than k vectors are skipped)."""
        scores, positions = self.dense_index.search_arrays(query_reps, topk, _filter=_filter)
        return RunResult(qids, scores, positions, self.dense_index.run_table())

    def _sparse_retrieve(self, sparse_query_vecs, qids, threshold=0., topk=1000, _filter=None):
        return self._sparse_retrieve_multithreaded(sparse_query_vecs, qids, threshold=threshold, topk=topk, _filter=_filter)

    def allowed_subsets(self, allowed_ids):
        """(dense positions, sparse positions) of an allow-list of database ids, each sorted, unique and on the device.  The two indexes
        number documents independently.  Every id must be in the dense index (ValueError naming it otherwise); one without a posting is
        unknown to the inverted index and is simply not in its list (it shares no term with any query)."""
        sparse = allowed_positions_on(allowed_ids, self.inverse_id_map(), self._dev, skip_unknown=True)
        return self.dense_index.allowed_subset(allowed_ids), sparse

    def allowed_group_filters(self, allowed_masks, query_group):
        """allowed_masks bool [G, dense index positions] (the numbering of allowed_mask) and query_group int [number of queries] -> the
        two heads' doc_filter.Filter("groups", ...): the dense head takes the rows as they are; for the sparse head every row is carried
        over to the inverted index's numbering (doc_mask_remap with the _position_maps table), one row at a time, stacked on the device.
        A document without a posting has no sparse position and simply drops out of the sparse row."""
        d_filt = Filter("groups", *self.dense_index.allowed_group_words(allowed_masks, query_group))
        _, s2d = self._position_maps()
        n_dense, n_sparse = self.dense_index.index.id_end, self.hip_index.n_docs
        s2d = s2d[:n_sparse] if s2d.numel() >= n_sparse else torch.cat([s2d, s2d.new_full((n_sparse - s2d.numel(),), -1)])
        s_words = torch.stack([doc_mask_remap(row, n_dense, s2d, n_sparse) for row in d_filt.data]) if n_sparse else \
            torch.zeros((d_filt.data.shape[0], 0), dtype=torch.int32, device=self._dev)
        return d_filt, Filter("groups", s_words, d_filt.groups)

    def _retrieve_both(self, q_loader, topk, threshold, allowed_ids=None, allowed_masks=None, query_group=None):
        """The two searches and their files (sparse/run.json + q_stats.json, dense/run.json): shared by retrieve and retrieve_fused."""
        one_filter("HybridRetriever.retrieve", allowed_masks, query_group, allowed_ids=allowed_ids)
        d_subset, s_subset = (None, None) if allowed_ids is None else (Filter("subset", t) for t in self.allowed_subsets(allowed_ids))
        if allowed_masks is not None:
            d_subset, s_subset = self.allowed_group_filters(allowed_masks, query_group)
        sparse_query_vecs, dense_query_vecs, qids = self._generate_query_vecs(q_loader)
        if allowed_masks is not None and d_subset.groups.numel() != len(qids):
            raise ValueError(f"HybridRetriever.retrieve: query_group must hold one group id per query ({len(qids)}), got {d_subset.groups.numel()}")
        sparse_res, sparse_stats = self._sparse_retrieve(sparse_query_vecs, qids, threshold=threshold, topk=topk, _filter=s_subset)
        dense_res = self._dense_retrieve(dense_query_vecs, qids, topk=topk, _filter=d_subset)
        with open(os.path.join(self.sparse_out_dir, "q_stats.json"), "w") as handler:
            json.dump(sparse_stats, handler)
        sparse_res.dump(os.path.join(self.sparse_out_dir, "run.json"))
        dense_res.dump(os.path.join(self.dense_out_dir, "run.json"))
        return sparse_query_vecs, dense_query_vecs, qids, sparse_res, dense_res

    def retrieve(self, q_loader, topk, id_dict=False, threshold=0., allowed_ids=None, allowed_masks=None, query_group=None, collapse=None,
                 hits=None):
        """allowed_ids (None: every document): database ids - both heads rank only these documents (allowed_subsets).  allowed_masks bool
        [G, dense index positions] (the numbering of allowed_mask()) with query_group int [number of queries]: a filter per query for
        both heads (allowed_group_filters); not together with allowed_ids.  collapse (None: rank passages): a `group_of` - dict on the
        database id, callable on it, or a sequence aligned with the DENSE index's order - makes both searches collapsed searches: both
        run.json files are keyed by group label (the topk best groups, each scored by its best passage under that head) and
        sparse/q_stats.json gains the route statistics of both heads ("collapse", "collapse_dense").  hits=m (with collapse only, else
        ValueError): both heads also return the up to m best passages inside every group (collapse.group_hits) - the two run.json files
        stay as they are, passage-level runs go to sparse/hits/run.json and dense/hits/run.json (SparseRetrieval.retrieve), both
        statistics gain "mean_hits", and the return value becomes (sparse run, dense run, sparse hits run, dense hits run)."""
        from .collapse import hits_of_no_collapse
        hits_of_no_collapse("HybridRetriever.retrieve", hits, collapse)
        if collapse is not None:
            return self._retrieve_both_collapsed(q_loader, topk, threshold, collapse, allowed_ids, allowed_masks, query_group, hits=hits)
        return self._retrieve_both(q_loader, topk, threshold, allowed_ids=allowed_ids, allowed_masks=allowed_masks, query_group=query_group)[3:]

    def _retrieve_both_collapsed(self, q_loader, topk, threshold, group_of, allowed_ids=None, allowed_masks=None, query_group=None, hits=None):
        one_filter("HybridRetriever.retrieve", allowed_masks, query_group, allowed_ids=allowed_ids)
        d_filt, s_filt = (None, None) if allowed_ids is None else (Filter("subset", t) for t in self.allowed_subsets(allowed_ids))
        if allowed_masks is not None:
            d_filt, s_filt = self.allowed_group_filters(allowed_masks, query_group)
        if not isinstance(group_of, dict) and not callable(group_of):       # a sequence: aligned with the dense index, the sparse head by id
            db_ids = self.dense_index.index_id_to_db_id
            labels = list(group_of)
            if len(labels) != len(db_ids):
                raise ValueError(f"collapse: a sequence of group labels is aligned with the dense index ({len(db_ids)} documents), got {len(labels)}")
            group_of = dict(zip(db_ids, labels))
        sparse_query_vecs, dense_query_vecs, qids = self._generate_query_vecs(q_loader)
        sparse_res, sparse_stats, *sparse_hits = self._retrieve_collapsed(sparse_query_vecs, qids, group_of, threshold, topk, s_filt, hits=hits)
        keys, table = self.dense_index.collapse_keys(group_of)
        q = _dense_queries(dense_query_vecs, self._dev)
        found = self.dense_index.index.search_collapsed(q, topk, keys, hits=hits, **_collapse_filter(d_filt))
        scores, _, gkeys, counts, route = found[:5]
        dense_res = RunResult(qids, to_host(scores), to_host(gkeys.to(torch.int64)), IdTable(table), to_host(counts))
        sparse_stats["collapse_dense"] = _collapse_stats(route)
        with open(os.path.join(self.sparse_out_dir, "q_stats.json"), "w") as handler:
            json.dump(sparse_stats, handler)
        sparse_res.dump(os.path.join(self.sparse_out_dir, "run.json"))
        dense_res.dump(os.path.join(self.dense_out_dir, "run.json"))
        if hits is None:
            return sparse_res, dense_res
        dense_hits = _hits_run(qids, found[5], self.dense_index.run_table())
        _dump_hits_run(sparse_hits[0], self.sparse_out_dir)
        _dump_hits_run(dense_hits, self.dense_out_dir)
        return sparse_res, dense_res, sparse_hits[0], dense_hits

    def _position_maps(self):
        """The two indexes number documents independently: (dense position -> sparse position, -1 where the inverted index has no
        such document, i.e. it has no posting), as a device tensor, built once."""
        if getattr(self, "_d2s", None) is None:
            inv = self.inverse_id_map()
            d2s = np.fromiter((inv.get(d) for d in self.dense_index.index_id_to_db_id), dtype=np.int64,
                              count=len(self.dense_index.index_id_to_db_id))
            s2d = np.full(max(1, self.sparse_index.nb_docs(), int(d2s.max(initial=-1)) + 1), -1, np.int64)
            s2d[d2s[d2s >= 0]] = np.nonzero(d2s >= 0)[0]
            self._d2s = torch.from_numpy(d2s).to(self._dev)
            self._s2d = torch.from_numpy(s2d).to(self._dev)
        return self._d2s, self._s2d

    def retrieve_fused(self, q_loader, topk, weights=(1.0, 1.0), threshold=0., allowed_ids=None, allowed_masks=None, query_group=None, collapse=None):
        """`retrieve` (the same two runs, the same bytes) plus {out_dir}/fused/run.json: per query the UNION of the two top-k lists,
        taken over database ids, is scored by BOTH heads with the pair kernels (a document only one search found gets its other
        score exactly, not a zero) and ranked by fused = float32(w_d * dense) + float32(w_s * sparse), top-k by (fused descending,
        sparse-index position ascending; a document without a posting has sparse score 0.0 and sorts after every indexed one).
        Every document of the inverted index must be in the dense index.  allowed_ids (None: every document): database ids - both
        heads, and with them the union that is fused, are restricted to these documents; allowed_masks / query_group as for retrieve: a
        filter per query, the union of the two restricted lists is fused.  Returns (sparse_res, dense_res, fused_res)."""
        from .collapse import not_under_collapse
        not_under_collapse("HybridRetriever.retrieve_fused", collapse)
        from .rerank import fused_scores, ranked_run
        sparse_query_vecs, dense_query_vecs, qids, sparse_res, dense_res = self._retrieve_both(
            q_loader, topk, threshold, allowed_ids=allowed_ids, allowed_masks=allowed_masks, query_group=query_group)
        dev, nq = self._dev, len(qids)
        d2s, s2d = self._position_maps()
        n_dense = int(d2s.numel())
        sp = torch.from_numpy(sparse_res.positions).to(dev)
        sp_valid = (sp >= 0) & (torch.arange(sp.shape[1], device=dev)[None, :] < torch.from_numpy(sparse_res.counts).to(dev)[:, None])
        dp = torch.from_numpy(dense_res.positions).to(dev)
        rows_s = torch.arange(nq, device=dev)[:, None].expand_as(sp)[sp_valid]
        sp_as_dense = s2d[sp[sp_valid]]
        if bool((sp_as_dense < 0).any()):
            raise KeyError("retrieve_fused: the inverted index holds a document the dense index does not")
        rows_d = torch.arange(nq, device=dev)[:, None].expand_as(dp)[dp >= 0]
        keys = torch.unique(torch.cat([rows_s * n_dense + sp_as_dense, rows_d * n_dense + dp[dp >= 0]]))     # sorted: by query, then dense position
        row, dpos = keys // max(1, n_dense), keys % max(1, n_dense)
        indptr = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        indptr[1:] = torch.cumsum(torch.bincount(row, minlength=nq), 0)
        q_dense = dense_query_vecs.to(device=dev, dtype=torch.float32)
        dense_s = self.dense_index.index.score_pairs(q_dense, indptr, dpos)
        spos = d2s[dpos]
        sparse_s = self.hip_index.score_pairs(sparse_query_vecs.row_ptr, sparse_query_vecs.cols, sparse_query_vecs.vals, indptr,
                                              torch.clamp(spos, min=0))
        sparse_s = torch.where(spos >= 0, sparse_s, torch.zeros_like(sparse_s))
        tie = torch.where(spos >= 0, spos, int(s2d.numel()) + dpos)
        fused_res = ranked_run(qids, fused_scores(dense_s, sparse_s, weights), dpos, tie, indptr, self.dense_index.run_table(), topk=topk)
        fused_dir = os.path.join(os.path.dirname(self.sparse_out_dir), "fused")
        os.makedirs(fused_dir, exist_ok=True)
        fused_res.dump(os.path.join(fused_dir, "run.json"))
        return sparse_res, dense_res, fused_res

    def retrieve_prf(self, *args, **kwargs):
        raise NotImplementedError("HybridRetriever.retrieve_prf: pseudo-relevance feedback is offered per head (SparseRetrieval.retrieve_prf, "
                                  "DenseFlatIndexer.search_prf), not on the hybrid retriever: fuse the two feedback runs with eval_fuse.py")

    def retrieve_mmr(self, *args, **kwargs):
        raise NotImplementedError("HybridRetriever.retrieve_mmr: the diversified search is offered per head (SparseRetrieval.retrieve_mmr, "
                                  "DenseFlatIndexer.search_mmr), not on the hybrid retriever: a combined dense + sparse similarity is not defined")

    def retrieve_rank_fused(self, q_loader, topk, method="rrf", c=60.0, weights=(1.0, 1.0), fused_topk=None, threshold=0., allowed_ids=None,
                            allowed_masks=None, query_group=None, collapse=None):
        """`retrieve` (the same two runs, the same bytes) plus {out_dir}/rank_fused/run.json: the two top-`topk` lists fused on the
        lists alone (fusion.fuse_hybrid_lists over scoring.rank_fuse; no pair is scored again and no weight needs tuning to the heads'
        score scales).  method "rrf": weights[l] / (c + rank) summed over the lists that hold the document; "minmax": weights[l] * the
        score normalised to [0, 1] over its list.  weights = (w_dense, w_sparse), finite and >= 0.  The fused run holds the fused_topk
        (default topk; at most sr_max_topk(), as is topk) best documents by (fused descending, retrieve_fused's tie: sparse-index
        position ascending, documents without a posting last).  Filters as for retrieve: the two restricted lists are fused.  Every
        document of the inverted index must be in the dense index (KeyError).  Returns (sparse_res, dense_res, fused_res)."""
        from .collapse import not_under_collapse
        not_under_collapse("HybridRetriever.retrieve_rank_fused", collapse)
        from . import fusion, hybrid, scoring
        hybrid.check_arguments(topk, weights)
        k, _, weights, c = scoring.rank_fuse_arguments(2, topk if fused_topk is None else fused_topk, method, weights, c)
        _, _, qids, sparse_res, dense_res = self._retrieve_both(q_loader, topk, threshold, allowed_ids=allowed_ids, allowed_masks=allowed_masks,
                                                                query_group=query_group)
        d2s, s2d = self._position_maps()
        dp, sp, ds, ss = (torch.from_numpy(x).to(self._dev) for x in (dense_res.positions, sparse_res.positions, dense_res.scores, sparse_res.scores))
        sc = None if sparse_res.counts is None else torch.from_numpy(sparse_res.counts).to(self._dev)
        scores, dpos, counts = fusion.fuse_hybrid_lists(dp, sp, sc, d2s, s2d, k, method=method, weights=weights, c=c, dense_scores=ds,
                                                        sparse_scores=ss)
        fused_res = RunResult(qids, to_host(scores), to_host(dpos), self.dense_index.run_table(), to_host(counts))
        fused_dir = os.path.join(os.path.dirname(self.sparse_out_dir), "rank_fused")
        os.makedirs(fused_dir, exist_ok=True)
        fused_res.dump(os.path.join(fused_dir, "run.json"))
        return sparse_res, dense_res, fused_res

    def score_candidates(self, sparse_query_vecs, qids, doc_id_lists, dense_query_vecs=None, weights=(1.0, 1.0)):
        """With dense_query_vecs: both heads score the given candidates (database ids; each index is given its own positions) and
        the rows are ranked by the fused score of retrieve_fused, ties by sparse-index position.  A document the dense index holds
        but the inverted index does not (it has no posting) gets sparse score 0.0 and sorts after the indexed ones at equal score,
        exactly as in retrieve_fused; an id the dense index does not hold is a KeyError.  Without dense_query_vecs: the sparse head
        alone (SparseRetrieval.score_candidates)."""
        if dense_query_vecs is None:
            return super().score_candidates(sparse_query_vecs, qids, doc_id_lists)
        from .rerank import fused_scores, ranked_run
        q = _as_query_csr(sparse_query_vecs, self._dev)
        indptr, dpos = self.dense_index.inverse_id_map().positions(doc_id_lists)      # KeyError: an id neither index knows
        dpos_t = torch.from_numpy(dpos).to(self._dev)
        d2s, s2d = self._position_maps()
        spos_t = d2s[dpos_t]
        dense_s = self.dense_index.index.score_pairs(dense_query_vecs.to(device=self._dev, dtype=torch.float32), indptr, dpos_t)
        sparse_s = self.hip_index.score_pairs(q.row_ptr, q.cols, q.vals, indptr, torch.clamp(spos_t, min=0))
        sparse_s = torch.where(spos_t >= 0, sparse_s, torch.zeros_like(sparse_s))     # no posting: no common term, 0.0 (as retrieve_fused)
        tie = torch.where(spos_t >= 0, spos_t, int(s2d.numel()) + dpos_t)
        return ranked_run(qids, fused_scores(dense_s, sparse_s, weights), dpos_t, tie, torch.from_numpy(indptr).to(self._dev),
                          self.dense_index.run_table())

    def allowed_mask(self, allowed_ids):
        """Database ids (any order, duplicates allowed) -> a boolean array over dense index positions, True at these documents: the
        allowed_mask of search_fused / retrieve_fused_exact (and of the dense index's search_knn / range_search).  An unknown id:
        ValueError naming it."""
        flags = np.zeros(self.dense_index.index.id_end, dtype=bool)
        flags[self.dense_index.allowed_subset(allowed_ids).cpu().numpy()] = True
        return flags

    def range_search(self, sparse_query_vecs, thresholds=0., sort=True, allowed_ids=None, allowed_mask=None, allowed_masks=None,
                     query_group=None):
        """SparseRetrieval.range_search on the inverted index.  allowed_ids / allowed_mask as there (allowed_mask over the document
        positions of the inverted index).  allowed_masks / query_group as for retrieve: bool [G, DENSE index positions] (the numbering
        of allowed_mask()), carried over to the inverted index's numbering once per call (allowed_group_filters) - a document without a
        posting has no sparse position and is in no list."""
        one_filter("range_search", allowed_masks, query_group, allowed_ids=allowed_ids, allowed_mask=allowed_mask)
        if allowed_masks is None:
            return super().range_search(sparse_query_vecs, thresholds, sort=sort, allowed_ids=allowed_ids, allowed_mask=allowed_mask)
        return super().range_search(sparse_query_vecs, thresholds, sort=sort, _filter=self.allowed_group_filters(allowed_masks, query_group)[1])

    def search_fused(self, sparse_query_vecs, dense_query_vecs, topk, weights=(1.0, 1.0), depths=None, fallback_bytes=1 << 30, qids=None,
                     allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None, collapse=None):
        """The EXACT top-k of the fused score of retrieve_fused over every document of the dense index (hybrid.search_fused: the
        union of the two heads' lists at depth depths[0] >= topk where a certificate proves it holds the true top-k, deeper lists
        for the queries it does not, a dense range search for what is left; the same result whatever route served a query).
        Returns (RunResult, stats): rows of (fused score, document) by fused descending, ties by sparse-index position ascending
        (documents without a posting after the indexed ones); stats = {"depth": per query the index into `depths` at which it was
        certified, -1 = range route; "union": candidates ranked; "range_hits"; "depths"}.  qids (None: 0 .. nq - 1) name the rows.
        topk >= 1 and two finite weights >= 0, else ValueError before any device work; the dense index must be in precision fp32 /
        fp32_filtered (ValueError).  allowed_mask (None: every document): a boolean array over dense index positions, the allowed_mask
        of search_knn - the exact top-k of the fused score over these documents alone (fewer than topk of them: shorter rows); build
        it from database ids with allowed_mask(ids).  allowed_masks bool [G, dense index positions] with query_group int [nq] (not
        together with allowed_mask): a filter per query - the exact top-k of the fused score over the documents of
        allowed_masks[query_group[q]] alone, for every group what allowed_mask=allowed_masks[g] returns for its queries.  Not supported
        (NotImplementedError): allowed_ids, and the doc-sharded classes."""
        from .collapse import not_under_collapse
        not_under_collapse("HybridRetriever.search_fused", collapse)
        from . import hybrid
        hybrid.check_arguments(topk, weights)
        if allowed_ids is not None:
            raise NotImplementedError("HybridRetriever.search_fused: an allow-list of ids (allowed_ids) is not taken by the exact fused "
                                      "search; pass the bitmap instead: allowed_mask=ret.allowed_mask(ids)")
        one_filter("HybridRetriever.search_fused", allowed_masks, query_group, allowed_mask=allowed_mask)
        how = {}
        if allowed_mask is not None:
            how = dict(mask=self.dense_index.allowed_mask_words(allowed_mask))
        elif allowed_masks is not None:
            words, groups = self.dense_index.allowed_group_words(allowed_masks, query_group)
            how = dict(masks=words, query_group=groups)
        q = _as_query_csr(sparse_query_vecs, self._dev)
        d2s, s2d = self._position_maps()
        dq = _dense_queries(dense_query_vecs, self._dev)
        scores, positions, counts, stats = hybrid.search_fused(self.dense_index.index, self.hip_index, d2s, s2d, dq, q.row_ptr, q.cols, q.vals,
                                                               topk, weights=weights, depths=depths, fallback_bytes=fallback_bytes, **how)
        qids = list(range(dq.shape[0])) if qids is None else qids
        return RunResult(qids, scores, positions, self.dense_index.run_table(), counts), stats

    def retrieve_fused_exact(self, q_loader, topk, weights=(1.0, 1.0), depths=None, fallback_bytes=1 << 30, allowed_ids=None,
                             allowed_mask=None, allowed_masks=None, query_group=None, collapse=None):
        """Encodes the queries once (both heads) and writes {out_dir}/fused_exact/run.json, next to the two heads' runs: the exact
        fused top-k of search_fused (allowed_mask, or allowed_masks with query_group in loader order, as there).  Returns (RunResult, stats).  The files of retrieve / retrieve_fused are
        not touched."""
        from .collapse import not_under_collapse
        not_under_collapse("HybridRetriever.retrieve_fused_exact", collapse)
        from . import hybrid
        hybrid.check_arguments(topk, weights)
        if allowed_ids is not None:
            raise NotImplementedError("HybridRetriever.retrieve_fused_exact: an allow-list of ids (allowed_ids) is not taken; pass the "
                                      "bitmap instead: allowed_mask=ret.allowed_mask(ids)")
        one_filter("HybridRetriever.retrieve_fused_exact", allowed_masks, query_group, allowed_mask=allowed_mask)
        sparse_query_vecs, dense_query_vecs, qids = self._generate_query_vecs(q_loader)
        res, stats = self.search_fused(sparse_query_vecs, dense_query_vecs, topk, weights=weights, depths=depths,
                                       fallback_bytes=fallback_bytes, qids=qids, allowed_mask=allowed_mask, allowed_masks=allowed_masks,
                                       query_group=query_group)
        out_dir = os.path.join(os.path.dirname(self.sparse_out_dir), "fused_exact")
        os.makedirs(out_dir, exist_ok=True)
        res.dump(os.path.join(out_dir, "run.json"))
        return res, stats
