"""Thin torch-tensor front ends over the scoring entry points of libsr_hip.so.

These hold device memory (torch tensors) and call the C ABI; all arithmetic is in
the HIP kernels (csrc/dense_score.hip, csrc/sparse_cert.hip, csrc/sparse_score.hip, csrc/topk.hip).
The reference-shaped classes in indexer.py are built on top of these.

What is here: DenseIndexHIP, SparseIndexHIP and the free functions (range_sort, sparse_csr_build, token_counts, bm25_weights, sparse_feedback, sparse_mmr, topk_merge, hybrid_union,
hybrid_rank, topk_collapse, group_members, segment_topm).  Every library call goes through one helper (`_call`: the index's device, the entry by name, torch's current stream,
the status checked under that name); a filtered variant of an entry is the same call with "_subset" / "_masked" appended to the name
and the filter's two arguments spliced in where the header puts them (_filter_args).  Each class checks its queries in one place
(DenseIndexHIP._queries, SparseIndexHIP._query_csr), the range searches share _thresholds, and add_host_rows / add_npy_file share
one pinned staging ring (DenseIndexHIP._add_staged).  Everything about document filters - packing, the resolver of a mask= argument,
the "only one filter" rule, the order of checks - lives in doc_filter.py; its public names are re-exported here, the module
everything imports from.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .doc_filter import (_call, _cuda_device, _mask_words, _ptr, _subset, _to_dev, _valid, allowed_positions, doc_list_from_mask,  # noqa: F401  (re-exported)
                         doc_mask_from_list, doc_mask_remap, group_argument, group_filter, group_ids_int32, mask_argument, mask_on_device,
                         one_filter, pack_doc_mask, pack_doc_masks, query_group_argument, read_allowed_ids_file)


def _thresholds(thresholds, nq, device):
    """The thresholds of a range search as fp32 [nq] on the device: one Python / numpy scalar for all queries, or a tensor / array [nq]."""
    if isinstance(thresholds, (int, float, np.floating, np.integer)):
        return torch.full((nq,), float(thresholds), dtype=torch.float32, device=device)
    thr = _to_dev(thresholds, torch.float32, device)
    if thr.dim() != 1 or thr.numel() != nq:
        raise ValueError(f"expected {nq} thresholds, got {tuple(thr.shape)}")
    return thr


def _filter_args(filt):
    """(suffix of the entry's name, the arguments spliced in where the header puts them) of a resolved filter: None, ("_subset", list,
    m), ("_masked", words, n_bits) or ("_grouped", words, n_groups, n_bits, group ids).  The caller keeps `filt`, and with it the
    tensors, until the call has been made."""
    if filt is None:
        return "", ()
    if filt[0] == "_grouped":
        return filt[0], (_ptr(filt[1]), filt[2], filt[3], _ptr(filt[4]))
    return filt[0], (_ptr(filt[1]), filt[2])


def _topk_outputs(nq, k, device, counts=False):
    """The output tensors of a top-k search: (scores fp32 [nq, k], ids int64 [nq, k]), and with counts=True (counts int32 [nq],)."""
    out = (torch.empty((nq, k), dtype=torch.float32, device=device), torch.empty((nq, k), dtype=torch.int64, device=device))
    return out + (torch.empty((nq,), dtype=torch.int32, device=device),) if counts else out


def _candidates(cand_indptr, cand_ids, nq, device):
    """(indptr int64 [nq + 1], ids int64 [max(1, total)], total) on the device; the shape of the lists is checked on the host side
    only where it is free (lengths), their content by the kernels."""
    cand_indptr = _to_dev(cand_indptr, torch.int64, device)
    cand_ids = _to_dev(cand_ids, torch.int64, device)
    if cand_indptr.dim() != 1 or cand_indptr.numel() != nq + 1:
        raise ValueError(f"expected cand_indptr of {nq + 1} entries, got {tuple(cand_indptr.shape)}")
    if cand_ids.dim() != 1:
        raise ValueError(f"expected 1-D cand_ids, got {tuple(cand_ids.shape)}")
    total = cand_ids.numel()
    # the kernels trust cand_indptr[nq] for the size of cand_ids and of the output: the one thing checked here
    if int(cand_indptr[-1]) != total:
        raise ValueError(f"cand_indptr ends at {int(cand_indptr[-1])}, cand_ids holds {total} ids")
    return cand_indptr, _valid(cand_ids), total


def range_sort(lims, scores, ids):
    """Reorders every list of a range result (lims int64 [nq + 1], scores fp32 [total], ids int64 [total]; any device) by score
    descending, ties by ascending id - the order of `search`, whose 64-bit key it sorts by (order-preserving score bits, then the
    complement of the id; ids below 2^32) - so that a list is a prefix of its query's full ranking.  Returns (scores, ids); lims holds."""
    total = scores.numel()
    if total == 0:
        return scores, ids
    bits = scores.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    order = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)          # larger score -> larger value
    key = ((order - 0x80000000) << 32) | (0xFFFFFFFF - ids)
    counts = lims[1:] - lims[:-1]
    query = torch.repeat_interleave(torch.arange(counts.numel(), device=scores.device), counts, output_size=total)
    by_key = torch.argsort(key, descending=True)
    perm = by_key[torch.argsort(query[by_key], stable=True)]
    return scores[perm], ids[perm]


class DenseIndexHIP:
    """Flat inner-product index resident in HBM (segments of [n, dim] rows, all fp32 or all fp16).

    row_dtype="fp32" (default): rows are kept as fp32.  A float16 tensor / array / .npy shard added to such an index (as its first
    rows) makes it an fp16 index all the same - the stored type follows the data.  row_dtype="fp16": fp32 input is rounded to
    float16 (to nearest even) on the device before it is added, and a finite value that does not fit float16 raises ValueError.
    An fp16 index holds half the bytes and streams half the bytes per small-batch search; every search / score_pairs result is
    bit for bit what an fp32 index over `rows.half().float()` returns (include/sr_hip.h sr_dense_index_add_f16)."""

    def __init__(self, dim, device=None, row_dtype="fp32"):
        if row_dtype not in ("fp32", "fp16"):
            raise ValueError(f"row_dtype must be 'fp32' or 'fp16', got {row_dtype!r}")
        self.row_dtype = row_dtype
        _lib.require_gpu()
        self.lib = _lib.load()
        self.dim = int(dim)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._h = ctypes.c_void_p()
        _lib.check(self.lib.sr_dense_index_create(ctypes.byref(self._h), self.dim), "sr_dense_index_create")
        self._segments = []  # keeps the device tensors alive (the C side holds non-owning views)
        self._segment_ids = []  # (id_base, id_stride) of each: mmr.stored_rows finds a document's row again
        self.precision = "fp32"          # what set_precision / set_batch_invariant last set (the C ABI has no getters)
        self.batch_invariant = False

    def _call(self, name, *args, stream=True):
        """The C-ABI entry `name` on this index, on its device (doc_filter._call)."""
        _call(self.device, name, self._h, *args, stream=stream, lib=self.lib)

    def _check_queries(self, queries):
        """dtype and shape of a query tensor; returns nq."""
        if queries.dtype != torch.float32 or queries.dim() != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"expected float32 [nq, {self.dim}] queries, got {queries.dtype} {tuple(queries.shape)}")
        return queries.shape[0]

    def _queries(self, queries):
        """The one check of a query tensor: dtype and shape, then cuda, then the index's device; returns it contiguous."""
        self._check_queries(queries)
        if not queries.is_cuda:
            raise ValueError("queries must be a cuda tensor")
        if queries.device != self.device:
            raise ValueError(f"queries live on {queries.device}, the index on {self.device}")
        return queries.contiguous()

    def _mask(self, mask, ndim=1):
        """The host step of a mask= / masks= argument of this index (doc_filter.mask_argument)."""
        return mask_argument(mask, lambda: self.id_end, "id_end", ndim)

    @staticmethod
    def _round_to_f16(rows, row0=0):
        """fp32 cuda rows -> float16 (round to nearest even, on the device); ValueError naming the first row in which a finite
        value leaves the float16 range (|x| >= 65520 rounds to infinity)."""
        half = rows.to(torch.float16)
        bad = (torch.isinf(half) & torch.isfinite(rows)).any(dim=1)
        if bool(bad.any()):
            r = int(torch.nonzero(bad)[0])
            raise ValueError(f"row {row0 + r} holds a finite value ({float(rows[r].abs().max()):.6g} at most) that float16 cannot "
                             "represent (largest finite value 65504): such rows cannot be stored as fp16")
        return half

    def add_device_rows(self, rows, id_base=None, id_stride=1):
        """rows: fp32 or fp16 cuda tensor [n, dim] (kept alive by this object, not copied).  With row_dtype="fp16" an fp32 tensor is
        rounded to float16 on the device first (that copy is what the index keeps)."""
        if rows.dtype not in (torch.float32, torch.float16) or rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"expected float32 or float16 [n, {self.dim}] rows, got {rows.dtype} {tuple(rows.shape)}")
        if not rows.is_cuda:
            raise ValueError("add_device_rows needs a cuda tensor")
        if rows.device != self.device:
            raise ValueError(f"rows live on {rows.device}, the index on {self.device}")
        if rows.dtype == torch.float32 and self.row_dtype == "fp16":
            rows = self._round_to_f16(rows)
        rows = rows.contiguous()
        if id_base is None:
            id_base = self.ntotal
        self._call("sr_dense_index_add_f16" if rows.dtype == torch.float16 else "sr_dense_index_add", _ptr(rows), rows.shape[0], int(id_base),
                   int(id_stride), stream=False)
        self._segments.append(rows)
        self._segment_ids.append((int(id_base), int(id_stride)))

    def stored_dtype(self):
        """"fp32" or "fp16": what the index's rows are stored as (an empty index: "fp32")."""
        return "fp16" if self.lib.sr_dense_index_row_dtype(self._h) == _lib.SR_DTYPE_F16 else "fp32"

    def owned_bytes(self):
        """Device bytes the library holds for the segments next to the caller's rows (bf16 planes, the certified filter's fp16
        plane and error terms); workspaces are not counted."""
        out = ctypes.c_int64(0)
        _lib.check(self.lib.sr_dense_index_owned_bytes(self._h, ctypes.byref(out)), "sr_dense_index_owned_bytes")
        return out.value

    def _staging(self, src_dtype, n):
        """(element type of the pinned staging ring and of the H2D copies, the HBM segment [n, dim], convert) for host rows of
        `src_dtype`: float16 sources travel and stay as float16; float32 sources travel as float32 and, under row_dtype="fp16", are
        rounded on the device piece by piece into a float16 segment (convert = True: no fp32 copy of the segment ever exists)."""
        if src_dtype == np.float16:
            return torch.float16, torch.empty((n, self.dim), dtype=torch.float16, device=self.device), False
        convert = self.row_dtype == "fp16"
        return torch.float32, torch.empty((n, self.dim), dtype=torch.float16 if convert else torch.float32, device=self.device), convert

    def _h2d_piece(self, dev, r0, r1, pinned, convert):
        """Queue the copy of a staged piece into rows [r0, r1) of the segment on the current (side) stream."""
        if not convert:
            dev[r0:r1].copy_(pinned, non_blocking=True)
            return
        tmp = pinned.to(self.device, non_blocking=True)
        dev[r0:r1].copy_(self._round_to_f16(tmp, r0))

    def _add_staged(self, src_dtype, n, fill, id_base, id_stride, piece_bytes, n_buffers, n_threads):
        """n host rows of `src_dtype` -> ONE HBM segment through a ring of pinned staging buffers: worker threads have
        fill(pinned_view, r0, r1) put rows [r0, r1) of the source into a buffer (a numpy view of its first r1 - r0 rows; the GIL is
        released inside) and queue the H2D copy of each piece on a side stream, so reads, host copies and PCIe transfers overlap and
        no second host copy of the matrix ever exists."""
        import threading
        from concurrent.futures import ThreadPoolExecutor
        stage_dt, dev, convert = self._staging(src_dtype, n)
        if n == 0:
            self.add_device_rows(dev, id_base=id_base, id_stride=id_stride)
            return
        piece_rows = max(1, int(piece_bytes) // ((2 if stage_dt == torch.float16 else 4) * self.dim))
        pieces = [(r0, min(n, r0 + piece_rows)) for r0 in range(0, n, piece_rows)]
        n_buffers = max(1, min(n_buffers, len(pieces)))
        with torch.cuda.device(self.device):
            side = torch.cuda.Stream()
            # `dev` came from the caching allocator on the current stream: a recycled block may still have kernels queued there
            side.wait_stream(torch.cuda.current_stream(self.device))
            bufs = [torch.empty((piece_rows, self.dim), dtype=stage_dt, pin_memory=True) for _ in range(n_buffers)]
            free = [torch.cuda.Event() for _ in range(n_buffers)]
            locks = [threading.Lock() for _ in range(n_buffers)]

            def move(i):
                r0, r1 = pieces[i]
                b = i % n_buffers
                with locks[b]:                          # pieces i, i + n_buffers, ... share buffer b, in order
                    free[b].synchronize()               # its previous H2D copy has left the buffer
                    fill(bufs[b].numpy()[:r1 - r0], r0, r1)
                    with torch.cuda.device(self.device), torch.cuda.stream(side):
                        self._h2d_piece(dev, r0, r1, bufs[b][:r1 - r0], convert)
                        free[b].record(side)
            with ThreadPoolExecutor(max_workers=max(1, min(n_threads, n_buffers))) as pool:
                list(pool.map(move, range(len(pieces))))
            side.synchronize()
        self.add_device_rows(dev, id_base=id_base, id_stride=id_stride)

    def add_host_rows(self, rows, buffer_size=50000, id_base=None, id_stride=1, piece_bytes=64 << 20, n_buffers=8, n_threads=8):
        """rows: np.float32 [n, dim] - an in-memory array or an np.load(..., mmap_mode="r") view of a shard file.
        Streamed into ONE HBM segment through the pinned ring (_add_staged): numpy releases the GIL for the copy of a piece, a
        memory-mapped source is read from the page cache / the file right there (the reference concatenates every shard on the
        host, eval_dense.py:113-121, then faiss copies it again, indexer.py:203).
        `buffer_size` (rows per add, indexer.py:198-208) is accepted for signature compatibility."""
        if rows.dtype not in (np.float32, np.float16) or rows.ndim != 2 or rows.shape[1] != self.dim:
            if rows.ndim != 2 or rows.shape[1] != self.dim:
                raise ValueError(f"expected [n, {self.dim}] rows, got {rows.shape}")
            rows = np.asarray(rows, dtype=np.float32)
        self._add_staged(rows.dtype, rows.shape[0], lambda view, r0, r1: np.copyto(view, rows[r0:r1]), id_base, id_stride, piece_bytes,
                         n_buffers, n_threads)

    def add_npy_file(self, path, id_base=None, id_stride=1, piece_bytes=64 << 20, n_buffers=8, n_threads=8):
        """One embs_{rank}_{chunk}.npy shard file -> one HBM segment, never loaded whole on the host: the ring's worker threads
        `preadv` pieces of the file straight into the pinned staging buffers (one kernel copy out of the page cache, no per-page
        mapping faults as a memory-mapped source costs, GIL released); a float16 shard moves half the bytes, file to HBM."""
        import os
        arr = np.load(path, mmap_mode="r")              # header only: shape, dtype, data offset
        if arr.dtype not in (np.float32, np.float16) or arr.ndim != 2 or arr.shape[1] != self.dim or not arr.flags["C_CONTIGUOUS"]:
            return self.add_host_rows(np.ascontiguousarray(arr, dtype=np.float32), id_base=id_base, id_stride=id_stride)
        src_dtype, n, offset0, row_bytes = arr.dtype, arr.shape[0], arr.offset, arr.dtype.itemsize * self.dim
        del arr
        fd = os.open(path, os.O_RDONLY)

        def fill(view, r0, r1):
            view = memoryview(view).cast("B")
            got, want = 0, (r1 - r0) * row_bytes
            while got < want:
                k = os.preadv(fd, [view[got:want]], offset0 + r0 * row_bytes + got)
                if k <= 0:
                    raise IOError(f"{path}: short read at row {r0}")
                got += k
        try:
            self._add_staged(src_dtype, n, fill, id_base, id_stride, piece_bytes, n_buffers, n_threads)
        finally:
            os.close(fd)

    @property
    def ntotal(self):
        return int(self.lib.sr_dense_index_ntotal(self._h))

    @property
    def id_end(self):
        """The largest document index of any segment, plus one: the length of a document mask (not ntotal: segments may be strided)."""
        return int(self.lib.sr_dense_index_id_end(self._h))

    def set_workspace_limit(self, nbytes):
        _lib.check(self.lib.sr_dense_index_set_workspace_limit(self._h, int(nbytes)))

    def set_batch_invariant(self, on=True):
        """One k order for every batch size: a query's results are the same bits alone and inside any batch (batches of <= 64
        queries then run the tiled kernels instead of the streaming one, ~4.4 instead of ~5.9 TB/s).  Off by default."""
        _lib.check(self.lib.sr_dense_index_set_batch_invariant(self._h, 1 if on else 0))
        self.batch_invariant = bool(on)

    def set_precision(self, mode):
        """"fp32" (default: the exact kernel), "fp32_filtered" (the same results bit for bit through a certified fp16 filter +
        exact re-score, ~7x faster for batches > 64 queries, one fp16 plane of the corpus in HBM), "bf16x3" / "bf16x6"
        (split-bf16 scores, not bit-identical; not available on an index of fp16 rows: SrHipError)."""
        code = {"fp32": 0, "bf16x3": 1, "bf16x6": 2, "fp32_filtered": 3}[mode]
        self._call("sr_dense_index_set_precision", code, stream=False)
        self.precision = mode

    def filter_stats(self):
        """(searches answered by the certified filter alone, searches where some or all queries were re-done by the exact kernel)."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self.lib.sr_dense_index_filter_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def filter_query_stats(self):
        """(queries certified by the filter, queries re-done by the exact kernel) so far."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self.lib.sr_dense_index_filter_query_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def search(self, queries, k, subset=None, mask=None):
        """queries: fp32 cuda tensor [nq, dim] -> (scores fp32 [nq,k], ids int64 [nq,k]) cuda tensors.  subset (None: the whole
        index): strictly ascending int64 ids as this method returns them, one allow-list for all queries - the result is the full
        ranking with every other document removed, cut to k (include/sr_hip.h sr_dense_search_subset); an id outside the index or
        out of order: ValueError naming its position.  mask: the same filter as a bitmap over [0, id_end) - a bool tensor / array
        of length id_end (packed on the device), or int32 / uint32 words already packed (pack_doc_mask) - with exactly the result
        of `subset` = the set positions (sr_dense_search_masked); a set bit that names no document: ValueError naming it.  One of
        the two at most."""
        one_filter("search", subset=subset, mask=mask)
        if mask is not None:
            mask = self._mask(mask)
        queries = self._queries(queries)
        filt = None
        if subset is not None:
            filt = ("_subset",) + _subset(subset, self.device)
        elif mask is not None:
            filt = ("_masked",) + mask_on_device(*mask, self.device)
        return self._search(queries, k, filt)

    def _search(self, queries, k, filt):
        nq = queries.shape[0]
        scores, ids = _topk_outputs(nq, k, self.device)
        suffix, spliced = _filter_args(filt)
        self._call("sr_dense_search" + suffix, _ptr(queries), nq, int(k), *spliced, _ptr(scores), _ptr(ids))
        return scores, ids

    def search_grouped(self, queries, k, masks, query_group):
        """Top-k of every query within its own group's documents (include/sr_hip.h sr_dense_search_grouped).  masks: one bitmap per group
        over [0, id_end) - bool [G, id_end] (tensor / array, packed on the device) or int32 / uint32 words [G, ceil(id_end / 32)] already
        packed (pack_doc_masks); query_group: int array / tensor [nq], query q searches under masks[query_group[q]].  The rows of a
        group's queries are exactly what search(those queries, k, mask=masks[g]) returns.  1 <= k <= sr_max_topk().  Wrong shapes, a wrong
        word count, a length mismatch or non-integer groups: ValueError before anything is uploaded; a group id outside [0, G) or a set
        bit that names no document: ValueError naming the query / the (group, bit), every row of the result is then padding."""
        queries, filt = self._groups(masks, query_group, queries)
        return self._search(queries, k, filt)

    def _groups(self, masks, query_group, queries):
        """The checks of a masks= / query_group= pair in the order doc_filter.py lists, then its device step: (queries contiguous,
        ("_grouped", words int32 [G, W] on the device, G, n_bits, group ids int32 [nq] on the device))."""
        argument = group_argument(masks, query_group, lambda: self._check_queries(queries), lambda: self.id_end, "id_end")
        return self._queries(queries), group_filter(argument, self.device)

    def _range_filter(self, who, queries, mask, masks, query_group):
        """(queries contiguous, the resolved filter of a range call: None, ("_masked", words, n_bits) or the tuple of _groups)."""
        one_filter(who, masks, query_group, mask=mask)
        if masks is not None:
            return self._groups(masks, query_group, queries)
        if mask is not None:
            mask = self._mask(mask)
        queries = self._queries(queries)
        return queries, (None if mask is None else ("_masked",) + mask_on_device(*mask, self.device))

    def range_search(self, queries, thresholds, sort=False, mask=None, masks=None, query_group=None):
        """Every document scoring above a threshold (faiss's IndexFlatIP.range_search; include/sr_hip.h sr_dense_range_count / _fill):
        queries fp32 cuda [nq, dim]; thresholds a float for all queries, or a tensor / array [nq].  Returns (lims int64 [nq + 1],
        scores fp32 [total], ids int64 [total]) as cuda tensors: the documents of query q with score > thresholds[q] are entries
        lims[q]:lims[q + 1], in (segment, row) order - ascending id for segments added in id order.  Scores are the exact chain of
        `score_pairs` for every nq.  sort=True: each list by score descending, ties by ascending id (range_sort).  mask (None: every
        document): a bitmap over [0, id_end) in the forms `search(mask=)` takes - only documents whose bit is set are returned
        (sr_dense_range_count_masked / _fill_masked; a set bit that names no document is ignored); one mask for all queries.
        masks + query_group (not together with mask): a bitmap per group and a group id per query in the forms `search_grouped` takes -
        query q gets the documents of masks[query_group[q]] (sr_dense_range_count_grouped / _fill_grouped): for every group exactly the
        lists of range_search(those queries, mask=masks[g]).  A group id outside [0, G): ValueError naming the query."""
        queries, filt = self._range_filter("range_search", queries, mask, masks, query_group)      # resolved once, shared by the two halves
        if filt is not None and filt[0] == "_masked" and filt[2] != self.id_end:
            raise ValueError(f"a mask of this index holds {self.id_end} flags (id_end), got {filt[2]}")
        queries, thr, lims, n = self._range_count(queries, thresholds, filt)
        scores, ids = self._range_fill(queries, thr, lims, n, filt)
        if sort:
            scores, ids = range_sort(lims, scores, ids)
        return lims, scores, ids

    def range_count(self, queries, thresholds, mask=None, masks=None, query_group=None):
        """The first half of range_search (sr_dense_range_count; under a mask sr_dense_range_count_masked, under masks + query_group
        sr_dense_range_count_grouped): returns (queries, thresholds [nq], lims int64 [nq + 1], total) - the contiguous tensors range_fill
        takes, and the sizes of the lists before anything of their size is allocated."""
        queries, filt = self._range_filter("range_count", queries, mask, masks, query_group)
        return self._range_count(queries, thresholds, filt)

    def _range_count(self, queries, thresholds, filt):
        nq = queries.shape[0]
        thr = _thresholds(thresholds, nq, self.device)
        lims = torch.empty((nq + 1,), dtype=torch.int64, device=self.device)
        total = ctypes.c_int64(0)
        suffix, spliced = _filter_args(filt)
        self._call("sr_dense_range_count" + suffix, _ptr(queries), nq, _ptr(thr), *spliced, _ptr(lims), ctypes.byref(total))
        return queries, thr, lims, total.value

    def range_fill(self, queries, thr, lims, n, mask=None, masks=None, query_group=None):
        """The second half (sr_dense_range_fill; under a mask sr_dense_range_fill_masked, under masks + query_group
        sr_dense_range_fill_grouped) for what the preceding range_count on this index returned, under the filter that count was given:
        (scores fp32 [n], ids int64 [n])."""
        queries, filt = self._range_filter("range_fill", queries, mask, masks, query_group)
        return self._range_fill(queries, thr, lims, n, filt)

    def _range_fill(self, queries, thr, lims, n, filt):
        suffix, spliced = _filter_args(filt)
        scores = torch.empty((max(1, n),), dtype=torch.float32, device=self.device)
        ids = torch.empty((max(1, n),), dtype=torch.int64, device=self.device)
        self._call("sr_dense_range_fill" + suffix, _ptr(queries), queries.shape[0], _ptr(thr), *spliced, _ptr(lims), _ptr(scores), _ptr(ids), n)
        return scores[:n], ids[:n]

    def search_collapsed(self, queries, k, keys, depths=None, fallback_bytes=1 << 30, subset=None, mask=None, masks=None, query_group=None,
                         hits=None, members=None):
        """The top-k distinct groups of every query, each represented and scored by its best passage (MaxP / field collapsing;
        collapse.py).  keys: int32 [id_end] tensor / array, the group key >= 0 of every document index.  Returns
        (scores fp32 [nq, k], ids int64 [nq, k] the best passages, keys int32 [nq, k], counts int32 [nq]) as cuda tensors, padded with
        (-FLT_MAX, -1, -1), and stats = {"depth": int64 [nq] the index into depths at which the query was proven complete, -1 = the
        full-ranking route; "groups_seen": int64 [nq]; "depths": the schedule} - exactly the first-occurrence-per-group row of the full
        ranking cut to k, whatever route served the query.  depths (default 4k, 16k, ... <= sr_max_topk()): the search depths of the
        rounds, each >= k, beyond sr_max_topk() allowed, clipped to the number of (allowed) documents; queries still open after the
        last depth are searched with k = that number, in sub-batches of fallback_bytes (a single query that does not fit: MemoryError
        naming it).  1 <= k <= sr_max_topk().  subset / mask / masks + query_group: the filters of `search` / `search_grouped`, one at
        most, resolved once per call; under masks the depths are clipped to sr_max_topk() (the grouped search's limit) and the
        full-ranking route runs group by group with mask=.  Precision other than "fp32" / "fp32_filtered": ValueError.
        Scores: every returned score is bit for bit score_pairs of (query, returned passage) and the ranking is by those scores.  Later
        rounds run on small sub-batches, and a batch of <= 64 queries otherwise accumulates in another order; the driver therefore
        switches set_batch_invariant(True) on for the duration of the call - every search of every round then accumulates in the
        pair scorer's order - and puts the caller's setting back afterwards.
        hits=m (1 <= m <= 64; None: off, the 5-tuple above unchanged): the tuple gains a sixth element (hit_scores fp32 [nq, k, m],
        hit_ids int64 [nq, k, m], hit_counts int32 [nq, k]) - for every returned group its passages that the call's filter allows for
        the query, by (score descending, id ascending), cut to m, padded with (-FLT_MAX, -1); hit_counts is the number of such
        passages before the cut (0 for a padding slot), min(hit_counts, m) entries of a list are hits, and hits[.., 0] is the group's
        representative, id and score bits.  Scores are score_pairs', computed inside the same batch-invariant scope; sub-batches
        are sized from fallback_bytes (collapse.group_hits).  members (None: built from keys per call): collapse.member_table(keys),
        prepared once.  stats gains "mean_hits", the mean number of hits returned per returned group."""
        from .collapse import dense_search_collapsed
        return dense_search_collapsed(self, queries, k, keys, depths=depths, fallback_bytes=fallback_bytes, subset=subset, mask=mask,
                                      masks=masks, query_group=query_group, hits=hits, members=members)

    def score_pairs(self, queries, cand_indptr, cand_ids):
        """Exact scores of given (query, document) pairs: queries fp32 cuda [nq, dim]; the candidates of query q are
        cand_ids[cand_indptr[q]:cand_indptr[q + 1]] (int64, the ids `search` returns; ragged, empty lists and repeats allowed, any
        length).  Returns fp32 cuda [total] - for every nq the fmaf chain of the exact score kernel, i.e. what `search` returns for
        that pair with more than 64 queries (include/sr_hip.h sr_dense_score_pairs).  An id outside the index: ValueError."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        cand_indptr, cand_ids, total = _candidates(cand_indptr, cand_ids, nq, self.device)
        out = torch.empty((max(1, total),), dtype=torch.float32, device=self.device)
        self._call("sr_dense_score_pairs", _ptr(queries), nq, _ptr(cand_indptr), _ptr(cand_ids), _ptr(out))
        return out[:total]

    def mmr(self, cand_ids, cand_rel, k, lam=0.5, counts=None):
        """Exact greedy Maximal Marginal Relevance over a candidate list per query (include/sr_hip.h sr_dense_mmr).
        cand_ids int64 [nq, n] (the ids `search` returns; id < 0 = padding), cand_rel fp32 [nq, n] the caller's relevance - a search's
        scores, a fused score, an RRF score; counts int32 [nq] the valid prefix of every row (None: n); 1 <= k <= n <=
        sr_mmr_max_candidates(), lam in [0, 1].  Pick 0 is the best candidate by (rel, id, position); pick t >= 1 maximises
        f32(f32(lam * rel_i) - f32((1 - lam) * m_i)), m_i = the largest inner product of stored row i with a selected row - every inner
        product the bits of `score_pairs` - ties by ascending id, then position.  Returns (ids int64 [nq, k], rel fp32 [nq, k] the picks'
        relevance, mmr fp32 [nq, k] the marginal value at the moment of each pick, pos int32 [nq, k] the picks' positions in their
        candidate row, counts int32 [nq]) as cuda tensors, padded with (-1, -FLT_MAX, -FLT_MAX, -1).  lam = 1 returns the first k candidates
        by (rel, id).  Rows and relevance must be finite (an overflowing inner product is outside the contract).  An id the index does
        not hold: ValueError naming query, entry and id."""
        from .mmr import mmr_arguments
        ids = _to_dev(cand_ids, torch.int64, self.device)
        rel = _to_dev(cand_rel, torch.float32, self.device)
        if ids.dim() != 2 or rel.shape != ids.shape:
            raise ValueError(f"expected cand_ids int64 [nq, n] and cand_rel fp32 of the same shape, got {tuple(ids.shape)} and {tuple(rel.shape)}")
        nq, n = ids.shape
        mmr_arguments("mmr", k, n, lam)
        if counts is not None:
            counts = _to_dev(counts, torch.int32, self.device)
            if counts.dim() != 1 or counts.numel() != nq:
                raise ValueError(f"expected {nq} counts, got {tuple(counts.shape)}")
        out_ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        out_rel = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        out_mmr = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        out_pos = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        out_counts = torch.empty((nq,), dtype=torch.int32, device=self.device)
        self._call("sr_dense_mmr", _ptr(ids), _ptr(rel), _ptr(counts), nq, n, int(k), float(lam), _ptr(out_ids), _ptr(out_rel), _ptr(out_mmr),
                   _ptr(out_pos), _ptr(out_counts))
        return out_ids, out_rel, out_mmr, out_pos, out_counts

    def search_mmr(self, queries, k, fetch_k, lam=0.5, subset=None, mask=None, masks=None, query_group=None):
        """Diversified search: the top fetch_k of `search` (under subset= / mask=) or of `search_grouped` (masks= + query_group=), then
        `mmr` over those rows with the search's scores as relevance.  k <= fetch_k <= sr_mmr_max_candidates().  Returns what `mmr`
        returns; pos is the pick's rank in the plain search.  lam = 1 returns the rows of search(queries, k), bit for bit."""
        from .mmr import mmr_arguments
        mmr_arguments("search_mmr", k, fetch_k, lam, masks, query_group, subset=subset, mask=mask)
        if masks is not None:
            scores, ids = self.search_grouped(queries, int(fetch_k), masks, query_group)
        else:
            scores, ids = self.search(queries, int(fetch_k), subset=subset, mask=mask)
        return self.mmr(ids, scores, k, lam)

    def feedback(self, queries, fb_ids, counts=None, n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0):
        """Rocchio's rebuilt queries (include/sr_hip.h sr_dense_feedback): queries fp32 cuda [nq, dim]; fb_ids int64
        [nq, depth] a ranked list per query of the ids `search` returns (id < 0 = padding), counts int32 [nq] its valid prefix (None:
        depth).  Of the valid entries the first min(n_pos, .) are the positive set, the last min(n_neg, what is left) the negative set;
        new = f32(f32(alpha * q) + f32(f32(beta / p) * P)), then f32(new - f32(f32(gamma / g) * N)) per column, P / N the sets' stored
        rows (fp16 rows widened exactly) summed in list order.  Returns fp32 cuda [nq, dim].  An id the index does not hold: ValueError
        naming query, entry and id."""
        from .prf import feedback_depth, prf_arguments
        prf_arguments("feedback", n_pos, n_neg, alpha, beta, gamma, depth=feedback_depth(fb_ids))
        ids = _to_dev(fb_ids, torch.int64, self.device)
        queries = self._queries(queries)
        nq = queries.shape[0]
        if ids.shape[0] != nq:
            raise ValueError(f"expected {nq} feedback rows, got {tuple(ids.shape)}")
        if counts is not None:
            counts = _to_dev(counts, torch.int32, self.device)
            if counts.dim() != 1 or counts.numel() != nq:
                raise ValueError(f"expected {nq} counts, got {tuple(counts.shape)}")
        out = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device)
        self._call("sr_dense_feedback", _ptr(queries), nq, _ptr(_valid(ids)), _ptr(counts), ids.shape[1], int(n_pos), int(n_neg), float(alpha),
                   float(beta), float(gamma), _ptr(out))
        return out

    def search_prf(self, queries, k, n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, fb_depth=None, subset=None, mask=None, masks=None,
                   query_group=None):
        """Search with pseudo-relevance feedback: the top fb_depth (default n_pos; >= n_pos + n_neg with a negative set) of `search`
        (under subset= / mask=) or of `search_grouped` (masks= + query_group=), `feedback` over those rows, then the search at k with the
        new queries under the same filter.  Returns (scores [nq, k], ids [nq, k], new queries [nq, dim]).  alpha = 1, beta = gamma = 0
        returns the rows of the plain search, bit for bit."""
        from .prf import prf_arguments
        depth = prf_arguments("search_prf", n_pos, n_neg, alpha, beta, gamma, first_round=True, fb_depth=fb_depth, allowed_masks=masks,
                              query_group=query_group, subset=subset, mask=mask)

        def search(qs, kk):
            if masks is not None:
                return self.search_grouped(qs, kk, masks, query_group)
            return self.search(qs, kk, subset=subset, mask=mask)
        _, fb = search(queries, depth)
        new = self.feedback(queries, fb, None, n_pos, n_neg, alpha, beta, gamma)
        scores, ids = search(new, int(k))
        return scores, ids, new

    def search_begin(self, queries, k, share):
        """First half of a doc-sharded search (include/sr_hip.h sr_dense_search_begin): returns lower [nq] fp32 (cuda) - per
        query a value at least ceil(k / share) documents of this index reach exactly (-inf where the filter does not apply).
        `queries` must be the same contiguous tensor that is passed to search_finish."""
        if self._queries(queries) is not queries:
            raise ValueError(f"expected a contiguous float32 cuda tensor [nq, {self.dim}], got {queries.dtype} {tuple(queries.shape)}")
        lower = torch.empty((queries.shape[0],), dtype=torch.float32, device=queries.device)
        self._call("sr_dense_search_begin", _ptr(queries), queries.shape[0], int(k), int(share), _ptr(lower))
        return lower

    def search_finish(self, queries, k, threshold=None):
        """Second half: threshold [nq] fp32 = the minimum of search_begin's values over all shards (None: a plain search).
        Returns (scores [nq, k], ids [nq, k]); rows may end in padding (id -1) - the shard returns what can reach the global top-k."""
        nq = queries.shape[0]
        scores, ids = _topk_outputs(nq, k, queries.device)
        if threshold is not None:
            threshold = threshold.to(device=queries.device, dtype=torch.float32).contiguous()
        self._call("sr_dense_search_finish", _ptr(queries), nq, int(k), _ptr(threshold), _ptr(scores), _ptr(ids))
        return scores, ids

    def close(self):
        if self._h:
            self.lib.sr_dense_index_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._segments = []
        self._segment_ids = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SparseIndexHIP:
    """CSR-by-term inverted index resident in HBM.

    indptr int64 [V+1], doc_ids int32 [nnz] (strictly ascending inside each term),
    vals fp32 [nnz]; n_docs = IndexDictOfArray.nb_docs().
    """

    def __init__(self, indptr, doc_ids, vals, n_docs, device=None):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.indptr = _to_dev(indptr, torch.int64, self.device)
        self.doc_ids = _valid(_to_dev(doc_ids, torch.int32, self.device))
        self.vals = _valid(_to_dev(vals, torch.float32, self.device))
        self.n_terms = self.indptr.numel() - 1
        self.n_docs = int(n_docs)
        self._forward = None            # forward_rows(): the doc-major CSR, built on first use
        self._h = ctypes.c_void_p()
        _call(self.device, "sr_sparse_index_create", ctypes.byref(self._h), _ptr(self.indptr), _ptr(self.doc_ids), _ptr(self.vals), self.n_terms,
              self.n_docs, lib=self.lib)

    def _call(self, name, *args, stream=True):
        """The C-ABI entry `name` on this index, on its device (doc_filter._call)."""
        _call(self.device, name, self._h, *args, stream=stream, lib=self.lib)

    def _query_csr(self, q_indptr, q_cols, q_vals):
        """Queries as CSR (tensors / arrays, any device) -> ((indptr int64 [nq + 1], cols int32, vals fp32) on the device, cols and
        vals with valid pointers, nq)."""
        q_indptr = _to_dev(q_indptr, torch.int64, self.device)
        q = (q_indptr, _valid(_to_dev(q_cols, torch.int32, self.device)), _valid(_to_dev(q_vals, torch.float32, self.device)))
        return q, q_indptr.numel() - 1

    def set_workspace_limit(self, nbytes):
        _lib.check(self.lib.sr_sparse_index_set_workspace_limit(self._h, int(nbytes)))

    def block_stats(self):
        """{"dense_terms", "block_calls", "fallback_calls"}: which of the two bit-identical scoring paths ran."""
        a, b, c = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self.lib.sr_sparse_index_block_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"dense_terms": a.value, "block_calls": b.value, "fallback_calls": c.value}

    def cert_stats(self):
        """Certified two-stage scorer (csrc/sparse_cert.hip): {"present", "dense_terms", "searches", "queries", "redone_exact", "doc_tiles",
        "candidates_rescored" (exact chains run by the certified path, rounded up to 16 per query), "batches_without_memory" (query batches
        the exact kernels served because the scorer's per-call buffers did not fit)}."""
        out = (ctypes.c_int64 * 8)()
        _lib.check(self.lib.sr_sparse_index_cert_stats(self._h, out), "sr_sparse_index_cert_stats")
        keys = ("present", "dense_terms", "searches", "queries", "redone_exact", "doc_tiles", "candidates_rescored", "batches_without_memory")
        return {k_: int(v) for k_, v in zip(keys, out)}

    def cert_record_keys(self, enable):
        """Test hook: keep the stage-1 keys of every (query, doc) pair of the following searches."""
        self._call("sr_sparse_index_cert_debug", 1 if enable else 0, None, 0, None, 0, None, None, stream=False)

    def cert_recorded_keys(self, nq):
        """(keys uint16 [nq_pad, n_tiles * 1024], consts fp32 [nq_pad, 6] = (c_q, s_q, rare terms, query terms, rare terms left out, the k-th best
        key the last top-k select of the scan saw: 0 if none ran), vscale, T) of the last search (after cert_record_keys(True))."""
        nq_pad = (nq + 31) // 32 * 32
        stride = self.cert_stats()["doc_tiles"] * 1024
        keys = np.empty((nq_pad, stride), dtype=np.uint16)
        consts = np.empty((nq_pad, 6), dtype=np.float32)
        vs, T = ctypes.c_float(0), ctypes.c_int32(0)
        self._call("sr_sparse_index_cert_debug", 2, keys.ctypes.data_as(ctypes.c_void_p), keys.size, consts.ctypes.data_as(ctypes.c_void_p),
                   nq_pad, ctypes.byref(vs), ctypes.byref(T), stream=False)
        return keys, consts, vs.value, T.value

    _CERT_BUFFERS = {"dslot": (1, np.int32), "vmax": (2, np.float32), "d16": (3, np.float16), "P": (4, np.uint32), "S": (5, np.uint32),
                     "E": (6, np.uint32), "fwd_indptr": (7, np.int64), "fwd_tv": (8, np.uint64), "bfrag": (9, np.float16),
                     "rare_term": (10, np.int32), "rare_w": (11, np.float32), "elig": (12, np.uint8), "cq": (13, np.float32),
                     "sq": (14, np.float32), "n_rare": (15, np.int32), "n_qt": (16, np.int32), "n_drop": (17, np.int32),
                     "m_count": (18, np.int32), "ap_ids": (19, np.int64), "uncert": (20, np.uint8)}

    def cert_readout(self, name):
        """Test hook (include/sr_hip.h sr_sparse_index_cert_readout): "info" -> {"T", "KS", "n_tiles", "e_stride", "V", "N", "nnz", "nq",
        "nq_pad", "k", "k_eff", "vscale"}; any other name of _CERT_BUFFERS -> that buffer as a flat numpy array of its element type."""
        what, dt = (0, np.int64) if name == "info" else self._CERT_BUFFERS[name]
        n = ctypes.c_int64(0)
        self._call("sr_sparse_index_cert_readout", what, None, 0, ctypes.byref(n), stream=False)
        out = np.empty(n.value // np.dtype(dt).itemsize, dtype=dt)
        self._call("sr_sparse_index_cert_readout", what, out.ctypes.data_as(ctypes.c_void_p), out.nbytes, ctypes.byref(n), stream=False)
        if name != "info":
            return out
        keys = ("T", "KS", "n_tiles", "e_stride", "V", "N", "nnz", "nq", "nq_pad", "k", "k_eff")
        info = {k_: int(v) for k_, v in zip(keys, out)}
        info["vscale"] = float(np.array([out[11]], np.int64).astype(np.uint32).view(np.float32)[0])
        return info

    def work_counters(self, enable):
        """Switch the query-block kernel's work counters on / off; returns what was counted since the last call:
        {"dense_columns_loaded", "dense_column_applications", "light_postings", "grouped_postings", "plan_entries", "workgroup_tiles"}."""
        out = (ctypes.c_uint64 * 6)()
        self._call("sr_sparse_index_work_counters", 1 if enable else 0, out, stream=False)
        keys = ("dense_columns_loaded", "dense_column_applications", "light_postings", "grouped_postings", "plan_entries", "workgroup_tiles")
        return {k_: int(v) for k_, v in zip(keys, out)}

    def _mask(self, mask):
        """The host step of a mask= argument of this index (doc_filter.mask_argument)."""
        return mask_argument(mask, lambda: self.n_docs, "n_docs")

    def search(self, q_indptr, q_cols, q_vals, k, threshold=0.0, id_base=0, id_stride=1, subset=None, mask=None):
        """Queries as CSR tensors. Returns (scores [nq,k], ids [nq,k], counts [nq]) cuda tensors.  subset (None: every document):
        strictly ascending int64 document positions in [0, n_docs), one allow-list for all queries (include/sr_hip.h
        sr_sparse_search_subset); a position outside the index or out of order: ValueError naming it.  mask: the same filter as a
        bitmap over [0, n_docs) - a bool tensor / array of length n_docs (packed on the device), or int32 / uint32 words already
        packed (pack_doc_mask) - with exactly the result of `subset` = the set positions (sr_sparse_search_masked).  One of the two
        at most."""
        one_filter("search", subset=subset, mask=mask)
        if mask is not None:
            mask = self._mask(mask)
        q, nq = self._query_csr(q_indptr, q_cols, q_vals)
        filt = None
        if mask is not None:
            filt = ("_masked",) + mask_on_device(*mask, self.device)
        elif subset is not None:
            filt = ("_subset",) + _subset(subset, self.device)
        return self._search(q, nq, k, threshold, filt, id_base, id_stride)

    def _search(self, q, nq, k, threshold, filt, id_base, id_stride):
        scores, ids, counts = _topk_outputs(nq, k, self.device, counts=True)
        suffix, spliced = _filter_args(filt)
        self._call("sr_sparse_search" + suffix, *map(_ptr, q), nq, int(k), float(threshold), *spliced, int(id_base), int(id_stride),
                   _ptr(scores), _ptr(ids), _ptr(counts))
        return scores, ids, counts

    def search_grouped(self, q_indptr, q_cols, q_vals, k, masks, query_group, threshold=0.0, id_base=0, id_stride=1):
        """Top-k of every query within its own group's documents (include/sr_hip.h sr_sparse_search_grouped).  masks: one bitmap per group
        over [0, n_docs) - bool [G, n_docs] (tensor / array, packed on the device) or int32 / uint32 words [G, ceil(n_docs / 32)] already
        packed (pack_doc_masks); query_group: int array / tensor [nq], query q searches under masks[query_group[q]].  The rows of a
        group's queries are exactly what search(those queries, k, mask=masks[g]) returns.  Returns (scores [nq,k], ids [nq,k], counts
        [nq]).  Wrong shapes, a wrong word count, a length mismatch or non-integer groups: ValueError before anything is uploaded; a group
        id outside [0, G): ValueError naming the query, every row of the result is then padding."""
        q, nq, filt = self._groups(masks, query_group, q_indptr, q_cols, q_vals)
        return self._search(q, nq, k, threshold, filt, id_base, id_stride)

    def _groups(self, masks, query_group, q_indptr, q_cols, q_vals):
        """As DenseIndexHIP._groups: (the query CSR on the device, nq, the "_grouped" filter)."""
        argument = group_argument(masks, query_group, lambda: len(q_indptr) - 1, lambda: self.n_docs, "n_docs")
        q, nq = self._query_csr(q_indptr, q_cols, q_vals)
        return q, nq, group_filter(argument, self.device)

    def _range_filter(self, who, q_indptr, q_cols, q_vals, mask, masks, query_group):
        """As DenseIndexHIP._range_filter: (the query CSR on the device, nq, the resolved filter of a range call)."""
        one_filter(who, masks, query_group, mask=mask)
        if masks is not None:
            return self._groups(masks, query_group, q_indptr, q_cols, q_vals)
        if mask is not None:
            mask = self._mask(mask)
        q, nq = self._query_csr(q_indptr, q_cols, q_vals)
        return q, nq, (None if mask is None else ("_masked",) + mask_on_device(*mask, self.device))

    def range_search(self, q_indptr, q_cols, q_vals, thresholds, id_base=0, id_stride=1, sort=False, mask=None, masks=None, query_group=None):
        """Every document scoring above a threshold - the full list of numba_score_float (scaling_retriever/indexer.py:324-344;
        include/sr_hip.h sr_sparse_range_count / _fill): queries as CSR as for `search`; thresholds a float for all queries, or a
        tensor / array [nq].  Returns (lims int64 [nq + 1], scores fp32 [total], ids int64 [total]) as cuda tensors: the documents of
        query q with score > thresholds[q] are entries lims[q]:lims[q + 1], in ascending document position, ids = id_base + position *
        id_stride.  A document without a common term scores 0.0 and is returned exactly under a negative threshold.  Scores are the
        chain of `score_pairs`.  sort=True: each list by score descending, ties by ascending id (range_sort).  mask (None: every
        document): a bitmap over [0, n_docs) in the forms `search(mask=)` takes - only documents whose bit is set are returned
        (sr_sparse_range_count_masked / _fill_masked), a document without a common term included when the threshold is negative.
        masks + query_group (not together with mask): a bitmap per group and a group id per query in the forms `search_grouped` takes -
        query q gets the documents of masks[query_group[q]] (sr_sparse_range_count_grouped / _fill_grouped): for every group exactly the
        lists of range_search(those queries, mask=masks[g]).  A group id outside [0, G): ValueError naming the query."""
        q, nq, filt = self._range_filter("range_search", q_indptr, q_cols, q_vals, mask, masks, query_group)
        thr = _valid(_thresholds(thresholds, nq, self.device))
        if sort and int(id_base) + (self.n_docs - 1) * int(id_stride) >= 1 << 32:
            raise ValueError("sort=True orders by the search's 64-bit key, which holds ids below 2^32; sort the lists of larger ids yourself")
        lims = torch.empty((nq + 1,), dtype=torch.int64, device=self.device)
        total = ctypes.c_int64(0)
        suffix, spliced = _filter_args(filt)
        head = (*map(_ptr, q), nq, _ptr(thr), *spliced, _ptr(lims))
        self._call("sr_sparse_range_count" + suffix, *head, ctypes.byref(total))
        n = total.value
        scores = torch.empty((max(1, n),), dtype=torch.float32, device=self.device)
        ids = torch.empty((max(1, n),), dtype=torch.int64, device=self.device)
        self._call("sr_sparse_range_fill" + suffix, *head, int(id_base), int(id_stride), _ptr(scores), _ptr(ids), n)
        scores, ids = scores[:n], ids[:n]
        if sort:
            scores, ids = range_sort(lims, scores, ids)
        return lims, scores, ids

    def search_collapsed(self, q_indptr, q_cols, q_vals, k, keys, threshold=0.0, id_base=0, id_stride=1, depths=None, fallback_bytes=1 << 30,
                         subset=None, mask=None, masks=None, query_group=None, hits=None, members=None):
        """The top-k distinct groups of every query, each represented and scored by its best passage (collapse.py):
        DenseIndexHIP.search_collapsed on this head.  Queries, threshold, id_base / id_stride as for `search` - only documents with
        score > threshold are ranked; keys int32 is indexed by the ids the search returns (id_base + position * id_stride), so it holds
        id_base + (n_docs - 1) * id_stride + 1 entries; the search's counts are handed to the device step.  Filters as for `search` /
        `search_grouped`, one at most.  Returns (scores, ids, keys, counts, stats) as there.  hits=m: the sixth element (hit_scores,
        hit_ids, hit_counts) as there - a hit must also score > threshold, the padding is (0, -1), ids are id_base + position *
        id_stride, scores sr_sparse_score_pairs'.  members (None: built per call): collapse.member_table of the keys BY DOCUMENT
        POSITION (keys[id_base + id_stride * arange(n_docs)]), the numbering of this head's bitmaps and pair scorer."""
        from .collapse import sparse_search_collapsed
        return sparse_search_collapsed(self, q_indptr, q_cols, q_vals, k, keys, threshold=threshold, id_base=id_base, id_stride=id_stride,
                                       depths=depths, fallback_bytes=fallback_bytes, subset=subset, mask=mask, masks=masks,
                                       query_group=query_group, hits=hits, members=members)

    def score_pairs(self, q_indptr, q_cols, q_vals, cand_indptr, cand_ids):
        """Exact scores of given (query, document) pairs: queries as for `search`, candidates as for DenseIndexHIP.score_pairs (ids =
        document positions).  Returns fp32 cuda [total]: the reference's term-serial chain, no threshold, 0.0 where nothing matches
        (include/sr_hip.h sr_sparse_score_pairs).  An id outside [0, n_docs): ValueError."""
        q, nq = self._query_csr(q_indptr, q_cols, q_vals)
        cand_indptr, cand_ids, total = _candidates(cand_indptr, cand_ids, nq, self.device)
        out = torch.empty((max(1, total),), dtype=torch.float32, device=self.device)
        self._call("sr_sparse_score_pairs", *map(_ptr, q), nq, _ptr(cand_indptr), _ptr(cand_ids), _ptr(out))
        return out[:total]

    def forward_rows(self):
        """The index by document: (indptr int64 [n_docs + 1], terms int32 [nnz] ascending inside a document, vals fp32 [nnz]) on the device,
        built on first use from the index's own CSR-by-term tensors with sparse_csr_expand_terms + sparse_csr_build (documents as the sort
        key: the stable sort over term-major input leaves the terms of a document ascending) and kept: 8 bytes per posting + 8 per
        document, until drop_forward_rows().  Independent of the certified scorer's private forward index."""
        if self._forward is None:
            nnz = int(self.indptr[-1])
            terms = sparse_csr_expand_terms(self.indptr, nnz)
            self._forward = sparse_csr_build(terms, self.doc_ids[:nnz], self.vals[:nnz], self.n_docs)
        return self._forward

    def drop_forward_rows(self):
        """Frees what forward_rows() keeps; the next call builds it again."""
        self._forward = None

    def feedback(self, q_indptr, q_cols, q_vals, fb_ids, counts=None, n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=128):
        """Rocchio's rebuilt queries over this index's documents (sparse_feedback below, on forward_rows()): queries as CSR as for
        `search` (columns strictly ascending inside a row), fb_ids int64 [nq, depth] document positions (a search's ids under id_base = 0,
        id_stride = 1; < 0 = padding), counts its valid prefix.  Returns (indptr, cols, vals) of the new queries."""
        from .prf import feedback_depth, prf_arguments
        prf_arguments("feedback", n_pos, n_neg, alpha, beta, gamma, max_terms, depth=feedback_depth(fb_ids))
        q, _ = self._query_csr(q_indptr, q_cols, q_vals)
        return sparse_feedback(*q, *self.forward_rows(), self.n_terms, fb_ids, counts=counts, n_pos=n_pos, n_neg=n_neg, alpha=alpha, beta=beta,
                               gamma=gamma, max_terms=max_terms)

    def search_prf(self, q_indptr, q_cols, q_vals, k, n_pos=10, n_neg=0, alpha=1.0, beta=0.75, gamma=0.0, max_terms=128, fb_depth=None,
                   threshold=0.0, id_base=0, id_stride=1, subset=None, mask=None, masks=None, query_group=None):
        """Search with pseudo-relevance feedback: the first round is `search` (subset= / mask=) or `search_grouped` (masks= + query_group=)
        at depth fb_depth (default n_pos; >= n_pos + n_neg with a negative set) in positions (id_base = 0, id_stride = 1), then `feedback`
        over its rows and counts, then the search at k with the new queries under the same filter, threshold, id_base and id_stride.
        Returns (scores [nq, k], ids [nq, k], counts [nq], (indptr, cols, vals) of the new queries).  With alpha = 1, beta = gamma = 0 and
        no binding max_terms the result is `search(k)` of the queries' positive terms, bit for bit."""
        from .prf import prf_arguments
        depth = prf_arguments("search_prf", n_pos, n_neg, alpha, beta, gamma, max_terms, first_round=True, fb_depth=fb_depth, allowed_masks=masks,
                              query_group=query_group, subset=subset, mask=mask)

        def search(q, kk, base, stride):
            if masks is not None:
                return self.search_grouped(*q, kk, masks, query_group, threshold=threshold, id_base=base, id_stride=stride)
            return self.search(*q, kk, threshold=threshold, id_base=base, id_stride=stride, subset=subset, mask=mask)
        q, _ = self._query_csr(q_indptr, q_cols, q_vals)             # uploaded once for the three steps
        _, fb, fb_counts = search(q, depth, 0, 1)
        new = self.feedback(*q, fb, fb_counts, n_pos, n_neg, alpha, beta, gamma, max_terms)
        scores, ids, counts = search(new, int(k), id_base, id_stride)
        return scores, ids, counts, new

    def mmr(self, cand_ids, cand_rel, k, lam=0.5, counts=None, sim="cosine"):
        """Exact greedy Maximal Marginal Relevance over a candidate list per query on this index's documents (sparse_mmr below, on
        forward_rows()): cand_ids int64 [nq, n] document positions (a search's ids under id_base = 0, id_stride = 1; < 0 = padding),
        cand_rel fp32 [nq, n], counts the valid prefix.  Returns what DenseIndexHIP.mmr returns."""
        return sparse_mmr(*self.forward_rows(), cand_ids, cand_rel, k, lam, counts=counts, sim=sim)

    def search_mmr(self, q_indptr, q_cols, q_vals, k, fetch_k, lam=0.5, sim="cosine", threshold=0.0, id_base=0, id_stride=1, subset=None,
                   mask=None, masks=None, query_group=None):
        """Diversified search: the top fetch_k of `search` (subset= / mask=) or of `search_grouped` (masks= + query_group=) in positions
        (id_base = 0, id_stride = 1), then `mmr` over those rows and counts with the search's scores as relevance, then the picks' ids
        as id_base + position * id_stride (padding stays -1).  k <= fetch_k <= sr_mmr_max_candidates().  Returns what `mmr` returns; pos
        is the pick's rank in the plain search.  lam = 1 returns the rows of search(k) - ids and scores - bit for bit."""
        from .mmr import mmr_arguments
        mmr_arguments("search_mmr", k, fetch_k, lam, masks, query_group, sim=sim, subset=subset, mask=mask)
        q, _ = self._query_csr(q_indptr, q_cols, q_vals)
        if masks is not None:
            scores, ids, counts = self.search_grouped(*q, int(fetch_k), masks, query_group, threshold=threshold)
        else:
            scores, ids, counts = self.search(*q, int(fetch_k), threshold=threshold, subset=subset, mask=mask)
        ids, rel, mmr, pos, counts = self.mmr(ids, scores, k, lam, counts=counts, sim=sim)
        if int(id_base) != 0 or int(id_stride) != 1:
            ids = torch.where(ids >= 0, int(id_base) + ids * int(id_stride), ids)
        return ids, rel, mmr, pos, counts

    def close(self):
        if self._h:
            self.lib.sr_sparse_index_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._forward = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sparse_csr_build(rows, cols, vals, n_terms, n_docs=0, sort_docs=False):
    """Doc-major postings (cuda tensors: rows int32 = global doc row, cols int32 = term, vals fp32; insertion order) -> CSR by term
    (indptr int64 [n_terms + 1], doc_ids int32, vals fp32) with sr_sparse_csr_build: this library's stable radix sort on the device.
    Replaces the per-posting append of IndexDictOfArray.add_batch_document (inverted_index.py:67-76)."""
    _lib.require_gpu()
    rows = rows.to(torch.int32).contiguous()
    cols = cols.to(torch.int32).contiguous()
    vals = vals.to(torch.float32).contiguous()
    nnz = rows.numel()
    dev = rows.device
    indptr = torch.empty(int(n_terms) + 1, dtype=torch.int64, device=dev)
    out_rows = torch.empty(max(1, nnz), dtype=torch.int32, device=dev)
    out_vals = torch.empty(max(1, nnz), dtype=torch.float32, device=dev)
    _call(dev, "sr_sparse_csr_build", _ptr(rows), _ptr(cols), _ptr(vals), nnz, int(n_terms), int(n_docs), 1 if sort_docs else 0, _ptr(indptr),
          _ptr(out_rows), _ptr(out_vals))
    return indptr, out_rows[:nnz], out_vals[:nnz]


def sparse_csr_expand_terms(indptr, nnz):
    """Term of every posting of a CSR-by-term index (indptr int64 [V + 1] on the device) -> int32 [nnz]: sr_sparse_csr_expand_terms."""
    _lib.require_gpu()
    indptr = indptr.to(torch.int64).contiguous()
    out = torch.empty(max(1, int(nnz)), dtype=torch.int32, device=indptr.device)
    _call(indptr.device, "sr_sparse_csr_expand_terms", _ptr(indptr), indptr.numel() - 1, int(nnz), _ptr(out))
    return out[:int(nnz)]


def token_counts(input_ids, attention_mask=None, skip_ids=(), n_terms=None):
    """Term frequencies of token rows (include/sr_hip.h sr_token_counts): input_ids int [B, L] and attention_mask [B, L]
    (None: every slot is real) as a loader delivers them, padding on either side; a slot counts when its mask is non-zero and its id is
    none of skip_ids (at most 16: BOS, EOS, pad).  Returns cuda tensors (row_ptr int64 [B + 1], cols int32 [nnz] - the distinct counted
    ids of a row, ascending -, vals fp32 [nnz] - their occurrences -, lengths int32 [B] - the counted slots of a row).  A counted id
    outside [0, n_terms): ValueError naming row, position and id.  L above sr_token_counts_max_len() (8192): ValueError."""
    _lib.require_gpu()
    if n_terms is None:
        raise ValueError("token_counts: n_terms (the size of the vocabulary) must be given")
    dev = _cuda_device(input_ids)
    ids = _to_dev(input_ids, torch.int64, dev)
    if ids.dim() != 2:
        raise ValueError(f"expected input_ids [B, L], got {tuple(ids.shape)}")
    B, L = ids.shape
    mask = None
    if attention_mask is not None:
        mask = _to_dev(attention_mask, torch.int64, dev)
        if mask.shape != ids.shape:
            raise ValueError(f"expected an attention_mask of shape {tuple(ids.shape)}, got {tuple(mask.shape)}")
    skip = [int(x) for x in skip_ids]
    if any(not -2 ** 31 <= x < 2 ** 31 for x in skip):
        raise ValueError(f"skip_ids must be int32 values, got {skip}")
    h_skip = (ctypes.c_int32 * max(1, len(skip)))(*skip)
    row_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    lengths = torch.empty(B, dtype=torch.int32, device=dev)
    # a guess first, and one more call with the size the first one names if it was short, as sparse_reps_to_csr; B * L always fits
    cap = max(1, min(B * L, 1 << 22))
    n = ctypes.c_int64(0)
    lib = _lib.load()
    with torch.cuda.device(dev):
        while True:
            cols = torch.empty(cap, dtype=torch.int32, device=dev)
            vals = torch.empty(cap, dtype=torch.float32, device=dev)
            rc = lib.sr_token_counts(_ptr(_valid(ids)), _ptr(mask if mask is None else _valid(mask)), B, L, h_skip, len(skip), int(n_terms),
                                     _ptr(row_ptr), _ptr(cols), _ptr(vals), _ptr(_valid(lengths)), cap, ctypes.byref(n), _lib.stream_ptr())
            if rc == _lib.SR_ERR_NOMEM and n.value > cap:
                cap = n.value
                continue
            _lib.check(rc, "sr_token_counts")
            break
    return row_ptr, cols[:n.value], vals[:n.value], lengths


def bm25_weights(indptr, doc_ids, tf, doc_len, idf, numer, a, s, out=None):
    """BM25 weights of a term-major CSR of term frequencies (include/sr_hip.h sr_bm25_weights): indptr int64
    [n_terms + 1], doc_ids int32 [nnz], tf fp32 [nnz], doc_len int32 [n_docs], idf fp32 [n_terms] on the device; numer, a, s the three
    fp32 scalars of bm25.bm25_scalars.  w = f32(idf[t] * f32(f32(tf * numer) / f32(tf + f32(a + f32(s * f32(doc_len[d])))))).  out: the
    fp32 [nnz] tensor to write (may be tf itself); None: a new one.  Returns it.  A document id outside [0, n_docs): ValueError."""
    _lib.require_gpu()
    dev = _cuda_device(tf)
    indptr = _to_dev(indptr, torch.int64, dev)
    doc_ids = _to_dev(doc_ids, torch.int32, dev)
    tf = _to_dev(tf, torch.float32, dev)
    doc_len = _to_dev(doc_len, torch.int32, dev)
    idf = _to_dev(idf, torch.float32, dev)
    nnz, n_terms = tf.numel(), indptr.numel() - 1
    if indptr.dim() != 1 or n_terms < 0 or doc_ids.shape != tf.shape or tf.dim() != 1 or idf.shape != (max(n_terms, 0),) or doc_len.dim() != 1:
        raise ValueError(f"expected indptr [n_terms + 1], doc_ids / tf [nnz], idf [n_terms], doc_len [n_docs]; got {tuple(indptr.shape)}, "
                         f"{tuple(doc_ids.shape)}, {tuple(tf.shape)}, {tuple(idf.shape)}, {tuple(doc_len.shape)}")
    # the kernel trusts indptr to end at nnz: the one thing checked here, as for candidate lists
    if int(indptr[-1]) != nnz or int(indptr[0]) != 0:
        raise ValueError(f"indptr runs from {int(indptr[0])} to {int(indptr[-1])}, the CSR holds {nnz} postings")
    if out is None:
        out = torch.empty(nnz, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == tf.shape):
        raise ValueError("out must be a contiguous fp32 cuda tensor of tf's shape")
    _call(dev, "sr_bm25_weights", _ptr(indptr), _ptr(_valid(doc_ids)), _ptr(_valid(tf)), n_terms, nnz, _ptr(_valid(doc_len)), doc_len.numel(),
          _ptr(_valid(idf)), float(numer), float(a), float(s), _ptr(_valid(out)))
    return out


def sparse_feedback(q_indptr, q_cols, q_vals, doc_indptr, doc_cols, doc_vals, n_terms, fb_ids, counts=None, n_pos=10, n_neg=0, alpha=1.0,
                    beta=0.75, gamma=0.0, max_terms=128):
    """Rocchio's rebuilt sparse queries (include/sr_hip.h sr_sparse_feedback): queries as CSR (columns strictly ascending
    inside a row), the documents as a doc-major CSR on the device (SparseIndexHIP.forward_rows()), fb_ids int64 [nq, depth] a ranked list
    of document positions per query (< 0 = padding), counts int32 [nq] its valid prefix (None: depth).  Of the valid entries the first
    min(n_pos, .) are the positive set, the last min(n_neg, what is left) the negative set; per term w = f32(f32(alpha * q) + f32(f32(beta
    / p) * P)), then f32(w - f32(f32(gamma / g) * N)), P / N summed in list order; terms with w > 0 are kept, of those the max_terms
    largest (w descending, term ascending; 0 = no limit), emitted with terms ascending.  Returns (indptr int64 [nq + 1], cols int32, vals
    fp32) cuda tensors.  A position outside [0, n_docs) or query columns out of order: ValueError naming the place."""
    from .prf import feedback_depth, prf_arguments
    prf_arguments("sparse_feedback", n_pos, n_neg, alpha, beta, gamma, max_terms, depth=feedback_depth(fb_ids))
    dev = doc_vals.device
    fb = _to_dev(fb_ids, torch.int64, dev)
    q_indptr = _to_dev(q_indptr, torch.int64, dev)
    q_cols, q_vals = _valid(_to_dev(q_cols, torch.int32, dev)), _valid(_to_dev(q_vals, torch.float32, dev))
    nq = q_indptr.numel() - 1
    if fb.shape[0] != nq:
        raise ValueError(f"expected {nq} feedback rows, got {tuple(fb.shape)}")
    if counts is not None:
        counts = _to_dev(counts, torch.int32, dev)
        if counts.dim() != 1 or counts.numel() != nq:
            raise ValueError(f"expected {nq} counts, got {tuple(counts.shape)}")
    doc_indptr = _to_dev(doc_indptr, torch.int64, dev)
    doc_cols, doc_vals = _valid(_to_dev(doc_cols, torch.int32, dev)), _valid(_to_dev(doc_vals, torch.float32, dev))
    n_docs, max_terms = doc_indptr.numel() - 1, int(max_terms)
    indptr = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    # a budget bounds the output; without one a guess (8 bytes each), and one more call with the size the first one names if it was short
    cap = max(1, nq * min(max_terms, int(n_terms)) if max_terms else nq * min(int(n_terms), 4096))
    n = ctypes.c_int64(0)
    lib = _lib.load()
    with torch.cuda.device(dev):
        while True:
            cols = torch.empty(cap, dtype=torch.int32, device=dev)
            vals = torch.empty(cap, dtype=torch.float32, device=dev)
            rc = lib.sr_sparse_feedback(_ptr(q_indptr), _ptr(q_cols), _ptr(q_vals), nq, _ptr(doc_indptr), _ptr(doc_cols), _ptr(doc_vals), n_docs,
                                        int(n_terms), _ptr(_valid(fb)), _ptr(counts), fb.shape[1], int(n_pos), int(n_neg), float(alpha),
                                        float(beta), float(gamma), max_terms, _ptr(indptr), _ptr(cols), _ptr(vals), cap, ctypes.byref(n),
                                        _lib.stream_ptr())
            if rc == _lib.SR_ERR_NOMEM and n.value > cap:
                cap = n.value
                continue
            _lib.check(rc, "sr_sparse_feedback")
            break
    return indptr, cols[:n.value], vals[:n.value]


def sparse_mmr(doc_indptr, doc_cols, doc_vals, cand_ids, cand_rel, k, lam=0.5, counts=None, sim="cosine"):
    """Exact greedy Maximal Marginal Relevance on the sparse head (include/sr_hip.h sr_sparse_mmr): the documents as a
    doc-major CSR on the device (SparseIndexHIP.forward_rows()), cand_ids int64 [nq, n] document positions (< 0 = padding), cand_rel fp32
    [nq, n] the caller's relevance, counts int32 [nq] the valid prefix of every row (None: n); 1 <= k <= n <= sr_mmr_max_candidates(),
    lam in [0, 1].  sim = "ip": the similarity of two documents is the term-serial chain over their common terms in ascending term
    order - the bits of `score_pairs` with one row as the query; sim = "cosine": that over f32(norm_i * norm_j), norm = f32(sqrt(ip(i,
    i))), +0.0 where a norm is zero.  Selection and the five returned tensors as DenseIndexHIP.mmr.  A position outside [0, n_docs):
    ValueError naming query, entry and id."""
    from .mmr import SIM_MODES, mmr_arguments
    dev = doc_vals.device
    ids = _to_dev(cand_ids, torch.int64, dev)
    rel = _to_dev(cand_rel, torch.float32, dev)
    if ids.dim() != 2 or rel.shape != ids.shape:
        raise ValueError(f"expected cand_ids int64 [nq, n] and cand_rel fp32 of the same shape, got {tuple(ids.shape)} and {tuple(rel.shape)}")
    nq, n = ids.shape
    mmr_arguments("sparse_mmr", k, n, lam, sim=sim)
    if counts is not None:
        counts = _to_dev(counts, torch.int32, dev)
        if counts.dim() != 1 or counts.numel() != nq:
            raise ValueError(f"expected {nq} counts, got {tuple(counts.shape)}")
    doc_indptr = _to_dev(doc_indptr, torch.int64, dev)
    doc_cols, doc_vals = _valid(_to_dev(doc_cols, torch.int32, dev)), _valid(_to_dev(doc_vals, torch.float32, dev))
    k = int(k)
    out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_rel = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_mmr = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_pos = torch.empty((nq, k), dtype=torch.int32, device=dev)
    out_counts = torch.empty((nq,), dtype=torch.int32, device=dev)
    _call(dev, "sr_sparse_mmr", _ptr(doc_indptr), _ptr(doc_cols), _ptr(doc_vals), doc_indptr.numel() - 1, _ptr(ids), _ptr(rel), _ptr(counts),
          nq, n, k, float(lam), SIM_MODES[sim], _ptr(out_ids), _ptr(out_rel), _ptr(out_mmr), _ptr(out_pos), _ptr(out_counts))
    return out_ids, out_rel, out_mmr, out_pos, out_counts


def topk_merge(scores, ids, pad_score=-3.402823466e38):
    """Merge per-shard top-k lists: scores fp32 [W, nq, k], ids int64 [W, nq, k] (cuda) -> ([nq,k], [nq,k])."""
    _lib.require_gpu()
    lib = _lib.load()
    if scores.dim() != 3 or ids.shape != scores.shape:
        raise ValueError("expected scores/ids of shape [n_lists, nq, k]")
    scores = scores.contiguous().float()
    ids = ids.contiguous().to(torch.int64)
    W, nq, k = scores.shape
    out_s = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    _lib.check(lib.sr_topk_merge(_ptr(scores), _ptr(ids), W, nq, k, float(pad_score), _ptr(out_s), _ptr(out_i),
                                 _lib.stream_ptr()), "sr_topk_merge")
    return out_s, out_i


def hybrid_union(a_ids, b_spos, b_counts, s2d, d2s, a_indptr=None):
    """Per query the set union of two lists of dense positions (sr_hybrid_union, csrc/hybrid_fuse.hip), all cuda tensors: a_ids int64
    [nq, kd] with negative padding in any order (a dense top-k, kd <= sr_max_topk()) - or, with a_indptr int64 [nq + 1], a CSR of
    strictly ascending positions of any length (range hits); b_spos int64 [nq, ks] SPARSE positions with b_counts int32 [nq] valid
    entries per row (ks <= sr_max_topk()), mapped through s2d on the device; d2s / s2d the two position maps (int64, -1 = none).
    Returns (indptr int64 [nq + 1], dpos, spos, tie int64 [total]): each query's union ascending and duplicate-free, spos = d2s[dpos],
    tie = spos where spos >= 0 else len(s2d) + dpos.  A sparse position without a dense document: ValueError naming it."""
    _lib.require_gpu()
    dev = b_spos.device
    b_spos = b_spos.to(torch.int64).contiguous()
    b_counts = b_counts.to(device=dev, dtype=torch.int32).contiguous()
    s2d, d2s = s2d.to(device=dev, dtype=torch.int64).contiguous(), d2s.to(device=dev, dtype=torch.int64).contiguous()
    if b_spos.dim() != 2 or b_counts.dim() != 1 or b_counts.numel() != b_spos.shape[0]:
        raise ValueError(f"expected b_spos [nq, ks] and b_counts [nq], got {tuple(b_spos.shape)} and {tuple(b_counts.shape)}")
    nq, ks = b_spos.shape
    a_ids = a_ids.to(device=dev, dtype=torch.int64).contiguous()
    if a_indptr is None:
        if a_ids.dim() != 2 or a_ids.shape[0] != nq:
            raise ValueError(f"expected a_ids [{nq}, kd], got {tuple(a_ids.shape)}")
        kd = a_ids.shape[1]
        capacity = nq * (kd + ks)
    else:
        a_indptr = a_indptr.to(device=dev, dtype=torch.int64).contiguous()
        if a_ids.dim() != 1 or a_indptr.dim() != 1 or a_indptr.numel() != nq + 1:
            raise ValueError(f"expected a CSR over {nq} queries, got a_indptr {tuple(a_indptr.shape)} and a_ids {tuple(a_ids.shape)}")
        if int(a_indptr[-1]) != a_ids.numel() or int(a_indptr[0]) != 0:      # the kernels trust a_indptr for the extent of a_ids
            raise ValueError(f"a_indptr runs from {int(a_indptr[0])} to {int(a_indptr[-1])}, a_ids holds {a_ids.numel()} positions")
        kd = 0
        capacity = a_ids.numel() + nq * ks
    indptr = torch.empty((nq + 1,), dtype=torch.int64, device=dev)
    out = torch.empty((3, max(1, capacity)), dtype=torch.int64, device=dev)
    keep = [_valid(t) for t in (a_ids, b_spos, b_counts, s2d, d2s)]
    p = [_ptr(t) for t in keep]
    total = ctypes.c_int64(0)
    _call(dev, "sr_hybrid_union", p[0], _ptr(a_indptr), kd, p[1], p[2], ks, p[3], s2d.numel(), p[4], d2s.numel(), nq, _ptr(indptr), _ptr(out[0]),
          _ptr(out[1]), _ptr(out[2]), capacity, ctypes.byref(total))
    n = total.value
    return indptr, out[0, :n], out[1, :n], out[2, :n]


def hybrid_rank(cand_indptr, dpos, spos, tie, dense_scores, sparse_scores, weights, k, D, S, complete, n_s2d, id_end):
    """Top-k of ragged candidate lists by (fused descending, tie ascending), the certificate and the range threshold (sr_hybrid_rank,
    csrc/hybrid_fuse.hip): cuda tensors as hybrid_union and the two score_pairs return them; weights (w_d, w_s); D, S fp32 [nq] the
    k'-th scores of the two searches, complete bool [nq] = the dense list held every document.  Returns (scores fp32 [nq, k] padded
    with -FLT_MAX, dense positions int64 [nq, k] padded with -1, counts int32 [nq], certified int32 [nq], threshold fp32 [nq])."""
    _lib.require_gpu()
    dev = cand_indptr.device
    nq = cand_indptr.numel() - 1
    i64 = [t.to(device=dev, dtype=torch.int64).contiguous() for t in (cand_indptr, dpos, spos, tie)]
    f32 = [t.to(device=dev, dtype=torch.float32).contiguous() for t in (dense_scores, sparse_scores, D, S)]
    complete = complete.to(device=dev, dtype=torch.uint8).contiguous()
    total = i64[1].numel()
    if any(t.numel() != total for t in (i64[2], i64[3], f32[0], f32[1])) or any(t.numel() != nq for t in (f32[2], f32[3], complete)):
        raise ValueError("hybrid_rank: the candidate arrays must share one length, and D, S, complete hold one entry per query")
    if nq < 0 or (nq > 0 and int(i64[0][-1]) != total):      # the kernel trusts cand_indptr for the extent of the candidate arrays
        raise ValueError(f"hybrid_rank: cand_indptr must hold nq + 1 >= 1 offsets ending at the {total} candidates")
    k = int(k)
    out_s = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=dev)
    out_i = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
    counts = torch.empty((nq,), dtype=torch.int32, device=dev)
    cert = torch.empty((nq,), dtype=torch.int32, device=dev)
    thr = torch.empty((nq,), dtype=torch.float32, device=dev)
    keep = [_valid(t) for t in (*i64[1:], f32[0], f32[1], f32[2], f32[3], complete, out_s, out_i, counts, cert, thr)]
    p = [_ptr(t) for t in keep]
    _call(dev, "sr_hybrid_rank", _ptr(i64[0]), *p[:5], nq, float(weights[0]), float(weights[1]), k, *p[5:8], int(n_s2d), int(id_end), *p[8:])
    return out_s, out_i, counts, cert, thr


FUSE_METHODS = {"rrf": _lib.SR_FUSE_RRF, "minmax": _lib.SR_FUSE_MINMAX}
FUSE_MAX_LISTS = 8


def rank_fuse_arguments(n_lists, k, method, weights, c):
    """The host checks of rank_fuse (touch no device) -> (k, method constant, weights as floats, c).  ValueError otherwise."""
    if method not in FUSE_METHODS:
        raise ValueError(f"rank_fuse: method must be one of {sorted(FUSE_METHODS)}, got {method!r}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"rank_fuse: k must be an integer >= 1, got {k!r}")
    if not 1 <= n_lists <= FUSE_MAX_LISTS:
        raise ValueError(f"rank_fuse: 1 to {FUSE_MAX_LISTS} lists are fused, got {n_lists}")
    weights = [1.0] * n_lists if weights is None else weights
    try:
        with np.errstate(over="ignore"):                        # a value beyond float32 becomes inf and is refused below
            w = [float(np.float32(float(x))) for x in weights]
            c = float(np.float32(float(c)))
    except (TypeError, ValueError):
        raise ValueError(f"rank_fuse: weights and c must be numbers, got {weights!r} and {c!r}") from None
    if len(w) != n_lists:
        raise ValueError(f"rank_fuse: one weight per list ({n_lists}), got {len(w)}")
    if not all(np.isfinite(x) and x >= 0 for x in w):
        raise ValueError(f"rank_fuse: the weights must be finite (as float32) and >= 0, got {weights!r}")
    if method == "rrf" and not (np.isfinite(c) and c > -1):
        raise ValueError(f"rank_fuse: c must be finite and > -1, got {c!r}")
    return int(k), FUSE_METHODS[method], w, c


def rank_fuse(ids, k, counts=None, scores=None, method="rrf", weights=None, c=60.0, return_ranks=False):
    """Rank fusion of L ranked lists per query on the device (sr_rank_fuse, csrc/rank_fuse.hip): ids int64 [L, nq, depth] cuda (or a list
    / tuple of L tensors [nq, depth] of one shape; id < 0 = padding), counts int32 [L, nq] the valid prefix of each row (None: depth),
    scores fp32 like ids (read by method="minmax" only).  method "rrf": sum_l weights[l] / (c + rank_l); "minmax": sum_l weights[l] *
    (s - min_l) / (max_l - min_l) over each list's valid entries (1.0 where max_l == min_l); the sum runs in list order, one rounded fp32
    add each.  weights (None: all ones) finite and >= 0.  Returns (scores fp32 [nq, k] padded with -FLT_MAX, ids int64 [nq, k] padded with
    -1, counts int32 [nq]) by (fused descending, id ascending), and with return_ranks=True also ranks int32 [nq, k, L]: the 1-based rank
    of the hit in each list, 0 = absent.  L <= 8, depth and k <= sr_max_topk(), L * depth <= 2 * sr_max_topk().  Argument errors are
    ValueErrors before the library is asked for a device; an id >= 2^32 or twice in one row: ValueError naming list, query, entry, id."""
    def stacked(x, what):
        if isinstance(x, (list, tuple)):
            if not x or not all(torch.is_tensor(t) for t in x) or any(t.shape != x[0].shape for t in x):
                raise ValueError(f"rank_fuse: {what} must be tensors of one shape [nq, depth]")
            x = torch.stack(list(x))
        if not torch.is_tensor(x) or x.dim() != 3:
            raise ValueError(f"rank_fuse: expected {what} [n_lists, nq, depth], got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        return x
    ids = stacked(ids, "ids")
    L, nq, depth = ids.shape
    k, method_id, w, c = rank_fuse_arguments(L, k, method, weights, c)
    if scores is not None:
        scores = stacked(scores, "scores")
        if scores.shape != ids.shape:
            raise ValueError(f"rank_fuse: scores {tuple(scores.shape)} and ids {tuple(ids.shape)} must share one shape")
    elif method == "minmax":
        raise ValueError("rank_fuse: method 'minmax' needs the scores of the lists")
    if counts is not None:
        if isinstance(counts, (list, tuple)):
            counts = torch.stack([torch.as_tensor(t) for t in counts])
        if not torch.is_tensor(counts) or tuple(counts.shape) != (L, nq):
            raise ValueError(f"rank_fuse: expected counts [{L}, {nq}], got {tuple(counts.shape) if torch.is_tensor(counts) else type(counts).__name__}")
    if depth < 1:
        raise ValueError("rank_fuse: the lists hold no entry (depth = 0)")
    _lib.require_gpu()
    dev = _cuda_device(ids)
    ids = ids.to(device=dev, dtype=torch.int64).contiguous()
    scores = None if scores is None else _valid(scores.to(device=dev, dtype=torch.float32).contiguous())
    counts = None if counts is None else _valid(counts.to(device=dev, dtype=torch.int32).contiguous())
    out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_c = torch.empty((nq,), dtype=torch.int32, device=dev)
    ranks = torch.empty((nq, k, L), dtype=torch.int32, device=dev) if return_ranks else None
    keep = [_valid(t) for t in (ids, out_s, out_i, out_c)]
    keep_r = None if ranks is None else _valid(ranks)
    _call(dev, "sr_rank_fuse", _ptr(keep[0]), _ptr(counts), _ptr(scores), L, nq, depth, method_id, (ctypes.c_float * L)(*w), c, k,
          _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), _ptr(keep_r))
    return (out_s, out_i, out_c, ranks) if return_ranks else (out_s, out_i, out_c)


def collapse_keys_argument(keys):
    """The host check of a group-key table (collapse.py): a 1-D int32 tensor / array, as given.  Touches no device."""
    if not torch.is_tensor(keys) and not isinstance(keys, np.ndarray):
        raise ValueError(f"keys must be an int32 tensor / array that maps a document index to its group key, got {type(keys).__name__}")
    if keys.dtype not in (np.int32, torch.int32):
        raise ValueError(f"keys must be int32 (one group key >= 0 per document index), got {keys.dtype}")
    if len(keys.shape) != 1:
        raise ValueError(f"expected 1-D keys, got {tuple(keys.shape)}")
    return keys


def topk_collapse(scores, ids, keys, k, counts=None, exhaustive=False):
    """Every ranked row -> its first k first-occurrence-per-group entries (sr_topk_collapse, csrc/topk_collapse.hip): scores fp32 / ids
    int64 [nq, row_len] cuda tensors as a search returns them (row_len of any size), keys int32 [n_keys] the group key >= 0 of every id,
    counts int32 [nq] the valid prefix of each row (the sparse search's; None: a row ends at its first negative id), exhaustive: the
    rows are whole rankings.  Returns (scores fp32 [nq, k], ids int64 [nq, k], keys int32 [nq, k], counts int32 [nq], complete int32
    [nq]) on the device, padded with (-FLT_MAX, -1, -1); complete[q] = 1: the row is the top-k groups of the full ranking.  1 <= k <=
    sr_max_topk().  An id outside [0, n_keys) or a negative key inside a row: ValueError naming the (query, position)."""
    keys = collapse_keys_argument(keys)
    if scores.dim() != 2 or ids.shape != scores.shape:
        raise ValueError(f"expected scores and ids of one shape [nq, row_len], got {tuple(scores.shape)} and {tuple(ids.shape)}")
    _lib.require_gpu()
    dev = scores.device
    scores, ids = scores.to(torch.float32).contiguous(), ids.to(device=dev, dtype=torch.int64).contiguous()
    keys = _to_dev(keys, torch.int32, dev)
    nq, row_len = scores.shape
    if counts is not None:
        counts = _to_dev(counts, torch.int32, dev)
        if counts.dim() != 1 or counts.numel() != nq:
            raise ValueError(f"expected {nq} counts, got {tuple(counts.shape)}")
        counts = _valid(counts)
    k = int(k)
    out_s = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=dev)
    out_i = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
    out_k = torch.empty((nq, max(k, 0)), dtype=torch.int32, device=dev)
    out_c = torch.empty((nq,), dtype=torch.int32, device=dev)
    done = torch.empty((nq,), dtype=torch.int32, device=dev)
    keep = [_valid(t) for t in (scores, ids, keys, out_s, out_i, out_k, out_c, done)]
    p = [_ptr(t) for t in keep]
    _call(dev, "sr_topk_collapse", p[0], p[1], _ptr(counts), nq, row_len, 1 if exhaustive else 0, p[2], keys.numel(), k, *p[3:])
    return out_s, out_i, out_k, out_c, done


def member_table_argument(members):
    """The host check of a member table (collapse.member_table): (uniq_keys int32 [G], member_indptr int64 [G + 1], member_ids int64 [n])
    as tensors, as given.  Touches no device."""
    if not isinstance(members, (tuple, list)) or len(members) != 3 or not all(torch.is_tensor(t) for t in members):
        raise ValueError("members must be the (uniq_keys, member_indptr, member_ids) tensors collapse.member_table returns")
    uniq, indptr, ids = members
    if uniq.dtype != torch.int32 or indptr.dtype != torch.int64 or ids.dtype != torch.int64 or uniq.dim() != 1 or indptr.dim() != 1 or ids.dim() != 1:
        raise ValueError(f"members must be 1-D (int32, int64, int64) tensors, got {uniq.dtype} {tuple(uniq.shape)}, {indptr.dtype} "
                         f"{tuple(indptr.shape)}, {ids.dtype} {tuple(ids.shape)}")
    if indptr.numel() != uniq.numel() + 1:
        raise ValueError(f"member_indptr must hold one offset more than there are keys ({uniq.numel()} + 1), got {indptr.numel()}")
    return uniq, indptr, ids


def _members_call(name, slot_keys, members, filt, tail):
    """One of the sr_group_members pair: slot_keys int32 [nq, kg] and the member table on one device; filt None, (words int32 [W], n_bits)
    or (words int32 [G, W], n_bits, group ids int32 [nq] or None); tail: the entry's own last arguments."""
    uniq, indptr, ids = members
    dev = slot_keys.device
    nq, kg = slot_keys.shape
    n_masks, n_bits, words, groups = 0, 0, None, None
    if filt is not None:
        words, n_bits = filt[0], int(filt[1])
        groups = filt[2] if len(filt) > 2 else None
        n_masks = 1 if words.dim() == 1 else int(words.shape[0])
        if words.shape[-1] != (n_bits + 31) // 32:
            raise ValueError(f"{n_bits} bits take {(n_bits + 31) // 32} words per mask, got {words.shape[-1]}")
        if groups is not None and (groups.dim() != 1 or groups.numel() != nq):
            raise ValueError(f"query_group must hold one group id per query ({nq}), got {tuple(groups.shape)}")
        if groups is None and n_masks != 1:
            raise ValueError(f"{n_masks} masks need a query_group")
    keep = [_valid(t) for t in (slot_keys, uniq, indptr, ids)] + [None if t is None else _valid(t) for t in (words, groups)]
    p = [_ptr(t) for t in keep]
    _call(dev, name, p[0], nq, kg, p[1], uniq.numel(), p[2], p[3], ids.numel(), p[4], n_masks, n_bits, p[5], *tail)


def _members_arguments(slot_keys, members, filt):
    """The checks of group_members_count / _fill that need no device, then everything on slot_keys' device."""
    uniq, indptr, ids = member_table_argument(members)
    if not torch.is_tensor(slot_keys) or slot_keys.dtype != torch.int32 or slot_keys.dim() != 2:
        raise ValueError("slot_keys must be an int32 [nq, kg] tensor (the keys a collapsed search returns)")
    _lib.require_gpu()
    if not slot_keys.is_cuda:
        raise ValueError("slot_keys must be a cuda tensor")
    dev = slot_keys.device
    members = tuple(t.to(dev).contiguous() for t in (uniq, indptr, ids))
    if filt is not None:
        words = filt[0].to(dev).contiguous()
        words = words if words.dtype == torch.int32 else words.view(torch.int32)
        groups = filt[2] if len(filt) > 2 else None
        if groups is not None:
            groups = group_ids_int32(groups, dev)
        filt = (words, int(filt[1]), groups)
    return slot_keys.contiguous(), members, filt


def group_members_count(slot_keys, members, filt=None):
    """The allowed members of every (query, slot) of a collapsed result, first half (sr_group_members_count, csrc/group_hits.hip):
    slot_keys int32 cuda [nq, kg] (negative: padding); members = collapse.member_table(...); filt None (no filter), (words int32 [W],
    n_bits) one bitmap for all queries, or (words int32 [G, W], n_bits, query_group [nq]) one per filter group.  Returns (indptr int64
    [nq * kg + 1] on the device, total): the exclusive scan in slot order of the slots' allowed members.  A key absent from the table,
    a group id outside [0, G), a member id outside the mask: ValueError naming the first."""
    slot_keys, members, filt = _members_arguments(slot_keys, members, filt)
    indptr = torch.empty((slot_keys.numel() + 1,), dtype=torch.int64, device=slot_keys.device)
    total = ctypes.c_int64(0)
    _members_call("sr_group_members_count", slot_keys, members, filt, (_ptr(indptr), ctypes.byref(total)))
    return indptr, total.value


def group_members_fill(slot_keys, members, indptr, total, filt=None):
    """Second half (sr_group_members_fill) for the inputs and the indptr of a preceding group_members_count: ids int64 [total], the allowed
    members of slot s at indptr[s] .. indptr[s + 1], ascending."""
    slot_keys, members, filt = _members_arguments(slot_keys, members, filt)
    indptr = _to_dev(indptr, torch.int64, slot_keys.device)
    if indptr.dim() != 1 or indptr.numel() != slot_keys.numel() + 1:
        raise ValueError(f"expected an indptr of {slot_keys.numel() + 1} entries, got {tuple(indptr.shape)}")
    total = int(total)
    out = torch.empty((max(1, total),), dtype=torch.int64, device=slot_keys.device)
    _members_call("sr_group_members_fill", slot_keys, members, filt, (_ptr(indptr), _ptr(out), total))
    return out[:total]


def group_members(slot_keys, members, filt=None):
    """group_members_count, then group_members_fill: (indptr int64 [nq * kg + 1], ids int64 [total])."""
    indptr, total = group_members_count(slot_keys, members, filt)
    return indptr, group_members_fill(slot_keys, members, indptr, total, filt)


MAX_HITS = 64               # sr_segment_topm keeps the running best one per lane of a wave


def hits_argument(who, m):
    """m of a top-m selection as an int in [1, MAX_HITS], or ValueError.  Touches no device."""
    try:
        mm = int(m)
        if mm != m or isinstance(m, bool):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{who}: the number of hits must be an integer in [1, {MAX_HITS}], got {m!r}") from None
    if not 1 <= mm <= MAX_HITS:
        raise ValueError(f"{who}: the number of hits must be an integer in [1, {MAX_HITS}], got {m!r}")
    return mm


def segment_topm(scores, ids, seg_indptr, m, threshold=None, pad_score=-3.402823466e38):
    """The m best entries of every segment of a scored CSR (sr_segment_topm, csrc/group_hits.hip): scores fp32 / ids int64 [total],
    segment s at seg_indptr[s] .. [s + 1] (int64 [n_segs + 1], from 0, never decreasing, ending at total), any length, ids in any order.
    Order: score descending (-0.0 = +0.0, read back as +0.0), then id ascending; threshold (None: off): only entries with score >
    threshold.  Returns (scores fp32 [n_segs, m], ids int64 [n_segs, m], counts int32 [n_segs]) on the device: the best min(m, count)
    entries, then (pad_score, -1); counts = the entries that took part, not cut to m.  1 <= m <= 64.  m, the shapes and - where
    seg_indptr is given on the host - its content are checked before anything touches a device; a seg_indptr on the device is checked
    there: ValueError either way."""
    m = hits_argument("segment_topm", m)
    if not torch.is_tensor(seg_indptr):
        seg_indptr = np.asarray(seg_indptr)
    host_indptr = None if torch.is_tensor(seg_indptr) and seg_indptr.is_cuda else np.asarray(seg_indptr)      # None: checked on the device
    if len(seg_indptr.shape) != 1 or seg_indptr.shape[0] < 1:
        raise ValueError("segment_topm: seg_indptr must be 1-D with n_segs + 1 >= 1 offsets")
    if len(scores.shape) != 1 or tuple(ids.shape) != tuple(scores.shape):
        raise ValueError(f"segment_topm: expected 1-D scores and ids of one length, got {tuple(scores.shape)} and {tuple(ids.shape)}")
    if host_indptr is not None:
        if host_indptr.dtype.kind not in "iu":
            raise ValueError(f"segment_topm: seg_indptr must hold integers, got {host_indptr.dtype}")
        if int(host_indptr[0]) != 0:
            raise ValueError(f"segment_topm: seg_indptr must start at 0, got {int(host_indptr[0])}")
        down = np.flatnonzero(np.diff(host_indptr.astype(np.int64)) < 0)
        if down.size:
            raise ValueError(f"segment_topm: seg_indptr decreases behind segment {int(down[0])}")
        if int(host_indptr[-1]) != scores.shape[0]:
            raise ValueError(f"segment_topm: seg_indptr ends at {int(host_indptr[-1])}, scores holds {scores.shape[0]} entries")
    _lib.require_gpu()
    dev = scores.device if torch.is_tensor(scores) and scores.is_cuda else _cuda_device()
    scores, ids = _to_dev(scores, torch.float32, dev), _to_dev(ids, torch.int64, dev)
    seg_indptr = _to_dev(seg_indptr, torch.int64, dev)
    n_segs = seg_indptr.numel() - 1
    if host_indptr is None and int(seg_indptr[-1]) != scores.numel():       # the kernel trusts seg_indptr[n_segs] for the arrays' extent
        raise ValueError(f"segment_topm: seg_indptr ends at {int(seg_indptr[-1])}, scores holds {scores.numel()} entries")
    out_s = torch.empty((n_segs, m), dtype=torch.float32, device=dev)
    out_i = torch.empty((n_segs, m), dtype=torch.int64, device=dev)
    out_c = torch.empty((n_segs,), dtype=torch.int32, device=dev)
    keep = [_valid(t) for t in (scores, ids, seg_indptr, out_s, out_i, out_c)]
    p = [_ptr(t) for t in keep]
    _call(dev, "sr_segment_topm", p[0], p[1], p[2], n_segs, m, 0 if threshold is None else 1, 0.0 if threshold is None else float(threshold),
          float(pad_score), p[3], p[4], p[5])
    return out_s, out_i, out_c
