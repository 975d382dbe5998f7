// Dense range search (gfx950): every document with score > thr[q], per query, as CSR (lims, scores, ids).
//
// Corresponds to faiss's IndexFlatIP.range_search(x, thresh) -> (lims, D, I), and on the dense head to what the reference's sparse
// scorer does with its threshold (numba_score_float, scaling_retriever/indexer.py:315-344: every document with score > threshold).
//
// Scores: the exact kernel's product (dense_score.hip) - v_mfma_f32_32x32x2_f32, documents as A rows, queries as B columns, per 8
// columns k = 8s + j then 8s + 4 + j - so every score is bit for bit the score of sr_dense_score_pairs, for every nq.  The loop is
// dense_score_pipe_kernel's (three LDS stages, one barrier per k-step); what differs is around it:
//
//   * a workgroup owns one query tile and one CHUNK of a segment - a run of consecutive 256-document tiles - and walks the chunk's
//     tiles in ascending row order, so everything it emits for a query is already in row order;
//   * pass 1 (count): per tile each lane counts the hits of its query and adds them to the query's LDS word (4 lanes share a query);
//     at the end of the chunk ONE word per (chunk, query) goes out with a plain store;
//   * a scan turns the (chunk, query) table into exclusive prefixes over the chunks (chunks are numbered in segment order, then row
//     order) and the per-query totals into lims;
//   * pass 2 (fill) runs the product again and starts each query at lims[q] + prefix[chunk][q].  Per tile every lane packs its hits
//     into one 32-bit word per 32-row block, the words go to an LDS bitmap [query][8 blocks], and after one barrier a hit's slot is
//     position + popcount(lower bits of its query's bitmap); after a second barrier the position (LDS, one per query of the tile)
//     advances by the tile's popcount.
//
// No global atomics anywhere: the result does not depend on the order workgroups run in, two calls give the same bytes.
//
// Under a document bitmap (sr_dense_range_count_masked / _fill_masked; MASKED in dense_range_kernel.h, instantiated by
// dense_range_masked.hip) a hit also needs the bit of its global index.  At the top of a tile every wave ballots the tile's 256 row
// bits in four steps (lane l tests rows l, 64 + l, 128 + l, 192 + l; rows past the chunk read as clear): four wave-uniform 64-bit
// words in scalar registers, the same in every wave, so nothing is added to the vector registers that live across the k-loop and no
// LDS or barrier is needed.  A tile whose 256 bits are all clear runs no k-loop - no loads, no MFMAs, no barriers; the decision is
// workgroup-uniform.  In the epilogue a block's 32 bits are ANDed into the hit word.
//
// Under a bitmap per query (sr_dense_range_count_grouped / _fill_grouped; GROUPED, instantiated by dense_range_grouped.hip) the ballot
// reads the UNION of the bitmaps of the groups that have a query - built once per count by launch_doc_masks_union and kept on the handle
// for the fill - and in the epilogue every lane tests its own query column's bitmap, found through the per-query word offsets the count
// put on the handle (launch_doc_mask_query_offsets, as the grouped search does).  Nothing of that is live across the k-loop.
#include "dense_range_kernel.h"
#include "dense_index.h"
#include "doc_mask.h"
#include "filter_args.h"
#include <algorithm>

// table[c][q]: counts -> exclusive prefixes over the chunks; lims[q + 1] := hits of query q (summed up by dense_range_lims_kernel)
__global__ __launch_bounds__(256) void dense_range_scan_kernel(uint32_t* table, int n_chunks, int64_t nq, int64_t* lims) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    uint32_t run = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const uint32_t v = table[(int64_t)c * nq + q];
        table[(int64_t)c * nq + q] = run;
        run += v;
    }
    lims[q + 1] = (int64_t)run;
    if (q == 0) lims[0] = 0;
}

// lims[1 .. nq] := inclusive sums, one workgroup: thread t owns a run of ceil(nq / 1024) queries
__global__ __launch_bounds__(1024) void dense_range_lims_kernel(int64_t* lims, int64_t nq) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (nq + 1023) / 1024;
    const int64_t b = 1 + t * per, e = b + per < nq + 1 ? b + per : nq + 1;
    int64_t sum = 0;
    for (int64_t i = b; i < e; ++i) sum += lims[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - sum;
    for (int64_t i = b; i < e; ++i) {
        run += lims[i];
        lims[i] = run;
    }
}

template <bool FILL>
static int launch_dense_range(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) {
    if (a.nq < 1 || n_chunks_seg < 1 || a.seg_rows < 1 || a.chunk_rows < 256 || a.chunk_rows % 256 != 0 ||
        ceil_div64(a.seg_rows, a.chunk_rows) != n_chunks_seg) {
        sr_set_error("dense range launch: bad chunking (%lld rows, chunks of %lld, %d chunks)", (long long)a.seg_rows, (long long)a.chunk_rows, n_chunks_seg);
        return SR_ERR_INVALID;
    }
    if (a.mask_qoff) return FILL ? launch_dense_range_fill_grouped(a, n_chunks_seg, s) : launch_dense_range_count_grouped(a, n_chunks_seg, s);    // dense_range_grouped.hip
    if (a.mask) return FILL ? launch_dense_range_fill_masked(a, n_chunks_seg, s) : launch_dense_range_count_masked(a, n_chunks_seg, s);      // dense_range_masked.hip
    return launch_dense_range_m<FILL, RangeFilter::all>(a, n_chunks_seg, s);
}
int launch_dense_range_count(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) { return launch_dense_range<false>(a, n_chunks_seg, s); }
int launch_dense_range_fill(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) { return launch_dense_range<true>(a, n_chunks_seg, s); }

int launch_range_scan(uint32_t* table, int n_chunks, int64_t nq, int64_t* d_lims, hipStream_t s) {
    hipLaunchKernelGGL(dense_range_scan_kernel, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, s, table, n_chunks, nq, d_lims);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(dense_range_lims_kernel, dim3(1), dim3(1024), 0, s, d_lims, nq);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// ---- host side: count + scan, then fill ---------------------------------------------------------------------------------------
// Chunk rows of a range search: a multiple of 256 such that the chunks of all segments number at most max_chunks.  *n_chunks = 0: no
// chunk size gives that few (more segments than max_chunks).
static int64_t dense_range_chunking(const sr_dense_index* idx, int64_t max_chunks, int64_t want_chunks, int* n_chunks) {
    int64_t tiles = 0;
    for (const DenseSegment& seg : idx->segs) tiles += ceil_div64(seg.n, 256);
    if (want_chunks > max_chunks) want_chunks = max_chunks;
    if (want_chunks < 1) want_chunks = 1;
    int64_t chunk_tiles = ceil_div64(tiles, want_chunks);
    *n_chunks = 0;
    if ((int64_t)idx->segs.size() > max_chunks) return 0;
    for (;; ++chunk_tiles) {          // the segments' last chunks are partial: at most segs.size() chunks over the target, a few steps
        int64_t n = 0;
        for (const DenseSegment& seg : idx->segs) n += ceil_div64(seg.n, chunk_tiles * 256);
        if (n <= max_chunks) { *n_chunks = (int)n; return chunk_tiles * 256; }
    }
}

// What a range search runs under: kind SR_RANGE_KIND_*; mask = the bitmap (masked) or the groups' stacked bitmaps (grouped); the last
// three for the grouped kind only.
struct DenseRangeFilter {
    int kind = SR_RANGE_KIND_ALL;
    const uint32_t* mask = nullptr;
    const uint32_t* qoff = nullptr;
    const uint32_t* mask_union = nullptr;
    int64_t words = 0;
};

static void dense_range_args(const sr_dense_index* idx, const DenseSegment& seg, const float* d_queries, int64_t nq, const float* d_thr,
                             const DenseRangeFilter& f, int chunk_base, DenseRangeArgs& a) {
    a = DenseRangeArgs{};
    a.D = seg.rows; a.Q = d_queries; a.thr = d_thr; a.seg_rows = seg.n; a.chunk_rows = idx->range_chunk_rows; a.chunk_base = chunk_base;
    a.H = idx->dim; a.nq = (int)nq; a.dtype = idx->row_dtype; a.id_base = seg.id_base; a.id_stride = seg.id_stride;
    a.table = idx->range_tab.p; a.mask = f.mask; a.mask_qoff = f.qoff; a.mask_union = f.mask_union; a.mask_words = f.words;
}

// the argument checks of every count, before any device work
static int dense_range_count_checks(const sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                    const int64_t* d_lims, const int64_t* total) {
    SR_REQUIRE(idx, "sr_dense_range_count: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_dense_range_count: bad nq=%lld", (long long)nq);
    SR_REQUIRE(d_lims && total, "sr_dense_range_count: null d_lims or total");
    SR_REQUIRE(nq == 0 || (d_queries && d_thresholds), "sr_dense_range_count: null queries or thresholds");
    SR_REQUIRE(((uintptr_t)d_queries & 15) == 0, "sr_dense_range_count: queries must be 16-byte aligned");
    return SR_OK;
}

// f.kind SR_RANGE_KIND_ALL: the unrestricted search.  The caller holds idx->mu and has run dense_range_count_checks.
static int dense_range_count_run(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                 const DenseRangeFilter& f, int64_t* d_lims, int64_t* total, sr_stream stream) {
    hipStream_t s = (hipStream_t)stream;
    idx->range_nq = -1;
    idx->range_kind = f.kind;
    *total = 0;
    if (nq == 0 || idx->ntotal == 0) {
        SR_TRY(sr_zero_lims(d_lims, nq, total, s));
        idx->range_nq = nq; idx->range_total = 0; idx->range_chunk_rows = 0;
        idx->range_segs = idx->segs.size(); idx->range_ntotal = idx->ntotal;
        return SR_OK;
    }
    if (idx->ntotal >= (1ll << 32)) {
        sr_set_error("sr_dense_range_count: %lld documents; the per-chunk counts are 32-bit", (long long)idx->ntotal);
        return SR_ERR_UNSUPPORTED;
    }
    // chunks x query tiles ~ the 2 048 workgroups of a launch of the exact search (dense_search.hip), rounded DOWN: one workgroup per CU and
    // every workgroup equally long, so 2 048 are 8 full rounds on 256 CUs and a few more would be a ninth, nearly empty one.  The table
    // (4 bytes per chunk and query) stays within the limit
    const int64_t qtiles = ceil_div64(nq, dense_range_query_tile(nq));
    int64_t max_chunks = idx->ws_limit / (4 * nq);
    if (max_chunks > SR_RANGE_MAX_CHUNKS) max_chunks = SR_RANGE_MAX_CHUNKS;
    int n_chunks = 0;
    int64_t chunk_rows = dense_range_chunking(idx, max_chunks, 2048 / qtiles, &n_chunks);
    if (const char* e = sr_dev_getenv("SR_RANGE_CHUNK_ROWS")) {       // dev switch, read per call: forces the chunk size
        const int64_t forced = atoll(e);
        SR_REQUIRE(forced >= 256 && forced % 256 == 0, "SR_RANGE_CHUNK_ROWS=%s must be a positive multiple of 256", e);
        chunk_rows = forced;
        int64_t n = 0;
        for (const DenseSegment& seg : idx->segs) n += ceil_div64(seg.n, forced);
        n_chunks = n <= max_chunks ? (int)n : 0;
    }
    if (n_chunks == 0) {
        sr_set_error("sr_dense_range_count: the chunk table needs at least %lld bytes of workspace for %lld queries and %zu segments "
                     "(limit %lld bytes, at most %d chunks)", (long long)(4 * nq * (int64_t)idx->segs.size()), (long long)nq, idx->segs.size(),
                     (long long)idx->ws_limit, SR_RANGE_MAX_CHUNKS);
        return SR_ERR_NOMEM;
    }
    const int64_t entries = (int64_t)n_chunks * nq;
    if (idx->range_tab.reserve(entries, nullptr) != SR_OK) {
        sr_set_error("sr_dense_range_count: out of device memory for the chunk table of %lld bytes", (long long)(entries * 4));
        return SR_ERR_NOMEM;
    }
    StreamOrder::Scope in_order(idx->order, s);
    idx->range_chunk_rows = chunk_rows;
    int chunk_base = 0;
    for (const DenseSegment& seg : idx->segs) {
        const int n_seg = (int)ceil_div64(seg.n, chunk_rows);
        DenseRangeArgs a;
        dense_range_args(idx, seg, d_queries, nq, d_thresholds, f, chunk_base, a);
        idx->prof.begin(s);
        SR_TRY(launch_dense_range_count(a, n_seg, s));
        idx->prof.end(s, 2.0 * (double)nq * (double)seg.n * idx->dim, (double)seg.n * idx->dim * (double)sr_dtype_size(idx->row_dtype));
        chunk_base += n_seg;
    }
    SR_TRY(launch_range_scan(idx->range_tab.p, n_chunks, nq, d_lims, s));
    int64_t h_total = 0;
    SR_CHECK_HIP(hipMemcpyAsync(&h_total, d_lims + nq, 8, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    *total = h_total;
    idx->range_nq = nq; idx->range_total = h_total;
    idx->range_segs = idx->segs.size(); idx->range_ntotal = idx->ntotal;
    return SR_OK;
}

static DenseRangeFilter dense_range_one_mask(const uint32_t* d_mask) {
    DenseRangeFilter f;
    f.kind = d_mask ? SR_RANGE_KIND_MASKED : SR_RANGE_KIND_ALL;
    f.mask = d_mask;
    return f;
}

extern "C" int sr_dense_range_count(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds, int64_t* d_lims,
                                    int64_t* total, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_count: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_TRY(dense_range_count_checks(idx, d_queries, nq, d_thresholds, d_lims, total));
    return dense_range_count_run(idx, d_queries, nq, d_thresholds, dense_range_one_mask(nullptr), d_lims, total, stream);
}

extern "C" int sr_dense_range_count_masked(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                           const uint32_t* d_mask_words, int64_t n_bits, int64_t* d_lims, int64_t* total, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_count_masked: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_REQUIRE(n_bits == dense_id_end(idx), "sr_dense_range_count_masked: n_bits=%lld, the index numbers its documents in [0, %lld)",
               (long long)n_bits, (long long)dense_id_end(idx));
    SR_REQUIRE(d_mask_words, "sr_dense_range_count_masked: null mask");
    SR_TRY(dense_range_count_checks(idx, d_queries, nq, d_thresholds, d_lims, total));
    return dense_range_count_run(idx, d_queries, nq, d_thresholds, dense_range_one_mask(d_mask_words), d_lims, total, stream);
}

// the two grouped halves' wording for sr_group_mask_checks
static const char* const DENSE_RANGE_BITS = "%s: n_bits=%lld, the index numbers its documents in [0, %lld)";

// Range count under a bitmap per query.  Before any scoring: the group ids are read back and checked (one wait for 4 nq bytes), the
// queries' word offsets and the union of the used groups' bitmaps go onto the handle (a second wait: the list of used groups is host
// memory).  Then the count of the other kinds with the grouped kernels.
extern "C" int sr_dense_range_count_grouped(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                            const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits, const int32_t* d_query_group,
                                            int64_t* d_lims, int64_t* total, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_count_grouped: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    const char* const who = "sr_dense_range_count_grouped";
    SR_TRY(sr_group_mask_checks(who, n_groups, n_bits, dense_id_end(idx), DENSE_RANGE_BITS));
    SR_TRY(sr_require_group_pointers(who, nq, d_group_words, d_query_group, n_bits));
    const int64_t n_words = doc_mask_words(n_bits);
    SR_TRY(dense_range_count_checks(idx, d_queries, nq, d_thresholds, d_lims, total));
    hipStream_t s = (hipStream_t)stream;
    idx->range_nq = -1;                               // whatever happens below, no earlier count can be filled from
    DenseRangeFilter f;
    f.kind = SR_RANGE_KIND_GROUPED;
    f.mask = d_group_words; f.words = n_words;
    std::vector<int32_t> grp, used;
    if (nq > 0) {
        StreamOrder::Scope in_order(idx->order, s);
        int64_t bad = -1;
        SR_TRY(sr_read_query_groups(d_query_group, nq, n_groups, s, &grp, &bad));
        if (bad >= 0) {
            SR_TRY(sr_zero_lims(d_lims, nq, total, s));
            return sr_bad_group_error(who, bad, grp[(size_t)bad], n_groups, " (nothing was scored)");
        }
        if (idx->ntotal > 0) {
            used = grp;
            std::sort(used.begin(), used.end());
            used.erase(std::unique(used.begin(), used.end()), used.end());
            const int64_t nq_pad = sr_query_offsets_len(nq);
            const int64_t scratch = 4 * (nq_pad + n_words + (int64_t)used.size());
            if (scratch > idx->ws_limit) {
                sr_set_error("sr_dense_range_count_grouped: the queries' word offsets and the union bitmap need %lld bytes of workspace (limit %lld bytes)",
                             (long long)scratch, (long long)idx->ws_limit);
                return SR_ERR_NOMEM;
            }
            SR_TRY(idx->range_qoff.reserve(nq_pad, "sr_dense_range_count_grouped"));
            SR_TRY(idx->range_union.reserve(n_words > 0 ? n_words : 1, "sr_dense_range_count_grouped"));
            SR_TRY(idx->range_used.reserve((int64_t)used.size(), "sr_dense_range_count_grouped"));
            SR_CHECK_HIP(hipMemcpyAsync(idx->range_used.p, used.data(), used.size() * 4, hipMemcpyHostToDevice, s));
            SR_TRY(launch_doc_masks_union(d_group_words, idx->range_used.p, (int64_t)used.size(), n_bits, idx->range_union.p, s));
            SR_TRY(sr_query_offsets(d_query_group, nq, n_bits, idx->range_qoff.p, s));
            SR_CHECK_HIP(hipStreamSynchronize(s));            // `used` (pageable host memory) was the source of an asynchronous copy
            f.qoff = idx->range_qoff.p; f.mask_union = idx->range_union.p;
        }
    }
    SR_TRY(dense_range_count_run(idx, d_queries, nq, d_thresholds, f, d_lims, total, stream));
    idx->range_groups = n_groups;
    return SR_OK;
}

// f: what the preceding count was given.  The caller holds idx->mu.
static int dense_range_fill(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds, const DenseRangeFilter& f,
                            const int64_t* d_lims, float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_fill: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30) && capacity >= 0, "sr_dense_range_fill: bad nq=%lld or capacity=%lld", (long long)nq, (long long)capacity);
    hipStream_t s = (hipStream_t)stream;
    SR_REQUIRE(idx->range_nq >= 0, "sr_dense_range_fill: no sr_dense_range_count precedes it on this handle");
    SR_REQUIRE(idx->range_kind == f.kind, "sr_dense_range_fill: the preceding count ran %s, this fill runs %s", sr_range_kind_text(idx->range_kind),
               sr_range_kind_text(f.kind));
    SR_REQUIRE(idx->range_nq == nq, "sr_dense_range_fill: nq=%lld, the preceding count had %lld", (long long)nq, (long long)idx->range_nq);
    SR_REQUIRE(idx->range_segs == idx->segs.size() && idx->range_ntotal == idx->ntotal, "sr_dense_range_fill: the index changed since the count");
    SR_REQUIRE(capacity >= idx->range_total, "sr_dense_range_fill: capacity=%lld is below the count's total of %lld", (long long)capacity,
               (long long)idx->range_total);
    if (idx->range_total == 0) return SR_OK;          // nothing to write (also nq = 0, empty index)
    SR_REQUIRE(d_queries && d_thresholds && d_lims && d_out_scores && d_out_ids, "sr_dense_range_fill: null pointer");
    SR_REQUIRE(((uintptr_t)d_queries & 15) == 0, "sr_dense_range_fill: queries must be 16-byte aligned");
    StreamOrder::Scope in_order(idx->order, s);
    int chunk_base = 0;
    for (const DenseSegment& seg : idx->segs) {
        const int n_seg = (int)ceil_div64(seg.n, idx->range_chunk_rows);
        DenseRangeArgs a;
        dense_range_args(idx, seg, d_queries, nq, d_thresholds, f, chunk_base, a);
        a.lims = d_lims; a.out_scores = d_out_scores; a.out_ids = d_out_ids; a.capacity = capacity;
        idx->prof.begin(s);
        SR_TRY(launch_dense_range_fill(a, n_seg, s));
        idx->prof.end(s, 2.0 * (double)nq * (double)seg.n * idx->dim, (double)seg.n * idx->dim * (double)sr_dtype_size(idx->row_dtype));
        chunk_base += n_seg;
    }
    return SR_OK;
}

extern "C" int sr_dense_range_fill(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds, const int64_t* d_lims,
                                   float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_fill: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    return dense_range_fill(idx, d_queries, nq, d_thresholds, dense_range_one_mask(nullptr), d_lims, d_out_scores, d_out_ids, capacity, stream);
}

extern "C" int sr_dense_range_fill_masked(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                          const uint32_t* d_mask_words, int64_t n_bits, const int64_t* d_lims, float* d_out_scores,
                                          int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_fill_masked: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_REQUIRE(n_bits == dense_id_end(idx), "sr_dense_range_fill_masked: n_bits=%lld, the index numbers its documents in [0, %lld)",
               (long long)n_bits, (long long)dense_id_end(idx));
    SR_REQUIRE(d_mask_words, "sr_dense_range_fill_masked: null mask");
    return dense_range_fill(idx, d_queries, nq, d_thresholds, dense_range_one_mask(d_mask_words), d_lims, d_out_scores, d_out_ids, capacity, stream);
}

// The grouped fill reads the word offsets and the union its count left on the handle: the group ids were checked there, and
// d_query_group is not read again (it must be the count's, as the bitmaps must).
extern "C" int sr_dense_range_fill_grouped(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                           const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits, const int32_t* d_query_group,
                                           const int64_t* d_lims, float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_fill_grouped: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_TRY(sr_group_mask_checks("sr_dense_range_fill_grouped", n_groups, n_bits, dense_id_end(idx), DENSE_RANGE_BITS));
    SR_TRY(sr_require_group_pointers("sr_dense_range_fill_grouped", nq, d_group_words, d_query_group, n_bits));
    const int64_t n_words = doc_mask_words(n_bits);
    DenseRangeFilter f;
    f.kind = SR_RANGE_KIND_GROUPED;
    f.mask = d_group_words; f.words = n_words; f.qoff = idx->range_qoff.p; f.mask_union = idx->range_union.p;
    SR_REQUIRE(idx->range_nq < 0 || idx->range_kind != SR_RANGE_KIND_GROUPED || idx->range_groups == n_groups,
               "sr_dense_range_fill_grouped: n_groups=%lld, the preceding count had %lld", (long long)n_groups, (long long)idx->range_groups);
    return dense_range_fill(idx, d_queries, nq, d_thresholds, f, d_lims, d_out_scores, d_out_ids, capacity, stream);
}
