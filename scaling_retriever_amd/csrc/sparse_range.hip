// Sparse range search (gfx950): every document with score > thr[q], per query, as CSR (lims, scores, ids) in document order.
//
// This is the reference's scorer before select_topk cuts its list (numba_score_float, scaling_retriever/indexer.py:324-344: a zeroed
// N-sized fp32 array per query, q_t * v scatter-added over each query term's posting list in term order, then every document with
// score > threshold, in document order).  The score array is tiled as in sparse_score.hip - a (query, 8 192-document tile) slice
// lives in LDS, each query term contributes the run of its posting list inside the tile, found through the index's skip table - but
// nothing is selected: the tile's hits leave the workgroup in document order.
//
//   * a workgroup of 256 threads owns one query and one CHUNK of consecutive doc tiles and walks them in ascending order, so
//     everything it emits for the query is already in document order;
//   * pass 1 (count): per tile every wave counts the hits of its quarter with ballots; at the end of the chunk ONE int32 per
//     (chunk, query) goes out with a plain store;
//   * a scan turns the (chunk, query) table into exclusive prefixes over the chunks and the per-query totals into lims;
//   * pass 2 (fill) reads its cell first and returns on 0 before it touches a posting; otherwise it accumulates again and a hit goes
//     to lims[q] + prefix[chunk][q] + hits of the chunk's earlier tiles + hits of the tile's lower waves + its rank in the wave.
//
// No global atomics anywhere: the result does not depend on the order workgroups run in, two calls give the same bytes.
//
// Under a document bitmap (sr_sparse_range_count_masked / _fill_masked, MASKED below) a hit also needs the bit of its position.  Per
// tile every wave loads the tile's 256 mask words, four per lane (reads beyond the bitmap's last word are clamped to 0, the last word's
// bits at or beyond n_docs cleared): all clear - the same answer in every wave, no barrier - and the tile is skipped before a posting is
// touched.  Otherwise lane l keeps word l of its wave's quarter, and the two words of a 64-document step come back with v_readlane and
// are ANDed into the step's hit ballot (sparse_range_step_hits: the one predicate of the count and of the fill).
#include "sparse_index.h"
#include "range_scan.h"
#include "filter_args.h"

#define SRR_TILE SR_SPARSE_TILE_DOCS
#define SRR_SUBS (SR_SPARSE_TILE_DOCS / SR_SPARSE_SKIP_DOCS)      // skip-table entries per tile
#define SRR_TERMS 64      // query terms fetched per batch: lane j of every wave holds term j
#define SRR_U 4           // postings per thread and group
#define SRR_GROUP (SRR_U * 256)
#define SRR_QUARTER (SRR_TILE / 4)
#define SRR_MAX_GRID_Y 65535
#define SRR_MAX_NQ (1ll << 24)   // the query is the grid's x index: 256 threads x 2^24 workgroups is the most one launch takes
#ifndef SRR_AHEAD
#define SRR_AHEAD 1        // groups of posting loads in flight while one is applied (0 or 1)
#endif

struct SparseRangeArgs {
    const int64_t* indptr;
    const int32_t* doc_ids;
    const float* vals;
    const int32_t* skip;      // sr_sparse_index::skip
    int n_tiles;
    int64_t n_docs, n_terms;
    const int64_t* q_indptr;
    const int32_t* q_cols;
    const float* q_vals;
    const float* thr;         // [nq]
    int64_t nq;
    int chunk_tiles;          // doc tiles per chunk
    int chunk_begin;          // first chunk of this launch
    int32_t* table;           // [n_chunks, nq]: count writes the hits of (chunk, query); the scan turns them into exclusive prefixes over the chunks
    // fill only
    const int64_t* lims;      // [nq + 1]
    int64_t id_base, id_stride;
    float* out_scores;
    int64_t* out_ids;
    int64_t capacity;
    // masked kernels only
    const uint32_t* mask;     // bitmap over document positions: ceil(n_docs / 32) words, nothing beyond them is read
    // grouped kernels only: `mask` holds the groups' bitmaps stacked, ceil(n_docs / 32) words each
    const int32_t* qgroup;    // [nq] the group of every query, each in [0, n_groups): checked by the count before any launch
};

__device__ inline int64_t srr_readlane64(int64_t v, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v & 0xffffffffll), j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), j);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The score slice of (query q, doc tile `tile`) in sc[0 .. SRR_TILE): zero fill, then the query's terms in the query's order.  The run
// of every term inside the tile comes from the skip table for a batch of 64 terms at once, lane j = term j (every wave holds the same
// 64 entries, read back with v_readlane), as in sparse_score_kernel; a run is cut into groups of SRR_GROUP postings, thread t takes
// postings t, t + 256, t + 512, t + 768 of a group (coalesced), and the next group's loads - of the same term or the next one with
// postings here - are issued before the current group is applied.  Loads are clamped to the run and always issued, lanes beyond the
// run's end update a dummy slot past the tile: no exec-mask branches.  Postings of one term never share a document, terms do: the
// barrier comes after a term's last group only.  The multiply and the add are separate fp32 operations.  Ends on a barrier.
__device__ __forceinline__ void sparse_range_accumulate(const SparseRangeArgs& a, float* sc, int64_t q, int tile, int tid) {
#pragma clang fp contract(off)
    const int lane = tid & 63;
    const int64_t doc0 = (int64_t)tile * SRR_TILE;
    for (int d = tid; d < SRR_TILE; d += 256) sc[d] = 0.f;
    __syncthreads();

    const int64_t tb = a.q_indptr[q], te = a.q_indptr[q + 1];
    const int skip_stride = a.n_tiles * SRR_SUBS + 1;
    for (int64_t t0 = tb; t0 < te; t0 += SRR_TERMS) {
        const int nt = (int)((te - t0) < SRR_TERMS ? (te - t0) : SRR_TERMS);
        int64_t seg_b = 0;
        int seg_n = 0;
        float seg_w = 0.f;
        if (lane < nt) {
            // a term the index does not know has an empty posting list (indexer.py:364-370)
            const int term = a.q_cols[t0 + lane];
            const bool known = term >= 0 && (int64_t)term < a.n_terms;
            const int32_t* sk = a.skip + (int64_t)(known ? term : 0) * skip_stride + tile * SRR_SUBS;
            const int b = sk[0], e = sk[SRR_SUBS];
            seg_n = known ? e - b : 0;
            seg_b = a.indptr[known ? term : 0] + b;
            seg_w = a.q_vals[t0 + lane];
        }
        uint64_t todo = __ballot(seg_n > 0);          // terms with postings here, walked in ascending lane = query order
        if (todo == 0) continue;

        struct Cur { int j, g, ngr, n; int64_t b; float w; };      // wave-uniform cursor over (term j, group g of that term)
        auto first_of = [&](uint64_t& m, Cur& c) {
            c.j = __builtin_ctzll(m);
            m &= m - 1;
            c.g = 0;
            c.n = __builtin_amdgcn_readlane(seg_n, c.j);
            c.ngr = (c.n + SRR_GROUP - 1) / SRR_GROUP;
            c.b = srr_readlane64(seg_b, c.j);
            c.w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(seg_w), c.j));
        };
        auto advance = [&](uint64_t& m, Cur& c) -> bool {      // false: c was the last group of the batch
            if (c.g + 1 < c.ngr) { ++c.g; return true; }
            if (m == 0) return false;
            first_of(m, c);
            return true;
        };
        auto load_group = [&](const Cur& c, int (&dd)[SRR_U], float (&vv)[SRR_U]) {
            const int32_t* ib = a.doc_ids + c.b;       // wave-uniform
            const float* vb = a.vals + c.b;
            const uint32_t p0 = (uint32_t)c.g * SRR_GROUP + (uint32_t)tid;
            const uint32_t last = (uint32_t)c.n - 1u;  // c.n >= 1: only terms with postings here are walked
#pragma unroll
            for (int u = 0; u < SRR_U; ++u) {
                const uint32_t p = p0 + 256u * u;
                const uint32_t pc = p < last ? p : last;
                dd[u] = ib[pc];
                vv[u] = vb[pc];
            }
        };
        auto apply_group = [&](const int (&dd)[SRR_U], const float (&vv)[SRR_U], const Cur& c) {
            const uint32_t left = (uint32_t)(c.n - c.g * SRR_GROUP);      // postings of the run from this group's first one on
            int d[SRR_U];
            float cur[SRR_U];
#pragma unroll
            for (int u = 0; u < SRR_U; ++u) {
                d[u] = ((uint32_t)tid + 256u * u < left) ? dd[u] - (int)doc0 : SRR_TILE + lane;
                cur[u] = sc[d[u]];
            }
#pragma unroll
            for (int u = 0; u < SRR_U; ++u) {
                const float prod = c.w * vv[u];
                sc[d[u]] = cur[u] + prod;
            }
            if (c.g == c.ngr - 1)      // term-serial: the next term may touch the same docs.  Behind lgkmcnt(0) only: the next group's loads stay in flight
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        };
        Cur head;
        first_of(todo, head);
        int dA[SRR_U];
        float vA[SRR_U];
#if SRR_AHEAD == 0      // measurement build (tools/build_variant.sh noahead -DSRR_AHEAD=0): every group is loaded, waited for, applied
        for (;;) {
            load_group(head, dA, vA);
            apply_group(dA, vA, head);
            Cur nx = head;
            if (!advance(todo, nx)) break;
            head = nx;
        }
#else
        int dB[SRR_U];
        float vB[SRR_U];
        load_group(head, dA, vA);
        for (;;) {
            const Cur cur = head;
            Cur nx = head;
            const bool more = advance(todo, nx);
            if (more) head = nx;
            load_group(head, dB, vB);                   // the last group of the batch is read twice
            apply_group(dA, vA, cur);
            if (!more) break;
#pragma unroll
            for (int u = 0; u < SRR_U; ++u) { dA[u] = dB[u]; vA[u] = vB[u]; }
        }
#endif
    }
}

// The hits of step st of a wave's quarter (64 documents, lane l holds document d with score s) as a lane mask; *mine = this lane's bit.
// Under a mask, mw is word l of the quarter's 64 mask words: the step's documents are the bits of words 2 st and 2 st + 1.
template <bool MASKED>
__device__ __forceinline__ uint64_t sparse_range_step_hits(float s, int d, int n_here, float thr, uint32_t mw, int st, int lane, bool* mine) {
    bool hit = d < n_here && s > thr;                       // strict; false for a NaN on either side
    uint64_t m = __ballot(hit);
    if constexpr (MASKED) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)mw, 2 * st), hi = (uint32_t)__builtin_amdgcn_readlane((int)mw, 2 * st + 1);
        m &= ((uint64_t)hi << 32) | lo;
        hit = (m >> lane) & 1ull;
    }
    *mine = hit;
    return m;
}

// hits of this wave's quarter of the tile: lanes read consecutive LDS words, 64 documents per step
template <bool MASKED>
__device__ __forceinline__ int sparse_range_wave_hits(const float* sc, int wave, int lane, int n_here, float thr, uint32_t mw) {
    int cnt = 0;
#pragma unroll 4
    for (int st = 0; st < SRR_QUARTER / 64; ++st) {
        const int d = wave * SRR_QUARTER + st * 64 + lane;
        bool hit;
        cnt += __popcll(sparse_range_step_hits<MASKED>(sc[d], d, n_here, thr, mw, st, lane, &hit));
    }
    return cnt;
}

// word wi of the bitmap over n_docs documents: 0 beyond the last word, the last word's bits at or beyond n_docs cleared
__device__ __forceinline__ uint32_t sparse_range_mask_word(const uint32_t* __restrict__ words, int64_t wi, int64_t n_docs) {
    const int64_t n_words = (n_docs + 31) >> 5;
    if (wi >= n_words) return 0u;
    uint32_t v = words[wi];
    const unsigned tail = (unsigned)(n_docs & 31);
    if (wi == n_words - 1 && tail != 0) v &= (1u << tail) - 1u;
    return v;
}

template <bool FILL, bool MASKED, bool GROUPED = false>
__device__ __forceinline__ void sparse_range_body(const SparseRangeArgs& a) {
    __shared__ float sc[SRR_TILE + 64];         // + one dummy slot per lane for the postings beyond a run's end
    __shared__ int wave_tot[4];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int chunk = a.chunk_begin + (int)blockIdx.y;
    const int tile_first = chunk * a.chunk_tiles;
    const int tile_end = tile_first + a.chunk_tiles < a.n_tiles ? tile_first + a.chunk_tiles : a.n_tiles;
    const float thr = a.thr[q];
    // GROUPED (with MASKED): the query's own bitmap - one workgroup serves one query, so the choice is workgroup-uniform
    const uint32_t* mask = a.mask;
    if constexpr (GROUPED) mask += (int64_t)a.qgroup[q] * ((a.n_docs + 31) >> 5);

    int64_t pos = 0, p_end = 0;          // fill: the write position of the chunk's next hit, and the end of the query's segment
    if (FILL) {
        pos = a.lims[q] + (int64_t)(uint32_t)a.table[(int64_t)chunk * a.nq + q];
        p_end = a.lims[q + 1] < a.capacity ? a.lims[q + 1] : a.capacity;
    }
    int wave_cnt = 0;                    // count: this wave's hits over the chunk

    for (int tile = tile_first; tile < tile_end; ++tile) {
        const int64_t doc0 = (int64_t)tile * SRR_TILE;
        const int n_here = (int)((a.n_docs - doc0) < SRR_TILE ? (a.n_docs - doc0) : SRR_TILE);
        uint32_t mw = 0;                 // MASKED: word `lane` of this wave's quarter of the tile's mask words
        if constexpr (MASKED) {
            uint32_t any = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t v = sparse_range_mask_word(mask, (int64_t)tile * (SRR_TILE / 32) + j * 64 + lane, a.n_docs);
                any |= v;
                mw = j == wave ? v : mw;
            }
            if (__ballot(any != 0) == 0) continue;      // no allowed document in the tile (every wave read the same 256 words): it contributes 0
        }
        sparse_range_accumulate(a, sc, q, tile, tid);
        const int mine = sparse_range_wave_hits<MASKED>(sc, wave, lane, n_here, thr, mw);
        if (!FILL) {
            wave_cnt += mine;
        } else {
            if (lane == 0) wave_tot[wave] = mine;
            __syncthreads();
            int below = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int c = wave_tot[w];
                below += w < wave ? c : 0;
                total += c;
            }
            if (mine) {
                int64_t p0 = pos + below;
                for (int st = 0; st < SRR_QUARTER / 64; ++st) {
                    const int d = wave * SRR_QUARTER + st * 64 + lane;
                    const float s = sc[d];
                    bool hit;
                    const uint64_t m = sparse_range_step_hits<MASKED>(s, d, n_here, thr, mw, st, lane, &hit);
                    if (m == 0) continue;
                    const int64_t p = p0 + __popcll(m & ((1ull << lane) - 1ull));      // consecutive positions: the stores coalesce
                    if (hit && p >= 0 && p < p_end) {          // never outside the query's segment, whatever the count saw
                        a.out_scores[p] = s;
                        a.out_ids[p] = a.id_base + (doc0 + d) * a.id_stride;
                    }
                    p0 += __popcll(m);
                }
            }
            pos += total;
        }
        __syncthreads();                 // the tile and the wave totals are re-used by the next tile
    }
    if (!FILL) {
        if (lane == 0) wave_tot[wave] = wave_cnt;
        __syncthreads();
        if (tid == 0) a.table[(int64_t)chunk * a.nq + q] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    }
}

template <bool MASKED, bool GROUPED = false>
__global__ __launch_bounds__(256) void sparse_range_count_kernel(SparseRangeArgs a) { sparse_range_body<false, MASKED, GROUPED>(a); }

// The chunk's cell first: table holds exclusive prefixes, so the cell's own count is the next chunk's prefix minus its own (the query's
// total minus its own for the last chunk).  0: the workgroup returns before it touches a posting.
template <bool MASKED, bool GROUPED = false>
__global__ __launch_bounds__(256) void sparse_range_fill_kernel(SparseRangeArgs a, int n_chunks) {
    const int64_t q = blockIdx.x;
    const int chunk = a.chunk_begin + (int)blockIdx.y;
    const int64_t mine = (int64_t)(uint32_t)a.table[(int64_t)chunk * a.nq + q];
    const int64_t next = chunk + 1 < n_chunks ? (int64_t)(uint32_t)a.table[(int64_t)(chunk + 1) * a.nq + q] : a.lims[q + 1] - a.lims[q];
    if (next == mine) return;            // block-uniform
    sparse_range_body<true, MASKED, GROUPED>(a);
}

static void sparse_range_args(const sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                              int64_t nq, const float* d_thr, const uint32_t* d_mask, const int32_t* d_qgroup, SparseRangeArgs& a) {
    a = SparseRangeArgs{};
    a.indptr = idx->indptr; a.doc_ids = idx->doc_ids; a.vals = idx->vals; a.skip = idx->skip.p;
    a.n_tiles = idx->n_tiles; a.n_docs = idx->n_docs; a.n_terms = idx->n_terms;
    a.q_indptr = d_q_indptr; a.q_cols = d_q_cols; a.q_vals = d_q_vals; a.thr = d_thr; a.nq = nq;
    a.chunk_tiles = idx->range_chunk_tiles; a.table = idx->range_tab.p; a.mask = d_mask; a.qgroup = d_qgroup;
}

// the three kinds of a range search on a handle: a fill needs a preceding count of its own kind
enum { SRR_KIND_ALL = 0, SRR_KIND_MASKED = 1, SRR_KIND_GROUPED = 2 };
static const char* srr_kind_text(int kind) {
    return kind == SRR_KIND_GROUPED ? "under filter groups" : kind == SRR_KIND_MASKED ? "under a mask" : "without a mask";
}

// the argument checks of every count, before any device work
static int sparse_range_count_checks(int64_t nq, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                     const float* d_thresholds, const int64_t* d_lims, const int64_t* total) {
    SR_REQUIRE(nq >= 0 && nq < SRR_MAX_NQ, "sr_sparse_range_count: bad nq=%lld (0 <= nq < 2^24: one workgroup per query and chunk in one launch)", (long long)nq);
    SR_REQUIRE(d_lims && total, "sr_sparse_range_count: null d_lims or total");
    SR_REQUIRE(nq == 0 || (d_q_indptr && d_q_cols && d_q_vals && d_thresholds), "sr_sparse_range_count: null queries or thresholds");
    return SR_OK;
}

// d_mask null: the unrestricted search; with d_qgroup: d_mask holds a bitmap per group, d_qgroup the checked group of every query.  The
// caller holds idx->mu.
static int sparse_range_count(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals, int64_t nq,
                              const float* d_thresholds, const uint32_t* d_mask, const int32_t* d_qgroup, int64_t* d_lims, int64_t* total,
                              sr_stream stream) {
    SR_TRY(sparse_range_count_checks(nq, d_q_indptr, d_q_cols, d_q_vals, d_thresholds, d_lims, total));
    const int kind = d_qgroup ? SRR_KIND_GROUPED : d_mask ? SRR_KIND_MASKED : SRR_KIND_ALL;
    hipStream_t s = (hipStream_t)stream;
    idx->range_nq = -1;
    idx->range_kind = kind;
    if (nq == 0 || idx->n_docs == 0) {
        SR_TRY(sr_zero_lims(d_lims, nq, total, s));
        idx->range_nq = nq; idx->range_total = 0; idx->range_chunks = 0; idx->range_chunk_tiles = 0;
        return SR_OK;
    }
    // one tile per chunk where the table fits the workspace limit, else the smallest chunk that does
    const int64_t max_chunks = idx->ws_limit / (4 * nq);
    if (max_chunks < 1) {
        sr_set_error("sr_sparse_range_count: the chunk table needs at least %lld bytes of workspace for %lld queries (limit %lld bytes)",
                     (long long)(4 * nq), (long long)nq, (long long)idx->ws_limit);
        return SR_ERR_NOMEM;
    }
    int64_t chunk_tiles = ceil_div64(idx->n_tiles, max_chunks < idx->n_tiles ? max_chunks : idx->n_tiles);
    if (const char* e = sr_dev_getenv("SR_SPARSE_RANGE_CHUNK_TILES")) {       // dev switch, read per call: forces the chunk size
        const int64_t forced = atoll(e);
        SR_REQUIRE(forced >= 1, "SR_SPARSE_RANGE_CHUNK_TILES=%s must be a positive number of tiles", e);
        chunk_tiles = forced < idx->n_tiles ? forced : idx->n_tiles;
        if (ceil_div64(idx->n_tiles, chunk_tiles) > max_chunks) {
            sr_set_error("sr_sparse_range_count: chunks of %lld tiles need a table of %lld bytes (limit %lld bytes)", (long long)chunk_tiles,
                         (long long)(4 * nq * ceil_div64(idx->n_tiles, chunk_tiles)), (long long)idx->ws_limit);
            return SR_ERR_NOMEM;
        }
    }
    const int n_chunks = (int)ceil_div64(idx->n_tiles, chunk_tiles);
    const int64_t entries = (int64_t)n_chunks * nq;
    if (idx->range_tab.reserve(entries, nullptr) != SR_OK) {
        sr_set_error("sr_sparse_range_count: out of device memory for the chunk table of %lld bytes", (long long)(entries * 4));
        return SR_ERR_NOMEM;
    }
    StreamOrder::Scope in_order(idx->order, s);
    idx->range_chunk_tiles = (int)chunk_tiles;
    SparseRangeArgs a;
    sparse_range_args(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, d_mask, d_qgroup, a);
    for (int c0 = 0; c0 < n_chunks; c0 += SRR_MAX_GRID_Y) {
        const int nc = n_chunks - c0 < SRR_MAX_GRID_Y ? n_chunks - c0 : SRR_MAX_GRID_Y;
        a.chunk_begin = c0;
        if (d_qgroup) hipLaunchKernelGGL((sparse_range_count_kernel<true, true>), dim3((unsigned)nq, (unsigned)nc), dim3(256), 0, s, a);
        else if (d_mask) hipLaunchKernelGGL(sparse_range_count_kernel<true>, dim3((unsigned)nq, (unsigned)nc), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(sparse_range_count_kernel<false>, dim3((unsigned)nq, (unsigned)nc), dim3(256), 0, s, a);
        SR_CHECK_LAUNCH();
    }
    SR_TRY(launch_range_scan(reinterpret_cast<uint32_t*>(idx->range_tab.p), n_chunks, nq, d_lims, s));
    int64_t h_total = 0;
    SR_CHECK_HIP(hipMemcpyAsync(&h_total, d_lims + nq, 8, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    *total = h_total;
    idx->range_nq = nq; idx->range_total = h_total; idx->range_chunks = n_chunks;
    return SR_OK;
}

extern "C" int sr_sparse_range_count(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                     int64_t nq, const float* d_thresholds, int64_t* d_lims, int64_t* total, sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_range_count: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    return sparse_range_count(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, nullptr, nullptr, d_lims, total, stream);
}

extern "C" int sr_sparse_range_count_masked(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                            int64_t nq, const float* d_thresholds, const uint32_t* d_mask_words, int64_t n_bits,
                                            int64_t* d_lims, int64_t* total, sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_range_count_masked: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_REQUIRE(n_bits == idx->n_docs, "sr_sparse_range_count_masked: n_bits=%lld, the index holds %lld documents", (long long)n_bits,
               (long long)idx->n_docs);
    SR_REQUIRE(d_mask_words, "sr_sparse_range_count_masked: null mask");
    return sparse_range_count(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, d_mask_words, nullptr, d_lims, total, stream);
}

// d_mask: what the preceding count was given (null: none).  The caller holds idx->mu.
static int sparse_range_fill(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals, int64_t nq,
                             const float* d_thresholds, int kind, const uint32_t* d_mask, const int32_t* d_qgroup, const int64_t* d_lims, int64_t id_base,
                             int64_t id_stride, float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < SRR_MAX_NQ && capacity >= 0, "sr_sparse_range_fill: bad nq=%lld (0 <= nq < 2^24) or capacity=%lld", (long long)nq, (long long)capacity);
    SR_REQUIRE(id_base >= 0 && id_stride >= 1, "sr_sparse_range_fill: need id_base >= 0 and id_stride >= 1, got %lld and %lld", (long long)id_base,
               (long long)id_stride);
    hipStream_t s = (hipStream_t)stream;
    SR_REQUIRE(idx->range_nq >= 0, "sr_sparse_range_fill: no sr_sparse_range_count precedes it on this handle");
    SR_REQUIRE(idx->range_kind == kind, "sr_sparse_range_fill: the preceding count ran %s, this fill runs %s", srr_kind_text(idx->range_kind),
               srr_kind_text(kind));
    SR_REQUIRE(idx->range_nq == nq, "sr_sparse_range_fill: nq=%lld, the preceding count had %lld", (long long)nq, (long long)idx->range_nq);
    SR_REQUIRE(capacity >= idx->range_total, "sr_sparse_range_fill: capacity=%lld is below the count's total of %lld", (long long)capacity,
               (long long)idx->range_total);
    if (idx->range_total == 0) return SR_OK;          // nothing to write (also nq = 0)
    SR_REQUIRE(d_q_indptr && d_q_cols && d_q_vals && d_thresholds && d_lims && d_out_scores && d_out_ids, "sr_sparse_range_fill: null pointer");
    StreamOrder::Scope in_order(idx->order, s);
    SparseRangeArgs a;
    sparse_range_args(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, d_mask, d_qgroup, a);
    a.lims = d_lims; a.id_base = id_base; a.id_stride = id_stride; a.out_scores = d_out_scores; a.out_ids = d_out_ids; a.capacity = capacity;
    const int n_chunks = idx->range_chunks;
    for (int c0 = 0; c0 < n_chunks; c0 += SRR_MAX_GRID_Y) {
        const int nc = n_chunks - c0 < SRR_MAX_GRID_Y ? n_chunks - c0 : SRR_MAX_GRID_Y;
        a.chunk_begin = c0;
        if (d_qgroup) hipLaunchKernelGGL((sparse_range_fill_kernel<true, true>), dim3((unsigned)nq, (unsigned)nc), dim3(256), 0, s, a, n_chunks);
        else if (d_mask) hipLaunchKernelGGL(sparse_range_fill_kernel<true>, dim3((unsigned)nq, (unsigned)nc), dim3(256), 0, s, a, n_chunks);
        else hipLaunchKernelGGL(sparse_range_fill_kernel<false>, dim3((unsigned)nq, (unsigned)nc), dim3(256), 0, s, a, n_chunks);
        SR_CHECK_LAUNCH();
    }
    return SR_OK;
}

extern "C" int sr_sparse_range_fill(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                    int64_t nq, const float* d_thresholds, const int64_t* d_lims, int64_t id_base, int64_t id_stride,
                                    float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_range_fill: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    return sparse_range_fill(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, SRR_KIND_ALL, nullptr, nullptr, d_lims, id_base, id_stride, d_out_scores,
                             d_out_ids, capacity, stream);
}

extern "C" int sr_sparse_range_fill_masked(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                           int64_t nq, const float* d_thresholds, const uint32_t* d_mask_words, int64_t n_bits,
                                           const int64_t* d_lims, int64_t id_base, int64_t id_stride, float* d_out_scores,
                                           int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_range_fill_masked: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_REQUIRE(n_bits == idx->n_docs, "sr_sparse_range_fill_masked: n_bits=%lld, the index holds %lld documents", (long long)n_bits,
               (long long)idx->n_docs);
    SR_REQUIRE(d_mask_words, "sr_sparse_range_fill_masked: null mask");
    return sparse_range_fill(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, SRR_KIND_MASKED, d_mask_words, nullptr, d_lims, id_base, id_stride, d_out_scores,
                             d_out_ids, capacity, stream);
}

// ---- under a bitmap per query (filter groups) ------------------------------------------------------------------------------------
// the two grouped halves' wording for sr_group_mask_checks
static const char* const SPARSE_RANGE_BITS = "%s: n_bits=%lld, the index holds %lld documents";

// One workgroup serves one (query, chunk), so the query's group only moves the base of the mask words (sparse_range_body<.., GROUPED>);
// the count reads the group ids back once (4 nq bytes) and checks them before anything is launched, and keeps a copy on the handle that
// its fill reads - the fill does not look at d_query_group again.
extern "C" int sr_sparse_range_count_grouped(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                             int64_t nq, const float* d_thresholds, const uint32_t* d_group_words, int64_t n_groups,
                                             int64_t n_bits, const int32_t* d_query_group, int64_t* d_lims, int64_t* total, sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_range_count_grouped: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    const char* const who = "sr_sparse_range_count_grouped";
    SR_TRY(sr_group_mask_checks(who, n_groups, n_bits, idx->n_docs, SPARSE_RANGE_BITS));
    SR_TRY(sr_require_group_pointers(who, nq, d_group_words, d_query_group, n_bits));
    SR_TRY(sparse_range_count_checks(nq, d_q_indptr, d_q_cols, d_q_vals, d_thresholds, d_lims, total));
    hipStream_t s = (hipStream_t)stream;
    idx->range_nq = -1;                               // whatever happens below, no earlier count can be filled from
    *total = 0;
    if (nq > 0) {
        std::vector<int32_t> grp;
        int64_t bad = -1;
        SR_TRY(sr_read_query_groups(d_query_group, nq, n_groups, s, &grp, &bad));
        if (bad >= 0) {
            SR_TRY(sr_zero_lims(d_lims, nq, total, s));
            return sr_bad_group_error(who, bad, grp[(size_t)bad], n_groups, " (nothing was scored)");
        }
    }
    SR_TRY(idx->range_qgroup.reserve(nq > 0 ? nq : 1, "sr_sparse_range_count_grouped"));      // never null: it names the kind below
    if (nq > 0) {
        SR_CHECK_HIP(hipMemcpyAsync(idx->range_qgroup.p, d_query_group, (size_t)nq * 4, hipMemcpyDeviceToDevice, s));
    }
    SR_TRY(sparse_range_count(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, d_group_words, idx->range_qgroup.p, d_lims, total, stream));
    idx->range_groups = n_groups;
    return SR_OK;
}

extern "C" int sr_sparse_range_fill_grouped(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                            int64_t nq, const float* d_thresholds, const uint32_t* d_group_words, int64_t n_groups,
                                            int64_t n_bits, const int32_t* d_query_group, const int64_t* d_lims, int64_t id_base,
                                            int64_t id_stride, float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_range_fill_grouped: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_TRY(sr_group_mask_checks("sr_sparse_range_fill_grouped", n_groups, n_bits, idx->n_docs, SPARSE_RANGE_BITS));
    SR_TRY(sr_require_group_pointers("sr_sparse_range_fill_grouped", nq, d_group_words, d_query_group, n_bits));
    SR_REQUIRE(idx->range_nq < 0 || idx->range_kind != SRR_KIND_GROUPED || idx->range_groups == n_groups,
               "sr_sparse_range_fill_grouped: n_groups=%lld, the preceding count had %lld", (long long)n_groups, (long long)idx->range_groups);
    return sparse_range_fill(idx, d_q_indptr, d_q_cols, d_q_vals, nq, d_thresholds, SRR_KIND_GROUPED, d_group_words, idx->range_qgroup.p, d_lims, id_base, id_stride, d_out_scores,
                             d_out_ids, capacity, stream);
}
