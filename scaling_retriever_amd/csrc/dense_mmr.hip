// Diversified dense search: exact greedy Maximal Marginal Relevance over a candidate list per query, on the rows the
// dense index already holds.  No reference counterpart: it extends DenseFlatIndexer.search_knn (scaling_retriever/indexer.py:191-217),
// whose result nothing diversifies.
//   sr_dense_mmr  one workgroup per query runs all k steps.  Set-up: every valid candidate id is resolved to its row pointer once (the
//                 segment walk of dense_pairs_kernel) and kept in LDS with its id, f32(lambda * rel) and its running m = the largest
//                 similarity to a selected row; a null row pointer is "not a candidate (any more)".  A step: the row picked last is the
//                 "query", every candidate still alive runs ITS serial fmaf chain against it in the pair scorer's tile shape (64
//                 candidates per wave, lane = candidate, rows fetched 64 columns at a time as coalesced 16-byte pieces and transposed
//                 through a padded LDS tile, the next chunk's loads in flight) - so sim(i, j) is bit for bit sr_dense_score_pairs' score
//                 of the query "row i as fp32" and document j.  The waves of the workgroup take tiles side by side and move through
//                 the chunks in step (the picked row's chunk is staged once for all of them); selected and padding lanes fetch no row
//                 of their own (they re-read one cached piece of the picked row, see `fetch`).  Then m = sim > m ? sim : m,
//                 v = f32(f32(lambda * rel) - f32(mu * m)) with contraction off, and a workgroup reduction picks the best by (v descending
//                 as floats, -0.0 == +0.0; id ascending; position ascending): a total order, so no atomic decides an output byte.
// Lazy rows, not a Gram matrix: k * n chains per query and no n^2 buffer.  Every loop is bounded by k, n and H; workgroups never
// communicate.  The ids are checked by a kernel of their own first (one atomicMin per OFFENDING id, as the pair scorer reports them): once it
// found an id the index does not hold, every query's outputs are padding.
#include "dense_index.h"
#include "mmr_select.h"
#include "subset_search.h"
#include <float.h>
#include <math.h>

#define MMR_KC 64                       // columns per chunk
#define MMR_TILE_FLOATS (64 * (MMR_KC + 1))
#define MMR_CAND_BYTES 24

struct MmrArgs {
    const PairSeg* segs; int n_segs;
    int H, n, k;
    const int64_t* ids; const float* rel; const int32_t* counts;
    float lambda, mu;
    int64_t* out_ids; float* out_rel; float* out_mmr; int32_t* out_pos; int32_t* out_counts;
    const PairStatus* st;
};

__global__ void mmr_check_kernel(const PairSeg* __restrict__ segs, int n_segs, int H, const int64_t* __restrict__ ids,
                                 const int32_t* __restrict__ counts, int64_t nq, int n, PairStatus* __restrict__ st) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nq * n) return;
    const int64_t q = p / n;
    const int i = (int)(p - q * n);
    const int64_t id = ids[p];
    if (i >= list_count(counts, q, n) || id < 0) return;
    int seg;
    int64_t elem;
    if (!pair_row_of(segs, n_segs, id, H, &seg, &elem)) atomicMin(&st->first_bad, (unsigned long long)p);
}

template <typename T>
__global__ __launch_bounds__(64 * MMR_MAX_WAVES) void dense_mmr_kernel(MmrArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ float qs[MMR_KC];                                // the picked row's chunk: read once per chunk, for every tile
    __shared__ MmrKey red[MMR_MAX_WAVES];
    const int n = a.n, H = a.H, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
    const T** s_row = reinterpret_cast<const T**>(smem_raw);    // [n] null: padding, or selected
    int64_t* s_id = reinterpret_cast<int64_t*>(s_row + n);      // [n]
    float* s_lr = reinterpret_cast<float*>(s_id + n);           // [n] f32(lambda * rel)
    float* s_m = s_lr + n;                                      // [n] largest similarity to a selected row
    float* tile = s_m + n + (size_t)w * MMR_TILE_FLOATS;        // this wave's [64][MMR_KC + 1]
    const int64_t q = blockIdx.x;
    const int64_t* ids = a.ids + q * n;
    const float* rel = a.rel + q * n;
    const int kk = a.k < n ? a.k : n;

    int picked = 0;
    if (a.st->first_bad == ~0ull) {                             // the check ran before this launch on the same stream
        const int cnt = list_count(a.counts, q, n);
        MmrKey mine;
        mine.ord = 0; mine.pos = -1; mine.id = 0;
        for (int i = tid; i < n; i += nt) {
            const T* row = nullptr;
            const int64_t id = ids[i];
            int seg;
            int64_t elem;
            if (i < cnt && id >= 0 && pair_row_of(a.segs, a.n_segs, id, H, &seg, &elem)) row = static_cast<const T*>(a.segs[seg].rows) + elem;
            const float r = rel[i];
            s_row[i] = row;
            s_id[i] = id;
            s_lr[i] = a.lambda * r;
            s_m[i] = -INFINITY;
            if (row) {
                MmrKey c;
                c.ord = sr_f2ord(r); c.pos = i; c.id = id;
                if (mmr_better(c, mine)) mine = c;
            }
        }
        __syncthreads();
        MmrKey best = mmr_block_best(mine, red, nw);            // pick 0: by (rel, id, position)
        float best_v = best.pos >= 0 ? s_lr[best.pos] : 0.f;
        const int n_tiles = (n + 63) >> 6, nch = (H + MMR_KC - 1) / MMR_KC;
        while (best.pos >= 0) {
            const T* prow = s_row[best.pos];
            __syncthreads();                                    // every thread holds the picked row
            if (tid == 0) {
                const int64_t o = q * a.k + picked;
                a.out_ids[o] = best.id;
                a.out_rel[o] = rel[best.pos];
                a.out_mmr[o] = best_v;
                a.out_pos[o] = best.pos;
                s_row[best.pos] = nullptr;
            }
            ++picked;
            __syncthreads();
            if (picked >= kk) break;

            mine.ord = 0; mine.pos = -1; mine.id = 0;
            float mine_v = 0.f;
            for (int t0 = 0; t0 < n_tiles; t0 += nw) {          // the waves' tiles of this round, chunk by chunk in step
                const int c0 = (t0 + w) * 64;                   // first candidate of this wave's tile (may lie beyond n: an idle wave)
                const int pos = c0 + lane;
                const bool alive = pos < n && s_row[pos] != nullptr;
                const bool any = __ballot(alive) != 0ull;       // a tile without a live candidate moves nothing
                const T* myp[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int c = c0 + i * 4 + (lane >> 4);
                    myp[i] = c < n ? s_row[c] : nullptr;
                }
                float acc = 0.f;
                // A row pointer that went through LDS is a generic pointer to the compiler: its loads would be flat loads, which count as
                // LDS traffic too - every wait for the tile would then wait for the next chunk's rows.  The rows are global memory.
                // The pieces stay as loaded (fp16 rows: 8 bytes) until their chunk's turn: widening them at the fetch would wait for them.
                typedef typename SrRow<T>::V RowV;
                typedef const RowV __attribute__((address_space(1)))* GlobalRowV;
                typedef const T __attribute__((address_space(1)))* GlobalT;
                auto fetch = [&](int k0, RowV (&v)[16], float& qv) {
                    const int col = k0 + (lane & 15) * 4;       // H % 16 == 0: a four-element piece is inside the row or beyond it
                    // Every lane loads, always: a branch around a load leaves the compiler unable to count the loads in flight, and it
                    // then waits for ALL of them - the next chunk's too - before it touches this chunk's.  A lane without a row (selected,
                    // padding, beyond H) reads the first piece of the picked row instead: one address for all of them, in cache (wave 0
                    // reads that row anyway), never used - a dead lane's tile row is never summed, columns beyond H are never visited.
#pragma unroll
                    for (int i = 0; i < 16; ++i) v[i] = *((myp[i] && col < H) ? (GlobalRowV)(uintptr_t)(myp[i] + col) : (GlobalRowV)(uintptr_t)prow);
                    const int kq = k0 + lane < H ? k0 + lane : H - 1;
                    qv = (float)*(GlobalT)(uintptr_t)(prow + kq);
                };
                auto chunk = [&](const RowV (&v)[16], float qv, int k0) {
                    mmr_lds_barrier();                          // the previous chunk is consumed
                    if (any) {
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            float* t = &tile[(i * 4 + (lane >> 4)) * (MMR_KC + 1) + (lane & 15) * 4];
                            const f32x4 x = SrRow<T>::widen(v[i]);
                            t[0] = x[0]; t[1] = x[1]; t[2] = x[2]; t[3] = x[3];
                        }
                    }
                    if (w == 0) qs[lane] = qv;
                    mmr_lds_barrier();
                    if (!any) return;
                    const float* trow = &tile[lane * (MMR_KC + 1)];
                    if (H - k0 >= MMR_KC) {
#pragma unroll
                        for (int s8 = 0; s8 < MMR_KC; s8 += 8)
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                acc = __builtin_fmaf(qs[s8 + jj], trow[s8 + jj], acc);
                                acc = __builtin_fmaf(qs[s8 + 4 + jj], trow[s8 + 4 + jj], acc);
                            }
                    } else {                                    // the last chunk of a dim that is not a multiple of 64: its columns only
                        for (int s8 = 0; s8 < H - k0; s8 += 8)
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                acc = __builtin_fmaf(qs[s8 + jj], trow[s8 + jj], acc);
                                acc = __builtin_fmaf(qs[s8 + 4 + jj], trow[s8 + 4 + jj], acc);
                            }
                    }
                };
                RowV va[16], vb[16];
                float qva, qvb;
                fetch(0, va, qva);
                for (int c = 0; c < nch; c += 2) {              // a fetch beyond H is not branched around either: it reads the one cached piece
                    fetch((c + 1) * MMR_KC, vb, qvb);
                    chunk(va, qva, c * MMR_KC);
                    if (c + 1 >= nch) break;
                    fetch((c + 2) * MMR_KC, va, qva);
                    chunk(vb, qvb, (c + 1) * MMR_KC);
                }
                if (alive) {
                    const float m_old = s_m[pos];
                    const float m = acc > m_old ? acc : m_old;
                    s_m[pos] = m;
                    const float pen = a.mu * m;
                    const float v = s_lr[pos] - pen;
                    MmrKey c;
                    c.ord = sr_f2ord(v); c.pos = pos; c.id = s_id[pos];
                    if (mmr_better(c, mine)) {
                        mine = c;
                        mine_v = v;
                    }
                }
            }
            best = mmr_block_best(mine, red, nw);
            // the winner's v, bits untouched (its key folds -0.0 into +0.0): from the thread that owns it
            if (best.pos >= 0 && mine.pos == best.pos) qs[0] = mine_v;
            __syncthreads();
            best_v = qs[0];
        }
    }
    for (int i = picked + tid; i < a.k; i += nt) {
        const int64_t o = q * a.k + i;
        a.out_ids[o] = -1;
        a.out_rel[o] = -FLT_MAX;
        a.out_mmr[o] = -FLT_MAX;
        a.out_pos[o] = -1;
    }
    if (tid == 0) a.out_counts[q] = picked;
}

int launch_id_list_check(const PairSeg* d_segs, int n_segs, int H, const int64_t* d_ids, const int32_t* d_counts, int64_t nq, int n,
                         PairStatus* d_status, hipStream_t s) {
    hipLaunchKernelGGL(mmr_check_kernel, dim3((unsigned)ceil_div64(nq * n, 256)), dim3(256), 0, s, d_segs, n_segs, H, d_ids, d_counts, nq, n,
                       d_status);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

extern "C" int sr_mmr_max_candidates(void) { return MMR_MAX_N; }

extern "C" int sr_dense_mmr(sr_dense_index* idx, const int64_t* d_ids, const float* d_rel, const int32_t* d_counts, int64_t nq, int64_t n,
                            int k, float lambda, int64_t* d_out_ids, float* d_out_rel, float* d_out_mmr, int32_t* d_out_pos,
                            int32_t* d_out_counts, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_mmr: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 28), "sr_dense_mmr: bad nq=%lld", (long long)nq);
    SR_REQUIRE(n >= 1 && n <= MMR_MAX_N, "sr_dense_mmr: %lld candidates per query: 1 to %d (sr_mmr_max_candidates) are held in LDS", (long long)n,
               MMR_MAX_N);
    SR_REQUIRE(k >= 1 && k <= MMR_MAX_N, "sr_dense_mmr: k = %d, 1 to %d are selected", k, MMR_MAX_N);
    SR_REQUIRE(lambda >= 0.f && lambda <= 1.f, "sr_dense_mmr: lambda = %g is not in [0, 1]", (double)lambda);
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_ids && d_rel && d_out_ids && d_out_rel && d_out_mmr && d_out_pos && d_out_counts, "sr_dense_mmr: null pointer");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    SR_TRY(dense_pair_segs(idx, "sr_dense_mmr"));
    SR_TRY(subset_status_begin(&idx->pair_status, s));
    const int n_segs = (int)idx->pair_segs_n;
    SR_TRY(launch_id_list_check(idx->pair_segs.p, n_segs, idx->dim, d_ids, d_counts, nq, (int)n, idx->pair_status, s));

    // as many waves as the list has tiles, up to 8, and as their 16.6 KB tiles fit beside the candidates' 24 bytes each
    int dev = 0, lds_max = 0;
    SR_CHECK_HIP(hipGetDevice(&dev));
    SR_CHECK_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    const int64_t cand_bytes = MMR_CAND_BYTES * n, tile_bytes = 4 * MMR_TILE_FLOATS, fixed_bytes = 1024;   // the kernel's static arrays, rounded up
    int nw = (int)ceil_div64(n, 64);
    if (nw > MMR_MAX_WAVES) nw = MMR_MAX_WAVES;
    const int64_t fit = ((int64_t)lds_max - fixed_bytes - cand_bytes) / tile_bytes;
    if (nw > fit) nw = (int)fit;
    SR_REQUIRE(nw >= 1, "sr_dense_mmr: %lld candidates do not fit the %d bytes of LDS of a workgroup", (long long)n, lds_max);
    const size_t lds = (size_t)(cand_bytes + nw * tile_bytes);

    MmrArgs a;
    a.segs = idx->pair_segs.p; a.n_segs = n_segs; a.H = idx->dim; a.n = (int)n; a.k = k;
    a.ids = d_ids; a.rel = d_rel; a.counts = d_counts;
    a.lambda = lambda; a.mu = 1.0f - lambda;
    a.out_ids = d_out_ids; a.out_rel = d_out_rel; a.out_mmr = d_out_mmr; a.out_pos = d_out_pos; a.out_counts = d_out_counts;
    a.st = idx->pair_status;
    const void* fn = idx->row_dtype == SR_DTYPE_F16 ? (const void*)dense_mmr_kernel<_Float16> : (const void*)dense_mmr_kernel<float>;
    static DeviceOnce lds_set[2];
    SR_TRY(sr_allow_lds(lds_set[idx->row_dtype == SR_DTYPE_F16 ? 1 : 0], fn, lds_max - (int)fixed_bytes));
    if (idx->row_dtype == SR_DTYPE_F16)
        hipLaunchKernelGGL(dense_mmr_kernel<_Float16>, dim3((unsigned)nq), dim3(64 * nw), lds, s, a);
    else
        hipLaunchKernelGGL(dense_mmr_kernel<float>, dim3((unsigned)nq), dim3(64 * nw), lds, s, a);
    SR_CHECK_LAUNCH();

    PairStatus h;
    SR_CHECK_HIP(hipMemcpyAsync(&h, idx->pair_status, sizeof(h), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    if (h.first_bad != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_ids + h.first_bad, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("sr_dense_mmr: candidate id %lld (query %llu, entry %llu) is not in the index (nothing was selected)", (long long)id,
                     h.first_bad / (unsigned long long)n, h.first_bad % (unsigned long long)n);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
