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
#include "dense_range.h"
#include "dense_index.h"

template <bool FILL, int WN, typename T>
__device__ __forceinline__ void dense_range_body(const DenseRangeArgs& a) {
    typedef typename SrRow<T>::V RowV;
    constexpr int WAVES_N = 4, WM = 4, BK = 16;
    constexpr int NT = 512, TM = 256, TN = 32 * WN * WAVES_N, LDK = BK + 4, KC = BK / 4, NSTAGE = 3;
    constexpr int PER_T = TM * KC / NT;                 // 16-B chunks per thread of the doc tile (= 2)
    constexpr int PER_TB = TN * KC / NT;                // ... of the query tile (2 or 1)
    constexpr int HALF_MFMAS = 4 * WM * WN;
    constexpr int MPO = WN == 2 ? 2 : 1;
    constexpr int BMP = TM / 32 + 1;                    // bitmap pitch in words: 9 is odd, the 32 query columns of a ds_write_b32 hit 32 banks
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [NSTAGE][TM][LDK]
    float* Bs = smem + NSTAGE * TM * LDK;   // [NSTAGE][TN][LDK]
    uint32_t* aux = reinterpret_cast<uint32_t*>(smem + NSTAGE * (TM + TN) * LDK);   // count: [TN] sums; fill: [TN][BMP] hit bitmap
    int64_t* posl = reinterpret_cast<int64_t*>(aux + TN * BMP);                       // fill: [TN] the running write position of each query

    const int q0 = blockIdx.x * TN;
    const int chunk = a.chunk_base + (int)blockIdx.y;
    const int64_t r_begin = (int64_t)blockIdx.y * a.chunk_rows;
    const int64_t r_end = r_begin + a.chunk_rows < a.seg_rows ? r_begin + a.chunk_rows : a.seg_rows;
    const int H = a.H;
    const int nk = H / BK;

    // per-query state of the chunk lives in LDS, not in registers: nothing lane-derived is live across the 256-register k-loop
    if (threadIdx.x < TN) {
        const int q = q0 + (int)threadIdx.x;
        if (FILL) posl[threadIdx.x] = q < a.nq ? a.lims[q] + (int64_t)a.table[(int64_t)chunk * a.nq + q] : 0;
        else aux[threadIdx.x] = 0;
    }   // made visible by the first tile's barriers

    for (int64_t row0 = r_begin; row0 < r_end; row0 += TM) {
        // hipcc would hoist every lane-derived value of a tile's set-up and epilogue out of this loop and spill it through the k-loop
        // (dense_split_kernel.h): the thread index is made opaque once per tile and once per epilogue, recomputing costs a few VALU
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = tid >> 6;
        const int wm = wave / WAVES_N, wn = wave % WAVES_N;
        const T* asrc[PER_T];
        const float* bsrc[PER_TB];
        int soff[PER_T];
#pragma unroll
        for (int i = 0; i < PER_T; ++i) {
            // chunk c -> (row r, k-chunk kc) as in dense_score_pipe_kernel: conflict-free stage writes, 64-byte row pieces
            const int c = tid + i * NT, kc = c & 3, grp = c >> 3;
            const int r = (grp >> 2) * 8 + (grp & 3) + 4 * ((c >> 2) & 1);
            soff[i] = r * LDK + kc * 4;
            int64_t row = row0 + r;
            row = row < r_end ? row : r_end - 1;          // rows past the chunk are clamped, their scores never emitted
            asrc[i] = static_cast<const T*>(a.D) + row * H + kc * 4;
            if (i < PER_TB) {
                int q = q0 + r;
                q = q < a.nq ? q : a.nq - 1;
                bsrc[i] = a.Q + (int64_t)q * H + kc * 4;
            }
        }
        const int aoff = (wm * WM * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
        const int boff = (wn * WN * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
        RowV ra[PER_T];
        f32x4 rb[PER_TB];
        auto gload = [&](int k0) {
#pragma unroll
            for (int i = 0; i < PER_T; ++i) ra[i] = *reinterpret_cast<const RowV*>(asrc[i] + k0);
#pragma unroll
            for (int i = 0; i < PER_TB; ++i) rb[i] = *reinterpret_cast<const f32x4*>(bsrc[i] + k0);
        };
        auto sstore = [&](int st) {
#pragma unroll
            for (int i = 0; i < PER_T; ++i) *reinterpret_cast<f32x4*>(&As[st * TM * LDK + soff[i]]) = SrRow<T>::widen(ra[i]);
#pragma unroll
            for (int i = 0; i < PER_TB; ++i) *reinterpret_cast<f32x4*>(&Bs[st * TN * LDK + soff[i]]) = rb[i];
        };
        auto frag = [&](int st, int sub, f32x4 (&af)[WM], f32x4 (&bf)[WN]) {
#pragma unroll
            for (int m = 0; m < WM; ++m) af[m] = *reinterpret_cast<const f32x4*>(&As[st * TM * LDK + aoff + m * 32 * LDK + 8 * sub]);
#pragma unroll
            for (int n = 0; n < WN; ++n) bf[n] = *reinterpret_cast<const f32x4*>(&Bs[st * TN * LDK + boff + n * 32 * LDK + 8 * sub]);
        };

        f32x16 acc[WM][WN];
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int n = 0; n < WN; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
#define SR_RANGE_MFMAS(AF, BF)                                                                                   \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                \
        _Pragma("unroll") for (int m = 0; m < WM; ++m)                                                           \
            _Pragma("unroll") for (int n = 0; n < WN; ++n)                                                       \
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(AF[m][j], BF[n][j], acc[m][n], 0, 0, 0);

        // The previous tile's k-loop ended on a barrier behind its last stage reads and writes, and its epilogue touches only
        // `aux`: the stages are free here.
        {   // prologue: three k-steps' loads in flight before the first stage is written
            RowV pa[2][PER_T];
            f32x4 pb[2][PER_TB];
#pragma unroll
            for (int st0 = 0; st0 < 2; ++st0) {
                const int k0 = (st0 < nk ? st0 : 0) * BK;
#pragma unroll
                for (int i = 0; i < PER_T; ++i) pa[st0][i] = *reinterpret_cast<const RowV*>(asrc[i] + k0);
#pragma unroll
                for (int i = 0; i < PER_TB; ++i) pb[st0][i] = *reinterpret_cast<const f32x4*>(bsrc[i] + k0);
            }
            gload(nk > 2 ? 2 * BK : 0);
#pragma unroll
            for (int st0 = 0; st0 < 2; ++st0) {
#pragma unroll
                for (int i = 0; i < PER_T; ++i) *reinterpret_cast<f32x4*>(&As[st0 * TM * LDK + soff[i]]) = SrRow<T>::widen(pa[st0][i]);
#pragma unroll
                for (int i = 0; i < PER_TB; ++i) *reinterpret_cast<f32x4*>(&Bs[st0 * TN * LDK + soff[i]]) = pb[st0][i];
            }
        }
        __syncthreads();
        f32x4 a0[WM], b0[WN], a1[WM], b1[WN];
        frag(0, 0, a0, b0);
        int st = 0;
        for (int kt = 0; kt < nk; ++kt) {     // the k-step of dense_score_pipe_kernel, issue order included
            const int st1 = st == NSTAGE - 1 ? 0 : st + 1;
            const int st2 = st1 == NSTAGE - 1 ? 0 : st1 + 1;
            frag(st, 1, a1, b1);
            sstore(st2);
            gload(kt + 3 < nk ? (kt + 3) * BK : H - BK);
            SR_RANGE_MFMAS(a0, b0)
#pragma unroll
            for (int i = 0; i < WM + WN; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, MPO, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
#pragma unroll
            for (int i = 0; i < PER_T + PER_TB; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, MPO, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
            }
#pragma unroll
            for (int i = 0; i < PER_T + PER_TB; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, MPO, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, HALF_MFMAS - MPO * (WM + WN + 2 * (PER_T + PER_TB)), 0);
            __builtin_amdgcn_sched_barrier(0);
            frag(st1, 0, a0, b0);
            SR_RANGE_MFMAS(a1, b1)
#pragma unroll
            for (int i = 0; i < WM + WN; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, MPO, 1);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, HALF_MFMAS - MPO * (WM + WN), 1);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            st = st1;
        }
#undef SR_RANGE_MFMAS

        // ---- epilogue.  Register r of block m is local row lr0 + 32 m + (r & 3) + 8 (r >> 2); the lane halves are 4 rows apart ----
        int tid_e = threadIdx.x;
        asm volatile("" : "+v"(tid_e));
        const int lane_e = tid_e & 63, half = lane_e >> 5;
        const int em = (tid_e >> 6) / WAVES_N, en = (tid_e >> 6) % WAVES_N;
        const int64_t left = r_end - row0;
        const int rows_valid = left < TM ? (int)left : TM;
        const int lr0 = em * WM * 32 + 4 * half;
        uint32_t word[WN][WM];
#pragma unroll
        for (int n = 0; n < WN; ++n) {
            const int qcol = en * WN * 32 + n * 32 + (lane_e & 31);
            const int q = q0 + qcol;
            const float thr = q < a.nq ? a.thr[q] : __builtin_inff();      // a column past nq: never a hit
            int cnt = 0;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                uint32_t w = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lr = lr0 + m * 32 + (r & 3) + 8 * (r >> 2);
                    const bool hit = lr < rows_valid && acc[m][n][r] > thr;      // strict; false for a NaN on either side
                    if (FILL) w |= (hit ? 1u : 0u) << ((r & 3) + 8 * (r >> 2));
                    else cnt += hit ? 1 : 0;
                }
                if (FILL) {
                    w <<= 4 * half;
                    w |= (uint32_t)__shfl_xor((int)w, 32);          // both halves now hold the block's 32 rows
                    word[n][m] = w;
                    if (half == 0) aux[qcol * BMP + em * WM + m] = w;
                }
            }
            if (!FILL && cnt) atomicAdd(&aux[qcol], (uint32_t)cnt);     // LDS add: the 4 lanes that share the query
        }
        if (FILL) {
            __syncthreads();
#pragma unroll
            for (int n = 0; n < WN; ++n) {
                const int qcol = en * WN * 32 + n * 32 + (lane_e & 31);
                int below = 0, total = 0;                          // hits of the query in the tile, and in the blocks below this wave's
#pragma unroll
                for (int b = 0; b < TM / 32; ++b) {
                    const int c = __popc(aux[qcol * BMP + b]);
                    total += c;
                    below += b < em * WM ? c : 0;
                }
                if (total == 0) continue;
                const int q = q0 + qcol;                           // has hits: q < nq
                int64_t p0 = posl[qcol] + below;
                int64_t p_end = a.lims[q + 1];
                p_end = p_end < a.capacity ? p_end : a.capacity;
#pragma unroll
                for (int m = 0; m < WM; ++m) {
                    const uint32_t w = word[n][m];
                    if (w & (0x0f0f0f0fu << (4 * half))) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int bit = (r & 3) + 8 * (r >> 2) + 4 * half;
                            if ((w >> bit) & 1u) {
                                const int64_t p = p0 + __popc(w & ((1u << bit) - 1u));
                                if (p >= 0 && p < p_end) {         // never outside the query's segment, whatever the count saw
                                    a.out_scores[p] = acc[m][n][r];
                                    a.out_ids[p] = a.id_base + (row0 + em * WM * 32 + m * 32 + bit) * a.id_stride;
                                }
                            }
                        }
                    }
                    p0 += __popc(w);
                }
            }
            __syncthreads();                                       // every reader of the positions is through
            if (tid_e < TN) {
                int total = 0;
#pragma unroll
                for (int b = 0; b < TM / 32; ++b) total += __popc(aux[tid_e * BMP + b]);
                posl[tid_e] += total;
            }   // bitmap and positions are next touched behind the next tile's k-loop barriers
        }
    }

    if (!FILL) {
        __syncthreads();
        if (threadIdx.x < TN && q0 + (int)threadIdx.x < a.nq) a.table[(int64_t)chunk * a.nq + q0 + threadIdx.x] = aux[threadIdx.x];
    }
}

template <int WN, typename T>
__global__ __launch_bounds__(512, 2) void dense_range_count_kernel(DenseRangeArgs a) { dense_range_body<false, WN, T>(a); }
template <int WN, typename T>
__global__ __launch_bounds__(512, 2) void dense_range_fill_kernel(DenseRangeArgs a) { dense_range_body<true, WN, T>(a); }

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

template <bool FILL, int WN, typename T>
static int launch_dense_range_t(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) {
    constexpr int TN = 128 * WN;
    constexpr size_t lds = sizeof(float) * 3 * (256 + TN) * (16 + 4) + (FILL ? (4 * (256 / 32 + 1) + 8) * (size_t)TN : 4 * (size_t)TN);
    static_assert(lds <= 160 * 1024, "one workgroup per CU");
    const void* fn = FILL ? reinterpret_cast<const void*>(&dense_range_fill_kernel<WN, T>)
                          : reinterpret_cast<const void*>(&dense_range_count_kernel<WN, T>);
    static DeviceOnce attr_once;
    bool* attr_slot = attr_once.pending();
    if (attr_slot) {
        SR_CHECK_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        *attr_slot = true;
    }
    dim3 grid((unsigned)ceil_div64(a.nq, TN), (unsigned)n_chunks_seg);
    if (FILL) hipLaunchKernelGGL((dense_range_fill_kernel<WN, T>), grid, dim3(512), lds, s, a);
    else hipLaunchKernelGGL((dense_range_count_kernel<WN, T>), grid, dim3(512), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
template <bool FILL>
static int launch_dense_range(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) {
    if (a.nq < 1 || n_chunks_seg < 1 || a.seg_rows < 1 || a.chunk_rows < 256 || a.chunk_rows % 256 != 0 ||
        ceil_div64(a.seg_rows, a.chunk_rows) != n_chunks_seg) {
        sr_set_error("dense range launch: bad chunking (%lld rows, chunks of %lld, %d chunks)", (long long)a.seg_rows, (long long)a.chunk_rows, n_chunks_seg);
        return SR_ERR_INVALID;
    }
    const bool wide = dense_range_query_tile(a.nq) == 256;
    if (a.dtype == SR_DTYPE_F16)
        return wide ? launch_dense_range_t<FILL, 2, _Float16>(a, n_chunks_seg, s) : launch_dense_range_t<FILL, 1, _Float16>(a, n_chunks_seg, s);
    return wide ? launch_dense_range_t<FILL, 2, float>(a, n_chunks_seg, s) : launch_dense_range_t<FILL, 1, float>(a, n_chunks_seg, s);
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

static void dense_range_args(const sr_dense_index* idx, const DenseSegment& seg, const float* d_queries, int64_t nq, const float* d_thr,
                             int chunk_base, DenseRangeArgs& a) {
    a = DenseRangeArgs{};
    a.D = seg.rows; a.Q = d_queries; a.thr = d_thr; a.seg_rows = seg.n; a.chunk_rows = idx->range_chunk_rows; a.chunk_base = chunk_base;
    a.H = idx->dim; a.nq = (int)nq; a.dtype = idx->row_dtype; a.id_base = seg.id_base; a.id_stride = seg.id_stride;
    a.table = idx->range_tab.p;
}

extern "C" int sr_dense_range_count(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds, int64_t* d_lims,
                                    int64_t* total, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_count: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_dense_range_count: bad nq=%lld", (long long)nq);
    SR_REQUIRE(d_lims && total, "sr_dense_range_count: null d_lims or total");
    SR_REQUIRE(nq == 0 || (d_queries && d_thresholds), "sr_dense_range_count: null queries or thresholds");
    SR_REQUIRE(((uintptr_t)d_queries & 15) == 0, "sr_dense_range_count: queries must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->range_nq = -1;
    *total = 0;
    if (nq == 0 || idx->ntotal == 0) {
        SR_CHECK_HIP(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * 8, s));
        SR_CHECK_HIP(hipStreamSynchronize(s));
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
        dense_range_args(idx, seg, d_queries, nq, d_thresholds, chunk_base, a);
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

extern "C" int sr_dense_range_fill(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds, const int64_t* d_lims,
                                   float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_range_fill: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30) && capacity >= 0, "sr_dense_range_fill: bad nq=%lld or capacity=%lld", (long long)nq, (long long)capacity);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_REQUIRE(idx->range_nq >= 0, "sr_dense_range_fill: no sr_dense_range_count precedes it on this handle");
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
        dense_range_args(idx, seg, d_queries, nq, d_thresholds, chunk_base, a);
        a.lims = d_lims; a.out_scores = d_out_scores; a.out_ids = d_out_ids; a.capacity = capacity;
        idx->prof.begin(s);
        SR_TRY(launch_dense_range_fill(a, n_seg, s));
        idx->prof.end(s, 2.0 * (double)nq * (double)seg.n * idx->dim, (double)seg.n * idx->dim * (double)sr_dtype_size(idx->row_dtype));
        chunk_base += n_seg;
    }
    return SR_OK;
}
