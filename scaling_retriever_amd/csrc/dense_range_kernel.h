// The dense range search's tile kernel (see dense_range.hip) and its launcher, as templates: dense_range.hip instantiates the unrestricted
// kernels, dense_range_masked.hip their twins under a document bitmap - an object of its own, as dense_split_masked.hip is - and
// dense_range_grouped.hip those under a bitmap per query.
#pragma once
#include "dense_range.h"

// Which documents a range search may return.  all: every indexed one.  masked: those whose bit is set in a.mask.  grouped: query q's own
// bitmap a.mask + a.mask_qoff[q] words decides its hits, and a.mask_union - the OR of the bitmaps of the groups that have a query - the
// tiles that are skipped.
enum class RangeFilter { all, masked, grouped };

// GROUPED epilogue: the mask bits of the 32 rows row_b .. row_b + 31 of the segment for one query (bitmap `words`, n_words long), bit =
// row within the block.  Stride 1: the block is 32 consecutive bits from id_base + row_b, two words joined by a funnel shift; a word at or
// beyond n_words reads as 0 (only a block that ends past the segment's rows reaches there, and those rows are never hits).
__device__ __forceinline__ uint32_t dense_range_block_bits(const uint32_t* __restrict__ words, int64_t n_words, int64_t bit0) {
    const int64_t w = bit0 >> 5;
    const unsigned sh = (unsigned)(bit0 & 31);
    const uint32_t lo = w < n_words ? words[w] : 0u;
    const uint32_t hi = (sh != 0 && w + 1 < n_words) ? words[w + 1] : 0u;
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

template <bool FILL, int WN, typename T, RangeFilter FILTER>
__device__ __forceinline__ void dense_range_body(const DenseRangeArgs& a) {
    constexpr bool MASKED = FILTER == RangeFilter::masked, GROUPED = FILTER == RangeFilter::grouped;
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
        uint64_t mbits[4] = {0, 0, 0, 0};     // MASKED: the mask bits of the tile's rows 64 j .. 64 j + 63, wave-uniform (GROUPED: the union's)
        if constexpr (MASKED || GROUPED) {
            const uint32_t* __restrict__ tile_mask = GROUPED ? a.mask_union : a.mask;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = row0 + 64 * j + lane;
                bool allowed = false;
                if (row < r_end) {                // an indexed document: its index is below id_end = the mask's n_bits
                    const int64_t bit = a.id_base + row * a.id_stride;
                    allowed = (tile_mask[bit >> 5] >> (unsigned)(bit & 31)) & 1u;
                }
                mbits[j] = __ballot(allowed);
            }
            if ((mbits[0] | mbits[1] | mbits[2] | mbits[3]) == 0) continue;      // every wave holds the same 256 bits: workgroup-uniform
        }
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
        uint32_t mrow[WM];                    // MASKED: the mask bits of this wave's four 32-row blocks, bit = row within the block
        if constexpr (MASKED) {
            const int em_u = __builtin_amdgcn_readfirstlane(em);
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                const uint64_t lo = em_u ? mbits[2 + (m >> 1)] : mbits[m >> 1];      // rows 128 em + 32 m .. + 31 (WM = 4)
                mrow[m] = (uint32_t)(lo >> (32 * (m & 1)));
            }
        }
#pragma unroll
        for (int n = 0; n < WN; ++n) {
            const int qcol = en * WN * 32 + n * 32 + (lane_e & 31);
            const int q = q0 + qcol;
            const float thr = q < a.nq ? a.thr[q] : __builtin_inff();      // a column past nq: never a hit
            // GROUPED: the column's own bitmap, loaded here, behind the k-loop (a.mask_qoff is padded to the query tile: 0 past nq)
            const uint32_t* qmask = nullptr;
            uint32_t mq[WM] = {0, 0, 0, 0};                              // GROUPED, stride 1: the column's bits of the wave's four 32-row blocks
            if constexpr (GROUPED) {
                __builtin_amdgcn_sched_barrier(0);                       // one column's eight words in flight at a time, not both columns'
                qmask = a.mask + a.mask_qoff[q];
                if (a.id_stride == 1) {
#pragma unroll
                    for (int m = 0; m < WM; ++m) mq[m] = dense_range_block_bits(qmask, a.mask_words, a.id_base + row0 + em * WM * 32 + m * 32);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            int cnt = 0;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                uint32_t w = 0;
                uint32_t mh = 0;
                if constexpr (MASKED) mh = mrow[m] >> (4 * half);      // this lane's rows: bits (r & 3) + 8 (r >> 2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lr = lr0 + m * 32 + (r & 3) + 8 * (r >> 2);
                    bool hit = lr < rows_valid && acc[m][n][r] > thr;      // strict; false for a NaN on either side
                    if constexpr (MASKED && !FILL) hit = hit && ((mh >> ((r & 3) + 8 * (r >> 2))) & 1u);
                    if (FILL || GROUPED) w |= (hit ? 1u : 0u) << ((r & 3) + 8 * (r >> 2));
                    else cnt += hit ? 1 : 0;
                }
                if constexpr (GROUPED) {      // w: this lane's 16 rows above the threshold; the column's own bitmap decides among them
                    if (a.id_stride == 1) {
                        w &= mq[m] >> (4 * half);
                    } else {                  // other strides: the bit of each such row, gathered (an indexed row: its bit lies below n_bits)
                        for (uint32_t t = w; t; t &= t - 1u) {
                            const int b = __ffs((int)t) - 1;
                            const int64_t bit = a.id_base + (row0 + lr0 + m * 32 + b) * a.id_stride;
                            if (!((qmask[bit >> 5] >> (unsigned)(bit & 31)) & 1u)) w &= ~(1u << b);
                        }
                    }
                    if (!FILL) cnt += __popc(w);
                }
                if (FILL) {
                    w <<= 4 * half;
                    w |= (uint32_t)__shfl_xor((int)w, 32);          // both halves now hold the block's 32 rows
                    if constexpr (MASKED) w &= mrow[m];
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

template <int WN, typename T, RangeFilter FILTER>
__global__ __launch_bounds__(512, 2) void dense_range_count_kernel(DenseRangeArgs a) { dense_range_body<false, WN, T, FILTER>(a); }
template <int WN, typename T, RangeFilter FILTER>
__global__ __launch_bounds__(512, 2) void dense_range_fill_kernel(DenseRangeArgs a) { dense_range_body<true, WN, T, FILTER>(a); }

template <bool FILL, int WN, typename T, RangeFilter FILTER>
static int launch_dense_range_t(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) {
    constexpr int TN = 128 * WN;
    constexpr size_t lds = sizeof(float) * 3 * (256 + TN) * (16 + 4) + (FILL ? (4 * (256 / 32 + 1) + 8) * (size_t)TN : 4 * (size_t)TN);
    static_assert(lds <= 160 * 1024, "one workgroup per CU");
    const void* fn = FILL ? reinterpret_cast<const void*>(&dense_range_fill_kernel<WN, T, FILTER>)
                          : reinterpret_cast<const void*>(&dense_range_count_kernel<WN, T, FILTER>);
    static DeviceOnce attr_once;
    SR_TRY(sr_allow_lds(attr_once, fn, (int)lds));
    dim3 grid((unsigned)ceil_div64(a.nq, TN), (unsigned)n_chunks_seg);
    if (FILL) hipLaunchKernelGGL((dense_range_fill_kernel<WN, T, FILTER>), grid, dim3(512), lds, s, a);
    else hipLaunchKernelGGL((dense_range_count_kernel<WN, T, FILTER>), grid, dim3(512), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
template <bool FILL, RangeFilter FILTER>
static int launch_dense_range_m(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) {
    const bool wide = dense_range_query_tile(a.nq) == 256;
    if (a.dtype == SR_DTYPE_F16)
        return wide ? launch_dense_range_t<FILL, 2, _Float16, FILTER>(a, n_chunks_seg, s) : launch_dense_range_t<FILL, 1, _Float16, FILTER>(a, n_chunks_seg, s);
    return wide ? launch_dense_range_t<FILL, 2, float, FILTER>(a, n_chunks_seg, s) : launch_dense_range_t<FILL, 1, float, FILTER>(a, n_chunks_seg, s);
}
