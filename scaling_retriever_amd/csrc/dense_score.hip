// Dense brute-force scoring Q . D^T with fused top-k filtering (gfx950).
//
// Replaces faiss.IndexFlatIP.search as used by DenseFlatIndexer.search_knn
// (scaling_retriever/indexer.py:191-217).  Exact fp32: products are accumulated
// by v_mfma_f32_32x32x2_f32 (f32 in / f32 acc), which is bit-for-bit a k-ordered
// fmaf chain.  Per 8-wide k group s the chain visits k = 8s+j (lane half 0) then
// 8s+4+j (half 1) for j = 0..3 - oracle/scoring.py::mfma_korder restates it.
//
// Layout: D row-major [N, H] fp32 in HBM (72.4 GB at N = 8 841 823, H = 2048),
// Q row-major [nq, H].  Docs are the MFMA A rows, queries the B columns, so in
// the accumulator a lane owns ONE query column (lane & 31) and 16 doc rows per
// 32x32 block: the tau compare is lane-local.  Scores never go to HBM; survivors
// (score >= tau[q]) are appended as 64-bit keys to the per-query candidate buffer
// (topk.hip).  A doc chunk = one launch; tau is raised between chunks (dense_search.hip).
// This file: the two kernels and their launch; the index handle is dense_index.hip's.
#include "dense_score.h"

// Row type T (common.h SrRow): float, or _Float16 for an index of fp16-stored rows - the doc tile is then fetched as 8-byte pieces
// (four halves per former 16-byte chunk) and widened to the f32x4 the stage write stores: LDS layout, MFMA loop and epilogue are the
// fp32 kernel's, and so is every result bit over the widened values.
// Tile = (32*WM*WAVES_M docs) x (32*WN*WAVES_N queries), 4 or 8 waves, BK = 16.
// 8 waves = 2 per SIMD: while one wave sits at the k-step barrier or waits for its LDS fragments,
// its SIMD partner keeps the (64-cycle) fp32 MFMA pipe busy.
template <typename T, int WAVES_M, int WAVES_N, int WM, int WN>
__global__ __launch_bounds__(64 * WAVES_M * WAVES_N, (WAVES_M * WAVES_N) / 4) void dense_score_kernel(DenseArgs a) {
    static_assert(WAVES_M * WAVES_N == 4 || WAVES_M * WAVES_N == 8, "4 or 8 waves per workgroup");
    constexpr int NT = 64 * WAVES_M * WAVES_N, BK = 16;
    constexpr int TM = 32 * WM * WAVES_M, TN = 32 * WN * WAVES_N, LDK = BK + 4, KC = BK / 4;
    constexpr int A_CHUNKS = TM * (BK / 4), B_CHUNKS = TN * (BK / 4);
    constexpr int A_PER_T = (A_CHUNKS + NT - 1) / NT, B_PER_T = (B_CHUNKS + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                  // [2][TM][LDK]
    float* Bs = smem + 2 * TM * LDK;   // [2][TN][LDK]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int64_t row0 = a.row_begin + (int64_t)blockIdx.x * TM;
    const int q0 = blockIdx.y * TN;
    const int H = a.H;

    const T* const D = static_cast<const T*>(a.D);
    f32x4 ra[A_PER_T], rb[B_PER_T];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < A_PER_T; ++i) {
            const int c = tid + i * NT;
            const int r = c / KC, kc = c % KC;
            const int64_t row = row0 + r;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c < A_CHUNKS && row < a.row_end) v = sr_load_row4<T>(D + row * H + k0 + kc * 4);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_PER_T; ++i) {
            const int c = tid + i * NT;
            const int r = c / KC, kc = c % KC;
            const int q = q0 + r;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c < B_CHUNKS && q < a.nq) v = *reinterpret_cast<const f32x4*>(a.Q + (int64_t)q * H + k0 + kc * 4);
            rb[i] = v;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_PER_T; ++i) {
            const int c = tid + i * NT;
            if (c < A_CHUNKS) *reinterpret_cast<f32x4*>(&As[(buf * TM + (c / KC)) * LDK + (c % KC) * 4]) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_PER_T; ++i) {
            const int c = tid + i * NT;
            if (c < B_CHUNKS) *reinterpret_cast<f32x4*>(&Bs[(buf * TN + (c / KC)) * LDK + (c % KC) * 4]) = rb[i];
        }
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    const int nk = H / BK;
    gload(0);
    sstore(0);
    __syncthreads();
    const int arow = wm * WM * 32 + (lane & 31);
    const int brow = wn * WN * 32 + (lane & 31);
    const int koff = 4 * (lane >> 5);
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gload((kt + 1) * BK);
#pragma unroll
        for (int s = 0; s < BK / 8; ++s) {
            f32x4 af[WM], bf[WN];
#pragma unroll
            for (int m = 0; m < WM; ++m)
                af[m] = *reinterpret_cast<const f32x4*>(&As[(buf * TM + arow + m * 32) * LDK + 8 * s + koff]);
#pragma unroll
            for (int n = 0; n < WN; ++n)
                bf[n] = *reinterpret_cast<const f32x4*>(&Bs[(buf * TN + brow + n * 32) * LDK + 8 * s + koff]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int m = 0; m < WM; ++m)
#pragma unroll
                    for (int n = 0; n < WN; ++n)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m][j], bf[n][j], acc[m][n], 0, 0, 0);
        }
        if (kt + 1 < nk) sstore(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: lane-local tau filter, append survivors -------------------
    const int half = lane >> 5;
    const int64_t left = a.row_end - row0;
    const int rows_valid = left < TM ? (int)left : TM;            // doc rows of this tile that exist
    const int lr0 = wm * WM * 32 + 4 * half;                      // local row of register 0 in block m = 0
    const uint32_t gid0 = a.id_base + (uint32_t)row0 * a.id_stride;
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int q = q0 + wn * WN * 32 + n * 32 + (lane & 31);
        if (q >= a.nq) continue;
        const float tq = a.tau[q];
        int cnt = 0;
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = lr0 + m * 32 + (r & 3) + 8 * (r >> 2);
                cnt += (lr < rows_valid && acc[m][n][r] >= tq) ? 1 : 0;
            }
        if (cnt == 0) continue;
        int pos = atomicAdd(&a.cand_count[q], cnt);
        uint64_t* dst = a.cand_keys + (int64_t)q * a.cand_cap;
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = lr0 + m * 32 + (r & 3) + 8 * (r >> 2);
                const float sc = acc[m][n][r];
                if (lr < rows_valid && sc >= tq) {
                    if (pos < a.cand_cap) dst[pos] = sr_make_key(sc, gid0 + (uint32_t)lr * a.id_stride);
                    ++pos;
                }
            }
    }
}

// ---- the same tile (256 docs x 256 queries, 8 waves, wave tile 128 x 64), software-pipelined ---------------------
// In dense_score_kernel every k-step ends  MFMAs -> ds_write -> barrier -> ds_read -> MFMAs: both waves of a SIMD belong
// to the same workgroup, reach the barrier together and then wait for their first fragments together, so the MFMA pipe
// drains once per k-step (rocprofv3 PMC: waves parked 14 % of their cycles, MFMA busy 84 %).  Here three LDS stages make
// the hand-offs a whole k-step old: during step kt the registers fetched two steps ahead are written to stage (kt + 2) % 3
// (last read in step kt - 1), and the first fragments of step kt + 1 are read - from a stage made visible by the
// PREVIOUS barrier - under the last MFMAs of step kt.  One barrier per k-step remains, with MFMAs issued right up to
// it and right after it.  Same k order per accumulator as dense_score_kernel: bit-identical scores.
// WN = 32-query blocks per wave: 2 -> 256 docs x 256 queries (wave tile 128 x 64), 1 -> 256 x 128 for 65-128 queries.
template <int WN, typename T>
__global__ __launch_bounds__(512, 2) void dense_score_pipe_kernel(DenseArgs a) {
    typedef typename SrRow<T>::V RowV;
    constexpr int WAVES_N = 4, WM = 4, BK = 16;
    constexpr int NT = 512, TM = 256, TN = 32 * WN * WAVES_N, LDK = BK + 4, KC = BK / 4, NSTAGE = 3;
    constexpr int PER_T = TM * KC / NT;                 // 16-B chunks per thread of the doc tile (= 2)
    constexpr int PER_TB = TN * KC / NT;                // ... of the query tile (2 or 1)
    constexpr int HALF_MFMAS = 4 * WM * WN;             // MFMAs per half k-step and wave
    constexpr int MPO = WN == 2 ? 2 : 1;                // MFMAs between two memory operations
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [NSTAGE][TM][LDK]
    float* Bs = smem + NSTAGE * TM * LDK;   // [NSTAGE][TN][LDK]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int64_t row0 = a.row_begin + (int64_t)blockIdx.x * TM;
    const int q0 = blockIdx.y * TN;
    const int H = a.H;

    // staging: thread t moves chunks t and t + 512 of each operand tile (row = chunk / 4, k-chunk = chunk % 4);
    // rows past the end are clamped (their scores are never emitted)
    const T* asrc[PER_T];
    const float* bsrc[PER_TB];
    int soff[PER_T];
#pragma unroll
    for (int i = 0; i < PER_T; ++i) {
        // chunk c -> (row r, k-chunk kc): the 8 lanes of a ds_write_b128 group take rows r and r + 4, whose 80-byte pitch
        // puts them 16 banks apart (rows r and r + 1 would overlap: 2-way conflicts on every stage write); a row is still
        // fetched as one 64-byte piece by 4 neighbouring lanes
        const int c = tid + i * NT, kc = c & 3, grp = c >> 3;
        const int r = (grp >> 2) * 8 + (grp & 3) + 4 * ((c >> 2) & 1);
        int64_t row = row0 + r;
        row = row < a.row_end ? row : a.row_end - 1;
        asrc[i] = static_cast<const T*>(a.D) + row * H + kc * 4;
        soff[i] = r * LDK + kc * 4;
        if (i < PER_TB) {
            int q = q0 + r;
            q = q < a.nq ? q : a.nq - 1;
            bsrc[i] = a.Q + (int64_t)q * H + kc * 4;
        }
    }
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

    f32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    const int aoff = (wm * WM * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
    const int boff = (wn * WN * 32 + (lane & 31)) * LDK + 4 * (lane >> 5);
    auto frag = [&](int st, int sub, f32x4 (&af)[WM], f32x4 (&bf)[WN]) {
#pragma unroll
        for (int m = 0; m < WM; ++m) af[m] = *reinterpret_cast<const f32x4*>(&As[st * TM * LDK + aoff + m * 32 * LDK + 8 * sub]);
#pragma unroll
        for (int n = 0; n < WN; ++n) bf[n] = *reinterpret_cast<const f32x4*>(&Bs[st * TN * LDK + boff + n * 32 * LDK + 8 * sub]);
    };
#define SR_DENSE_MFMAS(AF, BF)                                                                                   \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                \
        _Pragma("unroll") for (int m = 0; m < WM; ++m)                                                           \
            _Pragma("unroll") for (int n = 0; n < WN; ++n)                                                       \
                acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(AF[m][j], BF[n][j], acc[m][n], 0, 0, 0);

    const int nk = H / BK;
    {   // prologue: the first three k-steps' loads are all in flight before the first stage is written (one memory
        // latency instead of three)
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
    for (int kt = 0; kt < nk; ++kt) {
        const int st1 = st == NSTAGE - 1 ? 0 : st + 1;
        const int st2 = st1 == NSTAGE - 1 ? 0 : st1 + 1;
        // branch-free body (a branch makes hipcc wait for ALL outstanding LDS reads at the join): past the last k-steps
        // the extra stage writes / fragment reads / re-loads of the last k-block touch valid memory and are never used
        // Issue order inside a half (sched_group_barrier): the half's MFMAs start at once and its LDS / global operations are
        // dealt out between them, two MFMAs (128 cycles of pipe time) apart, so nothing queues up in front of the MFMA pipe
        // after the barrier.  First half: fragment reads of the second half, stage write of k-step kt + 2, global loads of
        // k-step kt + 3 (a whole k-step ahead of the write that consumes them).  Second half: first fragments of k-step kt + 1.
        frag(st, 1, a1, b1);
        sstore(st2);
        gload(kt + 3 < nk ? (kt + 3) * BK : H - BK);
        SR_DENSE_MFMAS(a0, b0)
#pragma unroll
        for (int i = 0; i < WM + WN; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, MPO, 0);  // MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);    // 1 DS read
        }
#pragma unroll
        for (int i = 0; i < PER_T + PER_TB; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, MPO, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);    // 1 DS write
        }
#pragma unroll
        for (int i = 0; i < PER_T + PER_TB; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, MPO, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // 1 VMEM read
        }
        __builtin_amdgcn_sched_group_barrier(0x008, HALF_MFMAS - MPO * (WM + WN + 2 * (PER_T + PER_TB)), 0);
        __builtin_amdgcn_sched_barrier(0);
        frag(st1, 0, a0, b0);
        SR_DENSE_MFMAS(a1, b1)
#pragma unroll
        for (int i = 0; i < WM + WN; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, MPO, 1);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, HALF_MFMAS - MPO * (WM + WN), 1);
        __builtin_amdgcn_sched_barrier(0);      // the barrier (and its lgkmcnt(0)) after the MFMAs that cover the reads
        __syncthreads();
        st = st1;
    }
#undef SR_DENSE_MFMAS

    // ---- epilogue: lane-local tau filter, append survivors (as dense_score_kernel) -------------------
    const int half = lane >> 5;
    const int64_t left = a.row_end - row0;
    const int rows_valid = left < TM ? (int)left : TM;
    const int lr0 = wm * WM * 32 + 4 * half;
    const uint32_t gid0 = a.id_base + (uint32_t)row0 * a.id_stride;
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int q = q0 + wn * WN * 32 + n * 32 + (lane & 31);
        if (q >= a.nq) continue;
        const float tq = a.tau[q];
        int cnt = 0;
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = lr0 + m * 32 + (r & 3) + 8 * (r >> 2);
                cnt += (lr < rows_valid && acc[m][n][r] >= tq) ? 1 : 0;
            }
        if (cnt == 0) continue;
        int pos = atomicAdd(&a.cand_count[q], cnt);
        uint64_t* dst = a.cand_keys + (int64_t)q * a.cand_cap;
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = lr0 + m * 32 + (r & 3) + 8 * (r >> 2);
                const float sc = acc[m][n][r];
                if (lr < rows_valid && sc >= tq) {
                    if (pos < a.cand_cap) dst[pos] = sr_make_key(sc, gid0 + (uint32_t)lr * a.id_stride);
                    ++pos;
                }
            }
    }
}

template <int WN, typename T>
static int launch_dense_pipe_t(const DenseArgs& a, int64_t rows, hipStream_t s) {
    constexpr int TN = 128 * WN;
    constexpr size_t lds = sizeof(float) * 3 * (256 + TN) * (16 + 4);
    static DeviceOnce attr_once;
    SR_TRY(sr_allow_lds(attr_once, dense_score_pipe_kernel<WN, T>, (int)lds));
    dim3 grid((unsigned)ceil_div64(rows, 256), (unsigned)ceil_div64(a.nq, TN));
    hipLaunchKernelGGL((dense_score_pipe_kernel<WN, T>), grid, dim3(512), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
template <int WN>
static int launch_dense_pipe(const DenseArgs& a, int64_t rows, hipStream_t s) {
    return a.dtype == SR_DTYPE_F16 ? launch_dense_pipe_t<WN, _Float16>(a, rows, s) : launch_dense_pipe_t<WN, float>(a, rows, s);
}

template <typename T, int WAVES_M, int WAVES_N, int WM, int WN>
static int launch_dense_t(const DenseArgs& a, int64_t rows, hipStream_t s) {
    constexpr int TM = 32 * WM * WAVES_M, TN = 32 * WN * WAVES_N;
    constexpr size_t lds = sizeof(float) * 2 * (TM + TN) * (16 + 4);
    static DeviceOnce attr_once;
    SR_TRY(sr_allow_lds(attr_once, dense_score_kernel<T, WAVES_M, WAVES_N, WM, WN>, (int)lds));
    dim3 grid((unsigned)ceil_div64(rows, TM), (unsigned)ceil_div64(a.nq, TN));
    hipLaunchKernelGGL((dense_score_kernel<T, WAVES_M, WAVES_N, WM, WN>), grid, dim3(64 * WAVES_M * WAVES_N), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
template <int WAVES_M, int WAVES_N, int WM, int WN>
static int launch_dense(const DenseArgs& a, int64_t rows, hipStream_t s) {
    return a.dtype == SR_DTYPE_F16 ? launch_dense_t<_Float16, WAVES_M, WAVES_N, WM, WN>(a, rows, s)
                                   : launch_dense_t<float, WAVES_M, WAVES_N, WM, WN>(a, rows, s);
}

// tile config by query count: every tile is 256 docs x dense_query_tile(nq) queries
int launch_dense_exact(const DenseArgs& a, int64_t rows, bool plain, hipStream_t s) {
    switch (dense_query_tile(a.nq)) {
        case 256: return plain ? launch_dense<2, 4, 4, 2>(a, rows, s) : launch_dense_pipe<2>(a, rows, s);
        case 128: return plain ? launch_dense<2, 2, 4, 2>(a, rows, s) : launch_dense_pipe<1>(a, rows, s);
        case 64: return launch_dense<4, 1, 2, 2>(a, rows, s);
        default: return launch_dense<4, 1, 2, 1>(a, rows, s);
    }
}

