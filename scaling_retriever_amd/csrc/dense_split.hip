// Dense scoring in split-bf16 arithmetic: inner products of fp32 operands on the bf16 MFMA pipe.
//
// Every fp32 operand is split into bf16 planes, x = p0 + p1 (+ p2), each plane the bf16 rounding of what
// the previous ones left over (the subtractions are exact in fp32; a finite x keeps finite planes: p0 saturates
// instead of rounding to inf; three planes reproduce every |x| >= 2^-110 exactly):
//   bf16x3:  q . d ~= q0.d0 + q0.d1 + q1.d0
//   bf16x6:  q . d ~= q0.d0 + q0.d1 + q1.d0 + q1.d1 + q0.d2 + q2.d0
// Error per pair against the true inner product, derived in tests/dense_split_cases.py (S = sum_i |q_i d_i| <= |q||d|):
//   bf16x3:  dropped terms <= (2 + 2^-6) 2^-16 S (|x - p0 - p1| <= 2^-17 |x|; reached to 3 %: 1.95 x 2^-16 S when every rounding
//            points the same way), + the fp32 accumulation of 3 H exact products, <= 3.1 H 2^-24 S.  NOT the error class of an fp32
//            dot product: 2^-15 S worst case.  Gaussian data shows ~1e-6 |q||d| at H = 256 (the errors cancel).
//   bf16x6:  dropped terms <= (1 + 2^-6) 2^-24 S, + the accumulation of 6 H exact products, <= 6.2 H 2^-24 S: the error class of an
//            fp32 dot product.
//   (+ a floor of 2^-134 sum_i (|q_i| + |d_i|) where planes fall under bf16's smallest subnormal; inf / NaN inputs: unspecified.)
// Products of bf16 pairs are exact in fp32 and v_mfma_f32_16x16x32_bf16 accumulates in fp32.  The plane pairs are
// accumulated smallest first.  3 (6) bf16 MFMAs at the 2.5 PF bf16 rate replace one fp32 MFMA at 157 TF.
//
// Implementation: ONE GEMM with an n_pairs x longer k loop.  k-tile kt in [0, n_pairs * H/64): pair = kt / (H/64);
// the doc operand streams D plane pair_d[pair], the query operand Q plane pair_q[pair].  Tile 256 docs x 256
// queries, 8 waves, LDS-DMA staging with source-side swizzle and the 4-phase fragment pipeline of
// csrc/gemm_bf16.hip.  Docs sit on the accumulator registers and queries on the lanes, so the tau filter is
// lane-local and survivors are appended as 64-bit keys exactly as in dense_score.hip.
#include "dense_split_kernel.h"

// ---- fp32 -> bf16 planes ---------------------------------------------------------------------------
__global__ void split_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ p0, unsigned short* __restrict__ p1,
                                  unsigned short* __restrict__ p2, int64_t n4) {
    // grid-stride: a launch may not carry 2^32 or more threads (HIP), and 8 841 823 x 2048 / 4 elements is 4.5e9
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 v = reinterpret_cast<const f32x4*>(src)[i];
        bf16x4 a, b, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned short h = f32_to_bf16_sat(v[e]);  // a finite value keeps finite planes (common.h)
            const float r1 = v[e] - bf16_to_f32(h);          // exact
            const unsigned short m = f32_to_bf16(r1);
            const float r2 = r1 - bf16_to_f32(m);            // exact
            a[e] = (short)h;
            b[e] = (short)m;
            c[e] = (short)f32_to_bf16(r2);
        }
        reinterpret_cast<bf16x4*>(p0)[i] = a;
        if (p1) reinterpret_cast<bf16x4*>(p1)[i] = b;
        if (p2) reinterpret_cast<bf16x4*>(p2)[i] = c;
    }
}

int launch_split_bf16(const float* src, unsigned short* p0, unsigned short* p1, unsigned short* p2, int64_t n_elems, hipStream_t s) {
    const int64_t n4 = n_elems / 4;
    if (n4 == 0) return SR_OK;
    int64_t blocks = ceil_div64(n4, 256);
    if (blocks > (1 << 22)) blocks = 1 << 22;          // 2^30 threads per launch, the rest by the grid stride
    hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, p0, p1, p2, n4);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// The plane split on its own, exported for tests/test_dense_split_gpu.py: a thin call into launch_split_bf16 with the arguments
// split_segment (dense_index.hip) / dense_pass_16bit (dense_search.hip) fill.  Everything is validated before a device is touched.
extern "C" int sr_split_bf16(const float* d_src, int64_t n, void* d_p0, void* d_p1, void* d_p2, sr_stream stream) {
    SR_REQUIRE(d_src && d_p0, "sr_split_bf16: null pointer");
    SR_REQUIRE(n >= 0 && n % 4 == 0, "sr_split_bf16: bad size n=%lld (n must be a multiple of 4)", (long long)n);
    SR_REQUIRE((uintptr_t)d_src % 16 == 0 && (uintptr_t)d_p0 % 8 == 0 && (uintptr_t)d_p1 % 8 == 0 && (uintptr_t)d_p2 % 8 == 0,
               "sr_split_bf16: d_src must be 16-byte aligned, the planes 8-byte aligned");
    return launch_split_bf16(d_src, (unsigned short*)d_p0, (unsigned short*)d_p1, (unsigned short*)d_p2, n, (hipStream_t)stream);
}

// Tile slot -> (doc tile, query tile).  Workgroups are dealt to the 8 XCDs round-robin by their linear id, every XCD has its
// own 4 MB L2, and 256 workgroups are resident at a time (one per CU), 32 per XCD.  xcd_order: the 32 tiles an XCD works on
// together form a block of 8 doc tiles x 4 query tiles (12 operand tiles behind 32 output tiles - in query-tile-fastest
// linear order they touch ~9 doc tiles and most of the query tiles), blocks walked query-block fastest so that a doc tile is
// fetched from HBM once and the query planes stay in the Infinity Cache.  Without it: query tile fastest.  Workgroups are
// persistent: workgroup b takes slots b, b + G, b + 2G, ... (G a multiple of 8, so all its slots belong to its XCD).
struct SplitGrid { int qt, dt, bq, bd, nbq, total; };
static inline SplitGrid split_grid(int64_t rows, int nq, int xcd_order) {
    SplitGrid g;
    g.qt = (int)ceil_div64(nq, SP_BM);
    g.dt = (int)ceil_div64(rows, SP_BN);
    g.bq = !xcd_order ? 1 : (g.qt % 4 == 0 ? 4 : g.qt % 2 == 0 ? 2 : 1);
    g.bd = 32 / g.bq;
    g.nbq = g.qt / g.bq;
    g.total = !xcd_order ? g.qt * g.dt : (int)(ceil_div64((int64_t)g.nbq * ceil_div64(g.dt, g.bd) * 32, 256) * 256);
    return g;
}

int launch_dense_split(const DenseSplitArgs& a, hipStream_t s) {
    const int64_t rows = a.row_end - a.row_begin;
    if (rows <= 0) return SR_OK;
    SR_REQUIRE(a.H % 64 == 0, "dense_split: dim %d must be a multiple of 64", a.H);
    SR_REQUIRE(a.n_pairs >= 1 && a.n_pairs <= 6 && a.n_pairs * (a.H / 64) >= 2, "dense_split: bad plane-pair count %d", a.n_pairs);
    SR_REQUIRE(!a.upper_bound || (a.n_pairs == 1 && a.dxy && a.qa), "dense_split: the upper-bound pass is one plane product");
    SR_REQUIRE(!a.mask || a.upper_bound, "dense_split: a document mask goes with the upper-bound pass only");
    SR_REQUIRE(!a.mask_qoff || a.mask, "dense_split: per-query mask offsets without a mask");
    constexpr size_t lds = 2 * (size_t)(SP_BN + SP_BM) * 128 + SP_BN * 2 * sizeof(float) + SP_BM * 4 * sizeof(float) + SP_BM * sizeof(float);
    static DeviceOnce attr_once[2];
    SR_TRY(sr_allow_lds(attr_once[0], dense_split_kernel<false, false>, (int)lds));
    SR_TRY(sr_allow_lds(attr_once[1], dense_split_kernel<true, false>, (int)lds));
    DenseSplitArgs b = a;
    if (const char* e = sr_dev_getenv("SR_SPLIT_BLOCKTEST")) if (atoi(e) == 0) b.dxy_gmax = nullptr;     // A/B switch: every bound formed
    SR_REQUIRE(!b.dxy_gmax || a.row_begin % SP_BN == 0, "dense_split: the block test needs launches that start on a tile boundary");
    b.xcd_order = 1;
    if (const char* e = sr_dev_getenv("SR_SPLIT_XCD")) b.xcd_order = atoi(e);     // A/B switch
    b.diag = 0;
#ifdef SR_DIAG_BUILD        // wrong results by design: read only by a diagnostic build (make EXTRA=-DSR_DIAG_BUILD), never by the product .so
    if (const char* e = sr_dev_getenv("SR_SPLIT_DIAG")) b.diag = atoi(e);         // timing only
#endif
    b.stamps = nullptr;
#ifdef SR_DIAG_BUILD
    if (sr_dev_getenv("SR_SPLIT_STAMPS")) {
        static unsigned long long* d_st = nullptr;
        static int calls = 0;
        if (!d_st) { SR_CHECK_HIP(hipMalloc((void**)&d_st, 32)); SR_CHECK_HIP(hipMemset(d_st, 0, 32)); }
        if (++calls % 272 == 0) {
            unsigned long long h[4];
            SR_CHECK_HIP(hipMemcpy(h, d_st, 32, hipMemcpyDeviceToHost));
            if (h[3]) fprintf(stderr, "[split stamps] tiles %llu: k-loop %.2f us, epilogue issue %.2f us, drain wait %.2f us\n", h[3],
                              h[0] * 0.01 / h[3], h[1] * 0.01 / h[3], h[2] * 0.01 / h[3]);
            SR_CHECK_HIP(hipMemset(d_st, 0, 32));
        }
        b.stamps = d_st;
    }
#endif
    const SplitGrid sg = split_grid(rows, a.nq, b.xcd_order);
    b.grid_qt = sg.qt; b.grid_dt = sg.dt; b.grid_bq = sg.bq; b.grid_bd = sg.bd; b.grid_nbq = sg.nbq; b.grid_total = sg.total;
    // one persistent workgroup per CU (130 KB of LDS each); SR_SPLIT_PERSIST=0: one workgroup per tile slot (A/B)
    int wgs = sr_cu_count();
    wgs -= wgs % 8;
    if (wgs < 8) wgs = 8;
    if (const char* e = sr_dev_getenv("SR_SPLIT_PERSIST")) if (atoi(e) == 0) wgs = sg.total;
    const dim3 grid((unsigned)(sg.total < wgs ? sg.total : wgs));
    if (a.mask_qoff) return launch_dense_split_grouped(b, grid.x, lds, s); // dense_split_grouped.hip: a bitmap per query
    if (a.mask) return launch_dense_split_masked(b, grid.x, lds, s);       // dense_split_masked.hip: the instantiation of an object of its own
    if (a.upper_bound) hipLaunchKernelGGL((dense_split_kernel<true, false>), grid, dim3(512), lds, s, b);
    else hipLaunchKernelGGL((dense_split_kernel<false, false>), grid, dim3(512), lds, s, b);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
