// Per-row term budget of the sparse head: sr_sparse_compact_topm = sr_sparse_compact that keeps, per row of reps [B, V], only the
// max_terms largest non-zeros (value descending as fp32 numbers, ties to the LOWER column), columns ascending in the output.
// No reference counterpart (the reference keeps every non-zero, indexer.py:259-260 / :393-399); DESIGN.md section 4.12.
//
//   topm_select_kernel   one workgroup per row.  ONE pass over the row counts the non-zeros, bins their order-preserving keys by
//                        the top 11 bits and stages the keys in LDS; a row over budget then narrows the cut key T in two more
//                        radix steps (11 + 10 bits) over the staged keys - or, when the row has more non-zeros than the stage
//                        holds, over the row again (it is 513 KB at V = 128 256: an L2 hit).  Out: T, how many entries equal to
//                        T are kept, and the row's output length.
//   topm_scan_kernel     row lengths -> row_ptr.
//   topm_fill_kernel     one workgroup per row, strips of 1 024 columns in column order: keep = key > T, or key == T and fewer
//                        than `ties` equal keys came before it in the row; ballot prefixes inside a wave, four wave totals in LDS.
// Plain loads and stores, no MFMA: the job is two passes over HBM per row in the common case, the same as sr_sparse_compact.
#include "common.h"

#define TOPM_THREADS 256
#define TOPM_STAGE 7168          // staged keys per row (28 KB; with the 8 KB of bins four workgroups share a CU's 160 KB)
#define TOPM_BINS 2048           // 11-bit digit
#define TOPM_UNROLL 4            // 16-byte loads in flight per thread in the counting pass

// four consecutive columns from i (a multiple of 4); columns >= V read as 0.  VEC: V % 4 == 0 and a 16-byte aligned base, so
// the four are all inside or all outside the row and one 16-byte load fetches them
template <bool VEC>
__device__ inline f32x4 topm_load4(const float* __restrict__ row, int64_t i, int64_t V) {
    if (VEC) return i < V ? *reinterpret_cast<const f32x4*>(row + i) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = i + e < V ? row[i + e] : 0.f;
    return v;
}

// exclusive prefix of v over the workgroup's 256 threads (thread order); wtot: 4 ints of LDS, free again after the next barrier
__device__ inline int topm_block_excl(int v, int* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off); if (lane >= off) incl += o; }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int wb = 0;
    for (int w = 0; w < wave; ++w) wb += wtot[w];
    return wb + incl - v;
}

// The bin that holds the need-th largest key: bins are walked from the top; sel[0] = that bin, sel[1] = need minus the count of the
// bins above it (>= 1, <= the bin's count).  Requires 1 <= need <= the sum of the bins.  Ends with a barrier.
template <int NB>
__device__ inline void topm_find_bin(const int* hist, int need, int* wtot, int* sel) {
    constexpr int PER = NB / TOPM_THREADS;
    const int j0 = threadIdx.x * PER;
    int sum = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) sum += hist[NB - 1 - (j0 + e)];
    const int excl = topm_block_excl(sum, wtot);
    if (excl < need && need <= excl + sum) {          // exactly one thread
        int acc = excl;
        for (int e = 0; e < PER; ++e) {
            const int bin = NB - 1 - (j0 + e), c = hist[bin];
            if (acc + c >= need) { sel[0] = bin; sel[1] = need - acc; break; }
            acc += c;
        }
    }
    __syncthreads();
}

// one radix step over the row's candidates: bins[(key >> SHIFT) & (NB - 1)] += 1 for every candidate with key >> PSHIFT == prefix
template <bool VEC, int PSHIFT, int SHIFT, int NB>
__device__ inline void topm_bin_pass(const float* __restrict__ row, int64_t V, const uint32_t* stage, int nnz, uint32_t prefix, int* hist) {
    for (int i = threadIdx.x; i < TOPM_BINS; i += TOPM_THREADS) hist[i] = 0;
    __syncthreads();
    if (nnz <= TOPM_STAGE) {
        for (int i = threadIdx.x; i < nnz; i += TOPM_THREADS) {
            const uint32_t key = stage[i];
            if ((key >> PSHIFT) == prefix) atomicAdd(&hist[(key >> SHIFT) & (NB - 1)], 1);
        }
    } else {
        for (int64_t i = (int64_t)threadIdx.x * 4; i < V; i += TOPM_THREADS * 4) {
            const f32x4 v = topm_load4<VEC>(row, i, V);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t key = sr_f2ord(v[e]);
                if (v[e] != 0.f && (key >> PSHIFT) == prefix) atomicAdd(&hist[(key >> SHIFT) & (NB - 1)], 1);
            }
        }
    }
    __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(TOPM_THREADS) void topm_select_kernel(const float* __restrict__ reps, int64_t V, int m,
                                                                   uint32_t* __restrict__ row_thr, int32_t* __restrict__ row_ties,
                                                                   int64_t* __restrict__ row_cnt) {
    __shared__ uint32_t stage[TOPM_STAGE];
    __shared__ int hist[TOPM_BINS];
    __shared__ int wtot[4];
    __shared__ int sel[2];
    __shared__ int s_cnt;
    const int64_t b = blockIdx.x;
    const float* __restrict__ row = reps + b * V;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    for (int i = tid; i < TOPM_BINS; i += TOPM_THREADS) hist[i] = 0;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    // counting pass: non-zeros of the row, their top-digit bins, and the keys themselves while the stage has room (any order)
    for (int64_t s0 = 0; s0 < V; s0 += TOPM_THREADS * 4 * TOPM_UNROLL) {          // the same trip count in every thread
        f32x4 v[TOPM_UNROLL];
#pragma unroll
        for (int u = 0; u < TOPM_UNROLL; ++u) v[u] = topm_load4<VEC>(row, s0 + (int64_t)(u * TOPM_THREADS + tid) * 4, V);
#pragma unroll
        for (int u = 0; u < TOPM_UNROLL; ++u) {
            uint64_t mk[4];
            int total = 0, before = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                mk[e] = __ballot(v[u][e] != 0.f);
                total += __popcll(mk[e]);
                before += __popcll(mk[e] & below);
            }
            if (total == 0) continue;                                  // wave-uniform
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt, total);
            base = __shfl(base, 0);
            int p = base + before;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (v[u][e] != 0.f) {
                    const uint32_t key = sr_f2ord(v[u][e]);
                    if (p < TOPM_STAGE) stage[p] = key;
                    ++p;
                    atomicAdd(&hist[key >> 21], 1);
                }
            }
        }
    }
    __syncthreads();
    const int nnz = s_cnt;
    if (nnz <= m) {            // under budget: every candidate is kept (a finite non-zero has key > 0)
        if (tid == 0) { row_thr[b] = 0u; row_ties[b] = 0; row_cnt[b] = nnz; }
        return;
    }
    topm_find_bin<TOPM_BINS>(hist, m, wtot, sel);
    uint32_t prefix = (uint32_t)sel[0];
    int need = sel[1];
    topm_bin_pass<VEC, 21, 10, 2048>(row, V, stage, nnz, prefix, hist);
    topm_find_bin<2048>(hist, need, wtot, sel);
    prefix = (prefix << 11) | (uint32_t)sel[0];
    need = sel[1];
    topm_bin_pass<VEC, 10, 0, 1024>(row, V, stage, nnz, prefix, hist);
    topm_find_bin<1024>(hist, need, wtot, sel);
    if (tid == 0) { row_thr[b] = (prefix << 10) | (uint32_t)sel[0]; row_ties[b] = sel[1]; row_cnt[b] = m; }
}

// row_ptr[b] = sum of row_cnt[< b], row_ptr[B] = total; one workgroup, every thread a run of consecutive rows
__global__ __launch_bounds__(TOPM_THREADS) void topm_scan_kernel(const int64_t* __restrict__ row_cnt, int64_t B, int64_t* __restrict__ row_ptr) {
    __shared__ int64_t tsum[TOPM_THREADS];
    const int tid = threadIdx.x;
    const int64_t per = (B + TOPM_THREADS - 1) / TOPM_THREADS;
    const int64_t r0 = per * tid, r1 = r0 + per < B ? r0 + per : B;
    int64_t sum = 0;
    for (int64_t r = r0; r < r1; ++r) sum += row_cnt[r];
    tsum[tid] = sum;
    __syncthreads();
    int64_t run = 0;
    for (int t = 0; t < tid; ++t) run += tsum[t];
    for (int64_t r = r0; r < r1; ++r) { row_ptr[r] = run; run += row_cnt[r]; }
    if (tid == TOPM_THREADS - 1) row_ptr[B] = run;
}

template <bool VEC>
__global__ __launch_bounds__(TOPM_THREADS) void topm_fill_kernel(const float* __restrict__ reps, int64_t V, const int64_t* __restrict__ row_ptr,
                                                                 const uint32_t* __restrict__ row_thr, const int32_t* __restrict__ row_ties,
                                                                 int32_t* __restrict__ cols, float* __restrict__ vals, int64_t capacity) {
    __shared__ int ttot[4], ktot[4];
    const int64_t b = blockIdx.x;
    const float* __restrict__ row = reps + b * V;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t T = row_thr[b];
    const int ties = row_ties[b];
    int64_t out = row_ptr[b];          // next output slot of the row (the same in every thread)
    int tie_run = 0;                   // entries equal to T in the columns before this strip
    f32x4 nxt = topm_load4<VEC>(row, (int64_t)tid * 4, V);
    for (int64_t i0 = 0; i0 < V; i0 += TOPM_THREADS * 4) {
        const int64_t i = i0 + tid * 4;
        const f32x4 v = nxt;
        nxt = topm_load4<VEC>(row, i + TOPM_THREADS * 4, V);
        uint32_t key[4];
        bool keep[4];
        int my_tie = tie_run;          // rank of this thread's first tie among the row's ties, in column order
        if (ties > 0) {                // a pruned row (the same branch in every thread)
            int wt = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                key[e] = sr_f2ord(v[e]);
                const uint64_t mk = __ballot(v[e] != 0.f && key[e] == T);
                wt += __popcll(mk);
                my_tie += __popcll(mk & below);
            }
            if (lane == 0) ttot[wave] = wt;
            __syncthreads();
            for (int w = 0; w < 4; ++w) { if (w < wave) my_tie += ttot[w]; tie_run += ttot[w]; }
        }
        int wk = 0, p = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool nz = v[e] != 0.f;
            if (ties > 0) {
                const bool tie = nz && key[e] == T;
                keep[e] = nz && (key[e] > T || (tie && my_tie < ties));
                my_tie += tie ? 1 : 0;
            } else {
                keep[e] = nz;
            }
            const uint64_t mk = __ballot(keep[e]);
            wk += __popcll(mk);
            p += __popcll(mk & below);
        }
        if (lane == 0) ktot[wave] = wk;
        __syncthreads();               // also orders this strip's reads of ttot before the next strip's writes
        int64_t q = out + p;
        for (int w = 0; w < 4; ++w) { if (w < wave) q += ktot[w]; out += ktot[w]; }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (keep[e]) {
                if (q < capacity) { cols[q] = (int32_t)(i + e); vals[q] = v[e]; }
                ++q;
            }
        }
        if (ties == 0) __syncthreads();   // ktot is rewritten next strip: a pruned row has the ttot barrier in between
    }
}

template <bool VEC>
static int topm_launch(const float* d_reps, int64_t B, int64_t V, int m, int64_t* d_row_ptr, int32_t* d_cols, float* d_vals,
                       int64_t capacity, int64_t* h_nnz, uint32_t* d_thr, int32_t* d_ties, int64_t* d_cnt, hipStream_t s) {
    hipLaunchKernelGGL(topm_select_kernel<VEC>, dim3((unsigned)B), dim3(TOPM_THREADS), 0, s, d_reps, V, m, d_thr, d_ties, d_cnt);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(topm_scan_kernel, dim3(1), dim3(TOPM_THREADS), 0, s, d_cnt, B, d_row_ptr);
    SR_CHECK_LAUNCH();
    int64_t total = 0;
    SR_CHECK_HIP(hipMemcpyAsync(&total, d_row_ptr + B, 8, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    *h_nnz = total;
    if (total > capacity || (total > 0 && (!d_cols || !d_vals))) {
        sr_set_error("sr_sparse_compact_topm: %lld entries, capacity %lld", (long long)total, (long long)capacity);
        return SR_ERR_NOMEM;
    }
    if (total > 0) {
        hipLaunchKernelGGL(topm_fill_kernel<VEC>, dim3((unsigned)B), dim3(TOPM_THREADS), 0, s, d_reps, V, d_row_ptr, d_thr, d_ties,
                           d_cols, d_vals, capacity);
        SR_CHECK_LAUNCH();
        SR_CHECK_HIP(hipStreamSynchronize(s));      // the per-row scratch below is released on return
    }
    return SR_OK;
}

extern "C" int sr_sparse_compact_topm(const float* d_reps, int64_t B, int64_t V, int64_t max_terms, int64_t* d_row_ptr, int32_t* d_cols,
                                      float* d_vals, int64_t capacity, int64_t* h_nnz, sr_stream stream) {
    SR_REQUIRE(max_terms >= 0, "sr_sparse_compact_topm: max_terms %lld is negative (0 = no limit)", (long long)max_terms);
    if (max_terms == 0) return sr_sparse_compact(d_reps, B, V, d_row_ptr, d_cols, d_vals, capacity, h_nnz, stream);
    SR_REQUIRE(d_reps && d_row_ptr && h_nnz && B >= 0 && V > 0, "sr_sparse_compact_topm: bad argument");
    SR_REQUIRE(V <= 0x7fffffff && B <= 0x7fffffff, "sr_sparse_compact_topm: B or V beyond int32");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) { *h_nnz = 0; return SR_OK; }
    const int m = (int)(max_terms < V ? max_terms : V);
    char* d_tmp = nullptr;             // per row: kept length (8 B), cut key (4 B), kept ties (4 B)
    SR_CHECK_HIP(hipMalloc((void**)&d_tmp, (size_t)B * 16));
    int64_t* d_cnt = reinterpret_cast<int64_t*>(d_tmp);
    uint32_t* d_thr = reinterpret_cast<uint32_t*>(d_tmp + (size_t)B * 8);
    int32_t* d_ties = reinterpret_cast<int32_t*>(d_tmp + (size_t)B * 12);
    const bool vec = V % 4 == 0 && (reinterpret_cast<uintptr_t>(d_reps) & 15) == 0;
    const int rc = vec ? topm_launch<true>(d_reps, B, V, m, d_row_ptr, d_cols, d_vals, capacity, h_nnz, d_thr, d_ties, d_cnt, s)
                       : topm_launch<false>(d_reps, B, V, m, d_row_ptr, d_cols, d_vals, capacity, h_nnz, d_thr, d_ties, d_cnt, s);
    if (rc != SR_OK) (void)hipStreamSynchronize(s);
    (void)hipFree(d_tmp);
    return rc;
}
