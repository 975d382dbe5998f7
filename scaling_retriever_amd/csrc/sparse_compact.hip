// sr_sparse_compact: dense sparse-head rows [B, V] -> CSR.  sr_sparse_compact_topm (sparse_prune.hip) is the same under a per-row term
// budget and calls this one when there is none.
#include "kernels.h"

// ---- sparse reps -> CSR (torch.nonzero order: row-major, cols ascending) ----------------
__global__ __launch_bounds__(256) void nnz_count_kernel(const float* __restrict__ reps, int64_t V, int64_t* __restrict__ row_nnz) {
    __shared__ int red[4];
    const int64_t b = blockIdx.x;
    int c = 0;
    for (int64_t i = threadIdx.x; i < V; i += 256) c += reps[b * V + i] != 0.f ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) row_nnz[b] = red[0] + red[1] + red[2] + red[3];
}
__global__ void nnz_scan_kernel(const int64_t* __restrict__ row_nnz, int64_t B, int64_t* __restrict__ row_ptr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int64_t run = 0;
        for (int64_t b = 0; b < B; ++b) { row_ptr[b] = run; run += row_nnz[b]; }
        row_ptr[B] = run;
    }
}
__global__ __launch_bounds__(256) void nnz_fill_kernel(const float* __restrict__ reps, int64_t V, const int64_t* __restrict__ row_ptr,
                                                       int32_t* __restrict__ cols, float* __restrict__ vals, int64_t capacity) {
    __shared__ int wtot[4];
    __shared__ int64_t base;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = row_ptr[b];
    __syncthreads();
    for (int64_t i0 = 0; i0 < V; i0 += 256) {
        const int64_t i = i0 + tid;
        const float v = i < V ? reps[b * V + i] : 0.f;
        const int nz = v != 0.f ? 1 : 0;
        int incl = nz;
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off); if (lane >= off) incl += o; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int wb = 0, tot = 0;
        for (int w = 0; w < 4; ++w) { if (w < wave) wb += wtot[w]; tot += wtot[w]; }
        const int64_t p = base + wb + incl - nz;
        if (nz && p < capacity) { cols[p] = (int32_t)i; vals[p] = v; }
        __syncthreads();
        if (tid == 0) base += tot;
        __syncthreads();
    }
}

extern "C" int sr_sparse_compact(const float* d_reps, int64_t B, int64_t V, int64_t* d_row_ptr, int32_t* d_cols, float* d_vals,
                                 int64_t capacity, int64_t* h_nnz, sr_stream stream) {
    SR_REQUIRE(d_reps && d_row_ptr && h_nnz && B >= 0 && V > 0, "sr_sparse_compact: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) { *h_nnz = 0; return SR_OK; }
    CallBuf<int64_t> d_cnt;        // per-row counts: read by the scan, which the copy of the total below waits for
    SR_TRY(d_cnt.reserve(B, "sr_sparse_compact"));
    hipLaunchKernelGGL(nnz_count_kernel, dim3((unsigned)B), dim3(256), 0, s, d_reps, V, d_cnt.p);
    hipLaunchKernelGGL(nnz_scan_kernel, dim3(1), dim3(64), 0, s, d_cnt.p, B, d_row_ptr);
    int64_t total = 0;
    SR_CHECK_HIP(hipMemcpyAsync(&total, d_row_ptr + B, 8, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    *h_nnz = total;
    if (total > capacity || (total > 0 && (!d_cols || !d_vals))) {
        sr_set_error("sr_sparse_compact: %lld non-zeros, capacity %lld", (long long)total, (long long)capacity);
        return SR_ERR_NOMEM;
    }
    if (total > 0) {
        hipLaunchKernelGGL(nnz_fill_kernel, dim3((unsigned)B), dim3(256), 0, s, d_reps, V, d_row_ptr, d_cols, d_vals, capacity);
        SR_CHECK_LAUNCH();
    }
    return SR_OK;
}
