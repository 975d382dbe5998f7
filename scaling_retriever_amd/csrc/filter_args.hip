// The one kernel of filter_args.h: a kernel cannot be inline in a header that four translation units include.
#include "filter_args.h"

__global__ void pad_rows_kernel(float* __restrict__ scores, int64_t* __restrict__ ids, int32_t* __restrict__ counts, int64_t nq, int64_t n,
                                float pad_score) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        scores[i] = pad_score;
        ids[i] = -1;
        if (counts && i < nq) counts[i] = 0;
    }
}

int launch_pad_rows(float* d_scores, int64_t* d_ids, int32_t* d_counts, int64_t nq, int k, float pad_score, hipStream_t s) {
    const int64_t n = nq * (int64_t)k;                    // k >= 1: n >= nq, the grid covers the counts too
    if (n <= 0) return SR_OK;
    const int64_t blocks = ceil_div64(n, 256) < 65536 ? ceil_div64(n, 256) : 65536;
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_scores, d_ids, d_counts, nq, n, pad_score);
    SR_CHECK_LAUNCH();
    SR_CHECK_HIP(hipStreamSynchronize(s));
    return SR_OK;
}
