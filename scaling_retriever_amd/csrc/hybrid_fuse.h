// Hybrid fusion (hybrid_fuse.hip): the set union of two candidate lists per query, and the ranking of a ragged candidate list by the
// fused score f32(f32(w_d * dense) + f32(w_s * sparse)) with the certificate of the exact hybrid search.
#pragma once
#include "common.h"

struct HybridStatus {                   // device words of a call: what the kernels found wrong (~0: nothing)
    unsigned long long first_bad_b;     // smallest flat position of list B whose sparse position maps to no dense document
    unsigned long long first_bad_a;     // smallest flat position of list A (or of the ranked list) that is outside the index
};

#define HF_THREADS 256
#define HF_EMPTY 0xffffffffu            // an unused slot of a sorted list: sorts behind every dense position

// exclusive prefix of v over the 256 threads of the workgroup (lw: 4 LDS words); total = the sum.  Two barriers.  Shared with
// topk_collapse.hip.
__device__ inline int hf_block_scan(int v, int* lw, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) lw[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += lw[w];
        total += lw[w];
    }
    __syncthreads();
    return base + incl - v;
}
