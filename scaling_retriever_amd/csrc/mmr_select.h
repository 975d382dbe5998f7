// What the two MMR kernels share (dense_mmr.hip, sparse_mmr.hip): the candidate cap, the order of a pick and its workgroup reduction,
// and the LDS-only barrier of a pick's inner steps.
#pragma once
#include "common.h"

#define MMR_MAX_N 1024                  // sr_mmr_max_candidates(): the candidates' state lives in LDS
#define MMR_MAX_WAVES 8

// a candidate's place in the order of a pick: larger ord first (sr_f2ord of rel or of v), then the smaller id, then the smaller position
struct MmrKey {
    uint32_t ord; int pos;              // pos < 0: no candidate
    int64_t id;
};
__device__ inline bool mmr_better(const MmrKey& a, const MmrKey& b) {
    if (a.pos < 0) return false;
    if (b.pos < 0) return true;
    if (a.ord != b.ord) return a.ord > b.ord;
    if (a.id != b.id) return a.id < b.id;
    return a.pos < b.pos;
}
// the best key of the workgroup, in every thread; red: one slot per wave.  Leaves a barrier behind the slots' last read.
__device__ inline MmrKey mmr_block_best(MmrKey mine, MmrKey* red, int nw) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        MmrKey o;
        o.ord = (uint32_t)__shfl_xor((int)mine.ord, off);
        o.pos = __shfl_xor(mine.pos, off);
        const int lo = __shfl_xor((int)(uint32_t)(mine.id & 0xffffffffll), off), hi = __shfl_xor((int)(mine.id >> 32), off);
        o.id = ((int64_t)hi << 32) | (int64_t)(uint32_t)lo;
        if (mmr_better(o, mine)) mine = o;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mine;
    __syncthreads();
    MmrKey best = red[0];
    for (int w = 1; w < nw; ++w) {
        const MmrKey o = red[w];
        if (mmr_better(o, best)) best = o;
    }
    __syncthreads();
    return best;
}

// A workgroup barrier that orders LDS alone.  __syncthreads() fences global memory as well and so waits for every load in flight -
// the next chunk's rows, fetched precisely to be in flight across the barriers of this chunk.  What the waves hand each other here
// (the tile, the picked row's chunk) lives in LDS; the rows are read-only.
__device__ inline void mmr_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
