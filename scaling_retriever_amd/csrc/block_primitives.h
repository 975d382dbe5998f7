// Workgroup primitives of the kernels that work on ranked lists (rank fusion, evaluation, feedback, hybrid search, the top-k sort,
// collapsed search, group hits): one bitonic sort, one scan, one min, one next-power-of-two.  Device inline code only.
#pragma once
#include "common.h"

// smallest power of two >= max(v, floor), floor itself a power of two (1 or 2 at every call site): the slots of a bitonic sort over
// v keys
__host__ __device__ inline int sr_pow2_at_least(int64_t v, int floor) {
    int p = floor;
    while (p < v) p <<= 1;
    return p;
}

// The compare-exchange network of a bitonic sort over P slots (a power of two >= 2) by a workgroup of THREADS threads:
// exchange(i, p, up) is called once per step for every pair i < p = i | j; up: the pair is to end with slot i <= slot p.  Thread t
// owns pairs t, t + THREADS, .. of a step's P / 2, so none idles and a change of THREADS leaves no pair without an owner.  One
// barrier per step, the last one behind the last step (P = 1, the one-slot list of hybrid_union_kernel: no step, no barrier).
template <int THREADS, bool DESC, typename F>
__device__ inline void sr_block_bitonic(int P, F exchange) {
    const int half = P >> 1;
    for (int size = 2; size <= P; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < half; t += THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                exchange(i, i | j, ((i & size) == 0) != DESC);
            }
            __syncthreads();
        }
}

// Bitonic sort of a[0, P), ascending or (DESC) descending; P a power of two >= 2.  a is LDS, or global memory that this workgroup
// alone touches (a workgroup's barriers order its global stores as they order its LDS stores).  The caller has a barrier behind its
// stores; the sort ends with a barrier.
template <int THREADS, bool DESC, typename T>
__device__ inline void sr_block_sort(T* a, int P) {
    sr_block_bitonic<THREADS, DESC>(P, [a](int i, int p, bool up) {
        const T x = a[i], y = a[p];
        if (up ? (x > y) : (x < y)) {
            a[i] = y;
            a[p] = x;
        }
    });
}

// the same over keys[0, P), every key's value carried along with it
template <int THREADS, bool DESC, typename K, typename V>
__device__ inline void sr_block_sort_kv(K* keys, V* vals, int P) {
    sr_block_bitonic<THREADS, DESC>(P, [keys, vals](int i, int p, bool up) {
        const K x = keys[i], y = keys[p];
        if (up ? (x > y) : (x < y)) {
            const V vx = vals[i], vy = vals[p];
            keys[i] = y; keys[p] = x;
            vals[i] = vy; vals[p] = vx;
        }
    });
}

// exclusive prefix of v over the 256 threads of the workgroup (lw: 4 LDS words); total = the sum.  Two barriers.
template <typename T>
__device__ inline T sr_block_scan(T v, T* lw, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) lw[wave] = incl;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += lw[w];
        total += lw[w];
    }
    __syncthreads();
    return base + incl - v;
}

// smallest v over the 256 threads of the workgroup (red: 4 LDS words).  Two barriers.
__device__ inline int sr_block_min(int v, int* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = red[w] < m ? red[w] : m;
    __syncthreads();
    return m;
}
