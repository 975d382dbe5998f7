// fp16-plane regime of the encoder (cfg.fp32_planes == SR_FP32_PLANES_F16): rows scaled by a power of two and split into two fp16 planes,
// and the gate/up bound that fixes the scale of a SwiGLU output row before its GEMM runs.  Weights are split by model_weights.hip.
#include "kernels.h"
#include <math.h>

// activations: one wave per row of src fp32 [T, K] -> [f1 | f0 | f0] (split_map_a; nseg = 3) or [f1 | f0] (nseg = 2: the consumer's
// weights have an all-zero g1 segment) + a_inv[t]; with w: the RMSNorm of the row
// first (x = embed[tok] if embed; y = (x * rsqrt(mean(x^2) + eps)) * w), i.e. rmsnorm_split_kernel on fp16 planes
__global__ __launch_bounds__(256) void rows_split_h_kernel(float* __restrict__ x, const float* __restrict__ embed,
                                                           const int* __restrict__ tok_id, const float* __restrict__ w,
                                                           bf16_t* __restrict__ xs, float* __restrict__ a_inv, int T, int K, float eps,
                                                           const float* __restrict__ gu_cmax, float* __restrict__ act_sc,
                                                           float* __restrict__ act_inv, int nseg) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float* xr = x + (int64_t)t * K;
    const float* src = embed ? embed + (int64_t)tok_id[t] * K : xr;
    float rs = 1.f;
    if (w) {
        float ss = 0.f;
        for (int i = lane * 4; i < K; i += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
            ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
            if (embed) *reinterpret_cast<f32x4*>(xr + i) = v;
        }
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
        rs = 1.0f / sqrtf(ss / (float)K + eps);
    }
    float mx = 0.f, s2 = 0.f;
    for (int i = lane * 4; i < K; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
        f32x4 g = {1.f, 1.f, 1.f, 1.f};
        if (w) g = *reinterpret_cast<const f32x4*>(w + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float y = w ? (v[c] * rs) * g[c] : v[c];
            mx = fmaxf(mx, fabsf(y));
            s2 += y * y;
        }
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float sc = row_scale_pow2(mx);
    if (lane == 0) a_inv[t] = 1.0f / sc;
    if (gu_cmax) {                              // see rows_split_h_reg_kernel
        for (int off = 32; off > 0; off >>= 1) s2 += __shfl_xor(s2, off);
        const float osc = row_scale_pow2(s2 * *gu_cmax * 1.02f);
        if (lane == 0) { act_sc[t] = osc; act_inv[t] = 1.0f / osc; }
    }
    bf16_t* orow = xs + (int64_t)t * K * nseg;
    for (int i = lane * 4; i < K; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
        f32x4 g = {1.f, 1.f, 1.f, 1.f};
        if (w) g = *reinterpret_cast<const f32x4*>(w + i);
        bf16x4 p0, p1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            unsigned short f0, f1;
            split_f16x2((w ? (v[c] * rs) * g[c] : v[c]) * sc, f0, f1);
            p0[c] = (short)f0; p1[c] = (short)f1;
        }
        *reinterpret_cast<bf16x4*>(orow + i) = p1;
        *reinterpret_cast<bf16x4*>(orow + K + i) = p0;
        if (nseg == 3) *reinterpret_cast<bf16x4*>(orow + 2 * K + i) = p0;
    }
}

// The same with the row held in registers between the passes (NV float4 per lane, K = 256 NV): one read of the row instead of
// up to three (sum of squares, maximum, split) - the row-split passes were 10 % of a fp32-regime query encode.
template <int NV>
__global__ __launch_bounds__(256) void rows_split_h_reg_kernel(float* __restrict__ x, const float* __restrict__ embed,
                                                               const int* __restrict__ tok_id, const float* __restrict__ w,
                                                               bf16_t* __restrict__ xs, float* __restrict__ a_inv, int T, float eps,
                                                               const float* __restrict__ gu_cmax, float* __restrict__ act_sc,
                                                               float* __restrict__ act_inv, int nseg) {
    constexpr int K = 256 * NV;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float* xr = x + (int64_t)t * K;
    const float* src = embed ? embed + (int64_t)tok_id[t] * K : xr;
    f32x4 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = *reinterpret_cast<const f32x4*>(src + lane * 4 + 256 * j);
    if (w) {
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            ss += v[j][0] * v[j][0] + v[j][1] * v[j][1] + v[j][2] * v[j][2] + v[j][3] * v[j][3];
            if (embed) *reinterpret_cast<f32x4*>(xr + lane * 4 + 256 * j) = v[j];
        }
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
        const float rs = 1.0f / sqrtf(ss / (float)K + eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(w + lane * 4 + 256 * j);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[j][c] = (v[j][c] * rs) * g[c];
        }
    }
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) mx = fmaxf(mx, fabsf(v[j][c]));
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float sc = row_scale_pow2(mx);
    if (lane == 0) a_inv[t] = 1.0f / sc;
    if (gu_cmax) {
        // scale of this row's SwiGLU output, known before the gate-up GEMM runs: |silu(g_j) u_j| <= |g_j||u_j| <=
        // |xn|^2 |wg_j||wu_j| <= |xn|^2 cmax (Cauchy-Schwarz; 1.02: the fp32 evaluation of the norms) - EPI_SWIGLU_SPLIT_H
        float s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) s2 += v[j][0] * v[j][0] + v[j][1] * v[j][1] + v[j][2] * v[j][2] + v[j][3] * v[j][3];
        for (int off = 32; off > 0; off >>= 1) s2 += __shfl_xor(s2, off);
        const float osc = row_scale_pow2(s2 * *gu_cmax * 1.02f);
        if (lane == 0) { act_sc[t] = osc; act_inv[t] = 1.0f / osc; }
    }
    bf16_t* orow = xs + (int64_t)t * K * nseg;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        bf16x4 p0, p1;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            unsigned short f0, f1;
            split_f16x2(v[j][c] * sc, f0, f1);
            p0[c] = (short)f0; p1[c] = (short)f1;
        }
        const int i = lane * 4 + 256 * j;
        *reinterpret_cast<bf16x4*>(orow + i) = p1;
        *reinterpret_cast<bf16x4*>(orow + K + i) = p0;
        if (nseg == 3) *reinterpret_cast<bf16x4*>(orow + 2 * K + i) = p0;
    }
}

// nseg: the segment count of the consuming GEMM's weights (2 or 3); gu_cmax (device float) / act_sc / act_inv: the row scales of
// the SwiGLU output this row will produce, or all null
int launch_rows_split_f16(float* x, const float* embed, const int* tok, const float* w, bf16_t* xs, float* inv, int T, int K, float eps,
                          int nseg, const float* gu_cmax, float* act_sc, float* act_inv, hipStream_t s) {
    const dim3 grid((unsigned)ceil_div64(T, 4)), block(256);
    switch (K) {
        case 2048: hipLaunchKernelGGL(rows_split_h_reg_kernel<8>, grid, block, 0, s, x, embed, tok, w, xs, inv, T, eps, gu_cmax, act_sc, act_inv, nseg); break;
        case 4096: hipLaunchKernelGGL(rows_split_h_reg_kernel<16>, grid, block, 0, s, x, embed, tok, w, xs, inv, T, eps, gu_cmax, act_sc, act_inv, nseg); break;
        case 8192: hipLaunchKernelGGL(rows_split_h_reg_kernel<32>, grid, block, 0, s, x, embed, tok, w, xs, inv, T, eps, gu_cmax, act_sc, act_inv, nseg); break;
        default: hipLaunchKernelGGL(rows_split_h_kernel, grid, block, 0, s, x, embed, tok, w, xs, inv, T, K, eps, gu_cmax, act_sc, act_inv, nseg);
    }
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// max over the MLP's feature pairs j of |w_gate_j| |w_up_j|, from the fp16 plane segments [w0 | w1 | w0] (nseg = 3) or [w0 | w0]
// (nseg = 2, w1 = 0) of the interleaved gate/up matrix (gate rows and up rows alternate in 16-row blocks) and the rows' inverse
// scales: one wave per pair
__global__ __launch_bounds__(256) void gu_cmax_kernel(const bf16_t* __restrict__ wgu_s, const float* __restrict__ wgu_i, int I, int K,
                                                      int nseg, float* __restrict__ cmax) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= I) return;
    const int64_t rg = (int64_t)(j / 16) * 32 + (j % 16), ru = rg + 16;
    float n2[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bf16_t* row = wgu_s + (h ? ru : rg) * nseg * (int64_t)K;
        float ss = 0.f;
        for (int i = lane; i < K; i += 64) {
            const float v = (float)__builtin_bit_cast(_Float16, row[i]) +
                            (nseg == 3 ? (float)__builtin_bit_cast(_Float16, row[K + i]) : 0.f);
            ss += v * v;
        }
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
        const float inv = wgu_i[h ? ru : rg];
        n2[h] = ss * inv * inv;
    }
    if (lane == 0) atomicMax(reinterpret_cast<unsigned int*>(cmax), __float_as_uint(sqrtf(n2[0]) * sqrtf(n2[1]) * 1.001f));
}

int launch_gu_cmax(const bf16_t* wgu_s, const float* wgu_i, int I, int K, int nseg, float* cmax, hipStream_t s) {
    SR_CHECK_HIP(hipMemsetAsync(cmax, 0, 4, s));
    hipLaunchKernelGGL(gu_cmax_kernel, dim3((unsigned)ceil_div64(I, 4)), dim3(256), 0, s, wgu_s, wgu_i, I, K, nseg, cmax);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// p[k] = what gu_cmax_kernel gives for the single pair j = k I / ns, k < ns: a sample of the p_j = |w_gate_j||w_up_j| whose median
// sr_model_finalize compares with their maximum.  One launch per pair on its own two rows (I = 1 at the pair's row of its 32-row block).
int launch_gu_pair_samples(const bf16_t* wgu_s, const float* wgu_i, int I, int K, int nseg, int ns, float* p, hipStream_t s) {
    SR_CHECK_HIP(hipMemsetAsync(p, 0, (size_t)ns * 4, s));
    for (int k = 0; k < ns; ++k) {
        const int64_t j = (int64_t)k * I / ns, row = (j / 16) * 32 + j % 16;
        hipLaunchKernelGGL(gu_cmax_kernel, dim3(1), dim3(256), 0, s, wgu_s + row * nseg * K, wgu_i + row, 1, K, nseg, p + k);
    }
    SR_CHECK_LAUNCH();
    return SR_OK;
}
