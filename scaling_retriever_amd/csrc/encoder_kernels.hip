// Small kernels of the encoder and their launch functions (kernels.h): the packing plan, RMSNorm of the bf16 regime and of the bf16-plane
// fp32 regime, the dense head and the sparse head's finish.  The layer loop that launches them: encoder.hip.
#include "kernels.h"
#include <math.h>

// ---- plan: per-row span ------------------------------------------------------
// mode 0 (dense) and 2 (both heads): span = [min(first1, L - len), L); pool_start = L - len (0 if len == 0)
// mode 1 (sparse): span = [first1, last1 + 1)
// row_shift (nullable, sr_encode_rows): row b sits row_shift[b] columns further right than in the batch it came from; positions
// (RoPE, pooling) are counted from there, so the row gets the position_ids it had in its own batch.
__global__ void plan_rows_kernel(const int64_t* __restrict__ mask, int B, int L, int mode, int* __restrict__ span_start,
                                 int* __restrict__ span_len, int* __restrict__ pool_start, int* __restrict__ row_len,
                                 const int* __restrict__ row_shift) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;  // 64 threads
    int len = 0, first = L, last = -1;
    for (int p = lane; p < L; p += 64) {
        if (mask[(int64_t)b * L + p] != 0) {
            ++len;
            first = p < first ? p : first;
            last = p > last ? p : last;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        len += __shfl_xor(len, off);
        const int f = __shfl_xor(first, off), l = __shfl_xor(last, off);
        first = f < first ? f : first;
        last = l > last ? l : last;
    }
    if (lane == 0) {
        int st, ln, ps;
        if (len == 0) {
            st = 0; ln = 0; ps = 0;
        } else if (mode != 1) {
            ps = L - len;
            st = first < ps ? first : ps;
            ln = L - st;
        } else {
            ps = first;
            st = first;
            ln = last + 1 - first;
        }
        span_start[b] = st;
        span_len[b] = ln;
        pool_start[b] = ps - (row_shift ? row_shift[b] : 0);     // compared with pos[], which carries the same shift
        row_len[b] = len;
    }
}

// exclusive scan of span_len -> cu_seqlens[B+1] (single workgroup, B <= 65536)
__global__ void plan_scan_kernel(const int* __restrict__ span_len, int B, int* __restrict__ cu) {
    __shared__ int part[256];
    const int tid = threadIdx.x;
    const int per = (B + 255) / 256;
    const int b0 = tid * per, b1 = (b0 + per) < B ? (b0 + per) : B;
    int s = 0;
    for (int b = b0; b < b1; ++b) s += span_len[b];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        cu[B] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int b = b0; b < b1; ++b) { cu[b] = run; run += span_len[b]; }
}

// per packed token: source position, token id, key flag, sequence id
__global__ void plan_tokens_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ mask, int L,
                                   const int* __restrict__ span_start, const int* __restrict__ cu, int* __restrict__ tok_id,
                                   int* __restrict__ pos, unsigned char* __restrict__ key_valid, int* __restrict__ seq_of,
                                   int vocab, int mode, const int* __restrict__ row_shift) {
    const int b = blockIdx.x;
    const int t0 = cu[b], n = cu[b + 1] - t0, st = span_start[b];
    const int shift = row_shift ? row_shift[b] : 0;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int p = st + j;
        int64_t id = ids[(int64_t)b * L + p];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);  // clamp (HF would raise an index error)
        tok_id[t0 + j] = (int)id;
        pos[t0 + j] = p - shift < 0 ? 0 : p - shift;     // a shift beyond the row's span start is a caller error: stay in the tables
        const bool valid = mask[(int64_t)b * L + p] != 0;
        key_valid[t0 + j] = valid ? 1 : 0;
        // sparse head: masked positions inside the span take no part in the max (-2 = skip row)
        seq_of[t0 + j] = (mode != 0 && !valid) ? -2 : b;
    }
}

// the plan's launches, shared by model_forward and the test hook sr_encode_plan (api.hip): spans + cu_seqlens, then - once the
// caller has read cu[B] and knows that the packed tokens fit - the per-token arrays
int launch_plan_rows(const int64_t* mask, int B, int L, int mode, int* span_start, int* span_len, int* pool_start, int* row_len,
                     const int* row_shift, int* cu, hipStream_t s) {
    hipLaunchKernelGGL(plan_rows_kernel, dim3(B), dim3(64), 0, s, mask, B, L, mode, span_start, span_len, pool_start, row_len, row_shift);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(256), 0, s, span_len, B, cu);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
int launch_plan_tokens(const int64_t* ids, const int64_t* mask, int B, int L, const int* span_start, const int* cu, int* tok_id, int* pos,
                       unsigned char* key_valid, int* seq_of, int vocab, int mode, const int* row_shift, hipStream_t s) {
    hipLaunchKernelGGL(plan_tokens_kernel, dim3(B), dim3(128), 0, s, ids, mask, L, span_start, cu, tok_id, pos, key_valid, seq_of, vocab,
                       mode, row_shift);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// ---- RMSNorm (fp32 variance) : one wave per token, optional embedding gather / pending residual -----
// x[t] = embed[tok_id[t]]            (if embed)
// x[t] += delta[t]                   (if delta: the bf16 output of the previous o_proj / down_proj GEMM - under the
//                                     reference's autocast nn.Linear returns bf16, which is then added to the fp32
//                                     residual stream; doing the add here keeps the GEMM epilogue at 2 B per element)
// xn[t] = bf16( x * rsqrt(mean(x^2) + eps) * w )
// NCH > 0: H == 256 * NCH and the row stays in registers between the two passes (all its loads in flight at once, no
// re-read of the freshly written row); NCH == 0: any H % 4 == 0, second pass re-reads the row.  Same arithmetic order.
template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_kernel(float* __restrict__ x, const float* __restrict__ embed,
                                                      const int* __restrict__ tok_id, const bf16_t* __restrict__ delta,
                                                      const float* __restrict__ w, bf16_t* __restrict__ xn,
                                                      float* __restrict__ xn_f32, int T, int H, float eps) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float* xr = x + (int64_t)t * H;
    const float* src = embed ? embed + (int64_t)tok_id[t] * H : xr;
    const bf16_t* dr = delta ? delta + (int64_t)t * H : nullptr;
    float ss = 0.f;
    if constexpr (NCH > 0) {
        f32x4 v[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = *reinterpret_cast<const f32x4*>(src + lane * 4 + c * 256);
        if (dr) {
            bf16x4 d[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) d[c] = *reinterpret_cast<const bf16x4*>(dr + lane * 4 + c * 256);
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[c][e] += bf16_to_f32((unsigned short)d[c][e]);
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            ss += v[c][0] * v[c][0] + v[c][1] * v[c][1] + v[c][2] * v[c][2] + v[c][3] * v[c][3];
            if (embed || dr) *reinterpret_cast<f32x4*>(xr + lane * 4 + c * 256) = v[c];
        }
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
        const float rs = 1.0f / sqrtf(ss / (float)H + eps);
        if (!w) return;   // residual add only
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int i = lane * 4 + c * 256;
            const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (v[c][e] * rs) * g[e];
            if (xn) {
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (short)f32_to_bf16(y[e]);
                *reinterpret_cast<bf16x4*>(xn + (int64_t)t * H + i) = o;
            }
            if (xn_f32) *reinterpret_cast<f32x4*>(xn_f32 + (int64_t)t * H + i) = y;
        }
    } else {
        for (int i = lane * 4; i < H; i += 256) {
            f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
            if (dr) {
                const bf16x4 d = *reinterpret_cast<const bf16x4*>(dr + i);
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] += bf16_to_f32((unsigned short)d[c]);
            }
            ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
            if (embed || dr) *reinterpret_cast<f32x4*>(xr + i) = v;
        }
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
        const float rs = 1.0f / sqrtf(ss / (float)H + eps);
        if (!w) return;   // residual add only
        for (int i = lane * 4; i < H; i += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);   // this lane's own writes (or the unchanged row)
            const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
            f32x4 y;
#pragma unroll
            for (int c = 0; c < 4; ++c) y[c] = (v[c] * rs) * g[c];
            if (xn) {
                bf16x4 o;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = (short)f32_to_bf16(y[c]);
                *reinterpret_cast<bf16x4*>(xn + (int64_t)t * H + i) = o;
            }
            if (xn_f32) *reinterpret_cast<f32x4*>(xn_f32 + (int64_t)t * H + i) = y;
        }
    }
}

int launch_rmsnorm(float* x, const float* embed, const int* tok_id, const bf16_t* delta, const float* w, bf16_t* xn,
                   float* xn_f32, int T, int H, float eps, hipStream_t s) {
    if (T == 0) return SR_OK;
    const dim3 grid((unsigned)ceil_div64(T, 4)), block(256);
#define SR_RMS(NCH) hipLaunchKernelGGL(rmsnorm_kernel<NCH>, grid, block, 0, s, x, embed, tok_id, delta, w, xn, xn_f32, T, H, eps)
    switch (H) {
        case 256: SR_RMS(1); break;
        case 512: SR_RMS(2); break;
        case 1024: SR_RMS(4); break;
        case 2048: SR_RMS(8); break;
        case 3072: SR_RMS(12); break;
        case 4096: SR_RMS(16); break;
        default: SR_RMS(0); break;
    }
#undef SR_RMS
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// ---- dense head: final RMSNorm -> per-token L2 normalise -> mean over pooled tokens -----
// (1) one wave per token: the two row statistics  rs = rsqrt(mean(x^2) + eps),  inv = 1 / max(||x rs w||, 1e-12)
__global__ __launch_bounds__(256) void dense_head_stats_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                               float2* __restrict__ stats, int T, int H, float eps) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    const float* xr = x + (int64_t)t * H;
    float ss = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);
    float s2 = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + i);
        const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
#pragma unroll
        for (int c = 0; c < 4; ++c) { const float y = (v[c] * rs) * g[c]; s2 += y * y; }
    }
    for (int off = 32; off > 0; off >>= 1) s2 += __shfl_xor(s2, off);
    if (lane == 0) stats[t] = make_float2(rs, 1.0f / fmaxf(sqrtf(s2), 1e-12f));
}
// (2) workgroup = (sequence, 256-column slab): out[b][c] = mean over pooled tokens of x[t][c] rs_t w[c] inv_t,
//     accumulated in token order (fp32), coalesced row reads.
__global__ __launch_bounds__(256) void dense_head_pool_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float2* __restrict__ stats, const int* __restrict__ cu,
                                                              const int* __restrict__ pos, const int* __restrict__ pool_start,
                                                              float* __restrict__ out, int H) {
    const int b = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    if (c >= H) return;
    const int t0 = cu[b], n = cu[b + 1] - t0, ps = pool_start[b];
    const float wc = w[c];
    float acc = 0.f;
    int cnt = 0;
    for (int j = 0; j < n; ++j) {
        const int t = t0 + j;
        if (pos[t] < ps) continue;
        const float2 st = stats[t];
        acc += ((x[(int64_t)t * H + c] * st.x) * wc) * st.y;
        ++cnt;
    }
    out[(int64_t)b * H + c] = cnt > 0 ? acc / (float)cnt : 0.f;
}

// ---- sparse head finish: reps = log(1 + relu(bf16_round(max_logit) * H^-0.25)) ----
__global__ void sparse_finish_kernel(float* __restrict__ out, int64_t n, float scale, int round_bf16) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = out[i];  // max over tokens of positive logits, 0 if none
    if (round_bf16) v = bf16_to_f32(f32_to_bf16(v));
    v *= scale;
    // the logarithm in double, rounded once: hipcc expands logf into v_log_f32 (1 ulp of log2 x) times ln 2, which is up to 2 ulps of
    // log x off (measured 1.99 at x = 371.879: tests/test_bf16_regime_gpu.py::test_sparse_finish holds the result to the 1 ulp the HIP
    // math API documents for logf).  The kernel stays bound by its 8 bytes per element.
    out[i] = (float)log((double)(fmaxf(v, 0.f) + 1.0f));
}

// the two launches of the dense head and the sparse head's finish, shared by head_dense / head_sparse and the test hooks
// sr_dense_head_pool / sr_sparse_finish (api.hip).  stats: [T] float2 scratch
int launch_dense_head(const float* x, const float* w, float2* stats, const int* cu, const int* pos, const int* pool_start, float* out,
                      int B, int T, int H, float eps, hipStream_t s) {
    hipLaunchKernelGGL(dense_head_stats_kernel, dim3((unsigned)ceil_div64(T, 4)), dim3(256), 0, s, x, w, stats, T, H, eps);
    hipLaunchKernelGGL(dense_head_pool_kernel, dim3((unsigned)B, (unsigned)ceil_div64(H, 256)), dim3(256), 0, s, x, w, stats, cu, pos,
                       pool_start, out, H);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
int launch_sparse_finish(float* out, int64_t n, float scale, int round_bf16, hipStream_t s) {
    hipLaunchKernelGGL(sparse_finish_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, out, n, scale, round_bf16);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// ---- RMSNorm of the fp32 regime: one wave per token, output as split-bf16 plane segments [T, n_seg * H] -------
// x[t] = embed[tok_id[t]] (if embed);  y = (x * rsqrt(mean(x^2) + eps)) * w in fp32 (HF LlamaRMSNorm on fp32 input)
__global__ __launch_bounds__(256) void rmsnorm_split_kernel(float* __restrict__ x, const float* __restrict__ embed,
                                                            const int* __restrict__ tok_id, const float* __restrict__ w,
                                                            bf16_t* __restrict__ xs, int T, int H, float eps, SplitMap map) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float* xr = x + (int64_t)t * H;
    const float* src = embed ? embed + (int64_t)tok_id[t] * H : xr;
    float ss = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        if (embed) *reinterpret_cast<f32x4*>(xr + i) = v;
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    const float rs = 1.0f / sqrtf(ss / (float)H + eps);
    bf16_t* orow = xs + (int64_t)t * H * map.n_seg;
    for (int i = lane * 4; i < H; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + i);
        const f32x4 g = *reinterpret_cast<const f32x4*>(w + i);
        bf16x4 pl[3];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            unsigned short a0, a1, a2;
            split_bf16x3((v[c] * rs) * g[c], a0, a1, a2);
            pl[0][c] = (short)a0; pl[1][c] = (short)a1; pl[2][c] = (short)a2;
        }
        for (int sg = 0; sg < map.n_seg; ++sg) {
            const int pi = map.plane[sg];
            *reinterpret_cast<bf16x4*>(orow + (int64_t)sg * H + i) = pi == 0 ? pl[0] : (pi == 1 ? pl[1] : pl[2]);
        }
    }
}

int launch_rmsnorm_split(float* x, const float* embed, const int* tok_id, const float* w, bf16_t* xs, int T, int H, float eps,
                         const SplitMap& map, hipStream_t s) {
    if (T == 0) return SR_OK;
    hipLaunchKernelGGL(rmsnorm_split_kernel, dim3((unsigned)ceil_div64(T, 4)), dim3(256), 0, s, x, embed, tok_id, w, xs, T, H, eps,
                       map);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
