// Error plumbing + misc entry points of the C ABI (include/sr_hip.h).
#include "kernels.h"
#include <stdlib.h>
#include <string>
#include <vector>

static thread_local std::string g_last_error;

void sr_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int sr_cu_count() {
    static int per_dev[SR_MAX_DEVICES] = {};
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= SR_MAX_DEVICES) d = 0;
    if (per_dev[d] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
        per_dev[d] = n;
    }
    return per_dev[d];
}

extern "C" const char* sr_last_error(void) { return g_last_error.c_str(); }
extern "C" int sr_version(void) { return 1; }
extern "C" int sr_max_topk(void) { return SR_MAX_TOPK; }

extern "C" int sr_gemm_bf16(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, int32_t epilogue, void* d_C,
                            const int32_t* d_seq_of, sr_stream stream) {
    SR_REQUIRE(d_A && d_W && d_C, "sr_gemm_bf16: null pointer");
    SR_REQUIRE(epilogue >= 0 && epilogue <= 4, "sr_gemm_bf16: unknown epilogue %d", epilogue);
    SR_REQUIRE(epilogue != EPI_SEGMAX || d_seq_of, "sr_gemm_bf16: epilogue 3 needs d_seq_of");
    GemmArgs g{};
    g.A = (const bf16_t*)d_A; g.W = (const bf16_t*)d_W; g.M = M; g.N = N; g.K = K; g.C = d_C; g.seq_of = d_seq_of; g.out_ld = N;
    if (epilogue != EPI_SEGMAX && d_seq_of && sr_dev_getenv("SR_GEMM_STAMPS")) {   // tools/micro diagnostics: d_seq_of carries the stamp buffer
        g.stamps = (unsigned long long*)d_seq_of;
        g.seq_of = nullptr;
    }
    return launch_gemm_bf16((GemmEpilogue)epilogue, g, (hipStream_t)stream);
}

extern "C" int sr_gemm_qkv_rope(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, void* d_C, const int32_t* d_pos,
                                const float* d_rope_cos, const float* d_rope_sin, int32_t n_rope, int32_t head_dim,
                                sr_stream stream) {
    SR_REQUIRE(d_A && d_W && d_C && d_pos && d_rope_cos && d_rope_sin, "sr_gemm_qkv_rope: null pointer");
    GemmArgs g{};
    g.A = (const bf16_t*)d_A; g.W = (const bf16_t*)d_W; g.M = M; g.N = N; g.K = K; g.C = d_C;
    g.pos = d_pos; g.rope_cos = d_rope_cos; g.rope_sin = d_rope_sin; g.n_rope = n_rope; g.head_dim = head_dim;
    return launch_gemm_bf16(EPI_QKV_ROPE, g, (hipStream_t)stream);
}

extern "C" int sr_gemm_qkv_rope_bias(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, void* d_C, const int32_t* d_pos,
                                     const float* d_rope_cos, const float* d_rope_sin, int32_t n_rope, int32_t head_dim,
                                     const float* d_bias, int32_t fp32_out, sr_stream stream) {
    SR_REQUIRE(d_A && d_W && d_C && d_pos && d_rope_cos && d_rope_sin, "sr_gemm_qkv_rope_bias: null pointer");
    SR_REQUIRE(fp32_out == 0 || fp32_out == 1, "sr_gemm_qkv_rope_bias: fp32_out must be 0 or 1");
    GemmArgs g{};
    g.A = (const bf16_t*)d_A; g.W = (const bf16_t*)d_W; g.M = M; g.N = N; g.K = K; g.C = d_C;
    g.pos = d_pos; g.rope_cos = d_rope_cos; g.rope_sin = d_rope_sin; g.n_rope = n_rope; g.head_dim = head_dim;
    g.bias = d_bias;
    return launch_gemm_bf16(fp32_out ? EPI_QKV_ROPE_F32 : EPI_QKV_ROPE, g, (hipStream_t)stream);
}

extern "C" int sr_attention_varlen(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, const int32_t* d_pos,
                                   const uint8_t* d_key_valid, const float* d_rope_cos, const float* d_rope_sin, int32_t B,
                                   int32_t num_heads, int32_t num_kv_heads, int32_t head_dim, sr_stream stream) {
    SR_REQUIRE(d_qkv && d_out && d_cu_seqlens && d_key_valid, "sr_attention_varlen: null pointer");
    SR_REQUIRE((d_rope_cos == nullptr) == (d_rope_sin == nullptr), "sr_attention_varlen: pass both rope tables or neither");
    SR_REQUIRE(!d_rope_cos || d_pos, "sr_attention_varlen: rope tables need d_pos");
    SR_REQUIRE(B >= 0 && num_heads > 0 && num_kv_heads > 0, "sr_attention_varlen: bad sizes");
    AttnArgs a{};
    a.qkv = (const bf16_t*)d_qkv; a.out = (bf16_t*)d_out; a.cu_seqlens = d_cu_seqlens; a.pos = d_pos; a.key_valid = d_key_valid;
    a.rope_cos = d_rope_cos; a.rope_sin = d_rope_sin; a.B = B; a.nh = num_heads; a.nkv = num_kv_heads; a.hd = head_dim;
    a.scale = 1.0f / sqrtf((float)head_dim);
    a.apply_rope = d_rope_cos ? 1 : 0;
    a.max_seqlen = 0;
    if (!a.apply_rope && B > 0) {   // test hook: fetch the lengths to pick the kernel the encoder would pick
        std::vector<int> cu((size_t)B + 1);
        SR_CHECK_HIP(hipMemcpyAsync(cu.data(), d_cu_seqlens, sizeof(int) * ((size_t)B + 1), hipMemcpyDeviceToHost, (hipStream_t)stream));
        SR_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        for (int b = 0; b < B; ++b) a.max_seqlen = cu[b + 1] - cu[b] > a.max_seqlen ? cu[b + 1] - cu[b] : a.max_seqlen;
    }
    return launch_attention(a, (hipStream_t)stream);
}

// fp32 attention of the encoder's fp32 regime (attention_f32.hip), exported for the per-kernel parity test: the arguments
// the encoder fills, both output forms.  max_seqlen sizes the grids and the MFMA kernel's LDS: the batch's true maximum.
extern "C" int sr_attention_varlen_f32(const float* d_qkv, float* d_out_f32, void* d_out_planes, int32_t fp32_planes,
                                       const int32_t* d_cu_seqlens, const uint8_t* d_key_valid, int32_t B, int32_t num_heads,
                                       int32_t num_kv_heads, int32_t head_dim, int32_t max_seqlen, sr_stream stream) {
    SR_REQUIRE(d_qkv && d_cu_seqlens && d_key_valid, "sr_attention_varlen_f32: null pointer");
    SR_REQUIRE((d_out_f32 != nullptr) != (d_out_planes != nullptr), "sr_attention_varlen_f32: pass exactly one of d_out_f32 / d_out_planes");
    SR_REQUIRE(d_out_f32 || fp32_planes == 2 || fp32_planes == 3, "sr_attention_varlen_f32: fp32_planes %d (2 or 3 for plane output)", fp32_planes);
    SR_REQUIRE(B >= 0 && max_seqlen >= 0 && num_heads > 0 && num_kv_heads > 0 && head_dim > 0, "sr_attention_varlen_f32: bad sizes");
    // the short-sequence kernel loads q / k / v and stores the fp32 output 16 bytes, the plane segments 8 bytes at a time
    SR_REQUIRE((uintptr_t)d_qkv % 16 == 0 && (uintptr_t)d_out_f32 % 16 == 0 && (uintptr_t)d_out_planes % 8 == 0,
               "sr_attention_varlen_f32: d_qkv and d_out_f32 must be 16-byte aligned, d_out_planes 8-byte aligned");
    AttnF32Args a{};
    a.qkv = d_qkv; a.out_f32 = d_out_f32; a.out = (bf16_t*)d_out_planes; a.cu_seqlens = d_cu_seqlens; a.key_valid = d_key_valid;
    a.B = B; a.nh = num_heads; a.nkv = num_kv_heads; a.hd = head_dim;
    a.scale = 1.0f / sqrtf((float)head_dim); a.max_seqlen = max_seqlen;
    if (!d_out_f32) a.out_map = split_map_a(fp32_planes);
    return launch_attention_f32(a, (hipStream_t)stream);
}

// fp16-plane GEMM of the encoder's fp32 regime, exported for the per-kernel parity test: C fp32 [M, N] += (A' @ W'^T) *
// a_scale[m] * w_scale[n], A' / W' = [rows, K] fp16 plane segments.
extern "C" int sr_gemm_f16_scaled(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, const float* d_a_scale,
                                  const float* d_w_scale, float* d_C, sr_stream stream) {
    SR_REQUIRE(d_A && d_W && d_C && d_a_scale && d_w_scale, "sr_gemm_f16_scaled: null pointer");
    GemmArgs g{};
    g.A = (const bf16_t*)d_A; g.W = (const bf16_t*)d_W; g.M = M; g.N = N; g.K = K; g.C = d_C; g.a_scale = d_a_scale; g.w_scale = d_w_scale;
    return launch_gemm_bf16(EPI_RESID_F32_H, g, (hipStream_t)stream);
}

// The other launches of the fp16-plane layer loop (layer_f16_planes, encoder.hip), exported for tests/test_fp32_planes_gpu.py: thin
// calls into the launch functions with the arguments the encoder fills.  Everything is validated before a device is touched.
extern "C" int sr_rows_split_f16(float* d_src, const float* d_embed, const int32_t* d_tok_id, const float* d_norm_w, float eps,
                                 int32_t T, int32_t K, int32_t nseg, void* d_planes, float* d_a_inv, const float* d_gu_cmax,
                                 float* d_act_sc, float* d_act_inv, sr_stream stream) {
    SR_REQUIRE(d_src && d_planes && d_a_inv, "sr_rows_split_f16: null pointer");
    SR_REQUIRE((d_embed == nullptr) == (d_tok_id == nullptr), "sr_rows_split_f16: pass both d_embed and d_tok_id or neither");
    SR_REQUIRE(!d_embed || d_norm_w, "sr_rows_split_f16: the embedding gather is part of the norm kernel and needs d_norm_w");
    SR_REQUIRE(!d_gu_cmax || (d_act_sc && d_act_inv), "sr_rows_split_f16: d_gu_cmax needs d_act_sc and d_act_inv");
    SR_REQUIRE(nseg == 2 || nseg == 3, "sr_rows_split_f16: nseg %d is not 2 or 3", nseg);
    SR_REQUIRE(T >= 0 && K > 0 && K % 4 == 0, "sr_rows_split_f16: bad sizes T=%d K=%d (K must be a multiple of 4)", T, K);
    SR_REQUIRE((uintptr_t)d_src % 16 == 0 && (uintptr_t)d_embed % 16 == 0 && (uintptr_t)d_norm_w % 16 == 0 && (uintptr_t)d_planes % 8 == 0,
               "sr_rows_split_f16: d_src, d_embed and d_norm_w must be 16-byte aligned, d_planes 8-byte aligned");
    if (T == 0) return SR_OK;
    return launch_rows_split_f16(d_src, d_embed, d_tok_id, d_norm_w, (bf16_t*)d_planes, d_a_inv, T, K, eps, nseg, d_gu_cmax, d_act_sc,
                                 d_act_inv, (hipStream_t)stream);
}

extern "C" int sr_gu_cmax_f16(const void* d_wgu_planes, const float* d_wgu_inv, int32_t I, int32_t K, int32_t nseg, float* d_cmax,
                              sr_stream stream) {
    SR_REQUIRE(d_wgu_planes && d_wgu_inv && d_cmax, "sr_gu_cmax_f16: null pointer");
    SR_REQUIRE(nseg == 2 || nseg == 3, "sr_gu_cmax_f16: nseg %d is not 2 or 3", nseg);
    SR_REQUIRE(I > 0 && I % 16 == 0 && K > 0, "sr_gu_cmax_f16: bad sizes I=%d K=%d (gate / up rows alternate in blocks of 16)", I, K);
    return launch_gu_cmax((const bf16_t*)d_wgu_planes, d_wgu_inv, I, K, nseg, d_cmax, (hipStream_t)stream);
}

extern "C" int sr_gemm_f16_planes(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t a_nseg,
                                  const float* d_a_scale, const float* d_w_scale, void* d_C, const int32_t* d_pos,
                                  const float* d_rope_cos, const float* d_rope_sin, int32_t n_rope, int32_t head_dim,
                                  const float* d_bias, const int32_t* d_seq_of, const float* d_out_scale, int32_t out_nseg,
                                  sr_stream stream) {
    SR_REQUIRE(d_A && d_W && d_C && d_a_scale && d_w_scale, "sr_gemm_f16_planes: null pointer");
    SR_REQUIRE(epilogue == EPI_QKV_ROPE_F32_H || epilogue == EPI_RESID_F32_H || epilogue == EPI_SWIGLU_F32_H || epilogue == EPI_SEGMAX_H ||
                   epilogue == EPI_SWIGLU_SPLIT_H, "sr_gemm_f16_planes: unknown epilogue %d (9 .. 13)", epilogue);
    SR_REQUIRE(a_nseg == 2 || a_nseg == 3, "sr_gemm_f16_planes: a_nseg %d is not 2 or 3", a_nseg);
    SR_REQUIRE(M >= 0 && N > 0 && K > 0 && K % 64 == 0 && K % a_nseg == 0,
               "sr_gemm_f16_planes: bad shape M=%d N=%d K=%d (K = a_nseg x features, a multiple of 64)", M, N, K);
    SR_REQUIRE(epilogue != EPI_QKV_ROPE_F32_H || (d_pos && d_rope_cos && d_rope_sin), "sr_gemm_f16_planes: epilogue 9 needs d_pos and both rope tables");
    SR_REQUIRE(epilogue == EPI_QKV_ROPE_F32_H || !d_bias, "sr_gemm_f16_planes: only epilogue 9 takes a bias");
    SR_REQUIRE(epilogue != EPI_SEGMAX_H || d_seq_of, "sr_gemm_f16_planes: epilogue 12 needs d_seq_of");
    SR_REQUIRE(epilogue != EPI_SWIGLU_SPLIT_H || d_out_scale, "sr_gemm_f16_planes: epilogue 13 needs d_out_scale");
    SR_REQUIRE(epilogue != EPI_SWIGLU_SPLIT_H || out_nseg == 2 || out_nseg == 3, "sr_gemm_f16_planes: out_nseg %d is not 2 or 3", out_nseg);
    GemmArgs g{};
    g.A = (const bf16_t*)d_A; g.W = (const bf16_t*)d_W; g.M = M; g.N = N; g.K = K; g.a_nseg = a_nseg; g.C = d_C;
    g.a_scale = d_a_scale; g.w_scale = d_w_scale;
    if (epilogue == EPI_QKV_ROPE_F32_H) {
        g.pos = d_pos; g.rope_cos = d_rope_cos; g.rope_sin = d_rope_sin; g.n_rope = n_rope; g.head_dim = head_dim; g.bias = d_bias;
    }
    if (epilogue == EPI_SEGMAX_H) { g.seq_of = d_seq_of; g.out_ld = N; }
    if (epilogue == EPI_SWIGLU_SPLIT_H) { g.out_scale = d_out_scale; g.out_nseg = out_nseg; }
    return launch_gemm_bf16((GemmEpilogue)epilogue, g, (hipStream_t)stream);
}

// What the bf16 regime (fp32_planes = 0) and the two heads launch besides the GEMMs and the attention, exported for
// tests/test_bf16_regime_gpu.py: thin calls into the launch functions of encoder_kernels.hip with the arguments the encoder fills.
// Everything is validated before a device is touched.
extern "C" int sr_rmsnorm_bf16(float* d_x, const float* d_embed, const int32_t* d_tok_id, const void* d_delta, const float* d_norm_w,
                               void* d_xn, float* d_xn_f32, float eps, int32_t T, int32_t H, sr_stream stream) {
    SR_REQUIRE(d_x, "sr_rmsnorm_bf16: null pointer");
    SR_REQUIRE((d_embed == nullptr) == (d_tok_id == nullptr), "sr_rmsnorm_bf16: pass both d_embed and d_tok_id or neither");
    SR_REQUIRE(d_norm_w || (!d_xn && !d_xn_f32), "sr_rmsnorm_bf16: an output needs d_norm_w (without it the call only adds the residual)");
    SR_REQUIRE(T >= 0 && H > 0 && H % 4 == 0, "sr_rmsnorm_bf16: bad sizes T=%d H=%d (H must be a multiple of 4)", T, H);
    SR_REQUIRE((uintptr_t)d_x % 16 == 0 && (uintptr_t)d_embed % 16 == 0 && (uintptr_t)d_norm_w % 16 == 0 && (uintptr_t)d_xn_f32 % 16 == 0 &&
                   (uintptr_t)d_delta % 8 == 0 && (uintptr_t)d_xn % 8 == 0,
               "sr_rmsnorm_bf16: d_x, d_embed, d_norm_w and d_xn_f32 must be 16-byte aligned, d_delta and d_xn 8-byte aligned");
    return launch_rmsnorm(d_x, d_embed, d_tok_id, (const bf16_t*)d_delta, d_norm_w, (bf16_t*)d_xn, d_xn_f32, T, H, eps, (hipStream_t)stream);
}

extern "C" int sr_dense_head_pool(const float* d_x, const float* d_norm_w, const int32_t* d_cu_seqlens, const int32_t* d_pos,
                                  const int32_t* d_pool_start, float eps, int32_t B, int32_t T, int32_t H, void* d_stats, float* d_out,
                                  sr_stream stream) {
    SR_REQUIRE(d_x && d_norm_w && d_cu_seqlens && d_pos && d_pool_start && d_stats && d_out, "sr_dense_head_pool: null pointer");
    SR_REQUIRE(B >= 0 && T >= 0 && H > 0 && H % 4 == 0, "sr_dense_head_pool: bad sizes B=%d T=%d H=%d (H must be a multiple of 4)", B, T, H);
    SR_REQUIRE((uintptr_t)d_x % 16 == 0 && (uintptr_t)d_norm_w % 16 == 0 && (uintptr_t)d_stats % 8 == 0,
               "sr_dense_head_pool: d_x and d_norm_w must be 16-byte aligned, d_stats 8-byte aligned");
    if (B == 0) return SR_OK;
    if (T == 0) {                      // as sr_encode_dense: a batch that packs to no token gives zero vectors
        SR_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)B * H * 4, (hipStream_t)stream));
        return SR_OK;
    }
    return launch_dense_head(d_x, d_norm_w, (float2*)d_stats, d_cu_seqlens, d_pos, d_pool_start, d_out, B, T, H, eps, (hipStream_t)stream);
}

extern "C" int sr_sparse_finish(float* d_out, int64_t n, float scale, int32_t round_bf16, sr_stream stream) {
    SR_REQUIRE(d_out, "sr_sparse_finish: null pointer");
    SR_REQUIRE(n >= 0 && n < ((int64_t)1 << 39), "sr_sparse_finish: bad size n=%lld", (long long)n);
    SR_REQUIRE(round_bf16 == 0 || round_bf16 == 1, "sr_sparse_finish: round_bf16 must be 0 or 1");
    if (n == 0) return SR_OK;
    return launch_sparse_finish(d_out, n, scale, round_bf16, (hipStream_t)stream);
}

extern "C" int sr_encode_plan(const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L, int32_t mode, int32_t vocab,
                              const int32_t* d_row_shift, int32_t* d_span_start, int32_t* d_span_len, int32_t* d_pool_start,
                              int32_t* d_row_len, int32_t* d_cu_seqlens, int32_t* d_tok_id, int32_t* d_pos, uint8_t* d_key_valid,
                              int32_t* d_seq_of, int64_t capacity, int64_t* n_tokens, sr_stream stream) {
    SR_REQUIRE(d_input_ids && d_attention_mask && d_span_start && d_span_len && d_pool_start && d_row_len && d_cu_seqlens && n_tokens,
               "sr_encode_plan: null pointer");
    SR_REQUIRE(capacity >= 0 && (capacity == 0 || (d_tok_id && d_pos && d_key_valid && d_seq_of)), "sr_encode_plan: null token array");
    SR_REQUIRE(mode >= 0 && mode <= 2, "sr_encode_plan: mode %d (0 dense, 1 sparse, 2 both)", mode);
    SR_REQUIRE(B >= 1 && B <= 65536 && L >= 1 && vocab >= 1 && (int64_t)B * L < ((int64_t)1 << 31),
               "sr_encode_plan: bad sizes B=%d L=%d vocab=%d", B, L, vocab);
    hipStream_t s = (hipStream_t)stream;
    SR_TRY(launch_plan_rows(d_attention_mask, B, L, mode, d_span_start, d_span_len, d_pool_start, d_row_len, d_row_shift, d_cu_seqlens, s));
    int T = 0;
    SR_CHECK_HIP(hipMemcpyAsync(&T, d_cu_seqlens + B, 4, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    *n_tokens = T;
    SR_REQUIRE(T <= capacity, "sr_encode_plan: the batch packs to %d tokens, the token arrays hold %lld", T, (long long)capacity);
    if (T == 0) return SR_OK;
    return launch_plan_tokens(d_input_ids, d_attention_mask, B, L, d_span_start, d_cu_seqlens, d_tok_id, d_pos, d_key_valid, d_seq_of, vocab,
                              mode, d_row_shift, s);
}
