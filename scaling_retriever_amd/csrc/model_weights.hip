// The encoder's model handle: sr_model_create / sr_model_destroy, weight loading into the internal layouts (sr_model_set_weight,
// sr_lora_merge) and sr_model_finalize.  The forward pass over the handle: encoder.hip.
#include "encoder_model.h"
#include <math.h>
#include <algorithm>
#include <string>

// ---- weights: convert / permute rows into the internal bf16 layout --------------------
// dst[row_map(r)][c] = bf16(src[r][c]);  row_map: dst_row = base + (interleave ? blk16(r) : r)
__global__ void convert_rows_kernel(const void* __restrict__ src, int src_dtype, int64_t rows, int64_t cols,
                                    bf16_t* __restrict__ dst_bf16, float* __restrict__ dst_f32, int64_t dst_row_base,
                                    int interleave /*0 none, 1 gate, 2 up*/) {
    const int64_t r = blockIdx.x;
    int64_t dr = r;
    if (interleave) dr = (r / 16) * 32 + (interleave == 2 ? 16 : 0) + (r % 16);
    dr += dst_row_base;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
        float v;
        if (src_dtype == SR_DTYPE_F32) v = reinterpret_cast<const float*>(src)[r * cols + c];
        else v = bf16_to_f32(reinterpret_cast<const bf16_t*>(src)[r * cols + c]);
        if (dst_bf16) dst_bf16[dr * cols + c] = f32_to_bf16(v);
        if (dst_f32) dst_f32[dr * cols + c] = v;
    }
}

// q / k / v bias (cfg.attention_bias): the values as fp32 and their bf16 roundings as fp32 (see LayerW::bqkv)
__global__ void convert_bias_kernel(const void* __restrict__ src, int src_dtype, int64_t n, float* __restrict__ dst_f32,
                                    float* __restrict__ dst_bf16r) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = src_dtype == SR_DTYPE_F32 ? reinterpret_cast<const float*>(src)[i] : bf16_to_f32(reinterpret_cast<const bf16_t*>(src)[i]);
    dst_f32[i] = v;
    dst_bf16r[i] = bf16_to_f32(f32_to_bf16(v));
}

// fp32 regime: the same rows as split-bf16 plane segments, dst[row_map(r)][sg * cols + c] = plane_{map.plane[sg]}(src[r][c])
__global__ void convert_rows_split_kernel(const void* __restrict__ src, int src_dtype, int64_t rows, int64_t cols,
                                          bf16_t* __restrict__ dst, int64_t dst_row_base, int interleave, SplitMap map) {
    const int64_t r = blockIdx.x;
    int64_t dr = r;
    if (interleave) dr = (r / 16) * 32 + (interleave == 2 ? 16 : 0) + (r % 16);
    dr += dst_row_base;
    bf16_t* drow = dst + dr * cols * map.n_seg;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) {
        float v;
        if (src_dtype == SR_DTYPE_F32) v = reinterpret_cast<const float*>(src)[r * cols + c];
        else v = bf16_to_f32(reinterpret_cast<const bf16_t*>(src)[r * cols + c]);
        unsigned short p[3];
        split_bf16x3(v, p[0], p[1], p[2]);
        for (int sg = 0; sg < map.n_seg; ++sg) drow[(int64_t)sg * cols + c] = p[map.plane[sg]];
    }
}

// ---- fp16-plane regime (cfg.fp32_planes == SR_FP32_PLANES_F16): rows scaled by a power of two, two fp16 planes ----
// weights: dst[row_map(r)] = [g0 | g1 | g0] (kernels.h split_map_w), w_inv[row_map(r)] = 1 / scale of that row; *lo_nz = 1 if
// any g1 of the row is nonzero (sr_model_finalize drops the all-zero g1 segment of a matrix, see pack_f16_weights)
__global__ __launch_bounds__(256) void convert_rows_split_h_kernel(const void* __restrict__ src, int src_dtype, int64_t rows, int64_t cols,
                                                                   bf16_t* __restrict__ dst, float* __restrict__ w_inv,
                                                                   int64_t dst_row_base, int interleave, int* __restrict__ lo_nz) {
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    int64_t dr = r;
    if (interleave) dr = (r / 16) * 32 + (interleave == 2 ? 16 : 0) + (r % 16);
    dr += dst_row_base;
    auto at = [&](int64_t c) {
        return src_dtype == SR_DTYPE_F32 ? reinterpret_cast<const float*>(src)[r * cols + c]
                                         : bf16_to_f32(reinterpret_cast<const bf16_t*>(src)[r * cols + c]);
    };
    float mx = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += 256) mx = fmaxf(mx, fabsf(at(c)));
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float sc = row_scale_pow2(mx);
    if (threadIdx.x == 0) w_inv[dr] = 1.0f / sc;
    bf16_t* drow = dst + dr * cols * 3;
    bool nz = false;
    for (int64_t c = threadIdx.x; c < cols; c += 256) {
        unsigned short f0, f1;
        split_f16x2(at(c) * sc, f0, f1);
        drow[c] = f0; drow[cols + c] = f1; drow[2 * cols + c] = f0;
        nz |= (f1 & 0x7fff) != 0;
    }
    if (nz) *lo_nz = 1;
}

// [N, 3K] = [g0 | g1 | g0] with g1 all zero -> [N, 2K] = [g0 | g0]: one workgroup per row, 16 bytes per lane and store
__global__ __launch_bounds__(256) void pack_rows_2seg_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int64_t K) {
    const int64_t r = blockIdx.x;
    const uint4* s0 = reinterpret_cast<const uint4*>(src + r * 3 * K);
    uint4* d = reinterpret_cast<uint4*>(dst + r * 2 * K);
    const int64_t kv = K / 8;
    for (int64_t i = threadIdx.x; i < kv; i += 256) {
        const uint4 v = s0[i];
        d[i] = v;
        d[kv + i] = v;
    }
}

// ---- LoRA merge: W += scale * B @ A -----------------------------------------------------
__global__ void lora_merge_kernel(float* __restrict__ W, const float* __restrict__ A, const float* __restrict__ Bm,
                                  int64_t out_f, int64_t in_f, int r, float scale) {
    const int64_t o = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in_f) return;
    float acc = 0.f;
    for (int k = 0; k < r; ++k) acc += Bm[o * r + k] * A[(int64_t)k * in_f + i];
    W[o * in_f + i] += scale * acc;
}

static void rope_tables(const sr_model_config& c, int max_pos, std::vector<float>& cosv, std::vector<float>& sinv) {
    // HF ROPE_INIT_FUNCTIONS["default" | "llama3"]; inv_freq kept in fp32, angles = fp32(pos) * inv_freq
    const int hd = c.head_dim, half = hd / 2;
    std::vector<float> inv(half);
    for (int i = 0; i < half; ++i) {
        double f = 1.0 / pow((double)c.rope_theta, (double)(2 * i) / (double)hd);
        if (c.rope_llama3) {
            const double factor = c.rope_factor, lo = c.rope_low_freq_factor, hi = c.rope_high_freq_factor;
            const double old = (double)c.rope_original_max_pos;
            const double low_wl = old / lo, high_wl = old / hi;
            const double wl = 2.0 * M_PI / f;
            const double f_l = wl > low_wl ? f / factor : f;
            if (!(wl < high_wl) && !(wl > low_wl)) {
                const double smooth = (old / wl - lo) / (hi - lo);
                f = (1.0 - smooth) * f_l / factor + smooth * f_l;
            } else {
                f = f_l;
            }
        }
        inv[i] = (float)f;
    }
    cosv.resize((size_t)max_pos * half);
    sinv.resize((size_t)max_pos * half);
    for (int p = 0; p < max_pos; ++p)
        for (int i = 0; i < half; ++i) {
            const float ang = (float)p * inv[i];
            cosv[(size_t)p * half + i] = (float)cos((double)ang);
            sinv[(size_t)p * half + i] = (float)sin((double)ang);
        }
}

// every device buffer of the model but the fp32-regime workspace (ensure_fp32_workspace, encoder.hip), the pinned copy of cu_seqlens
// and the RoPE tables; on failure the caller deletes the model, which frees what was allocated
static int model_allocate(sr_model* m) {
    const sr_model_config& c = m->cfg;
    DeviceArena& mem = m->mem;
    const int64_t H = m->d.H, I = m->d.I, V = m->d.V, nq = m->d.nq, n_qkv = m->d.n_qkv, Tm = m->Tm, Bm = m->Bm;
    const int64_t nsg = c.fp32_planes ? split_map_w(c.fp32_planes).n_seg : 0;      // plane segments of a weight row
    const bool f16p = c.fp32_planes == SR_FP32_PLANES_F16;
    SR_TRY(mem.alloc(m->embed, V * H));
    if (c.has_lm_head) SR_TRY(mem.alloc(m->lm_head, V * H));
    if (c.has_lm_head && nsg) SR_TRY(mem.alloc(m->lm_head_s, V * H * nsg));
    if (c.has_lm_head && f16p) SR_TRY(mem.alloc(m->lm_head_i, V));
    if (f16p) {
        SR_TRY(mem.alloc(m->lo_nz, 4 * (int64_t)c.num_layers + 1, true));
        SR_TRY(mem.alloc(m->gu_cmax, c.num_layers, true));
    }
    SR_TRY(mem.alloc(m->norm_w, H));
    for (LayerW& l : m->layers) {
        SR_TRY(mem.alloc(l.wqkv, n_qkv * H));
        SR_TRY(mem.alloc(l.wo, H * nq));
        SR_TRY(mem.alloc(l.wgu, 2 * I * H));
        SR_TRY(mem.alloc(l.wdown, H * I));
        if (nsg) {
            SR_TRY(mem.alloc(l.wqkv_s, n_qkv * H * nsg));
            SR_TRY(mem.alloc(l.wo_s, H * nq * nsg));
            SR_TRY(mem.alloc(l.wgu_s, 2 * I * H * nsg));
            SR_TRY(mem.alloc(l.wdown_s, H * I * nsg));
        }
        if (f16p) {
            SR_TRY(mem.alloc(l.wqkv_i, n_qkv));
            SR_TRY(mem.alloc(l.wo_i, H));
            SR_TRY(mem.alloc(l.wgu_i, 2 * I));
            SR_TRY(mem.alloc(l.wdown_i, H));
        }
        SR_TRY(mem.alloc(l.ln1, H));
        SR_TRY(mem.alloc(l.ln2, H));
        if (c.attention_bias) {
            SR_TRY(mem.alloc(l.bqkv, n_qkv));
            SR_TRY(mem.alloc(l.bqkv_r, n_qkv));
        }
    }
    SR_TRY(mem.alloc(m->rope_cos, (int64_t)m->max_pos * (c.head_dim / 2)));
    SR_TRY(mem.alloc(m->rope_sin, (int64_t)m->max_pos * (c.head_dim / 2)));
    // activations that feed GEMMs are read up to the tile edge: keep them finite
    SR_TRY(mem.alloc(m->x, Tm * H));
    SR_TRY(mem.alloc(m->xn, Tm * H, true));
    SR_TRY(mem.alloc(m->qkv, Tm * n_qkv));
    SR_TRY(mem.alloc(m->attn, Tm * nq, true));
    SR_TRY(mem.alloc(m->act, Tm * I, true));
    SR_TRY(mem.alloc(m->delta, Tm * H));
    SR_TRY(mem.alloc(m->span_start, Bm));
    SR_TRY(mem.alloc(m->span_len, Bm));
    SR_TRY(mem.alloc(m->pool_start, Bm));
    SR_TRY(mem.alloc(m->row_len, Bm));
    SR_TRY(mem.alloc(m->cu, Bm + 1));
    SR_TRY(mem.alloc(m->tok_id, Tm));
    SR_TRY(mem.alloc(m->pos, Tm));
    SR_TRY(mem.alloc(m->seq_of, Tm));
    SR_TRY(mem.alloc(m->key_valid, Tm));
    if (hipHostMalloc((void**)&m->h_cu, (size_t)(2 * Bm + 2) * 4) != hipSuccess) {
        sr_set_error("sr_model_create: hipHostMalloc failed");
        return SR_ERR_NOMEM;
    }
    std::vector<float> cs, sn;
    rope_tables(c, m->max_pos, cs, sn);
    if (hipMemcpy(m->rope_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        sr_set_error("sr_model_create: rope table upload failed");
        return SR_ERR_HIP;
    }
    return SR_OK;
}

extern "C" int sr_model_create(sr_model** out, const sr_model_config* cfg) {
    SR_REQUIRE(out && cfg, "sr_model_create: null argument");
    const sr_model_config& c = *cfg;
    SR_REQUIRE(c.vocab_size > 0 && c.hidden_size > 0 && c.intermediate_size > 0 && c.num_layers > 0,
               "sr_model_create: bad dimensions");
    SR_REQUIRE(c.num_heads > 0 && c.num_kv_heads > 0 && c.num_heads % c.num_kv_heads == 0,
               "sr_model_create: num_heads %d must be a multiple of num_kv_heads %d", c.num_heads, c.num_kv_heads);
    SR_REQUIRE(c.head_dim == 64 || c.head_dim == 128, "sr_model_create: head_dim %d not supported (64 or 128)", c.head_dim);
    SR_REQUIRE(c.hidden_size % 64 == 0 && c.intermediate_size % 64 == 0,
               "sr_model_create: hidden_size and intermediate_size must be multiples of 64");
    SR_REQUIRE(c.vocab_size % 16 == 0 || !c.has_lm_head, "sr_model_create: vocab_size must be a multiple of 16 for the sparse head");
    SR_REQUIRE(c.max_batch_tokens > 0 && c.max_batch_seqs > 0 && c.max_batch_seqs <= 65536, "sr_model_create: bad workspace sizes");
    SR_REQUIRE(c.fp32_planes == 0 || c.fp32_planes == 2 || c.fp32_planes == 3 || c.fp32_planes == SR_FP32_PLANES_F16,
               "sr_model_create: fp32_planes must be 0, 2, 3 or 16");
    SR_REQUIRE(c.attention_bias == 0 || c.attention_bias == 1, "sr_model_create: attention_bias must be 0 or 1");
    sr_model* m = new sr_model();
    m->cfg = c;
    const int nq_ = c.num_heads * c.head_dim, nkv_ = c.num_kv_heads * c.head_dim;
    m->d = ModelDims{c.hidden_size, c.intermediate_size, c.vocab_size, nq_, nkv_, nq_ + 2 * nkv_, c.head_dim};
    m->Tm = (int)(ceil_div64(c.max_batch_tokens, 128) * 128);
    m->Bm = c.max_batch_seqs;
    m->max_pos = 8192;
    m->layers.resize(c.num_layers);
    const int rc = model_allocate(m);
    if (rc != SR_OK) {
        delete m;
        return rc;
    }
    *out = m;
    return SR_OK;
}

extern "C" int sr_model_destroy(sr_model* m) {
    delete m;
    return SR_OK;
}

// ---- weight loading -------------------------------------------------------------------------------------------
// where the rows of a checkpoint tensor go: row r lands in row row_base + (interleave ? blk16(r) : r) of every destination that is set
struct WeightDst {
    bf16_t* bf16 = nullptr;     // bf16 regime
    float* f32 = nullptr;       // embedding table, norm weights
    bf16_t* planes = nullptr;   // fp32 regime: plane segments (cfg.fp32_planes says which)
    float* inv = nullptr;       // fp16 planes: inverse row scales
    int* lo_nz = nullptr;       // fp16 planes: set to 1 if a row has a nonzero low plane
    int64_t row_base = 0;
    int interleave = 0;         // 0 none, 1 gate, 2 up
};

static int convert_rows(const void* src, int dtype, int64_t rows, int64_t cols, const WeightDst& d, int planes, hipStream_t s) {
    hipLaunchKernelGGL(convert_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, src, dtype, rows, cols, d.bf16, d.f32, d.row_base,
                       d.interleave);
    if (d.planes && planes == SR_FP32_PLANES_F16)
        hipLaunchKernelGGL(convert_rows_split_h_kernel, dim3((unsigned)rows), dim3(256), 0, s, src, dtype, rows, cols, d.planes, d.inv,
                           d.row_base, d.interleave, d.lo_nz);
    else if (d.planes && planes)
        hipLaunchKernelGGL(convert_rows_split_kernel, dim3((unsigned)rows), dim3(256), 0, s, src, dtype, rows, cols, d.planes, d.row_base,
                           d.interleave, split_map_w(planes));
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// a matrix or norm weight of one layer: checkpoint name behind "model.layers.N.", shape, destination, bit of LayerW::have
struct LayerTensor {
    const char* suffix;
    int64_t rows, cols;
    WeightDst dst;
    unsigned have_bit;
};

extern "C" int sr_model_set_weight(sr_model* m, const char* name, const void* d_ptr, int dtype, int64_t rows, int64_t cols,
                                   sr_stream stream) {
    SR_REQUIRE(m && name && d_ptr, "sr_model_set_weight: null argument");
    SR_REQUIRE(dtype == SR_DTYPE_F32 || dtype == SR_DTYPE_BF16, "sr_model_set_weight: dtype %d not supported", dtype);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(m->mu);
    // finalize fixes the plane layout of every matrix (pack_f16_weights): a later weight would not fit it
    SR_REQUIRE(!m->finalized, "sr_model_set_weight: the model is already finalized; weights are fixed from then on");
    const sr_model_config& c = m->cfg;
    const int64_t H = m->d.H, I = m->d.I, V = m->d.V, nq = m->d.nq, nkv = m->d.nkv;
    auto lo_flag = [&](int64_t i) { return m->lo_nz ? m->lo_nz + i : nullptr; };     // null outside the fp16-plane regime
    const int64_t lo_lm = 4 * (int64_t)c.num_layers;
    std::string n(name);
#define SHAPE_REQ(r, cc) SR_REQUIRE(rows == (r) && cols == (cc), "sr_model_set_weight: %s has shape [%lld, %lld], expected [%lld, %lld]", name, (long long)rows, (long long)cols, (long long)(r), (long long)(cc))
    if (n == "model.embed_tokens.weight") {
        SHAPE_REQ(V, H);
        const bool tied = c.has_lm_head && c.tie_word_embeddings;
        WeightDst dst;
        dst.f32 = m->embed;
        if (tied) { dst.bf16 = m->lm_head; dst.planes = m->lm_head_s; dst.inv = m->lm_head_i; dst.lo_nz = lo_flag(lo_lm); }
        SR_TRY(convert_rows(d_ptr, dtype, V, H, dst, c.fp32_planes, s));
        m->have_embed = true;
        if (tied) m->have_lm_head = true;
        return SR_OK;
    }
    if (n == "lm_head.weight") {
        SR_REQUIRE(c.has_lm_head, "sr_model_set_weight: model was created without an lm_head");
        SHAPE_REQ(V, H);
        WeightDst dst;
        dst.bf16 = m->lm_head; dst.planes = m->lm_head_s; dst.inv = m->lm_head_i; dst.lo_nz = lo_flag(lo_lm);
        SR_TRY(convert_rows(d_ptr, dtype, V, H, dst, c.fp32_planes, s));
        m->have_lm_head = true;
        return SR_OK;
    }
    if (n == "model.norm.weight") {
        SHAPE_REQ(H, 1);
        WeightDst dst;
        dst.f32 = m->norm_w;
        SR_TRY(convert_rows(d_ptr, dtype, H, 1, dst, c.fp32_planes, s));
        m->have_norm = true;
        return SR_OK;
    }
    int li = -1;
    char rest[128] = {0};
    if (sscanf(name, "model.layers.%d.%127s", &li, rest) == 2 && li >= 0 && li < c.num_layers) {
        LayerW& l = m->layers[li];
        std::string r(rest);
        int* const lo = lo_flag(4 * li);
        auto flag = [&](int k) { return lo ? lo + k : nullptr; };
        const LayerTensor tensors[] = {
            //                                             bf16     f32      planes     inv        lo_nz    row base  interleave
            {"self_attn.q_proj.weight", nq, H,            {l.wqkv,  nullptr, l.wqkv_s,  l.wqkv_i,  flag(0), 0,        0}, 1},
            {"self_attn.k_proj.weight", nkv, H,           {l.wqkv,  nullptr, l.wqkv_s,  l.wqkv_i,  flag(0), nq,       0}, 2},
            {"self_attn.v_proj.weight", nkv, H,           {l.wqkv,  nullptr, l.wqkv_s,  l.wqkv_i,  flag(0), nq + nkv, 0}, 4},
            {"self_attn.o_proj.weight", H, nq,            {l.wo,    nullptr, l.wo_s,    l.wo_i,    flag(1), 0,        0}, 8},
            {"mlp.gate_proj.weight", I, H,                {l.wgu,   nullptr, l.wgu_s,   l.wgu_i,   flag(2), 0,        1}, 16},
            {"mlp.up_proj.weight", I, H,                  {l.wgu,   nullptr, l.wgu_s,   l.wgu_i,   flag(2), 0,        2}, 32},
            {"mlp.down_proj.weight", H, I,                {l.wdown, nullptr, l.wdown_s, l.wdown_i, flag(3), 0,        0}, 64},
            {"input_layernorm.weight", H, 1,              {nullptr, l.ln1,   nullptr,   nullptr,   nullptr, 0,        0}, 128},
            {"post_attention_layernorm.weight", H, 1,     {nullptr, l.ln2,   nullptr,   nullptr,   nullptr, 0,        0}, 256},
        };
        for (const LayerTensor& t : tensors) {
            if (r != t.suffix) continue;
            SHAPE_REQ(t.rows, t.cols);
            SR_TRY(convert_rows(d_ptr, dtype, t.rows, t.cols, t.dst, c.fp32_planes, s));
            l.have |= t.have_bit;
            return SR_OK;
        }
        if (c.attention_bias && (r == "self_attn.q_proj.bias" || r == "self_attn.k_proj.bias" || r == "self_attn.v_proj.bias")) {
            const int which = r[10] == 'q' ? 0 : (r[10] == 'k' ? 1 : 2);
            const int64_t n_b = which == 0 ? nq : nkv, base = which == 0 ? 0 : (which == 1 ? nq : nq + nkv);
            SHAPE_REQ(n_b, 1);
            hipLaunchKernelGGL(convert_bias_kernel, dim3((unsigned)ceil_div64(n_b, 256)), dim3(256), 0, s, d_ptr, dtype, n_b, l.bqkv + base,
                               l.bqkv_r + base);
            SR_CHECK_LAUNCH();
            l.have_bias |= 1u << which;
            return SR_OK;
        }
    }
#undef SHAPE_REQ
    sr_set_error("sr_model_set_weight: unknown tensor name '%s'", name);
    return SR_ERR_INVALID;
}

// fp16-plane regime: a matrix whose g1 plane is all zero (bf16-valued weights, always: 8 significand bits fit the fp16 plane g0
// of their power-of-two scaled row, and where an element lies so far below the row maximum that g0 is subnormal and drops bits,
// what it drops is at most 2^-25, which rounds to a zero g1 - tests/model_load_cases.py) is re-packed from [N, 3K] = [g0 | g1 | g0] to
// [N, 2K] = [g0 | g0], out of place.  The GEMM's middle product f0 . g1 only added exact zeros to the fp32 accumulators (an MFMA
// does not flush its C input), so the 2-segment GEMM - same k order for what remains - gives the same bits with 2/3 of the work.
static int pack_f16_weights(sr_model* m, bf16_t*& w, int& nseg, bool lo_nz, int64_t rows, int64_t K) {
    if (nseg == 2 || lo_nz) return SR_OK;
    bf16_t* p = nullptr;
    SR_CHECK_HIP(hipMalloc((void**)&p, (size_t)(rows * 2 * K * 2)));
    hipLaunchKernelGGL(pack_rows_2seg_kernel, dim3((unsigned)rows), dim3(256), 0, nullptr, w, p, K);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(p);
        sr_set_error("sr_model_finalize: re-packing a [%lld, %lld] weight matrix failed: %s", (long long)rows, (long long)K,
                     hipGetErrorString(e));
        return SR_ERR_HIP;
    }
    m->mem.replace(w, p);
    nseg = 2;
    return SR_OK;
}

extern "C" int sr_model_finalize(sr_model* m) {
    SR_REQUIRE(m, "sr_model_finalize: null model");
    std::lock_guard<std::mutex> lock(m->mu);
    SR_REQUIRE(m->have_embed, "sr_model_finalize: model.embed_tokens.weight missing");
    SR_REQUIRE(m->have_norm, "sr_model_finalize: model.norm.weight missing");
    SR_REQUIRE(!m->cfg.has_lm_head || m->have_lm_head, "sr_model_finalize: lm_head.weight missing");
    for (int i = 0; i < m->cfg.num_layers; ++i)
        SR_REQUIRE(m->layers[i].have == 511, "sr_model_finalize: layer %d is missing tensors (mask 0x%x)", i, m->layers[i].have);
    if (m->cfg.attention_bias)
        for (int i = 0; i < m->cfg.num_layers; ++i)
            SR_REQUIRE(m->layers[i].have_bias == 7,
                       "sr_model_finalize: layer %d is missing self_attn.{q,k,v}_proj.bias (attention_bias = 1; mask 0x%x)", i,
                       m->layers[i].have_bias);
    // sr_model_set_weight converted the planes on the CALLER's streams; a non-blocking stream does not order with the null
    // stream the reduction below runs on, and a cmax read from half-written planes would let EPI_SWIGLU_SPLIT_H overflow fp16
    SR_CHECK_HIP(hipDeviceSynchronize());
    if (m->cfg.fp32_planes == SR_FP32_PLANES_F16) {
        const sr_model_config& c = m->cfg;
        const int64_t H = m->d.H, I = m->d.I, V = m->d.V, nq = m->d.nq;
        std::vector<int> nz((size_t)(4 * c.num_layers + 1));
        SR_CHECK_HIP(hipMemcpy(nz.data(), m->lo_nz, nz.size() * 4, hipMemcpyDeviceToHost));
        // dev switch SR_F16_WEIGHT_SEGS=3: keep [g0 | g1 | g0] everywhere (A/B, and the reference of the bit-identity tests)
        const char* env_seg = sr_dev_getenv("SR_F16_WEIGHT_SEGS");
        if (!(env_seg && *env_seg == '3')) {
            for (int i = 0; i < c.num_layers; ++i) {
                LayerW& l = m->layers[i];
                SR_TRY(pack_f16_weights(m, l.wqkv_s, l.qkv_seg, nz[4 * i + 0] != 0, m->d.n_qkv, H));
                SR_TRY(pack_f16_weights(m, l.wo_s, l.o_seg, nz[4 * i + 1] != 0, H, nq));
                SR_TRY(pack_f16_weights(m, l.wgu_s, l.gu_seg, nz[4 * i + 2] != 0, 2 * I, H));
                SR_TRY(pack_f16_weights(m, l.wdown_s, l.down_seg, nz[4 * i + 3] != 0, H, I));
            }
            if (c.has_lm_head) SR_TRY(pack_f16_weights(m, m->lm_head_s, m->lm_head_seg, nz[4 * c.num_layers] != 0, V, H));
        }
        // row bound of every layer's SwiGLU output (EPI_SWIGLU_SPLIT_H), and whether the layer may use it.  The bound B = |xn|^2 cmax
        // fixes the row's scale before the GEMM runs; the low fp16 plane has an absolute floor of 2^-39 B, which stays below the
        // 2^-22 of the split relative to the row's largest element r only while B / r <= 2^17.  Typically r ~ |xn|^2 median_j(p_j) / H
        // with p_j = |w_gate_j||w_up_j| (the cosines of a random direction are ~ H^-1/2), so B / r ~ H cmax / median(p): a layer runs
        // fused while that is below 2^16 (one bit for silu(g) ~ g / 2), else unfused.  The median comes from up to 256
        // evenly spaced pairs, each through gu_cmax_kernel on its own two rows (I = 1 at the pair's row of its 32-row block).
        const int ns = (int)(I < 256 ? I : 256);
        CallBuf<float> d_p;
        SR_TRY(d_p.reserve(ns + 1, "sr_model_finalize"));
        std::vector<float> p((size_t)ns + 1);
        for (int i = 0; i < c.num_layers; ++i) {
            LayerW& l = m->layers[i];
            SR_TRY(launch_gu_cmax(l.wgu_s, l.wgu_i, (int)I, (int)H, l.gu_seg, m->gu_cmax + i, nullptr));
            SR_TRY(launch_gu_pair_samples(l.wgu_s, l.wgu_i, (int)I, (int)H, l.gu_seg, ns, d_p.p, nullptr));
            SR_CHECK_HIP(hipMemcpyAsync(d_p.p + ns, m->gu_cmax + i, 4, hipMemcpyDeviceToDevice, nullptr));
            SR_CHECK_HIP(hipMemcpy(p.data(), d_p.p, (size_t)(ns + 1) * 4, hipMemcpyDeviceToHost));
            const float cmax = p[(size_t)ns];
            std::nth_element(p.begin(), p.begin() + ns / 2, p.begin() + ns);
            const float med = p[(size_t)(ns / 2)];
            l.fused_act = !(cmax > 0.f) || (float)H * cmax < 65536.f * med;
        }
    }
    SR_CHECK_HIP(hipDeviceSynchronize());
    m->finalized = true;
    return SR_OK;
}

extern "C" int sr_model_weight_segments(sr_model* m, int32_t* out, int64_t capacity, int64_t* n) {
    SR_REQUIRE(m && n, "sr_model_weight_segments: null argument");
    SR_REQUIRE(m->finalized, "sr_model_weight_segments: sr_model_finalize was not called");
    const sr_model_config& c = m->cfg;
    std::vector<int32_t> v;
    const bool f16p = c.fp32_planes == SR_FP32_PLANES_F16;
    const int32_t plain = c.fp32_planes ? split_map_w(c.fp32_planes).n_seg : 0;
    for (const LayerW& l : m->layers) {
        v.push_back(f16p ? l.qkv_seg : plain); v.push_back(f16p ? l.o_seg : plain);
        v.push_back(f16p ? l.gu_seg : plain); v.push_back(f16p ? l.down_seg : plain);
    }
    if (c.has_lm_head) v.push_back(f16p ? m->lm_head_seg : plain);
    *n = (int64_t)v.size();
    SR_REQUIRE(capacity >= 0 && (capacity == 0 || out), "sr_model_weight_segments: bad output buffer");
    for (int64_t i = 0; i < capacity && i < (int64_t)v.size(); ++i) out[i] = v[(size_t)i];
    return SR_OK;
}

extern "C" int sr_model_fused_act_layers(sr_model* m, int32_t* out, int64_t capacity, int64_t* n) {
    SR_REQUIRE(m && n, "sr_model_fused_act_layers: null argument");
    SR_REQUIRE(m->finalized, "sr_model_fused_act_layers: sr_model_finalize was not called");
    const bool f16p = m->cfg.fp32_planes == SR_FP32_PLANES_F16;
    *n = f16p ? (int64_t)m->layers.size() : 0;
    SR_REQUIRE(capacity >= 0 && (capacity == 0 || out), "sr_model_fused_act_layers: bad output buffer");
    for (int64_t i = 0; i < capacity && i < *n; ++i) out[i] = m->layers[(size_t)i].fused_act ? 1 : 0;
    return SR_OK;
}

// Test-only read-out of what loading left on the device (include/sr_hip.h): no kernel, one device-to-host copy per call.
extern "C" int sr_model_readout(sr_model* m, int32_t layer, int32_t buffer, int32_t kind, void* h_dst, int64_t capacity_bytes,
                                int64_t* n_bytes, int64_t* n_rows, int64_t* row_elems) {
    SR_REQUIRE(m && n_bytes && n_rows && row_elems, "sr_model_readout: null argument");
    std::lock_guard<std::mutex> lock(m->mu);
    const sr_model_config& c = m->cfg;
    const int64_t H = m->d.H, I = m->d.I, V = m->d.V, nq = m->d.nq, n_qkv = m->d.n_qkv, half = c.head_dim / 2;
    const bool f16p = c.fp32_planes == SR_FP32_PLANES_F16;
    const int plain = c.fp32_planes ? split_map_w(c.fp32_planes).n_seg : 0;       // plane segments outside the fp16-plane regime
    // a weight matrix [rows, K] in its three forms; seg = its plane segments as they stand (fp16 planes: 3, or 2 once finalize packed it)
    struct Matrix { const bf16_t* w; const bf16_t* planes; const float* inv; int64_t rows, K; int seg; };
    const void* src = nullptr;
    int64_t rows = 0, elems = 0, esize = 4;
    auto matrix = [&](const Matrix& x) {
        if (kind == SR_READOUT_BF16) { src = x.w; rows = x.rows; elems = x.K; esize = 2; }
        else if (kind == SR_READOUT_PLANES) { src = x.planes; rows = x.rows; elems = x.K * (f16p ? x.seg : plain); esize = 2; }
        else if (kind == SR_READOUT_W_INV) { src = x.inv; rows = x.rows; elems = 1; }
    };
    auto vec_f32 = [&](const float* p, int64_t n_, int64_t per_row) {
        if (kind == SR_READOUT_F32) { src = p; rows = n_; elems = per_row; }
    };
    if (layer == -1) {
        switch (buffer) {
            case SR_READOUT_EMBED: vec_f32(m->embed, V, H); break;
            case SR_READOUT_LM_HEAD: matrix(Matrix{m->lm_head, m->lm_head_s, m->lm_head_i, V, H, m->lm_head_seg}); break;
            case SR_READOUT_NORM: vec_f32(m->norm_w, H, 1); break;
            case SR_READOUT_ROPE_COS: vec_f32(m->rope_cos, m->max_pos, half); break;
            case SR_READOUT_ROPE_SIN: vec_f32(m->rope_sin, m->max_pos, half); break;
            default: break;
        }
    } else {
        SR_REQUIRE(layer >= 0 && layer < c.num_layers, "sr_model_readout: layer %d outside [-1, %d)", layer, c.num_layers);
        const LayerW& l = m->layers[(size_t)layer];
        switch (buffer) {
            case SR_READOUT_QKV: matrix(Matrix{l.wqkv, l.wqkv_s, l.wqkv_i, n_qkv, H, l.qkv_seg}); break;
            case SR_READOUT_O: matrix(Matrix{l.wo, l.wo_s, l.wo_i, H, nq, l.o_seg}); break;
            case SR_READOUT_GATE_UP: matrix(Matrix{l.wgu, l.wgu_s, l.wgu_i, 2 * I, H, l.gu_seg}); break;
            case SR_READOUT_DOWN: matrix(Matrix{l.wdown, l.wdown_s, l.wdown_i, H, I, l.down_seg}); break;
            case SR_READOUT_LN1: vec_f32(l.ln1, H, 1); break;
            case SR_READOUT_LN2: vec_f32(l.ln2, H, 1); break;
            case SR_READOUT_BIAS:
                if (kind == SR_READOUT_F32) { src = l.bqkv; rows = n_qkv; elems = 1; }
                else if (kind == SR_READOUT_BF16_AS_F32) { src = l.bqkv_r; rows = n_qkv; elems = 1; }
                break;
            default: break;
        }
    }
    SR_REQUIRE(src, "sr_model_readout: layer %d has no buffer %d of kind %d in this model", layer, buffer, kind);
    const int64_t bytes = rows * elems * esize;
    *n_bytes = bytes;
    *n_rows = rows;
    *row_elems = elems;
    if (!h_dst || capacity_bytes == 0) return SR_OK;         // size query
    SR_REQUIRE(capacity_bytes >= bytes, "sr_model_readout: buffer too small");
    SR_CHECK_HIP(hipDeviceSynchronize());                    // sr_model_set_weight converted on the caller's streams
    SR_CHECK_HIP(hipMemcpy(h_dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return SR_OK;
}

extern "C" int sr_lora_merge(float* d_W, const float* d_A, const float* d_B, int64_t out_features, int64_t in_features,
                             int32_t r, float scale, sr_stream stream) {
    SR_REQUIRE(d_W && d_A && d_B && out_features > 0 && in_features > 0 && r > 0, "sr_lora_merge: bad argument");
    SR_REQUIRE(out_features < 65536 * 32, "sr_lora_merge: out_features too large");
    // out_features is the grid's y dimension: what the device does not take is refused here, not by a failed launch
    int dev = 0, max_y = 0;
    SR_CHECK_HIP(hipGetDevice(&dev));
    SR_CHECK_HIP(hipDeviceGetAttribute(&max_y, hipDeviceAttributeMaxGridDimY, dev));
    SR_REQUIRE(out_features <= max_y, "sr_lora_merge: out_features %lld exceeds the device's grid limit maxGridSize[1] = %d",
               (long long)out_features, max_y);
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)ceil_div64(in_features, 256), (unsigned)out_features), dim3(256), 0,
                       (hipStream_t)stream, d_W, d_A, d_B, out_features, in_features, r, scale);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
