// The model handle of the encoder: dimensions, weights in their internal layouts, workspaces.  Included by model_weights.hip (create,
// weight loading, finalize) and encoder.hip (the forward pass) only.
#pragma once
#include "kernels.h"
#include <mutex>
#include <vector>

// Precision regimes:
//   PREC_BF16  torch.autocast(bf16): documents (indexer.py:46-52, :255-256) and sparse queries (:390-391)
//   PREC_FP32  no autocast: dense queries (eval_dense.py:94-106) and examples/quick_start.py - every nn.Linear is an fp32
//              GEMM there.  Here each GEMM runs on the bf16 MFMA pipe over split-bf16 planes of BOTH operands
//              (kernels.h: SplitMap; 3 planes / 6 products carry the full 24-bit significands, fp32 accumulate), the
//              activations between GEMMs stay fp32 (residual stream, rotated q/k/v, softmax, SwiGLU) and are split into
//              planes by the kernel that produces them.
enum { PREC_BF16 = 0, PREC_FP32 = 1 };

// widths of the model, computed once by sr_model_create
struct ModelDims {
    int H, I, V;        // hidden, intermediate, vocabulary
    int nq, nkv;        // q features = num_heads head_dim, k (= v) features = num_kv_heads head_dim
    int n_qkv;          // rows of the fused q | k | v matrix = nq + 2 nkv
    int hd;
};

// Owner of a handle's device allocations: every hipMalloc is recorded with the member that points to it, and the destructor (or
// release) frees them all and resets those members.  The members stay typed raw pointers.
struct DeviceArena {
    struct Block { void* p; void** slot; };
    std::vector<Block> blocks;
    DeviceArena() = default;
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() { release(); }
    // ptr = room for n elements, cleared if zero
    template <typename T>
    int alloc(T*& ptr, int64_t n, bool zero = false) {
        const size_t bytes = (size_t)n * sizeof(T);
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            sr_set_error("sr_model_create: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
            return SR_ERR_NOMEM;
        }
        ptr = (T*)p;
        blocks.push_back(Block{p, (void**)&ptr});
        if (zero) SR_CHECK_HIP(hipMemset(p, 0, bytes));
        return SR_OK;
    }
    // ptr's block was rebuilt out of place: free the old one, ptr and the record take the new one
    template <typename T>
    void replace(T*& ptr, T* now) {
        for (Block& b : blocks)
            if (b.slot == (void**)&ptr) { (void)hipFree(b.p); b.p = now; ptr = now; return; }
    }
    void release() {
        for (Block& b : blocks) { (void)hipFree(b.p); *b.slot = nullptr; }
        blocks.clear();
    }
};

struct LayerW {
    bf16_t* wqkv = nullptr;   // [(nh + 2 nkv) hd, H]
    bf16_t* wo = nullptr;     // [H, nh hd]
    bf16_t* wgu = nullptr;    // [2 I, H], gate/up interleaved in 16-row blocks
    bf16_t* wdown = nullptr;  // [H, I]
    float* ln1 = nullptr;     // [H]
    float* ln2 = nullptr;     // [H]
    unsigned have = 0;        // bit per tensor: q k v o gate up down ln1 ln2
    // fp32 regime (cfg.fp32_planes > 0): the same matrices as split-bf16 plane segments along K, [rows, n_seg * K]
    bf16_t *wqkv_s = nullptr, *wo_s = nullptr, *wgu_s = nullptr, *wdown_s = nullptr;
    // fp16-plane regime: inverse power-of-two scale of every weight row
    float *wqkv_i = nullptr, *wo_i = nullptr, *wgu_i = nullptr, *wdown_i = nullptr;
    // fp16-plane regime, decided by sr_model_finalize: the gate-up GEMM writes the down_proj's planes itself (EPI_SWIGLU_SPLIT_H).
    // false = the row bound is loose for these weights: fp32 SwiGLU output + row split, which scales by the row's maximum
    bool fused_act = true;
    // fp16-plane regime: K segments of wqkv_s, wo_s, wgu_s, wdown_s - 3 = [g0 | g1 | g0], 2 = [g0 | g0] (g1 all zero, dropped by
    // sr_model_finalize); the activations feeding each GEMM are split to the same count
    int qkv_seg = 3, o_seg = 3, gu_seg = 3, down_seg = 3;
    // cfg.attention_bias (Qwen2): bias of the q, k and v rows, [(nh + 2 nkv) hd] fp32 in the order of wqkv, added by the QKV + RoPE
    // epilogues.  bqkv = the checkpoint's values (fp32 regime), bqkv_r = their bf16 roundings held as fp32 (bf16 regime: autocast
    // casts an nn.Linear's bias to bf16)
    float *bqkv = nullptr, *bqkv_r = nullptr;
    unsigned have_bias = 0;   // bit per bias: q k v
};

struct sr_model {
    sr_model_config cfg;
    ModelDims d;
    int Tm = 0, Bm = 0;        // workspace capacity (tokens rounded up to 128, sequences)
    int max_pos = 0;
    float* embed = nullptr;    // fp32 [V, H]
    bf16_t* lm_head = nullptr; // bf16 [V, H] (sparse head)
    bf16_t* lm_head_s = nullptr;   // fp32 regime: [V, n_seg * H] plane segments
    float* lm_head_i = nullptr;    // fp16-plane regime: [V] inverse row scales
    int lm_head_seg = 3;           // fp16-plane regime: K segments of lm_head_s (see LayerW::qkv_seg)
    int* lo_nz = nullptr;          // fp16-plane regime: [4 num_layers + 1] device flags, 1 = the matrix has a nonzero g1 plane
                                   // (layer l: 4 l + 0 qkv, 1 o, 2 gate-up, 3 down; 4 num_layers: lm_head)
    float* gu_cmax = nullptr;      // fp16-plane regime: [num_layers] max_j |w_gate_j||w_up_j| of each layer, see gu_cmax_kernel
    float* norm_w = nullptr;   // [H]
    std::vector<LayerW> layers;
    bool have_embed = false, have_norm = false, have_lm_head = false, finalized = false;
    float* rope_cos = nullptr; // [max_pos, hd/2]
    float* rope_sin = nullptr;
    // workspace
    float* x = nullptr;        // [Tm, H] fp32 residual stream
    bf16_t* xn = nullptr;      // [Tm, H]
    bf16_t* qkv = nullptr;     // [Tm, (nh + 2 nkv) hd]
    bf16_t* attn = nullptr;    // [Tm, nh hd]
    bf16_t* act = nullptr;     // [Tm, I]
    bf16_t* delta = nullptr;   // [Tm, H] bf16 output of o_proj / down_proj, added to x by the next norm kernel
    int *span_start = nullptr, *span_len = nullptr, *pool_start = nullptr, *row_len = nullptr, *cu = nullptr;
    int *tok_id = nullptr, *pos = nullptr, *seq_of = nullptr;
    unsigned char* key_valid = nullptr;
    // fp32-regime workspace, allocated by the first fp32 encode call (ensure_fp32_workspace, encoder.hip)
    bf16_t* xs = nullptr;      // [Tm, n_seg * H]    normed hidden state, plane segments
    float* qkv_f = nullptr;    // [Tm, (nh + 2 nkv) hd] rotated q/k/v, fp32
    bf16_t* attn_s = nullptr;  // [Tm, n_seg * nh hd]
    bf16_t* act_s = nullptr;   // [Tm, n_seg * I]
    float *attn_f = nullptr, *act_f = nullptr;                  // fp16-plane regime: fp32 attention / SwiGLU outputs before the row split
    float *xs_i = nullptr, *attn_i = nullptr, *act_i = nullptr; // ... and the inverse row scales of xs / attn_s / act_s
    float* act_sc = nullptr;                                     // forward row scales of the fused SwiGLU split
    DeviceArena mem;           // weights, tables and the workspace above
    DeviceArena mem_fp32;      // the fp32-regime workspace
    int* h_cu = nullptr;       // pinned host copy of cu_seqlens
    int last_T = 0;
    std::mutex mu;
    StreamOrder order;     // chains calls that arrive on different streams (one set of activation buffers)

    sr_model() = default;
    sr_model(const sr_model&) = delete;
    ~sr_model() {
        if (h_cu) (void)hipHostFree(h_cu);
        order.release();
    }
};
