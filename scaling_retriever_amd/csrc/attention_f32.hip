// fp32 bidirectional GQA attention over packed var-len sequences (gfx950) - the fp32 regime of the encoder.
//
// The reference encodes dense queries WITHOUT autocast (eval_dense.py:94-106): SDPA then runs on fp32 q/k/v with an
// fp32 softmax (math path; the float mask of scaling_retriever/modeling/bidirectional_llama.py:138-161 rules out the
// flash kernel).  Attention is ~1 % of the encoder's FLOPs and the fp32 regime is the query side (sequences of ~9
// tokens, 64 at most), so this kernel is plain fp32 FMA work, not MFMA:
//   workgroup = (sequence, q head, block of 16 q rows); its 4 waves own 4 q rows each.
//   keys are walked in chunks of 64: the K chunk is staged once in LDS ([64][hd + 1] floats: a lane = one key reads
//   its row conflict-free, q is a broadcast read), scores / softmax are lane-local + wave reductions, the softmax is
//   carried online across chunks (running max and sum per q row), and P.V reads V rows straight from global memory
//   (lane = head dim: coalesced), p broadcast from LDS.
// q/k arrive rotated (RoPE is fused into the QKV GEMM epilogue).  The output is stored as the split-bf16 plane
// segments the o_proj GEMM consumes (kernels.h: SplitMap).
#include "kernels.h"
#include <math.h>

#define AF_KC 64      // keys per chunk
#define AF_RPW 4      // q rows per wave
#define AF_ROWS 16    // q rows per workgroup

// The FMA kernels below promise the same bits from both of them, and plane segments that are the split of the very value the
// fp32 output form stores.  Both used to rest on what hipcc happened to contract: it built the last four products of a score
// with packed multiplies and plain adds in attention_f32_kernel (a fused chain in attention_f32_gqa_kernel), and it fused
// o * inv into split_bf16x3's first residual (fma(o, inv, -p0): planes of the unrounded product).  So every multiply-add of
// the two kernels is an explicit fmaf, and the output value is rounded to fp32 once, here, before it is stored or split.
__device__ inline float af_mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

template <int HD>
__global__ __launch_bounds__(256) void attention_f32_kernel(AttnF32Args a) {
    constexpr int DPL = HD / 64;                     // head dims per lane
    __shared__ float Ks[AF_KC][HD + 1];
    __shared__ float qs[AF_ROWS][HD];
    __shared__ float ps[AF_ROWS][AF_KC];
    __shared__ unsigned char kval[AF_KC];
    const int b = blockIdx.x, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = a.cu_seqlens[b];
    const int S = a.cu_seqlens[b + 1] - t0;
    const int r0 = blockIdx.z * AF_ROWS;
    if (r0 >= S || S <= a.only_gt) return;
    const int G = a.nh / a.nkv, kvh = h / G;
    const int ld = (a.nh + 2 * a.nkv) * HD;
    const int koff = a.nh * HD + kvh * HD, voff = (a.nh + a.nkv) * HD + kvh * HD;
    const int nrows = (S - r0) < AF_ROWS ? (S - r0) : AF_ROWS;

    for (int i = tid; i < nrows * HD; i += 256) {
        const int r = i / HD, d = i % HD;
        qs[r][d] = a.qkv[(int64_t)(t0 + r0 + r) * ld + h * HD + d];
    }
    float m[AF_RPW], l[AF_RPW], o[AF_RPW][DPL];
#pragma unroll
    for (int r = 0; r < AF_RPW; ++r) {
        m[r] = -INFINITY;
        l[r] = 0.f;
#pragma unroll
        for (int e = 0; e < DPL; ++e) o[r][e] = 0.f;
    }
    for (int k0 = 0; k0 < S; k0 += AF_KC) {
        const int nk = (S - k0) < AF_KC ? (S - k0) : AF_KC;
        __syncthreads();                              // previous chunk fully consumed (and qs visible)
        for (int i = tid; i < nk * HD; i += 256) {
            const int k = i / HD, d = i % HD;
            Ks[k][d] = a.qkv[(int64_t)(t0 + k0 + k) * ld + koff + d];
        }
        if (tid < AF_KC) kval[tid] = (tid < nk) ? a.key_valid[t0 + k0 + tid] : 0;
        __syncthreads();
        const bool valid = kval[lane] != 0;
#pragma unroll
        for (int r = 0; r < AF_RPW; ++r) {
            const int row = wave * AF_RPW + r;      // wave-uniform
            if (row >= nrows) break;
            float s = 0.f;
            for (int d = 0; d < HD; ++d) s = fmaf(qs[row][d], Ks[lane][d], s);
            s = valid ? s * a.scale : -INFINITY;
            float mx = s;
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            if (mx == -INFINITY) continue;          // every key of this chunk is masked
            const float m_new = fmaxf(m[r], mx);
            const float corr = expf(m[r] - m_new);  // 0 on the first chunk (m = -inf)
            const float p = valid ? expf(s - m_new) : 0.f;
            float sum = p;
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
            l[r] = fmaf(l[r], corr, sum);
            m[r] = m_new;
            ps[row][lane] = p;                      // same wave writes and reads this row: no barrier needed
            __builtin_amdgcn_wave_barrier();
            float acc[DPL];
#pragma unroll
            for (int e = 0; e < DPL; ++e) acc[e] = 0.f;
            for (int k = 0; k < nk; ++k) {
                const float pk = ps[row][k];
                const float* vrow = a.qkv + (int64_t)(t0 + k0 + k) * ld + voff;
#pragma unroll
                for (int e = 0; e < DPL; ++e) acc[e] = fmaf(pk, vrow[lane + 64 * e], acc[e]);
            }
#pragma unroll
            for (int e = 0; e < DPL; ++e) o[r][e] = fmaf(o[r][e], corr, acc[e]);
        }
    }
    const int64_t ldo = (int64_t)a.out_map.n_seg * a.nh * HD;
#pragma unroll
    for (int r = 0; r < AF_RPW; ++r) {
        const int row = wave * AF_RPW + r;
        if (row >= nrows) break;
        const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;
        if (a.out_f32) {
#pragma unroll
            for (int e = 0; e < DPL; ++e) a.out_f32[(int64_t)(t0 + r0 + row) * a.nh * HD + h * HD + lane + 64 * e] = af_mul_rn(o[r][e], inv);
            continue;
        }
        bf16_t* orow = a.out + (int64_t)(t0 + r0 + row) * ldo;
#pragma unroll
        for (int e = 0; e < DPL; ++e) {
            unsigned short p[3];
            split_bf16x3(af_mul_rn(o[r][e], inv), p[0], p[1], p[2]);
            const int col = h * HD + lane + 64 * e;
            for (int sg = 0; sg < a.out_map.n_seg; ++sg) orow[(int64_t)sg * a.nh * HD + col] = p[a.out_map.plane[sg]];
        }
    }
}

// The same attention with ONE workgroup per (sequence, KV head, block of 16 q rows): wave w serves q head kvh * G + w, all
// 16 rows of the block four at a time, and the G waves share the staged K chunk; with head_dim 64 the V chunk is staged next
// to it, so that P.V no longer waits for one dependent global load per key (the critical path of the kernel above on the
// ~9-token sequences of the query side: query encode 362 -> 355 ms; grouping the heads alone changed nothing).  Same
// arithmetic per (row, head) as the kernel above (same chunking, same summation order): bit-identical outputs.
template <int HD, int G>
__global__ __launch_bounds__(64 * G) void attention_f32_gqa_kernel(AttnF32Args a) {
    constexpr int DPL = HD / 64;
    constexpr bool V_LDS = HD <= 64;                 // the V chunk too, while both fit the 64 KB of static LDS
    __shared__ float Ks[AF_KC][HD + 1];
    __shared__ float Vs[V_LDS ? AF_KC : 1][V_LDS ? HD : 1];
    __shared__ float qs[G][HD];
    __shared__ float ps[G][AF_KC];
    __shared__ unsigned char kval[AF_KC];
    const int b = blockIdx.x, kvh = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = kvh * G + wave;
    const int t0 = a.cu_seqlens[b];
    const int S = a.cu_seqlens[b + 1] - t0;
    const int r0 = blockIdx.z * AF_ROWS;
    if (r0 >= S || S <= a.only_gt) return;
    const int ld = (a.nh + 2 * a.nkv) * HD;
    const int koff = a.nh * HD + kvh * HD, voff = (a.nh + a.nkv) * HD + kvh * HD;
    const int nrows = (S - r0) < AF_ROWS ? (S - r0) : AF_ROWS;
    const int64_t ldo = (int64_t)a.out_map.n_seg * a.nh * HD;
    // four q rows at a time (their running max / sum / output stay in registers); the K chunk is staged again for every
    // group of four - a few hundred floats for the sequences this kernel is for
    for (int rq = 0; rq < nrows; rq += AF_RPW) {
        float m[AF_RPW], l[AF_RPW], o[AF_RPW][DPL];
#pragma unroll
        for (int r = 0; r < AF_RPW; ++r) {
            m[r] = -INFINITY;
            l[r] = 0.f;
#pragma unroll
            for (int e = 0; e < DPL; ++e) o[r][e] = 0.f;
        }
        for (int k0 = 0; k0 < S; k0 += AF_KC) {
            const int nk = (S - k0) < AF_KC ? (S - k0) : AF_KC;
            __syncthreads();                              // previous chunk fully consumed
            for (int i = tid; i < nk * HD; i += 64 * G) {
                const int k = i / HD, d = i % HD;
                Ks[k][d] = a.qkv[(int64_t)(t0 + k0 + k) * ld + koff + d];
                if constexpr (V_LDS) Vs[k][d] = a.qkv[(int64_t)(t0 + k0 + k) * ld + voff + d];
            }
            if (tid < AF_KC) kval[tid] = (tid < nk) ? a.key_valid[t0 + k0 + tid] : 0;
            __syncthreads();
            const bool valid = kval[lane] != 0;
#pragma unroll
            for (int r = 0; r < AF_RPW; ++r) {
                const int row = rq + r;                 // workgroup-uniform
                if (row >= nrows) break;
#pragma unroll
                for (int e = 0; e < DPL; ++e) qs[wave][lane + 64 * e] = a.qkv[(int64_t)(t0 + r0 + row) * ld + h * HD + lane + 64 * e];
                __builtin_amdgcn_wave_barrier();        // the wave's own row: LDS operations of one wave execute in order
                float s = 0.f;
                for (int d = 0; d < HD; ++d) s = fmaf(qs[wave][d], Ks[lane][d], s);
                s = valid ? s * a.scale : -INFINITY;
                float mx = s;
                for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
                if (mx == -INFINITY) continue;          // every key of this chunk is masked
                const float m_new = fmaxf(m[r], mx);
                const float corr = expf(m[r] - m_new);
                const float p = valid ? expf(s - m_new) : 0.f;
                float sum = p;
                for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
                l[r] = fmaf(l[r], corr, sum);
                m[r] = m_new;
                ps[wave][lane] = p;
                __builtin_amdgcn_wave_barrier();
                float acc[DPL];
#pragma unroll
                for (int e = 0; e < DPL; ++e) acc[e] = 0.f;
                for (int k = 0; k < nk; ++k) {
                    const float pk = ps[wave][k];
                    if constexpr (V_LDS) {               // one dependent global load per key was the kernel's critical path
                        acc[0] = fmaf(pk, Vs[k][lane], acc[0]);
                    } else {
                        const float* vrow = a.qkv + (int64_t)(t0 + k0 + k) * ld + voff;
#pragma unroll
                        for (int e = 0; e < DPL; ++e) acc[e] = fmaf(pk, vrow[lane + 64 * e], acc[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < DPL; ++e) o[r][e] = fmaf(o[r][e], corr, acc[e]);
            }
        }
#pragma unroll
        for (int r = 0; r < AF_RPW; ++r) {
            const int row = rq + r;
            if (row >= nrows) break;
            const float inv = l[r] > 0.f ? 1.0f / l[r] : 0.f;
            if (a.out_f32) {
#pragma unroll
                for (int e = 0; e < DPL; ++e) a.out_f32[(int64_t)(t0 + r0 + row) * a.nh * HD + h * HD + lane + 64 * e] = af_mul_rn(o[r][e], inv);
                continue;
            }
            bf16_t* orow = a.out + (int64_t)(t0 + r0 + row) * ldo;
#pragma unroll
            for (int e = 0; e < DPL; ++e) {
                unsigned short p[3];
                split_bf16x3(af_mul_rn(o[r][e], inv), p[0], p[1], p[2]);
                const int col = h * HD + lane + 64 * e;
                for (int sg = 0; sg < a.out_map.n_seg; ++sg) orow[(int64_t)sg * a.nh * HD + col] = p[a.out_map.plane[sg]];
            }
        }
    }
}

// ---- sequences of at most 64 tokens (the query side: MS MARCO Dev queries are ~9 tokens): fp32 MFMA -----------------------
// v_mfma_f32_16x16x4_f32 multiplies and accumulates in fp32 (bitwise a chain of fmaf, MI355X_MICROARCH.md), so this is still
// exact-fp32 attention; what changes against the kernels above is the shape of the work.  They give a key to every lane and
// a q row to a wave step, which leaves 55 of 64 lanes idle on a 9-token sequence and walks the rows one after another
// (405 us per layer for 16 384 query tokens against a ~75 us floor for reading q/k/v and writing the output once).  Here:
//   workgroup = (sequence, KV head), its 4 waves = the 4 q heads of the group; K and V of the head are staged once in LDS
//   ([keys][hd + 1] floats: conflict-free operand reads), each wave stages its own q rows;
//   S^T = K Q^T per (16 keys x 16 q rows) block - 16 MFMAs for head dim 64 - so that a lane owns ONE q row (its column of
//   S^T): softmax statistics are lane-local + two cross-group shuffles, and the S^T accumulators ARE the A operand of
//   P V (keys contracted in the order 4 g + m: lane group g supplies its register m to MFMA m; V rows are read to match).
// The contraction order is fixed per (row, head) and independent of the batch: outputs do not depend on batch composition.
//
// NKB >= 1 is the product's form, built for bandwidth (the kernel is a chain of memory round trips on ~9-token sequences, so
// what counts is how many workgroups a CU holds and how few round trips each of them waits for):
//   * LDS holds K and V only, 2 x 16 NKB x (hd + 1) floats, NKB = the key-block count ceil(S / 16) of the sequences the LAUNCH
//     serves (launch_attention_f32_mfma: one launch per class 1..4 when the caller knows the class counts, else one launch sized
//     by the batch's longest sequence) - 8.3 KB at NKB = 1 and head dim 64 instead of 33-50 KB by the batch's longest sequence;
//   * q goes from global memory into the MFMA operand registers: lane (g, c) loads the 16-byte pieces 16 i + 4 g .. + 3 of q row c
//     and two half / row swaps per register pair transpose each 4 x 4 piece across the lane groups (af_transpose_groups);
//   * the K / V loads, the q loads of the first q block and the key_valid loads are all issued before the one barrier;
//   * the output block is transposed inside the quads (af_transpose_quad), so a lane stores 4 consecutive head dims of one
//     row: 16 bytes (fp32 form) or 8 bytes per plane segment.
// NKB = 0 keeps the form before that (dev switch SR_ATTN_F32_LAYOUT=0: LDS by the batch's longest sequence, q staged through
// LDS, 4- / 2-byte stores) as the other side of the A/B and of the bit-identity test.  Both forms feed the same values to the
// same MFMA chains and run the same softmax statements, so they give the same bits.

// x[e] of lane group g = M[g][e]  ->  x[k] of lane group g = M[k][g], for the four 16-lane groups of a wave
__device__ __forceinline__ void af_swap32(float& vdst, float& src) {      // lanes 32-63 of vdst <-> lanes 0-31 of src
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(vdst), __float_as_uint(src), false, false);
    vdst = __uint_as_float(r[0]);
    src = __uint_as_float(r[1]);
}
__device__ __forceinline__ void af_swap16(float& vdst, float& src) {      // odd 16-lane rows of vdst <-> even rows of src
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(vdst), __float_as_uint(src), false, false);
    vdst = __uint_as_float(r[0]);
    src = __uint_as_float(r[1]);
}
__device__ __forceinline__ void af_transpose_groups(f32x4& x) {
    // on scalars: __builtin_bit_cast of a vector ELEMENT reads element 0 whatever the index (hipcc 7)
    float x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    af_swap32(x0, x2);
    af_swap32(x1, x3);
    af_swap16(x0, x1);
    af_swap16(x2, x3);
    x = f32x4{x0, x1, x2, x3};
}
// x[r] of lane i of a quad = N[r][i]  ->  x[e] of lane i = N[i][e]  (quad_perm moves: lane ^ 2, then lane ^ 1)
__device__ __forceinline__ float af_quad_xor(float v, int sel) {          // the value of lane ^ 2 (sel 0x4E) or lane ^ 1 (0xB1) of the quad
    return sel == 0x4E ? __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true))
                       : __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}
__device__ __forceinline__ void af_transpose_quad(f32x4& x, int i) {
    float x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    const bool hi2 = (i & 2) != 0, hi1 = (i & 1) != 0;
    const float r0 = af_quad_xor(hi2 ? x0 : x2, 0x4E), r1 = af_quad_xor(hi2 ? x1 : x3, 0x4E);
    if (hi2) { x0 = r0; x1 = r1; } else { x2 = r0; x3 = r1; }
    const float s0 = af_quad_xor(hi1 ? x0 : x1, 0xB1), s1 = af_quad_xor(hi1 ? x2 : x3, 0xB1);
    if (hi1) { x0 = s0; x2 = s1; } else { x1 = s0; x3 = s1; }
    x = f32x4{x0, x1, x2, x3};
}

// waves per SIMD the registers are held to (= workgroups per CU: a workgroup is one wave per SIMD).  Head dim 64: 8 (64 registers)
// for class 1, whose 8.3 KB of LDS admit that many, 6 (80 registers, the form before the plan) for the others.  Head dim 128, whose
// q operand alone is 32 registers: 5 (96, the form before the plan) for classes 1 and 2, 4 (128) for classes 3 and 4, whose 50 / 66 KB
// of LDS admit 3 / 2 workgroups anyway.  The form before the plan keeps the compiler's own choice.
__host__ __device__ constexpr int af_mfma_waves(int hd, int nkb) {
    return nkb == 0 ? 1 : (hd == 64 ? (nkb == 1 ? 8 : 6) : (nkb <= 2 ? 5 : 4));
}

template <int HD, int NKB>
__global__ __launch_bounds__(256, af_mfma_waves(HD, NKB)) void attention_f32_mfma_kernel(AttnF32Args a) {
    constexpr int LDK = HD + 1, CB = HD / 16;
    constexpr bool OLD = NKB == 0;
    constexpr int MKB = OLD ? 4 : NKB;              // key blocks the registers are sized for
    extern __shared__ float af_smem[];
    const int b = blockIdx.x, kvh = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = a.cu_seqlens[b];
    const int S = a.cu_seqlens[b + 1] - t0;
    if (S <= 0 || S > a.only_le) return;
    const int nkb = (S + 15) >> 4;                  // key blocks = q blocks (<= 4)
    if (!OLD && (a.nkb_only ? nkb != a.nkb_only : nkb > NKB)) return;      // another launch's class
    const int SP = nkb * 16;
    float* Ks = af_smem;
    float* Vs = Ks + SP * LDK;
    const int G = a.nh / a.nkv;                     // 4 (checked at launch)
    const int h = kvh * G + wave;
    const int ld = (a.nh + 2 * a.nkv) * HD;
    const int koff = a.nh * HD + kvh * HD, voff = (a.nh + a.nkv) * HD + kvh * HD;
    const int g = lane >> 4, c = lane & 15;
    f32x4 qv[CB];                                   // NKB >= 1: the q operand, qv[i][k] = q[row c][16 i + 4 k + g] once transposed
    auto load_q = [&](int qb) {
#pragma unroll
        for (int i = 0; i < CB; ++i) {
            qv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (16 * qb + c < S) qv[i] = *reinterpret_cast<const f32x4*>(a.qkv + (int64_t)(t0 + 16 * qb + c) * ld + h * HD + 16 * i + 4 * g);
        }
    };
    if constexpr (OLD) {
        for (int i = tid; i < SP * (HD / 4); i += 256) {          // rows beyond the sequence are zeros (0 * p = 0, never NaN)
            const int k = i / (HD / 4), d = (i % (HD / 4)) * 4;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (k < S) {
                kv = *reinterpret_cast<const f32x4*>(a.qkv + (int64_t)(t0 + k) * ld + koff + d);
                vv = *reinterpret_cast<const f32x4*>(a.qkv + (int64_t)(t0 + k) * ld + voff + d);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { Ks[k * LDK + d + e] = kv[e]; Vs[k * LDK + d + e] = vv[e]; }
        }
    }
    // NKB >= 1: every global load the first q block needs is issued before the first LDS write: K and V (16-byte pieces, at most 4 of
    // each per thread in flight at head dim 64 and 2 at 128, where q holds 32 registers; a class with more takes further passes), q, key_valid
    constexpr int NIT = OLD ? 1 : NKB * HD / 64;    // 16-byte pieces of K (and of V) per thread
    constexpr int CHMAX = HD == 64 ? 4 : 2, CH = NIT > CHMAX ? CHMAX : NIT;
    // validity of the keys this lane's S^T registers hold: key = 16 kb + 4 g + r
    unsigned vmask = 0;
    auto load_vmask = [&]() {
#pragma unroll
        for (int kb = 0; kb < MKB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * kb + 4 * g + r;
                if (key < S && a.key_valid[t0 + key]) vmask |= 1u << (4 * kb + r);
            }
    };
    if constexpr (OLD) {
        load_vmask();
    } else {
#pragma unroll
        for (int it0 = 0; it0 < NIT; it0 += CH) {
            f32x4 kreg[CH], vreg[CH];
#pragma unroll
            for (int it = 0; it < CH; ++it) {
                const int i = tid + 256 * (it0 + it), k = i / (HD / 4), d = (i % (HD / 4)) * 4;
                kreg[it] = f32x4{0.f, 0.f, 0.f, 0.f};
                vreg[it] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (k < S) {                        // rows beyond the sequence are zeros (0 * p = 0, never NaN)
                    kreg[it] = *reinterpret_cast<const f32x4*>(a.qkv + (int64_t)(t0 + k) * ld + koff + d);
                    vreg[it] = *reinterpret_cast<const f32x4*>(a.qkv + (int64_t)(t0 + k) * ld + voff + d);
                }
            }
            if (it0 == 0) {
                load_q(0);
                load_vmask();
            }
#pragma unroll
            for (int it = 0; it < CH; ++it) {
                const int i = tid + 256 * (it0 + it), k = i / (HD / 4), d = (i % (HD / 4)) * 4;
                if (k < SP) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { Ks[k * LDK + d + e] = kreg[it][e]; Vs[k * LDK + d + e] = vreg[it][e]; }
                }
            }
            if (it0 + CH < NIT) __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();
    const int64_t ldo = (int64_t)a.out_map.n_seg * a.nh * HD;
    for (int qb = 0; qb < nkb; ++qb) {
        f32x4 st[MKB];
        if constexpr (OLD) {
            // this wave's q rows 16 qb .. + 16 of head h (its own LDS region: LDS operations of one wave execute in order)
            float* Qs = Vs + SP * LDK + wave * 16 * LDK;
            for (int i = lane; i < 16 * (HD / 4); i += 64) {
                const int r = i / (HD / 4), d = (i % (HD / 4)) * 4;
                f32x4 qr = {0.f, 0.f, 0.f, 0.f};
                if (16 * qb + r < S) qr = *reinterpret_cast<const f32x4*>(a.qkv + (int64_t)(t0 + 16 * qb + r) * ld + h * HD + d);
#pragma unroll
                for (int e = 0; e < 4; ++e) Qs[r * LDK + d + e] = qr[e];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int i = 0; i < CB; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) qv[i][k] = Qs[c * LDK + 16 * i + 4 * k + g];
        } else {
            if (HD != 64 && qb > 0) load_q(qb);
#pragma unroll
            for (int i = 0; i < CB; ++i) af_transpose_groups(qv[i]);
        }
#pragma unroll
        for (int kb = 0; kb < MKB; ++kb) {
            st[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (kb < nkb) {
#pragma unroll
                for (int kk = 0; kk < HD / 4; ++kk)
                    st[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(16 * kb + c) * LDK + 4 * kk + g], qv[kk >> 2][kk & 3], st[kb], 0, 0, 0);
            }
        }
        if constexpr (!OLD) {
            // the phases keep to themselves: V operand reads hoisted above the softmax would cost the registers the workgroups per CU rest on
            __builtin_amdgcn_sched_barrier(0);
            // head dim 64: the next q block's loads fly under the softmax and P V (at 128 the registers do not allow it)
            if (HD == 64 && qb + 1 < nkb) load_q(qb + 1);
        }
        // softmax over the keys of q row c (this lane's column of S^T): registers, then the 4 lane groups.  Key blocks beyond
        // MKB would only add max(m, -inf) and sum + 0: the same bits without them
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < MKB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool v = (vmask >> (4 * kb + r)) & 1;
                st[kb][r] = v ? st[kb][r] * a.scale : -INFINITY;
                m = fmaxf(m, st[kb][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float sum = 0.f;
#pragma unroll
        for (int kb = 0; kb < MKB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = (m > -INFINITY && st[kb][r] > -INFINITY) ? expf(st[kb][r] - m) : 0.f;
                st[kb][r] = p;
                sum += p;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;       // every key masked: the row is zero
#pragma unroll
        for (int kb = 0; kb < MKB; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) st[kb][r] *= inv;
        if constexpr (!OLD) __builtin_amdgcn_sched_barrier(0);
        // O = P V: output block cb = head dims 16 cb .. + 16; lane holds O[q row 4 g + r][16 cb + c]
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            // four output blocks (independent MFMA chains) at a time: all eight of head dim 128 in flight cost 32 registers more
            if (!OLD && cb == 4) __builtin_amdgcn_sched_barrier(0);
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < MKB; ++kb) {
                if (kb < nkb) {
#pragma unroll
                    for (int mm = 0; mm < 4; ++mm)
                        o = __builtin_amdgcn_mfma_f32_16x16x4f32(st[kb][mm], Vs[(16 * kb + 4 * g + mm) * LDK + 16 * cb + c], o, 0, 0, 0);
                }
            }
            if constexpr (OLD) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * qb + 4 * g + r;
                    if (row >= S) continue;
                    const int col = h * HD + 16 * cb + c;
                    if (a.out_f32) {
                        a.out_f32[(int64_t)(t0 + row) * a.nh * HD + col] = o[r];
                    } else {
                        unsigned short p[3];
                        split_bf16x3(o[r], p[0], p[1], p[2]);
                        bf16_t* orow = a.out + (int64_t)(t0 + row) * ldo;
                        for (int sg = 0; sg < a.out_map.n_seg; ++sg) orow[(int64_t)sg * a.nh * HD + col] = p[a.out_map.plane[sg]];
                    }
                }
            } else {
                // lane (g, 4 j + i) now holds O[q row 4 g + i][16 cb + 4 j .. + 3]: the 4 lanes of a quad write 64 bytes of a row
                af_transpose_quad(o, c & 3);
                const int row = 16 * qb + 4 * g + (c & 3);
                if (row >= S) continue;
                const int col = h * HD + 16 * cb + (c & 12);
                if (a.out_f32) {
                    *reinterpret_cast<f32x4*>(a.out_f32 + (int64_t)(t0 + row) * a.nh * HD + col) = o;
                } else {
                    unsigned short p[4][3];
#pragma unroll
                    for (int e = 0; e < 4; ++e) split_bf16x3(o[e], p[e][0], p[e][1], p[e][2]);
                    bf16_t* orow = a.out + (int64_t)(t0 + row) * ldo;
                    for (int sg = 0; sg < a.out_map.n_seg; ++sg) {
                        const int pl = a.out_map.plane[sg];
                        bf16x4 w;
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] = (short)(pl == 0 ? p[e][0] : (pl == 1 ? p[e][1] : p[e][2]));
                        *reinterpret_cast<bf16x4*>(orow + (int64_t)sg * a.nh * HD + col) = w;
                    }
                }
            }
        }
    }
}

template <int HD, int NKB>
static int launch_attention_f32_mfma_cfg(const AttnF32Args& a, size_t lds, hipStream_t s) {
    static DeviceOnce attr_once;
    constexpr int max_sp = NKB ? 16 * NKB : 64;
    SR_TRY(sr_allow_lds(attr_once, attention_f32_mfma_kernel<HD, NKB>, (int)(sizeof(float) * (2 * max_sp + (NKB ? 0 : 64)) * (HD + 1))));
    const dim3 grid((unsigned)a.B, (unsigned)a.nkv), block(256);
    SR_REQUIRE(grid.y <= 65535, "attention(fp32): grid too large");
    hipLaunchKernelGGL((attention_f32_mfma_kernel<HD, NKB>), grid, block, lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// one launch of the new form for sequences of at most 16 nkb tokens (a.nkb_only set: of exactly that class)
template <int HD>
static int launch_attention_f32_mfma_class(const AttnF32Args& a, int nkb, hipStream_t s) {
    const size_t lds = sizeof(float) * (size_t)(2 * 16 * nkb) * (HD + 1);
    switch (nkb) {
        case 1: return launch_attention_f32_mfma_cfg<HD, 1>(a, lds, s);
        case 2: return launch_attention_f32_mfma_cfg<HD, 2>(a, lds, s);
        case 3: return launch_attention_f32_mfma_cfg<HD, 3>(a, lds, s);
        default: return launch_attention_f32_mfma_cfg<HD, 4>(a, lds, s);
    }
}

// Launch plan of the <= 64-token kernel.  A sequence's LDS need is set by ITS key-block count nkb = ceil(S / 16), and LDS is what
// bounds the workgroups per CU, so sequences are served by class: one launch per nkb = 1..4 over the whole batch, a workgroup
// leaving at once when its sequence belongs to another launch (one scalar load; at the bench batch 97 % of the sequences are in
// class 1).  The caller that holds cu_seqlens on the host (model_forward, after the sync it already has) passes the class
// counts and empty classes are not launched; a call without them runs ONE launch sized by the batch's longest sequence, which
// serves every class.  The bits of a sequence are the same on every route.
// SR_ATTN_F32_LAYOUT (dev switch, read per call): 0 = the form before the plan (one launch, LDS by the batch's longest sequence,
// q through LDS, element stores); 2 = a launch per class up to the longest sequence's even without counts (tests).
template <int HD>
static int launch_attention_f32_mfma(const AttnF32Args& a_in, hipStream_t s) {
    AttnF32Args a = a_in;
    const int top = (int)ceil_div64(a.max_seqlen < 64 ? a.max_seqlen : 64, 16);
    const char* env = sr_dev_getenv("SR_ATTN_F32_LAYOUT");
    if (env && *env == '0') {
        const size_t lds = sizeof(float) * (size_t)(2 * 16 * top + 4 * 16) * (HD + 1);
        return launch_attention_f32_mfma_cfg<HD, 0>(a, lds, s);
    }
    const bool force = env && *env == '2';
    if (!a.have_classes && !force) {
        a.nkb_only = 0;
        return launch_attention_f32_mfma_class<HD>(a, top, s);
    }
    for (int nkb = 1; nkb <= top; ++nkb) {
        if (a.have_classes && a.class_seqs[nkb - 1] == 0) continue;
        a.nkb_only = nkb;
        SR_TRY(launch_attention_f32_mfma_class<HD>(a, nkb, s));
    }
    return SR_OK;
}

int launch_attention_f32(const AttnF32Args& a_in, hipStream_t s) {
    AttnF32Args a = a_in;
    SR_REQUIRE(a.nh % a.nkv == 0, "attention(fp32): num_heads %d not a multiple of num_kv_heads %d", a.nh, a.nkv);
    SR_REQUIRE(a.out_f32 || (a.out_map.n_seg >= 1 && a.out_map.n_seg <= SR_MAX_SEG), "attention(fp32): bad segment map");
    if (a.B == 0 || a.max_seqlen <= 0) return SR_OK;
    const int G = a.nh / a.nkv;
    a.only_le = 0; a.only_gt = 0;
    const char* env_m = sr_dev_getenv("SR_ATTN_F32_MFMA");    // A/B switch: 0 = the FMA kernels below for every length
    if (G == 4 && (a.hd == 64 || a.hd == 128) && !(env_m && *env_m == '0')) {
        // The kernel is chosen PER SEQUENCE: <= 64 tokens -> the fp32-MFMA kernel, longer -> the FMA kernels.  A mixed batch runs
        // both launches, each skipping the other's sequences (choosing by the batch's longest sequence made the bits
        // of a short sequence depend on its neighbours).
        a.only_le = 64;
        SR_TRY(a.hd == 64 ? launch_attention_f32_mfma<64>(a, s) : launch_attention_f32_mfma<128>(a, s));
        if (a.max_seqlen <= 64) return SR_OK;
        a.only_le = 0; a.only_gt = 64;
    }
    const char* env = sr_dev_getenv("SR_ATTN_F32_GQA");       // A/B switch: 0 = one workgroup per q head
    if (G == 4 && !(env && *env == '0')) {
        const dim3 grid((unsigned)a.B, (unsigned)a.nkv, (unsigned)ceil_div64(a.max_seqlen, AF_ROWS)), block(256);
        SR_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "attention(fp32): grid too large");
        switch (a.hd) {
            case 64: hipLaunchKernelGGL((attention_f32_gqa_kernel<64, 4>), grid, block, 0, s, a); break;
            case 128: hipLaunchKernelGGL((attention_f32_gqa_kernel<128, 4>), grid, block, 0, s, a); break;
            default: sr_set_error("attention(fp32): head_dim %d not supported (64 or 128)", a.hd); return SR_ERR_UNSUPPORTED;
        }
        SR_CHECK_LAUNCH();
        return SR_OK;
    }
    const dim3 grid((unsigned)a.B, (unsigned)a.nh, (unsigned)ceil_div64(a.max_seqlen, AF_ROWS)), block(256);
    SR_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "attention(fp32): grid too large");
    switch (a.hd) {
        case 64: hipLaunchKernelGGL(attention_f32_kernel<64>, grid, block, 0, s, a); break;
        case 128: hipLaunchKernelGGL(attention_f32_kernel<128>, grid, block, 0, s, a); break;
        default: sr_set_error("attention(fp32): head_dim %d not supported (64 or 128)", a.hd); return SR_ERR_UNSUPPORTED;
    }
    SR_CHECK_LAUNCH();
    return SR_OK;
}
