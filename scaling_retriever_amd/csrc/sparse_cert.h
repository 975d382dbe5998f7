// State of the certified two-stage sparse scorer: the index-side structures sparse_cert_build.hip makes once and the per-call buffers
// sparse_cert.hip grows on demand.  The calls other files use are declared in sparse_index.h.
#pragma once
#include "sparse_index.h"
#include <vector>

#define SC_DT 1024                    // docs per tile
#define SC_MB (SC_DT / 32)            // 32-doc M blocks per tile
#define SC_TMAX 128                   // dense terms (MFMA K), at most: 8 k-steps of B fragments in registers, 8 KB of them in LDS

// Every device buffer is a DeviceBuf: reserve() where it is filled, release() in sparse_cert_destroy, nothing else.
struct SparseCert {
    int T = 0, KS = 0;                // dense terms (multiple of 16) and MFMA k-steps
    int n_tiles = 0;
    float vscale = 1.f;               // power of two applied to the values before the fp16 rounding
    DeviceBuf<int32_t> dslot;         // [V] dense slot of a term, -1 = rare
    DeviceBuf<float> vmax;            // [V] largest value of a posting list
    DeviceBuf<_Float16> d16;          // [n_tiles][SC_MB][KS][64][8]: MFMA A fragments (row = doc, k = dense slot); a matrix wave streams 4 KS KB per tile
    DeviceBuf<uint32_t> P;            // [nnz] packed postings: (doc % SC_DT / 2) * 4 | doc % 2  (byte offset of the doc's LDS word | its half) | fp16(v * vscale) << 16
    DeviceBuf<uint32_t> S;            // [V][n_tiles + 1]: first posting (absolute index) of term t with doc >= tile * SC_DT
    DeviceBuf<uint32_t> E;            // [V][e_stride]: the run of term t inside tile i in one word: 0 = empty, a packed posting | 2 = its only
                                      // posting, 0xffff0000 | length = two or more postings (in P from the running start on)
    int e_stride = 0;                 // n_tiles rounded up to 4, + 4: 16-byte rows, a 16-byte read never leaves its row
    DeviceBuf<int64_t> fwd_indptr;    // doc-major forward index, terms ascending inside a doc
    DeviceBuf<uint64_t> fwd_tv;       // [nnz] term << 32 | value bits: one 16-byte load per lane brings two postings of a row
    // per-call plan (grown on demand, cert_ensure_call_buffers)
    DeviceBuf<_Float16> bfrag;        // [nq_pad / 32][KS][64][8]: MFMA B fragments (k = dense slot, col = query)
    DeviceBuf<int32_t> rare_term;     // [nq_pad][SC_MAXRT], -1 = none
    DeviceBuf<float> rare_w;          // [nq_pad][SC_MAXRT]: q_t * s_q * 65535 / vscale
    DeviceBuf<float> cq;              // [nq_pad]: MFMA sum -> [0, 1]
    DeviceBuf<float> sq;              // [nq_pad]: score -> [0, 0.98]
    DeviceBuf<int32_t> n_rare;        // [nq_pad]
    DeviceBuf<int32_t> n_qt;          // [nq_pad]
    DeviceBuf<int32_t> n_drop;        // [nq_pad] rare terms left out of stage 1 (weight below fp16's normal range)
    DeviceBuf<float> tau2;            // [nq_pad] k-th best key so far (topk_compact2), 0 until a select has run: the band below it is the filter threshold
    DeviceBuf<uint8_t> elig;          // [nq_pad]
    DeviceBuf<uint8_t> overflow;      // [nq_pad]
    DeviceBuf<int32_t> m_count;       // [nq_pad] candidates to re-score
    DeviceBuf<int64_t> ap_ids;        // [nq_pad][2 k_eff] approximate top lists
    DeviceBuf<int> d_n_uncert;        // [4]: uncertified queries, candidates re-scored (in units of 16), largest rare-term count, queries on the fast path
    DeviceBuf<uint8_t> d_uncert;      // flags of a search's batch (kept: a hipMalloc / hipFree pair per search synchronises the device)
    TopkWS ws;
    // statistics (sr_sparse_index_cert_stats)
    int64_t n_calls = 0, n_queries = 0, n_uncert = 0, n_rescored = 0;
    DeviceBuf<uint16_t> dump;         // debug: [nq_pad][n_tiles * SC_DT] keys of the last search (sr_sparse_index_cert_debug)
    bool want_dump = false;
    // what sr_sparse_index_cert_readout needs beyond the buffers themselves: the index's posting count and the shape of the last search
    int64_t nnz = 0, last_nq = 0, last_nq_pad = 0;
    int last_k = 0, last_k_eff = 0;
    std::vector<uint8_t> h_uncert;    // the last search's uncertified flags, kept on the host while the key recording is on
    DeviceBuf<unsigned long long> d_stamps;   // [80] dev switch SR_CERT_STAMPS of a -DSC_STAMPS=1 build
    DeviceBuf<uint32_t> mask_pad;     // [n_tiles * SC_MB] a search's document bitmap as the masked score kernel walks it (sparse_cert_mask_pad), allocated on first use
    // a grouped search's bitmaps (sparse_cert_group_pad), allocated on first use and grown on demand
    DeviceBuf<uint32_t> group_pad;    // [n_groups + 1][n_tiles * SC_MB]: every group's bitmap in the kernel's length, then their union
    DeviceBuf<uint32_t> group_qoff;   // [nq rounded up to 32]: word offset of the query's group in group_pad, 0 behind the last query
};
