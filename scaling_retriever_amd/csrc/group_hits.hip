// Hits inside the groups of a collapsed search (scaling_retriever_amd/collapse.py group_hits): the two device steps
// around the pair scorers - which members of a (query, group) slot the query's filter allows, and the m best entries of every segment
// of a scored CSR.  No reference counterpart: the reference ranks passages only.
//   sr_group_members_count / _fill  eight lanes per (query, slot): the slot's key is found in the ascending table of distinct keys by
//                     binary search (all eight lanes read the same words), then the lanes walk the group's ascending member list eight
//                     ids at a time, test each against the query's bitmap and rank the allowed ones inside the step with one ballot -
//                     so a slot's members come out in ascending order with no atomic.  A workgroup owns 256 consecutive slots; count
//                     leaves a number per slot and a sum per workgroup, one workgroup scans the sums, a third kernel turns the numbers
//                     into the CSR offsets.  What is wrong with the input is recorded per workgroup as the smallest (slot, kind) and
//                     reduced by the scanning workgroup: the first offender in slot order, the same on every run.
//   sr_segment_topm   one wave per segment walks tiles of 64 entries.  The running best 64 sit one per lane, sorted; a tile is sorted
//                     by an in-wave bitonic network on the (score, id) order (no wider than the tile: 8 entries take 6 stages, 64
//                     take 21) and merged into them by one reversed compare and a 6-stage bitonic merge - cross-lane exchanges only,
//                     no LDS array, no atomic.  Once m entries are held, a tile none of whose entries beats the m-th is skipped after
//                     one ballot, which is what keeps a tenant-sized segment cheap.
#include "block_primitives.h"
#include "filter_args.h"
#include <float.h>
#include <limits.h>

#define GH_THREADS 256                          // the four waves of sr_block_scan
#define GH_LANES 8                              // lanes per slot
#define GH_GROUPS (GH_THREADS / GH_LANES)       // slots a workgroup works on at a time
#define GH_SLOTS 256                            // slots per workgroup
#define GH_NONE (~0ull)
#define GH_CHECK_PER 4096                       // offsets per workgroup of the CSR check

// what a kernel found wrong, as (position << 2) | kind: the minimum over a call is its first offender
enum { GH_BAD_GROUP = 1, GH_BAD_KEY = 2, GH_BAD_MEMBER = 3, GH_BAD_START = 1, GH_BAD_ORDER = 2 };

struct MembersArgs {
    const int32_t* slot_keys; int64_t n_slots, kg;
    const int32_t* uniq; int64_t n_groups; const int64_t* member_indptr; const int64_t* member_ids; int64_t n_members;
    const uint32_t* words; int64_t n_masks, n_bits, n_words; const int32_t* query_group;
    int32_t* cnt; long long* block_sums;                                // count
    const int64_t* out_indptr; int64_t* out_ids; int64_t capacity;      // fill
    unsigned long long* block_status; long long* block_detail;
};

template <bool FILL>
__global__ __launch_bounds__(GH_THREADS) void group_members_kernel(MembersArgs a) {
    __shared__ unsigned long long best;
    __shared__ long long sums[GH_GROUPS];
    const int tid = threadIdx.x, sub = tid & (GH_LANES - 1), grp = tid / GH_LANES;
    const int shift = (tid & 63) & ~(GH_LANES - 1);                     // where this slot's lanes sit in the wave's ballot
    if (tid == 0) best = GH_NONE;
    __syncthreads();
    long long sum = 0, my_detail = -1;
    unsigned long long my_bad = GH_NONE;
    const int64_t base = (int64_t)blockIdx.x * GH_SLOTS;
    for (int it = 0; it < GH_SLOTS / GH_GROUPS; ++it) {
        const int64_t slot = base + (int64_t)it * GH_GROUPS + grp;
        if (slot >= a.n_slots) break;
        int code = 0, n_allowed = 0;
        long long detail = -1;
        const int32_t key = a.slot_keys[slot];
        if (key >= 0) {                                                 // a negative key is padding: no members
            int64_t mask_i = 0;
            if (a.n_masks > 0 && a.query_group) {
                mask_i = a.query_group[slot / a.kg];
                if (mask_i < 0 || mask_i >= a.n_masks) code = GH_BAD_GROUP;
            }
            int64_t g = -1;
            if (!code) {
                int64_t lo = 0, hi = a.n_groups;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (a.uniq[mid] < key) lo = mid + 1; else hi = mid;
                }
                if (lo < a.n_groups && a.uniq[lo] == key) g = lo; else code = GH_BAD_KEY;
            }
            if (!code) {
                int64_t lo = a.member_indptr[g], hi = a.member_indptr[g + 1];
                lo = lo < 0 ? 0 : (lo > a.n_members ? a.n_members : lo);       // whatever the table holds, nothing outside it is read
                hi = hi < lo ? lo : (hi > a.n_members ? a.n_members : hi);
                const uint32_t* w = a.n_masks > 0 ? a.words + mask_i * a.n_words : nullptr;
                int64_t at = 0, end = 0;
                if (FILL) {
                    at = a.out_indptr[slot];
                    end = a.out_indptr[slot + 1];
                    end = end > a.capacity ? a.capacity : end;
                }
                if (!FILL && !w) {
                    n_allowed = (int)(hi - lo);
                } else {
                    for (int64_t b = lo; b < hi; b += GH_LANES) {
                        const int64_t i = b + sub;
                        const int64_t id = i < hi ? a.member_ids[i] : 0;
                        bool ok = i < hi;
                        if (w && ok) {
                            if (id < 0 || id >= a.n_bits) {
                                ok = false;
                                if (detail < 0) detail = i;
                            } else {
                                ok = (w[id >> 5] >> (id & 31)) & 1u;
                            }
                        }
                        const unsigned bits = (unsigned)(__ballot(ok) >> shift) & ((1u << GH_LANES) - 1);
                        if (FILL) {
                            const int64_t p = at + __popc(bits & ((1u << sub) - 1));
                            if (ok && p >= 0 && p < end) a.out_ids[p] = id;
                            at += __popc(bits);
                        }
                        n_allowed += __popc(bits);
                    }
                    unsigned long long d = detail < 0 ? GH_NONE : (unsigned long long)detail;
#pragma unroll
                    for (int off = 1; off < GH_LANES; off <<= 1) {
                        const unsigned long long o = __shfl_xor(d, off);
                        d = o < d ? o : d;
                    }
                    if (d != GH_NONE) {
                        code = GH_BAD_MEMBER;
                        detail = (long long)d;
                    }
                }
            }
        }
        if (sub == 0) {
            if (!FILL) {
                a.cnt[slot] = code ? 0 : n_allowed;
                sum += code ? 0 : n_allowed;
            }
            if (code && my_bad == GH_NONE) {                            // a lane group's slots ascend: its first is its smallest
                my_bad = ((unsigned long long)slot << 2) | (unsigned)code;
                my_detail = detail;
            }
        }
    }
    if (my_bad != GH_NONE) atomicMin(&best, my_bad);                    // LDS
    if (!FILL && sub == 0) sums[grp] = sum;
    __syncthreads();
    if (my_bad != GH_NONE && my_bad == best) a.block_detail[blockIdx.x] = my_detail;
    if (tid == 0) {
        a.block_status[blockIdx.x] = best;
        if (best == GH_NONE) a.block_detail[blockIdx.x] = -1;
        if (!FILL) {
            long long t = 0;
            for (int i = 0; i < GH_GROUPS; ++i) t += sums[i];
            a.block_sums[blockIdx.x] = t;
        }
    }
}

// One workgroup: sums [n_sums] -> their exclusive prefix in place; out3 = {the smallest status word, its workgroup's detail (-1 without
// one), the sum}; *d_total (nullable) = the sum.  per_block: positions per workgroup of the kernel that wrote the status words.
__global__ __launch_bounds__(GH_THREADS) void gh_finish_kernel(long long* sums, int64_t n_sums, const unsigned long long* status,
                                                               const long long* detail, int64_t n_status, int64_t per_block,
                                                               int64_t* d_total, long long* out3) {
    __shared__ long long lw[4];
    __shared__ unsigned long long first;
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int64_t b0 = 0; b0 < n_sums; b0 += GH_THREADS) {
        const int64_t i = b0 + tid;
        const long long v = i < n_sums ? sums[i] : 0;
        long long total;
        const long long excl = sr_block_scan(v, lw, total);
        if (i < n_sums) sums[i] = carry + excl;
        carry += total;
    }
    if (tid == 0) first = GH_NONE;
    __syncthreads();
    unsigned long long mine = GH_NONE;
    for (int64_t i = tid; i < n_status; i += GH_THREADS) {
        const unsigned long long s = status[i];
        mine = s < mine ? s : mine;
    }
    if (mine != GH_NONE) atomicMin(&first, mine);                       // LDS
    __syncthreads();
    if (tid == 0) {
        out3[0] = (long long)first;
        out3[1] = (first == GH_NONE || !detail) ? -1 : detail[(int64_t)(first >> 2) / per_block];
        out3[2] = carry;
        if (d_total) *d_total = carry;
    }
}

// out_indptr[slot] = the scanned sum of its workgroup + the prefix of the counts before it inside the workgroup
__global__ __launch_bounds__(GH_THREADS) void group_members_offsets_kernel(const int32_t* cnt, const long long* block_off, int64_t n_slots,
                                                                           int64_t* out_indptr) {
    __shared__ long long lw[4];
    const int64_t slot = (int64_t)blockIdx.x * GH_SLOTS + threadIdx.x;
    const long long v = slot < n_slots ? cnt[slot] : 0;
    long long total;
    const long long excl = sr_block_scan(v, lw, total);
    if (slot < n_slots) out_indptr[slot] = block_off[blockIdx.x] + excl;
}

static int members_run(bool fill, const char* who, const int32_t* d_slot_keys, int64_t nq, int64_t kg, const int32_t* d_uniq_keys,
                       int64_t n_groups, const int64_t* d_member_indptr, const int64_t* d_member_ids, int64_t n_members,
                       const uint32_t* d_mask_words, int64_t n_masks, int64_t n_bits, const int32_t* d_query_group, int64_t* d_indptr,
                       int64_t* total, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 31) && kg >= 0 && kg < (1ll << 31) && nq * kg < (1ll << 38), "%s: bad sizes nq = %lld, kg = %lld", who,
               (long long)nq, (long long)kg);
    SR_REQUIRE(n_groups >= 0 && n_groups < (1ll << 31) && n_members >= 0 && n_members < (1ll << 31), "%s: bad member table sizes", who);
    SR_REQUIRE(n_masks >= 0 && n_bits >= 0 && n_masks < (1ll << 31), "%s: bad mask sizes", who);
    SR_REQUIRE(d_slot_keys && d_uniq_keys && d_member_indptr && d_member_ids && d_indptr && (fill ? d_out_ids != nullptr : total != nullptr),
               "%s: null pointer", who);
    SR_REQUIRE(n_masks == 0 || d_mask_words, "%s: null pointer (n_masks = %lld without d_mask_words)", who, (long long)n_masks);
    SR_REQUIRE(n_masks <= 1 || d_query_group, "%s: null pointer (%lld masks need d_query_group)", who, (long long)n_masks);
    SR_REQUIRE(!fill || capacity >= 0, "%s: bad capacity", who);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_slots = nq * kg;
    if (n_slots == 0) {
        if (!fill) {
            SR_CHECK_HIP(hipMemsetAsync(d_indptr, 0, sizeof(int64_t), s));
            *total = 0;
        }
        return SR_OK;
    }
    const int64_t nb = ceil_div64(n_slots, GH_SLOTS);
    // the call's scratch, freed when it returns: a count per slot (count only), then per workgroup a sum, a status word and its detail,
    // then the three words read back
    const size_t cnt_bytes = fill ? 0 : (((size_t)n_slots * sizeof(int32_t) + 7) & ~(size_t)7);
    const size_t bytes = cnt_bytes + (size_t)nb * 24 + 3 * sizeof(long long);
    CallBuf<unsigned char> scratch;
    if (scratch.reserve((int64_t)bytes, nullptr) != SR_OK) {
        sr_set_error("%s: out of device memory for %zu scratch bytes", who, bytes);
        return SR_ERR_NOMEM;
    }
    MembersArgs a;
    a.slot_keys = d_slot_keys; a.n_slots = n_slots; a.kg = kg;
    a.uniq = d_uniq_keys; a.n_groups = n_groups; a.member_indptr = d_member_indptr; a.member_ids = d_member_ids; a.n_members = n_members;
    a.words = d_mask_words; a.n_masks = n_masks; a.n_bits = n_bits; a.n_words = ceil_div64(n_bits, 32); a.query_group = d_query_group;
    a.cnt = reinterpret_cast<int32_t*>(scratch.p);
    a.block_sums = reinterpret_cast<long long*>(scratch.p + cnt_bytes);
    a.block_status = reinterpret_cast<unsigned long long*>(a.block_sums + nb);
    a.block_detail = reinterpret_cast<long long*>(a.block_status + nb);
    a.out_indptr = d_indptr; a.out_ids = d_out_ids; a.capacity = capacity;
    long long* d_out3 = a.block_detail + nb;
    if (fill) hipLaunchKernelGGL(group_members_kernel<true>, dim3((unsigned)nb), dim3(GH_THREADS), 0, s, a);
    else hipLaunchKernelGGL(group_members_kernel<false>, dim3((unsigned)nb), dim3(GH_THREADS), 0, s, a);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(gh_finish_kernel, dim3(1), dim3(GH_THREADS), 0, s, a.block_sums, fill ? 0 : nb, a.block_status, a.block_detail, nb,
                       (int64_t)GH_SLOTS, fill ? nullptr : d_indptr + n_slots, d_out3);
    SR_CHECK_LAUNCH();
    if (!fill) {
        hipLaunchKernelGGL(group_members_offsets_kernel, dim3((unsigned)nb), dim3(GH_THREADS), 0, s, a.cnt, a.block_sums, n_slots, d_indptr);
        SR_CHECK_LAUNCH();
    }
    long long h[3] = {-1, -1, 0};
    SR_TRY(sr_read_back(h, d_out3, sizeof(h), s));
    if ((unsigned long long)h[0] != GH_NONE) {
        const long long slot = (long long)((unsigned long long)h[0] >> 2), q = slot / kg, j = slot % kg;
        const int code = (int)(h[0] & 3);
        if (code == GH_BAD_GROUP) {
            int32_t g = 0;
            SR_CHECK_HIP(hipMemcpy(&g, d_query_group + q, sizeof(g), hipMemcpyDeviceToHost));
            return sr_bad_group_error(who, q, g, n_masks, "");
        } else if (code == GH_BAD_KEY) {
            int32_t key = 0;
            SR_CHECK_HIP(hipMemcpy(&key, d_slot_keys + slot, sizeof(key), hipMemcpyDeviceToHost));
            sr_set_error("%s: query %lld, slot %lld: key %d is not in the member table", who, q, j, (int)key);
        } else {
            long long id = 0;
            SR_CHECK_HIP(hipMemcpy(&id, d_member_ids + h[1], sizeof(id), hipMemcpyDeviceToHost));
            sr_set_error("%s: query %lld, slot %lld: member id %lld (entry %lld of the member table) is outside the mask's [0, %lld)", who, q, j,
                         id, h[1], (long long)n_bits);
        }
        return SR_ERR_INVALID;
    }
    if (!fill) *total = h[2];
    return SR_OK;
}

extern "C" int sr_group_members_count(const int32_t* d_slot_keys, int64_t nq, int64_t kg, const int32_t* d_uniq_keys, int64_t n_groups,
                                      const int64_t* d_member_indptr, const int64_t* d_member_ids, int64_t n_members,
                                      const uint32_t* d_mask_words, int64_t n_masks, int64_t n_bits, const int32_t* d_query_group,
                                      int64_t* d_out_indptr, int64_t* total, sr_stream stream) {
    return members_run(false, "sr_group_members_count", d_slot_keys, nq, kg, d_uniq_keys, n_groups, d_member_indptr, d_member_ids, n_members,
                       d_mask_words, n_masks, n_bits, d_query_group, d_out_indptr, total, nullptr, 0, stream);
}

extern "C" int sr_group_members_fill(const int32_t* d_slot_keys, int64_t nq, int64_t kg, const int32_t* d_uniq_keys, int64_t n_groups,
                                     const int64_t* d_member_indptr, const int64_t* d_member_ids, int64_t n_members,
                                     const uint32_t* d_mask_words, int64_t n_masks, int64_t n_bits, const int32_t* d_query_group,
                                     const int64_t* d_out_indptr, int64_t* d_out_ids, int64_t capacity, sr_stream stream) {
    return members_run(true, "sr_group_members_fill", d_slot_keys, nq, kg, d_uniq_keys, n_groups, d_member_indptr, d_member_ids, n_members,
                       d_mask_words, n_masks, n_bits, d_query_group, const_cast<int64_t*>(d_out_indptr), nullptr, d_out_ids, capacity, stream);
}

// ------------------------------------------------------------------------------------------------------------ sr_segment_topm
// An entry is (o, id): o the order-preserving word of its score (sr_f2ord: -0.0 and +0.0 share one), id its document.  An empty place is
// (0, INT64_MAX), which every entry beats: ids are below INT64_MAX.
#define GH_NO_ID LLONG_MAX

__device__ inline bool gh_beats(uint32_t ao, long long aid, uint32_t bo, long long bid) { return ao > bo || (ao == bo && aid < bid); }

// compare-exchange with lane ^ j: this lane keeps the better of the two (take_better) or the worse
__device__ inline void gh_exchange(uint32_t& o, long long& id, int j, bool take_better) {
    const uint32_t oo = __shfl_xor(o, j);
    const long long oid = __shfl_xor(id, j);
    const bool swap = take_better ? gh_beats(oo, oid, o, id) : gh_beats(o, id, oo, oid);
    if (swap) {
        o = oo;
        id = oid;
    }
}

// first bad offset of a CSR: indptr[0] != 0, or indptr[i + 1] < indptr[i]; per workgroup the smallest (i << 2) | kind
__global__ __launch_bounds__(GH_THREADS) void segment_check_kernel(const int64_t* indptr, int64_t n_segs, unsigned long long* block_status) {
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) best = GH_NONE;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * GH_CHECK_PER;
    unsigned long long mine = GH_NONE;
    for (int r = 0; r < GH_CHECK_PER / GH_THREADS && mine == GH_NONE; ++r) {
        const int64_t i = base + (int64_t)r * GH_THREADS + threadIdx.x;
        if (i >= n_segs) break;
        const int64_t lo = indptr[i], hi = indptr[i + 1];
        if (i == 0 && lo != 0) mine = GH_BAD_START;
        else if (hi < lo) mine = ((unsigned long long)i << 2) | GH_BAD_ORDER;
    }
    if (mine != GH_NONE) atomicMin(&best, mine);                        // LDS
    __syncthreads();
    if (threadIdx.x == 0) block_status[blockIdx.x] = best;
}

struct TopmArgs {
    const float* scores; const int64_t* ids; const int64_t* indptr; int64_t n_segs; int m; int use_threshold; float threshold, pad_score;
    float* out_scores; int64_t* out_ids; int32_t* out_counts;
};

__global__ __launch_bounds__(GH_THREADS) void segment_topm_kernel(TopmArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * (GH_THREADS / 64) + (threadIdx.x >> 6);
    if (seg >= a.n_segs) return;                                        // whole waves: no barrier below
    const int64_t n_all = a.indptr[a.n_segs];
    int64_t lo = a.indptr[seg], hi = a.indptr[seg + 1];
    lo = lo < 0 ? 0 : (lo > n_all ? n_all : lo);                        // a CSR the check rejects is still read inside its arrays
    hi = hi < lo ? lo : (hi > n_all ? n_all : hi);
    uint32_t ro = 0;                                                    // the running best, sorted: lane 0 the best
    long long rid = GH_NO_ID;
    long long kept = 0;
    bool have = false;
    for (int64_t base = lo; base < hi; base += 64) {
        const int64_t i = base + lane;
        uint32_t o = 0;
        long long id = GH_NO_ID;
        if (i < hi) {
            const float sc = a.scores[i];
            if (!a.use_threshold || sc > a.threshold) {
                o = sr_f2ord(sc);
                id = a.ids[i];
            }
        }
        const bool valid = id != GH_NO_ID;
        kept += __popcll(__ballot(valid));
        if (have) {                                                     // nothing in the tile beats the m-th best: skip it
            const uint32_t ko = __shfl(ro, a.m - 1);
            const long long kid = __shfl(rid, a.m - 1);
            if (!__any(valid && gh_beats(o, id, ko, kid))) continue;
        }
        const int64_t left = hi - base;
        int width = 64;                                                 // the sort is no wider than the tile: a power of two
        if (left < 64) {
            width = 1;
            while (width < left) width <<= 1;
        }
        for (int k = 2; k <= width; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) gh_exchange(o, id, j, ((lane & j) == 0) == ((lane & k) == 0));
        if (!have) {
            ro = o;
            rid = id;
            have = true;
            continue;
        }
        // the best 64 of the two sorted lists: lane by lane the better of the running entry and the tile reversed is a bitonic row
        const uint32_t vo = __shfl(o, 63 - lane);
        const long long vid = __shfl(id, 63 - lane);
        if (gh_beats(vo, vid, ro, rid)) {
            ro = vo;
            rid = vid;
        }
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) gh_exchange(ro, rid, j, (lane & j) == 0);
    }
    if (lane < a.m) {
        const bool valid = rid != GH_NO_ID;
        a.out_scores[seg * a.m + lane] = valid ? sr_ord2f(ro) : a.pad_score;
        a.out_ids[seg * a.m + lane] = valid ? rid : -1;
    }
    if (lane == 0) a.out_counts[seg] = kept > INT_MAX ? INT_MAX : (int32_t)kept;
}

extern "C" int sr_segment_topm(const float* d_scores, const int64_t* d_ids, const int64_t* d_seg_indptr, int64_t n_segs, int m,
                               int use_threshold, float threshold, float pad_score, float* d_out_scores, int64_t* d_out_ids,
                               int32_t* d_out_counts, sr_stream stream) {
    SR_REQUIRE(m >= 1 && m <= 64, "sr_segment_topm: m = %d is outside [1, 64] (the running best sit one per lane)", m);
    SR_REQUIRE(n_segs >= 0 && n_segs < (1ll << 32), "sr_segment_topm: bad n_segs = %lld", (long long)n_segs);
    SR_REQUIRE(d_scores && d_ids && d_seg_indptr && d_out_scores && d_out_ids && d_out_counts, "sr_segment_topm: null pointer");
    if (n_segs == 0) return SR_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = ceil_div64(n_segs, GH_CHECK_PER);
    const size_t bytes = (size_t)nb * sizeof(unsigned long long) + 3 * sizeof(long long);
    CallBuf<unsigned char> scratch;
    if (scratch.reserve((int64_t)bytes, nullptr) != SR_OK) {
        sr_set_error("sr_segment_topm: out of device memory for %zu scratch bytes", bytes);
        return SR_ERR_NOMEM;
    }
    unsigned long long* d_status = reinterpret_cast<unsigned long long*>(scratch.p);
    long long* d_out3 = reinterpret_cast<long long*>(d_status + nb);
    TopmArgs a;
    a.scores = d_scores; a.ids = d_ids; a.indptr = d_seg_indptr; a.n_segs = n_segs; a.m = m; a.use_threshold = use_threshold;
    a.threshold = threshold; a.pad_score = pad_score; a.out_scores = d_out_scores; a.out_ids = d_out_ids; a.out_counts = d_out_counts;
    hipLaunchKernelGGL(segment_check_kernel, dim3((unsigned)nb), dim3(GH_THREADS), 0, s, d_seg_indptr, n_segs, d_status);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(gh_finish_kernel, dim3(1), dim3(GH_THREADS), 0, s, (long long*)nullptr, (int64_t)0, d_status,
                       (const long long*)nullptr, nb, (int64_t)GH_CHECK_PER, (int64_t*)nullptr, d_out3);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(segment_topm_kernel, dim3((unsigned)ceil_div64(n_segs, GH_THREADS / 64)), dim3(GH_THREADS), 0, s, a);
    SR_CHECK_LAUNCH();
    long long h[3] = {-1, -1, 0};
    SR_TRY(sr_read_back(h, d_out3, sizeof(h), s));          // behind the last launch: no copy is in flight when a launch fails
    if ((unsigned long long)h[0] != GH_NONE) {
        const long long i = (long long)((unsigned long long)h[0] >> 2);
        if ((h[0] & 3) == GH_BAD_START) sr_set_error("sr_segment_topm: seg_indptr must start at 0");
        else sr_set_error("sr_segment_topm: seg_indptr decreases behind segment %lld", i);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
