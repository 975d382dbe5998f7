// Document bitmaps (doc_mask.hip): the two forms of a document filter - a strictly ascending list of global doc indices and a bitmap
// over [0, n_bits), bit (i & 31) of word i >> 5 - and the conversions between them.  What faiss calls IDSelectorBitmap.
#pragma once
#include "common.h"
#include "pair_score.h"

#define SR_DOC_MASK_BLOCK_BITS 8192      // bits per workgroup of the mask -> list kernels: 256 words, one per thread
static inline int64_t doc_mask_words(int64_t n_bits) { return ceil_div64(n_bits, 32); }
static inline int64_t doc_mask_blocks(int64_t n_bits) { return ceil_div64(n_bits, SR_DOC_MASK_BLOCK_BITS); }

// words [ceil(n_bits / 32)] := 0, then bit list[j] set for every j < m (atomic or: repeats are harmless).  An entry outside [0, n_bits)
// sets nothing and raises *d_bad (nullable) to 1.  st (nullable): the status word of a search - once its check kernel has found an
// offender nothing is scattered.
int launch_doc_mask_from_list(const int64_t* d_list, int64_t m, uint32_t* d_words, int64_t n_bits, const PairStatus* st, int* d_bad,
                              hipStream_t s);
// The set bits below n_bits as an ascending list, in two steps so that a caller can size the list in between:
//   count   popcount per word, summed per workgroup into d_blocks [doc_mask_blocks(n_bits)], then an exclusive scan of those in place;
//           *d_count = the number of set bits
//   expand  every workgroup writes its bits in ascending order from its scanned offset; entries at or beyond `capacity` are dropped
// Bits of the last word at or beyond n_bits are ignored.
int launch_doc_mask_count(const uint32_t* d_words, int64_t n_bits, int64_t* d_blocks, int64_t* d_count, hipStream_t s);
int launch_doc_mask_expand(const uint32_t* d_words, int64_t n_bits, const int64_t* d_blocks, int64_t* d_list, int64_t capacity, hipStream_t s);
// The two ways the filtered searches use them.  d_blocks [doc_mask_blocks(n_bits) + 1]: the count's scratch, then the number of set bits.
//   count_sync  the count, and *m := the number of set bits: one 8-byte read-back, one wait
//   list        d_list [m] := the ascending list of a bitmap whose m set bits are known: the count runs for the per-workgroup offsets
//               the expansion starts from; no wait
int doc_mask_count_sync(const uint32_t* d_words, int64_t n_bits, int64_t* d_blocks, hipStream_t s, int64_t* m);
int doc_mask_list(const uint32_t* d_words, int64_t n_bits, int64_t m, int64_t* d_blocks, int64_t* d_list, hipStream_t s);

// ---- filter groups (sr_dense_search_grouped): n_groups bitmaps stacked as [n_groups, W], W = doc_mask_words(n_bits) ----
// d_valid [W] |= the positions id_base + r * id_stride, r < n, of one segment (those below n_bits; the caller has zeroed the words)
int launch_doc_mask_add_segment(uint32_t* d_valid, int64_t n_bits, int64_t n, int64_t id_base, int64_t id_stride, hipStream_t s);
// One word-parallel pass over all groups: d_counts[g] := the set bits of group g below n_bits; d_counts[n_groups] := the smallest
// (g * W + word) * 32 + bit over the set bits below n_bits that are not set in d_valid, ~0 if there is none (d_valid null: every
// position names a document, nothing is tested).  n_groups * W < 2^32.
int launch_doc_masks_check(const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits, const uint32_t* d_valid, int64_t* d_counts,
                           hipStream_t s);
// d_union [W] := the OR of the bitmaps of the groups d_used[0 .. n_used) (int32, each in [0, n_groups)); all zero for n_used = 0.  The
// grouped range search skips the tiles where it is clear.
int launch_doc_masks_union(const uint32_t* d_group_words, const int32_t* d_used, int64_t n_used, int64_t n_bits, uint32_t* d_union,
                           hipStream_t s);
// d_qoff[q] := d_query_group[q] * W for q < nq (group ids already checked), 0 for nq <= q < nq_pad
int launch_doc_mask_query_offsets(const int32_t* d_query_group, int64_t nq, int64_t nq_pad, int64_t n_bits, uint32_t* d_qoff, hipStream_t s);
