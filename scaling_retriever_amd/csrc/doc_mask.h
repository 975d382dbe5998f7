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
