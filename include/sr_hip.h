/* sr_hip.h - C ABI of libsr_hip.so, the MI355X (gfx950) encode + retrieval hot path
 * of scaling-retriever.
 *
 * Every entry point replaces one piece of the reference's Python hot path; the
 * reference interface it stands in for is cited as file:line into
 * HansiZeng/scaling-retriever.  Plain C types only: opaque handles, device
 * pointers (what torch's tensor.data_ptr() returns), sizes, and a hipStream_t
 * passed as void*.  All functions return 0 on success, non-zero on error
 * (sr_last_error() then holds a message for the calling thread).  The library
 * never frees caller memory; output buffers are caller-allocated.
 *
 * Threading: the reference calls its scorer from 4 Python threads with the GIL
 * released (scaling_retriever/indexer.py:325,459), so search entry points are
 * re-entrant: each handle owns its workspace and serialises concurrent calls on
 * an internal mutex (the GPU runs a whole query batch per call; threads are a
 * CPU artefact of the reference) and, when those calls arrive on different
 * streams, chains their device work through an event so that the workspace is
 * never used by two calls at once.  Different handles never share mutable state.
 */
#ifndef SR_HIP_H
#define SR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SR_OK 0
#define SR_ERR_INVALID 1
#define SR_ERR_HIP 2
#define SR_ERR_NOMEM 3
#define SR_ERR_UNSUPPORTED 4

#define SR_DTYPE_F32 0
#define SR_DTYPE_BF16 1
#define SR_DTYPE_F16 2 /* IEEE binary16: row storage of a dense index (sr_dense_index_add_f16) */

typedef void* sr_stream; /* hipStream_t; NULL = default stream */

const char* sr_last_error(void);
int sr_version(void);
/* Largest k served by the in-LDS top-k path (4096).  Not a limit on k: every search and merge below accepts
 * 1 <= k <= 2^30 (the dense search: see sr_dense_search); a larger k goes through a top-k in global memory with the same
 * results (any other k: SR_ERR_INVALID). */
int sr_max_topk(void);

/* ------------------------------------------------------------------ dense ---
 * Replaces DenseFlatIndexer.init_index / index_data / search_knn
 * (scaling_retriever/indexer.py:191-217) over faiss.IndexFlatIP:
 * exact fp32 inner products, k best per query, sorted descending; ties broken
 * by ascending doc index; rows padded with (-FLT_MAX, -1) when ntotal < k.   */
typedef struct sr_dense_index sr_dense_index;

int sr_dense_index_create(sr_dense_index** out, int dim);
/* Registers a segment of `n_rows` fp32 row-major [n_rows, dim] embeddings that
 * already live in device memory (non-owning view; caller keeps it alive).
 * Global doc index of local row r is id_base + r * id_stride (id_stride = W and
 * id_base = rank reproduces the reference's g_row = row*W + rank sharding,
 * indexer.py:262).  Global indices must fit in 32 bits.                      */
int sr_dense_index_add(sr_dense_index* idx, const float* d_rows, int64_t n_rows,
                       int64_t id_base, int64_t id_stride);
/* The same for rows stored as IEEE binary16 (half the HBM bytes of the index, half the bytes every search streams): a
 * non-owning view of row-major binary16 [n_rows, dim] in device memory, 16-byte aligned; id rules as above.  An index holds
 * EITHER fp32 rows OR fp16 rows - its first non-empty add decides; adding the other kind returns SR_ERR_INVALID and leaves
 * the index unchanged.
 * Contract: on an fp16 index every entry point below (sr_dense_search, _begin / _finish, sr_dense_score_pairs, any k,
 * batch-invariant on or off, SR_PRECISION_FP32 and SR_PRECISION_FP32_FILTERED) returns BIT FOR BIT what the same call returns
 * on an fp32 index whose rows are those binary16 values widened to fp32 (widening is exact; subnormals, +-0, inf and NaN
 * included).  The kernels read the fp16 rows and widen them in registers, in the k order of the fp32 kernels; the library never
 * keeps an fp32 copy of the rows (sr_dense_index_owned_bytes).  The only loss of information is the caller's one rounding at
 * ingest, fp32 -> binary16 to nearest even: for |x| in the normal range of binary16 the score of a pair then differs from the
 * score of the unrounded row by at most 2^-11 * sum_i |q_i d_i| <= 2^-11 |q| |d| (plus the fp32 chain's own rounding).
 * SR_PRECISION_BF16X3 and SR_PRECISION_BF16X6 are not available on an fp16 index (an 11-bit significand does not fit one bf16
 * plane): sr_dense_index_set_precision returns SR_ERR_UNSUPPORTED for them, and so does this call on an index in one of
 * these two modes.                                                                                                             */
int sr_dense_index_add_f16(sr_dense_index* idx, const void* d_rows_f16, int64_t n_rows,
                           int64_t id_base, int64_t id_stride);
/* SR_DTYPE_F32 or SR_DTYPE_F16: what the index's rows are stored as (an empty index: SR_DTYPE_F32; a null index: -1). */
int sr_dense_index_row_dtype(const sr_dense_index* idx);
/* *out = device bytes the LIBRARY holds per segment, summed over the segments: the bf16 planes of the split precisions and the
 * certified filter's fp16 plane with its per-document (x, y) terms and their per-128-document maxima.  The rows themselves
 * belong to the caller and workspaces (candidate buffers, query planes) are not counted.  0 for an index that was only ever
 * searched in SR_PRECISION_FP32 - whatever its row type: no mode keeps a widened copy of fp16 rows.                        */
int sr_dense_index_owned_bytes(sr_dense_index* idx, int64_t* out);
int64_t sr_dense_index_ntotal(const sr_dense_index* idx);
/* d_queries: fp32 [nq, dim] on device.  1 <= k <= 2^30, and a k above sr_max_topk() at most sr_max_topk() beyond the
 * index's document count (k <= ntotal + 4096: rows of at most 4096 padding entries; a larger k is SR_ERR_INVALID, as any
 * k > 4096 was before).  The caller provides d_out_scores fp32 [nq, k] and
 * d_out_ids int64 [nq, k] (global doc indices).  For k > sr_max_topk() the running top-k (16 k bytes per query) and the
 * select's buffers (4 k bytes per query) count against the workspace limit next to the candidate buffer; a call that does not
 * fit runs in query sub-batches of more than 64 queries each (same bits as one batch).  If even the smallest such batch does
 * not fit, the call returns SR_ERR_NOMEM (the byte count in sr_last_error()) and writes nothing.  The certified filter of
 * SR_PRECISION_FP32_FILTERED needs k + 64 candidates in the in-LDS path: a larger k runs the exact kernel.
 * Order of every top-k this library returns (dense, sparse, subset / masked, merge): score descending with the scores compared as
 * float values, then doc index ascending.  -0.0 and +0.0 are one score: between them the doc index alone decides, and a returned
 * score of -0.0 reads back as +0.0.                                                                                          */
int sr_dense_search(sr_dense_index* idx, const float* d_queries, int64_t nq, int k,
                    float* d_out_scores, int64_t* d_out_ids, sr_stream stream);
/* Arithmetic of the score kernel for query batches > 64:
 *   SR_PRECISION_FP32   (default) exact fp32 MFMA, bit-for-bit a k-ordered fmaf chain;
 *   SR_PRECISION_BF16X3 fp32 operands split into bf16 hi + lo, q.d ~= qh.dh + qh.dl + ql.dh on the
 *                       bf16 MFMA pipe with fp32 accumulation, ~3x faster.  Per pair, with S = sum_i |q_i d_i|
 *                       (<= |q||d|): |score - q.d| <= (2 + 2^-6) 2^-16 S from the dropped terms (reached to 3 % by
 *                       data whose roundings all point one way) + 3.1 dim 2^-24 S from the accumulation of 3 dim
 *                       exact products: about 2^-15 S, NOT the size of an fp32 summation-order change.  Typical
 *                       (Gaussian) data shows ~1e-6 |q||d| at dim 256, where the roundings cancel.  Keeps a
 *                       library-owned bf16 copy of every segment (same bytes as the fp32 rows). */
#define SR_PRECISION_FP32 0
#define SR_PRECISION_BF16X3 1
/*   SR_PRECISION_BF16X6 three bf16 planes per operand (the full 24-bit significand), six products:
 *                       |score - q.d| <= (1 + 2^-6) 2^-24 S + 6.2 dim 2^-24 S per pair - the error class of an fp32
 *                       dot product (typical data: ~1e-7 |q||d|); ~1.7x faster than fp32 MFMA; keeps three bf16
 *                       planes per segment.
 *   Both: the bounds are derived in tests/dense_split_cases.py and held for every pair by tests/test_dense_split_gpu.py;
 *   add 2^-134 sum_i (|q_i| + |d_i|) where operands are so small that planes fall under bf16's smallest subnormal.
 *   A finite operand has finite planes (the first plane saturates at the largest finite bf16 number instead of
 *   rounding to infinity).  Scores of operands that hold inf or NaN are unspecified in these two modes.          */
#define SR_PRECISION_BF16X6 2
/*   SR_PRECISION_FP32_FILTERED  the SAME results as SR_PRECISION_FP32, bit for bit, several times faster for batches
 *                       > 64 queries: one fp16 plane product (fp16 rounding of the query x fp16 rounding of the document,
 *                       both scaled by powers of two) plus a per-pair error term e(q, j) built from the ACTUAL rounding
 *                       residuals |d - d0|, |q - q0| (Cauchy-Schwarz) gives an upper bound U >= the exact fp32 score of
 *                       every pair; the 3k documents with the largest U are the candidates, those that can still reach
 *                       the top-k are re-scored with the exact fp32 fmaf chain, and the certificate U_3k < (k-th exact
 *                       score found) proves that the result is the exact top-k.  A query without a certificate (more
 *                       than 2k near-ties at the cut, a zero or non-finite query) is re-done by the exact kernel, that
 *                       query alone.  Keeps one fp16 plane + 8 bytes per document (half the bytes of the fp32 rows);
 *                       without room for it, or for data that is not finite, the exact kernel is used.            */
#define SR_PRECISION_FP32_FILTERED 3
int sr_dense_index_set_precision(sr_dense_index* idx, int mode);
/* Doc-sharded search in two halves (replaces nothing in the reference, which scores on ONE process: eval_dense.py:191; this
 * is the multi-GPU row of SURVEY.md 8e).  Every rank calls _begin on its shard: d_lower [nq] receives, per query, a value that
 * at least ceil(k / share) documents of THIS shard reach exactly (share = number of shards).  The minimum of d_lower over the
 * shards (one small all-reduce) is therefore not above the global k-th exact score; every rank passes it to _finish as
 * d_threshold and re-scores only the candidates that can reach the GLOBAL top-k (about k / share of them instead of k).  The
 * shard's [nq, k] output then holds those (padding: score -FLT_MAX, id -1); sr_topk_merge of the shards' outputs is the global
 * top-k, bit for bit what one index over all documents returns.  When the certified filter does not apply, d_lower is -inf and
 * _finish is a plain sr_dense_search (d_threshold may be null); that is always the case for k > sr_max_topk() - 64.  k as for
 * sr_dense_search.  Do not interleave other searches on the handle between the two. */
int sr_dense_search_begin(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, int share,
                          float* d_lower, sr_stream stream);
int sr_dense_search_finish(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const float* d_threshold,
                           float* d_out_scores, int64_t* d_out_ids, sr_stream stream);
/* searches of more than 64 queries answered by the filter alone / with some (or all) queries re-done by the exact kernel.  A
 * search with k > sr_max_topk() is counted in neither: the filter is never eligible for it.                               */
int sr_dense_index_filter_stats(sr_dense_index* idx, int64_t* n_filtered, int64_t* n_fallback);
/* the same per query: queries certified by the filter / re-done by the exact kernel so far */
int sr_dense_index_filter_query_stats(sr_dense_index* idx, int64_t* n_certified, int64_t* n_redone);
/* Workspace ceiling in bytes for candidate buffers (default 4 GiB). */
int sr_dense_index_set_workspace_limit(sr_dense_index* idx, int64_t bytes);
/* on != 0: batches of <= 64 queries run the tiled kernels instead of the streaming one, so that EVERY batch size accumulates in
 * one k order: a query's ids and fp32 scores are then the same bits alone, in a batch of 8 and in a batch of 6 980 (cost: a pass
 * of <= 32 queries reads D at ~4.4 TB/s instead of ~5.9).  Off (default): batches <= 64 and larger ones are each exact fp32 chains
 * but differ in the last bit - as faiss's IndexFlatIP.search does between its small-batch loop and its sgemm path (the switch at
 * 20 queries that /root/reference/scaling_retriever/indexer.py:211 inherits).                                                     */
int sr_dense_index_set_batch_invariant(sr_dense_index* idx, int on);
/* Scores of GIVEN (query, document) pairs from the rows the index already holds.  Replaces DecoderOnlyBiDense.rerank_forward
 * (scaling_retriever/modeling/llm_encoder.py:593-615: `(query_rep * doc_rep).sum(dim=-1)` after encoding both sides of every
 * pair again) behind eval_reranker.py:107-160 for documents that are in the index.  Candidates as CSR over the queries:
 * d_cand_indptr int64 [nq + 1] (starts at 0, never decreases; total = d_cand_indptr[nq]), d_cand_ids int64 [total] = global doc
 * indices as sr_dense_search returns them (id_base + row * id_stride of a segment); lists may be empty, may repeat a document and
 * have no length limit.  d_out_scores fp32 [total]: out[p] for d_cand_indptr[q] <= p < d_cand_indptr[q + 1] is the fp32 fmaf chain
 * of query q and that document in the k order of the exact score kernel (per 8 columns k = 8s + j, then 8s + 4 + j, j = 0..3), for
 * EVERY nq: a pair's score does not depend on what else is in the call.  It therefore equals, bit for bit, the score sr_dense_search
 * returns for that pair whenever the search accumulates in that order - more than 64 queries, or dim % 256 != 0, or
 * sr_dense_index_set_batch_invariant(idx, 1) - in every precision mode whose results are the exact kernel's (SR_PRECISION_FP32,
 * SR_PRECISION_FP32_FILTERED).  An id that is in no segment: SR_ERR_INVALID, sr_last_error() names the first such pair (found on
 * the device); d_out_scores then holds NaN at the offending pairs and scores elsewhere - do not use it.  A d_cand_indptr that does
 * not start at 0 or decreases: SR_ERR_INVALID, nothing written.  The work is queued on `stream`; the call then waits for it once,
 * to read that status back (no other host synchronisation, no size read-back before the launch).                              */
int sr_dense_score_pairs(sr_dense_index* idx, const float* d_queries, int64_t nq, const int64_t* d_cand_indptr,
                         const int64_t* d_cand_ids, float* d_out_scores, sr_stream stream);
/* Top-k within a SUBSET of the documents: one allow-list shared by all queries of the call (what faiss offers as IDSelector on a
 * flat index).  No reference counterpart: DenseFlatIndexer.search_knn (scaling_retriever/indexer.py:191-217) always ranks the whole
 * index; this extends it.  d_subset int64 [m] on the device, STRICTLY ASCENDING global doc indices as sr_dense_search returns them
 * (id_base + row * id_stride of a segment; fp32- and fp16-stored rows alike), m >= 0.  The result is what sr_dense_search with
 * k = ntotal returns after the documents outside the subset are removed and the list is cut to k: order, tie order (ascending doc
 * index) and padding (-FLT_MAX, -1; every row when m = 0) as there.  k as for sr_dense_search with m in place of the document count
 * (k <= m + 4096).  Scores: the fp32 fmaf chain in the exact kernel's k order for EVERY nq - the contract of sr_dense_score_pairs, so a
 * returned score equals the score sr_dense_score_pairs gives that (query, document), bit for bit, and the score of sr_dense_search
 * whenever that search accumulates in the same order (see there); it does not depend on m, on nq or on what else is in the subset.
 * A tile of 64 subset rows is gathered once per block of 16 queries: a row is read from HBM at most ceil(nq / 16) times.  Nothing
 * of size nq x m is allocated: the subset goes through in slabs, and the queries in sub-batches, sized from the handle's workspace
 * limit (8 bytes per query and slab entry; for k > sr_max_topk() the large select's buffers as in sr_dense_search) with the same
 * bits; SR_ERR_NOMEM if one query with a slab of 64 entries does not fit.  Errors: an entry that is in no segment, or is not above
 * its predecessor: SR_ERR_INVALID, found on the device, sr_last_error() names the first offending position; every output row is
 * then padding.  Synchronisation as sr_dense_score_pairs: the work is queued on `stream`, the call waits for it once to read the
 * status back, no size is read back before the launches.                                                                        */
int sr_dense_search_subset(sr_dense_index* idx, const float* d_queries, int64_t nq, int k,
                           const int64_t* d_subset, int64_t m,
                           float* d_out_scores, int64_t* d_out_ids, sr_stream stream);
/* Two routes serve sr_dense_search_subset, with the same bits.  gather: the kernel described above.  mask: on an index in
 * SR_PRECISION_FP32_FILTERED, under the conditions the unrestricted filtered search has (nq > 64, max(3k, k + 2048) <= sr_max_topk()
 * candidates - k <= 1 365; the unrestricted search cuts a longer list to sr_max_topk() instead - with room for k + 64, dim % 64 == 0
 * and >= 128, every segment filterable), the list is turned into a bitmap and the
 * certified filter's upper-bound pass runs over ALL rows on the MFMA pipe with one bit test where a pair would become a key: a
 * document whose bit is clear never becomes a key, so the thresholds and the certificate are quantities over the allowed set and the
 * filter's argument holds for that set word for word.  Candidates are re-scored by the exact chain as in sr_dense_search; queries left
 * without a certificate are re-done by the gather route over the list, those alone (more than half the batch: all of it) - its chains
 * are the exact kernel's, so no masked exact kernel exists.  sr_dense_index_filter_stats / _filter_query_stats count such a search like
 * any other.  Rule: the mask route where it applies and nq * m >= 6 980 * 130 000 (where the two met on one box); dev switch
 * SR_SUBSET_DENSE_ROUTE=gather|mask forces one (read per call; `mask` where it does not apply is served by gather).  The mask route
 * reads the call's status once BEFORE its pass instead of at the end; a bad list is then handled by the gather route as above.  The
 * handle keeps the bitmap (id_end / 8 bytes), allocated on first use.  Not under a mask: the sparse head, doc-sharded search,
 * the streaming / bf16x3 / bf16x6 passes, batches of <= 64 queries (gather).  A mask per query: sr_dense_search_grouped below.   */
/* The largest document index of any segment, plus one (not ntotal: segments have id_base / id_stride); 0 for an empty index, -1 for a
 * null one.  The length in bits of a document bitmap of this index.                                                              */
int64_t sr_dense_index_id_end(const sr_dense_index* idx);
/* Document bitmaps: bit (i & 31) of word i >> 5 stands for global doc index i (what faiss calls IDSelectorBitmap).
 * sr_doc_mask_from_list: d_words uint32 [ceil(n_bits / 32)] := 0, then the bit of every entry of d_list int64 [m] set (any order,
 * repeats allowed).  An entry outside [0, n_bits) sets nothing: SR_ERR_INVALID after the other entries were set.  Waits for the
 * stream once to read that status.
 * sr_doc_list_from_mask: the set bits below n_bits as an ascending list (popcount per word, scan, ordered expand) into d_list int64
 * [capacity]; *d_count (device) = the number of set bits, written even when it exceeds capacity (the list then holds the first
 * `capacity` of them).  Bits of the last word at or beyond n_bits are ignored.  Waits for the stream (its scan scratch is freed).    */
int sr_doc_mask_from_list(const int64_t* d_list, int64_t m, uint32_t* d_words, int64_t n_bits, sr_stream stream);
int sr_doc_list_from_mask(const uint32_t* d_words, int64_t n_bits, int64_t* d_list, int64_t capacity,
                          int64_t* d_count, sr_stream stream);
/* A bitmap carried over to another numbering: bit i of d_dst_words uint32 [ceil(n_dst_bits / 32)] := bit d_map[i] of d_src_words where
 * 0 <= d_map[i] < n_src_bits (d_map int64 [n_dst_bits] on the device), else 0; the unused bits of the last word are 0.  Entries of
 * d_map may repeat.  One thread per destination word, no atomics, queued on `stream`, no read-back.  The exact hybrid search turns a
 * mask over dense positions into one over sparse positions with it (d_map = s2d).                                                  */
int sr_doc_mask_remap(const uint32_t* d_src_words, int64_t n_src_bits, const int64_t* d_map, int64_t n_dst_bits,
                      uint32_t* d_dst_words, sr_stream stream);
/* sr_dense_search_subset with the allow-list given as a bitmap: d_mask_words uint32 [ceil(n_bits / 32)] on the device, n_bits ==
 * sr_dense_index_id_end(idx) (anything else: SR_ERR_INVALID before any device work).  Returns EXACTLY what sr_dense_search_subset
 * returns for the ascending list of the set bits - ids, score bits, tie order, padding, limits on k (with m = the number of set bits) -
 * whichever route served the call.  The bitmap is expanded to that list on the device (8 m bytes on the handle, sized by one 8-byte
 * read-back of the count), the list goes through the check of sr_dense_search_subset, then the same two routes and route rule.  A
 * set bit that names no document (a gap of a strided segment): SR_ERR_INVALID, sr_last_error() names the first such bit; the
 * status is read once, every output row is then padding (for any k) and the index stays usable.  The call waits for the stream twice
 * before any scoring (the count, then the status), and on the mask route once more for the certificate's flags.                   */
int sr_dense_search_masked(sr_dense_index* idx, const float* d_queries, int64_t nq, int k,
                           const uint32_t* d_mask_words, int64_t n_bits,
                           float* d_out_scores, int64_t* d_out_ids, sr_stream stream);
/* Dense top-k under per-query document filters (filter groups).  d_group_words uint32 [n_groups, W] on the device, W =
 * ceil(n_bits / 32): n_groups bitmaps in the bit convention of sr_dense_search_masked, stacked; n_bits == sr_dense_index_id_end(idx);
 * d_query_group int32 [nq] on the device: query q searches under bitmap d_query_group[q].  One group is sr_dense_search_masked,
 * n_groups == nq a filter of its own per query; a group without queries is allowed.
 * Result: for every group g, the output rows of the queries with d_query_group[q] == g are EXACTLY what sr_dense_search_masked returns
 * for those queries alone, in their order, under bitmap g - ids, score bits, tie order (ascending doc index) and padding (-FLT_MAX, -1:
 * a group with fewer than k allowed documents, or none) - for every group size, 1 included, on fp32 and fp16 rows, contiguous and
 * strided segments, whichever route served the call (the subset searches' scores do not depend on nq, so this is well defined).
 * k: 1 <= k <= sr_max_topk(); a larger k is SR_ERR_INVALID.  Sizes: n_groups >= 1 and n_groups * W < 2^32.
 * Errors, all SR_ERR_INVALID: n_bits != id_end, a bad k or n_groups, or a null pointer with nq > 0 - before any device work; an entry of
 * d_query_group outside [0, n_groups) - sr_last_error() names the first such query; a set bit below n_bits that names no document (a
 * gap of a strided segment) - sr_last_error() names the first such (group, bit).  In the last two cases nothing is scored, every
 * output row is padding and the index stays usable.  The bitmaps are tested in one word-parallel pass against a bitmap of the indexed
 * positions (id_end / 8 bytes on the handle, built from the segment table, rebuilt when a segment was added; not needed, not built, for
 * stride-1 segments that cover [0, id_end)) - no group is expanded to a list to be validated.
 * Routes, the same bits.  (1) The grouped pass: under the conditions of the masked search's mask route (SR_PRECISION_FP32_FILTERED,
 * nq > 64, k <= 1 365, dim % 64 == 0, dim >= 128, every segment filterable) the certified filter's upper-bound pass with the bit test
 * reading the query's own bitmap (4 nq bytes of word offsets on the handle); thresholds, certificate and re-score are per-query
 * quantities over that query's allowed documents, so the filter's argument holds as for one mask.  Queries left without a certificate
 * are re-done by the gather route under their own group's list, those alone, group by group.  (2) The group loop, everywhere else: per
 * group with a query in it, its queries gathered, its bitmap expanded to the ascending list (8 m_g bytes on the handle, one group at a
 * time), the gather route, the rows scattered back.  Rule: the pass where it applies and sum_g nq_g * m_g >= 6 980 * 130 000 - the
 * constant of the subset searches, measured for ONE group; the loop's per-group overhead moves the real crossover down as groups
 * multiply, and that has not been measured.  Dev switch SR_GROUPED_DENSE_ROUTE=pass|loop forces one (read per call; `pass` where it
 * does not apply is served by the loop).
 * Synchronisation: the call waits for the stream twice before any scoring - the group ids (4 nq bytes), then the per-group counts with
 * the gap check's word (8 n_groups + 8 bytes); then the pass route once for the certificate's flags, as the masked search does, and
 * once more only if queries were re-done; the loop route once at its end.
 * sr_dense_index_filter_stats / _filter_query_stats count a call that ran the grouped pass like any filtered search (the loop: not at
 * all).  Also under groups: the range search (sr_dense_range_count_grouped / _fill_grouped below) and, in Python, the exact hybrid
 * search (hybrid.search_fused(masks=, query_group=)).  Not offered under groups: k > sr_max_topk(), doc-sharded search.  The sparse
 * head under groups is sr_sparse_search_grouped.                                                                                    */
int sr_dense_search_grouped(sr_dense_index* idx, const float* d_queries, int64_t nq, int k,
                            const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits,
                            const int32_t* d_query_group,
                            float* d_out_scores, int64_t* d_out_ids, sr_stream stream);
/* Range search: EVERY document whose score exceeds a per-query threshold, as CSR - faiss's IndexFlatIP.range_search(x, thresh) ->
 * (lims, D, I) with one threshold per query, and on the dense head what the reference's sparse scorer does with its threshold
 * (numba_score_float, scaling_retriever/indexer.py:315-344: every document with score > threshold).  Two calls, because the size of
 * the result is not known before the scores are:
 *   sr_dense_range_count  d_thresholds fp32 [nq] on the device.  Writes d_lims int64 [nq + 1] (device; lims[0] = 0, lims[q + 1] -
 *       lims[q] = the number of documents with score > thr[q]) and *total (host) = lims[nq]; it waits for the stream once, to read
 *       those 8 bytes.  The handle keeps a table of per-chunk prefixes (4 bytes per query and chunk of rows, at most 1 024 chunks,
 *       counted against the workspace limit: fewer, longer chunks under a small limit, SR_ERR_NOMEM with the byte count when one chunk
 *       per segment does not fit), nq and a stamp of the segment list.
 *   sr_dense_range_fill   the same queries, thresholds and d_lims.  For query q, d_out_scores fp32 / d_out_ids int64 [capacity] hold at
 *       lims[q] .. lims[q + 1] every indexed document with score > thr[q] and nothing else, in (segment, row) order - ascending doc index
 *       whenever the segments cover ascending id ranges.  Needs a preceding sr_dense_range_count on this handle with the same nq and an
 *       unchanged index, and capacity >= that count's total: anything else is SR_ERR_INVALID and nothing is written.  Queued on
 *       `stream`, no read-back.  As with _begin / _finish, do not interleave other range calls on the handle.  With queries or
 *       thresholds other than the count's the lists are not meaningful, but no entry outside its query's segment of the output (and
 *       none at or beyond capacity) is ever written.
 * A hit is score > thr[q], strict; a NaN score or threshold is never a hit, +inf returns nothing, -inf every document with a score
 * above -inf.  nq = 0 or an empty index: lims all zero, total 0.  Scores: the exact fp32 chain of sr_dense_score_pairs (per 8 columns
 * k = 8s + j, then 8s + 4 + j) for EVERY nq, 1 included, whatever sr_dense_index_set_precision says: a returned score equals
 * sr_dense_score_pairs of that pair bit for bit, and sr_dense_search's wherever that search accumulates in this order.  fp32 and fp16
 * rows alike (the twin contract of sr_dense_index_add_f16).  No atomics: two calls return the same bytes.  Under a document bitmap:
 * sr_dense_range_count_masked / _fill_masked below; under a bitmap per query: sr_dense_range_count_grouped / _fill_grouped.  Not
 * offered: a range search under a list (a caller with a short list has sr_dense_score_pairs), doc-sharded, or on the certified
 * filter's 16-bit pass.                                                                                           */
int sr_dense_range_count(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                         int64_t* d_lims, int64_t* total, sr_stream stream);
int sr_dense_range_fill(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                        const int64_t* d_lims, float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream);
/* The range search under a document bitmap: d_mask_words uint32 [ceil(n_bits / 32)] on the device, in the bit convention
 * of sr_dense_search_masked, n_bits == sr_dense_index_id_end(idx) (anything else: SR_ERR_INVALID before any device work).  A hit is
 * score > thr[q] AND the bit of the document's global index is set; everything else is the contract of sr_dense_range_count / _fill
 * word for word: (segment, row) order, the score bits of sr_dense_score_pairs for every nq, fp32 and fp16 rows, no atomics, the
 * guard p < min(lims[q + 1], capacity) on every store, and the pairing on the handle - a fill needs a preceding count of the same kind
 * with the same nq (a masked fill after an unmasked count, or the reverse: SR_ERR_INVALID) and the count's bitmap.  Bits are
 * consulted only at the indices of indexed documents: a set bit in a gap of a strided segment is ignored, not an error (unlike
 * sr_dense_search_masked, which names it), bits of the last word at or beyond n_bits are ignored, and the library never reads past
 * word ceil(n_bits / 32) - 1.  The bitmap is read in place by both passes: keep it unchanged between the count and its fill.  A
 * 256-row tile whose bits are all clear is skipped whole (no loads, no MFMAs), so a clustered filter costs about its share of
 * non-empty tiles; under a uniformly random filter nearly every tile holds an allowed row and the pass costs what the unrestricted
 * one does.  Per-query masks: sr_dense_range_count_grouped / _fill_grouped below.  Not offered: doc-sharded.                       */
int sr_dense_range_count_masked(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                const uint32_t* d_mask_words, int64_t n_bits, int64_t* d_lims, int64_t* total, sr_stream stream);
int sr_dense_range_fill_masked(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                               const uint32_t* d_mask_words, int64_t n_bits, const int64_t* d_lims, float* d_out_scores,
                               int64_t* d_out_ids, int64_t capacity, sr_stream stream);
/* The range search under a document bitmap PER QUERY (filter groups): d_group_words uint32 [n_groups, W], W =
 * ceil(n_bits / 32), one bitmap per group in the convention above, n_bits == sr_dense_index_id_end(idx); d_query_group int32 [nq]: query
 * q searches under bitmap d_query_group[q].  All on the device.
 * Contract: for every group g the lists of the queries with d_query_group[q] == g are EXACTLY what sr_dense_range_count_masked /
 * _fill_masked return for those queries under bitmap g - lengths, ids, score bits (the chain of sr_dense_score_pairs) and (segment, row)
 * order - on fp32 and fp16 rows, contiguous and strided segments, for every nq, 1 included.  One group is the masked call byte for byte;
 * n_groups == nq, a group without a query and an all-clear bitmap are all valid.  The guard p < min(lims[q + 1], capacity) is on every
 * store; no atomics: two calls return the same bytes.  Bits are consulted only at the indices of indexed documents (a set bit in a gap
 * of a strided segment is ignored) and nothing past word W - 1 of a group's bitmap is read.
 * A 256-row tile is skipped when the UNION of the bitmaps of the groups that have a query is clear there; the count builds that union
 * (W words) and the queries' word offsets (4 bytes per query, rounded up to 256 queries) on the handle, counted against the workspace
 * limit (SR_ERR_NOMEM with the byte count where they do not fit), and the fill reuses both: the fill does not read d_query_group again,
 * which - like the bitmaps - must be what the count was given.  The hit test reads the query's own bitmap behind the product of a tile.
 * Errors, all SR_ERR_INVALID.  Before any device work: n_bits != id_end, n_groups < 1, n_groups * W >= 2^32, a null pointer with nq > 0.
 * An entry of d_query_group outside [0, n_groups): found before any scoring (the count waits for the stream once to read the 4 nq
 * bytes), sr_last_error() names the first such query, d_lims is written as zeros and *total as 0, and no fill can follow.  Pairing on
 * the handle: three kinds - unrestricted, masked, grouped; a fill needs a preceding count of its own kind with the same nq (and, grouped,
 * the same n_groups); any mix is SR_ERR_INVALID and nothing is written.
 * Not offered under groups: doc-sharded indexes.                                                                                   */
int sr_dense_range_count_grouped(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                 const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits, const int32_t* d_query_group,
                                 int64_t* d_lims, int64_t* total, sr_stream stream);
int sr_dense_range_fill_grouped(sr_dense_index* idx, const float* d_queries, int64_t nq, const float* d_thresholds,
                                const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits, const int32_t* d_query_group,
                                const int64_t* d_lims, float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream);
int sr_dense_index_destroy(sr_dense_index* idx);
/* Measurement hook: while enabled, every launch of the score kernel is bracketed by HIP
 * events on the search stream.  _read synchronises those events and returns the number
 * of launches, their summed duration (ms) and the algorithmic work they covered
 * (2*nq*rows*dim FLOP, rows*dim*4 bytes of D - *2 for fp16-stored rows), then clears the log. */
int sr_dense_index_profile(sr_dense_index* idx, int enable);
int sr_dense_index_profile_read(sr_dense_index* idx, int64_t* n_launches, double* total_ms,
                                double* total_flop, double* total_d_bytes);

/* ----------------------------------------------------------------- sparse ---
 * Replaces SparseRetrieval.numba_score_float + select_topk
 * (scaling_retriever/indexer.py:315-344): per query, term-serial
 * scores[doc] += q_t * v (unfused fp32 multiply-add, ascending query-term
 * order), keep docs with score > threshold, k best; sorted descending, ties by
 * ascending doc index.  The index is the IndexDictOfArray posting lists
 * (scaling_retriever/utils/inverted_index.py:15-105) laid out as CSR by term. */
typedef struct sr_sparse_index sr_sparse_index;

/* d_indptr int64 [n_terms+1], d_doc_ids int32 [nnz], d_vals fp32 [nnz], all on
 * device (non-owning views).  Inside each posting list doc ids must be strictly
 * ascending (checked).  n_docs = IndexDictOfArray.nb_docs().                  */
int sr_sparse_index_create(sr_sparse_index** out, const int64_t* d_indptr,
                           const int32_t* d_doc_ids, const float* d_vals,
                           int64_t n_terms, int64_t n_docs, sr_stream stream);
/* Queries as CSR: d_q_indptr int64 [nq+1] (non-decreasing), d_q_cols int32, d_q_vals fp32 (term
 * order inside a query = accumulation order).  A term id outside [0, n_terms) is an
 * empty posting list, as in the reference's vocabulary-filled dict (indexer.py:364-370).  Outputs [nq, k] padded with
 * (0, -1); d_out_counts int32 [nq] = number of valid entries per row.  1 <= k <= 2^30: the caller provides [nq, k]
 * outputs; for k > sr_max_topk() the query batches shrink so that the running top-k (20 k bytes per query with the select's
 * buffers) and one 8 192-doc tile of candidates per query fit the workspace limit, SR_ERR_NOMEM if one query does not.
 * Global doc index = id_base + doc * id_stride.                              */
int sr_sparse_search(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols,
                     const float* d_q_vals, int64_t nq, int k, float threshold,
                     int64_t id_base, int64_t id_stride,
                     float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts,
                     sr_stream stream);
int sr_sparse_index_set_workspace_limit(sr_sparse_index* idx, int64_t bytes);
/* Scores of GIVEN (query, document) pairs.  Replaces DecoderOnlyBiSparse.rerank_forward (scaling_retriever/modeling/llm_encoder.py:
 * 593-615 as inherited by the sparse classes: both sides encoded again, then the product summed over the vocabulary) behind
 * eval_reranker.py:107-160.  Queries as for sr_sparse_search, candidates as for sr_dense_score_pairs; d_cand_ids = document positions
 * in [0, n_docs) (what sr_sparse_search returns with id_base 0, id_stride 1).  out[p] = scores[doc] of numba_score_float
 * (scaling_retriever/indexer.py:324-340): for each query term in the order given - repeated terms each time they appear, term ids
 * outside [0, n_terms) skipped - an unfused fp32 multiply then add, from +0.0f.  No threshold: a pair without a common term scores
 * 0.0f.  Any query and any index sr_sparse_search accepts; the bits do not depend on the route (the forward index of the certified
 * scorer where the index has one and the query's terms are valid and strictly ascending, the posting lists otherwise; dev switch
 * SR_PAIR_SPARSE_ROUTE=postings forces the latter).  Errors, d_out_scores after an error and synchronisation: as
 * sr_dense_score_pairs.                                                                                                         */
int sr_sparse_score_pairs(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                          int64_t nq, const int64_t* d_cand_indptr, const int64_t* d_cand_ids, float* d_out_scores,
                          sr_stream stream);
/* sr_sparse_search within a SUBSET of the documents, one allow-list shared by all queries.  No reference counterpart: it extends
 * SparseRetrieval.numba_score_float + select_topk (scaling_retriever/indexer.py:315-344), which score the whole collection.
 * d_subset int64 [m] on the device, STRICTLY ASCENDING document positions in [0, n_docs) (as for sr_sparse_score_pairs), m >= 0.
 * Queries, threshold, id_base / id_stride, outputs, padding (0, -1) and d_out_counts as sr_sparse_search, 1 <= k <= 2^30: the result is
 * what sr_sparse_search with k = n_docs returns after the documents outside the subset are removed and the list is cut to k.  Scores
 * are the term-serial unfused chain of sr_sparse_search / sr_sparse_score_pairs and do not depend on m, nq or the rest of the subset.
 * Three routes, the same bits.  pairs: one wave per (query, subset document) on the chains of sr_sparse_score_pairs, for m < n_docs /
 * 16.  array: the score array per 8 192-document tile with a gathered select over the subset's entries, above that.  mask: where
 * sr_sparse_search would run the certified scorer (the index has one, k + 1 024 <= sr_max_topk(), n_docs >= 8 (k + 1 024)), the list is
 * turned into a bitmap and the scorer's pass runs over the whole collection with one bit test where a document would become a
 * stage-1 key; its certificate then holds for the allowed documents alone, the candidates are re-scored by the exact chain from the
 * forward index, and queries it hands back are re-done by pairs / array over the list.  Rule: the mask route where it applies and
 * nq * m >= 64 * 1 000 000 (where it met the faster list route on one box at 8.84 M documents, for 64 and for 6 980 queries:
 * DESIGN.md 4.16), else pairs / array as above.  Dev switch SR_SUBSET_SPARSE_ROUTE=pairs|array|mask forces one (read per call; mask
 * where the scorer does not apply, or for an empty list, is served by the pairs / array rule); the mask route reads the
 * call's status once BEFORE its pass instead of at the end, and then waits for the stream as sr_sparse_search does.  Workspace, errors
 * (a position outside [0, n_docs) or not above its predecessor) and synchronisation otherwise as sr_dense_search_subset.          */
int sr_sparse_search_subset(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols,
                            const float* d_q_vals, int64_t nq, int k, float threshold,
                            const int64_t* d_subset, int64_t m, int64_t id_base, int64_t id_stride,
                            float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, sr_stream stream);
/* sr_sparse_search_subset with the allow-list given as a bitmap (what faiss calls IDSelectorBitmap): d_mask_words uint32
 * [ceil(n_bits / 32)] on the device, bit (i & 31) of word i >> 5 stands for document position i, n_bits == n_docs (anything else:
 * SR_ERR_INVALID before any device work).  Bits of the last word at or beyond n_bits are ignored, as in sr_doc_list_from_mask, and the
 * library never reads past that word.  Every position names a document, so a set bit is never invalid.  Returns EXACTLY what
 * sr_sparse_search_subset returns for the ascending list of the set bits - ids, score bits, tie order, padding (0, -1), counts,
 * threshold semantics, id_base / id_stride, limits on k, workspace errors (with m = the number of set bits) - whichever route served
 * the call; the routes, the route rule and its dev switch are those of sr_sparse_search_subset.  The list is expanded on the device
 * (8 m bytes on the handle) only where pairs / array serve the call or re-do queries the mask route hands back; the mask route keeps
 * a copy of the bitmap in the length its kernel walks (n_docs / 8 bytes rounded up to whole 1 024-document tiles, counted against the
 * workspace limit).  sr_sparse_index_cert_stats counts a masked pass like any other.  The call waits for the stream once for the
 * count of set bits, then on the mask route as sr_sparse_search does (twice per batch of 8 192 queries, and once more per batch with
 * handed-back queries); on the list routes not again.  Not under a mask: doc-sharded search (a mask per query is
 * sr_sparse_search_grouped below; the range search under a mask is sr_sparse_range_count_masked / _fill_masked).                   */
int sr_sparse_search_masked(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols,
                            const float* d_q_vals, int64_t nq, int k, float threshold,
                            const uint32_t* d_mask_words, int64_t n_bits, int64_t id_base, int64_t id_stride,
                            float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, sr_stream stream);
/* Filter groups for the sparse head: every query searches within its OWN set of allowed documents, in one call (the counterpart of
 * sr_dense_search_grouped).  d_group_words uint32 [n_groups, W], W = ceil(n_bits / 32): one bitmap per group in the bit convention of
 * sr_sparse_search_masked, n_bits == n_docs; bits of a row's last word at or beyond n_bits are ignored and the library never reads past
 * a row.  d_query_group int32 [nq]: query q searches under bitmap d_query_group[q].  All on the device.
 * Contract: for every group g the output rows of the queries with d_query_group[q] == g are EXACTLY what sr_sparse_search_masked returns
 * for those queries alone, in their order, under bitmap g - counts, ids, score bits, tie order, padding (0, -1), threshold semantics,
 * id_base / id_stride - whichever route served the call.  n_groups == nq, a group without queries and an all-zero bitmap are all valid.
 * 1 <= k <= 2^30, as for the masked search.
 * Errors, all SR_ERR_INVALID.  Before any device work: n_bits != n_docs, n_groups < 1, (n_groups + 1) * n_tiles * 32 >= 2^32 (n_tiles =
 * ceil(n_docs / 1 024)), a bad k, or a null pointer with nq > 0.  An entry of d_query_group outside [0, n_groups): sr_last_error()
 * names the first such query, nothing is scored, every output row is padding with count 0, and the index stays usable.  Every sparse
 * position names a document, so a set bit is never invalid.
 * Routes, the same bits.  (1) The grouped pass, where sr_sparse_search_masked's mask route is eligible (the index has the certified
 * scorer, k + 1 024 <= sr_max_topk(), n_docs >= 8 (k + 1 024)), at least one group with a query has a set bit, and the scorer's copy of
 * the bitmaps - every group in the length its kernel walks plus their union, (n_groups + 1) * n_tiles * 128 bytes on the handle,
 * allocated on first use and grown on demand - fits the workspace limit: ONE pass of the certified scorer in which the bit test reads
 * the query's own bitmap (4 bytes of word offset per query on the handle) and the block skip reads the union.  Thresholds, band cut and
 * certificate are per-query quantities over that query's allowed documents, so the scorer's argument holds as for one mask.  Queries it
 * hands back (not eligible, band does not fit, fewer than k allowed documents with a non-zero key - the queries of an all-zero group
 * among them, which are then not scored at all -, candidate overflow, no memory for the batch) are re-done by the list routes (pairs /
 * array) under their own group's list, those alone, group by group, the list expanded one group at a time (8 m_g bytes on the handle);
 * there is no second, wider-band pass under groups.  (2) The group loop, everywhere else: per group with a query in it, its queries
 * gathered into a CSR of their own, the body of sr_sparse_search_masked under that group's bitmap (which picks pairs / array / mask by
 * its own rule and dev switch, and serves any k), the rows scattered back.  Rule: the pass where it is eligible and
 * sum_g nq_g * m_g >= 64 * 1 000 000 - the constant of the masked search, measured for ONE group; the loop's per-group overhead moves
 * the real crossing down as groups multiply.  Dev switch SR_GROUPED_SPARSE_ROUTE=pass|loop forces one (read per call;
 * `pass` where it is not eligible is served by the loop).
 * Synchronisation: the call waits for the stream twice before any scoring - the group ids (4 nq bytes), then the per-group counts of
 * set bits (8 n_groups bytes, one word-parallel pass over all bitmaps).  Then the pass waits as sr_sparse_search does (twice per batch
 * of 8 192 queries) and, for a batch with handed-back queries, once for their flags, once for the query offsets (8 (nq + 1) bytes) and
 * once at the end of the re-do; the loop waits once for the query offsets, per group as sr_sparse_search_masked does, and once at its
 * end.  sr_sparse_index_cert_stats counts a grouped pass like any other search; the loop's masked bodies count as they do on their own.
 * Also under groups: the range search (sr_sparse_range_count_grouped / _fill_grouped below) and, in Python, the exact hybrid search.
 * Not offered under groups: doc-sharded search.                                                                                    */
int sr_sparse_search_grouped(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols,
                             const float* d_q_vals, int64_t nq, int k, float threshold,
                             const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits,
                             const int32_t* d_query_group, int64_t id_base, int64_t id_stride,
                             float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, sr_stream stream);
/* Range search: EVERY document whose score exceeds a per-query threshold, as CSR.  This is what the reference's scorer computes before
 * select_topk cuts it (numba_score_float, scaling_retriever/indexer.py:324-344: the score array starts at zero, every query term is
 * scatter-added in term order, then every document with score > threshold is returned in document order), with one threshold per query;
 * the reference's scalar is the special case.  Two calls, because the size of the result is not known before the scores are:
 *   sr_sparse_range_count  queries as for sr_sparse_search (term order = accumulation order, a repeated term counts each time, a term
 *       id outside [0, n_terms) is an empty list), 0 <= nq < 2^24 per call (a larger nq: SR_ERR_INVALID); d_thresholds fp32 [nq] on the device.  Writes d_lims int64 [nq + 1] (device; lims[0] =
 *       0, lims[q + 1] - lims[q] = the number of documents with score > thr[q]) and *total (host) = lims[nq]; it waits for the stream
 *       once, to read those 8 bytes.  The handle keeps a table of 4 bytes per (query, chunk of doc tiles) - one 8 192-document tile per
 *       chunk by default, counted against sr_sparse_index_set_workspace_limit: where 4 * nq * tiles exceeds the limit a chunk grows to
 *       the smallest number of tiles that fits, SR_ERR_NOMEM with the byte count when one chunk per query does not - together with nq,
 *       the chunk size and the total.
 *   sr_sparse_range_fill   the same queries, thresholds and d_lims.  For query q, d_out_scores fp32 / d_out_ids int64 [capacity] hold at
 *       lims[q] .. lims[q + 1] every hit and nothing else, in ascending document position d; ids = id_base + d * id_stride in int64
 *       (id_base >= 0, id_stride >= 1; no 32-bit limit, no key is packed).  Needs a preceding sr_sparse_range_count on this handle with
 *       the same nq, and capacity >= that count's total: anything else is SR_ERR_INVALID and nothing is written.  Queued on `stream`, no
 *       read-back.  Do not interleave other range calls on the handle.  Every store is guarded by p < min(lims[q + 1], capacity): with
 *       queries or thresholds other than the count's the lists are not meaningful, but no entry outside its query's segment of the
 *       output (and none at or beyond capacity) is ever written.
 * A hit is score > thr[q], strict, over every document position in [0, n_docs).  A document that shares no term with the query has score
 * +0.0f and is a hit exactly when thr[q] < 0, as in the reference.  A NaN score or threshold is never a hit, +inf returns nothing, -inf
 * every document with a score above -inf.  nq = 0 or n_docs = 0: lims all zero, total 0.  Scores: the term-serial chain
 * of sr_sparse_search / sr_sparse_score_pairs - an unfused fp32 multiply then add, in the query's term order, from +0.0f - so a returned
 * score equals sr_sparse_score_pairs of that pair bit for bit.  No global atomic takes part in placing a result: two calls return the
 * same bytes.  Under a document bitmap: sr_sparse_range_count_masked / _fill_masked below; under a bitmap per query:
 * sr_sparse_range_count_grouped / _fill_grouped.  Not offered: a range search under a list, doc-sharded, or on the certified scorer's
 * 16-bit stage.                                                                                                     */
int sr_sparse_range_count(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                          int64_t nq, const float* d_thresholds, int64_t* d_lims, int64_t* total, sr_stream stream);
int sr_sparse_range_fill(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                         int64_t nq, const float* d_thresholds, const int64_t* d_lims, int64_t id_base, int64_t id_stride,
                         float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream);
/* The range search under a document bitmap: d_mask_words uint32 [ceil(n_bits / 32)] on the device, bit (i & 31) of word
 * i >> 5 stands for document position i, n_bits == n_docs (anything else: SR_ERR_INVALID before any device work).  A hit is score >
 * thr[q] AND the bit of the document position is set; a document without a common term (score +0.0f) under a negative threshold is a
 * hit exactly when its bit is set.  Everything else is the contract of sr_sparse_range_count / _fill: document order, the score bits
 * of sr_sparse_score_pairs, the table / chunk rules, the store guard, no global atomics, and the pairing on the handle - a fill needs
 * a preceding count of the same kind with the same nq, and the count's bitmap.  Bits of the last word at or beyond n_bits are
 * ignored and the library never reads past word ceil(n_bits / 32) - 1 (the kernels clamp their reads; no copy is kept).  The bitmap is
 * read in place by both passes: keep it unchanged between the count and its fill.  An 8 192-document tile whose 256 words are all zero
 * is skipped before a posting is touched.  Per-query masks: sr_sparse_range_count_grouped / _fill_grouped below.  Not offered:
 * doc-sharded.                                                                                                                       */
int sr_sparse_range_count_masked(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                 int64_t nq, const float* d_thresholds, const uint32_t* d_mask_words, int64_t n_bits,
                                 int64_t* d_lims, int64_t* total, sr_stream stream);
int sr_sparse_range_fill_masked(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                int64_t nq, const float* d_thresholds, const uint32_t* d_mask_words, int64_t n_bits,
                                const int64_t* d_lims, int64_t id_base, int64_t id_stride, float* d_out_scores, int64_t* d_out_ids,
                                int64_t capacity, sr_stream stream);
/* The range search under a document bitmap PER QUERY (filter groups): d_group_words uint32 [n_groups, W], W =
 * ceil(n_bits / 32), one bitmap per group over document positions, n_bits == n_docs; d_query_group int32 [nq]: query q searches under
 * bitmap d_query_group[q].  All on the device.  Contract: for every group g the lists of the queries with d_query_group[q] == g are
 * EXACTLY what sr_sparse_range_count_masked / _fill_masked return for those queries under bitmap g - counts, ids, score bits, document
 * order, id_base / id_stride, and the zero-score documents of the allowed set under a negative threshold.  One group is the masked call
 * byte for byte; n_groups == nq, a group without a query and an all-clear bitmap are valid.  A workgroup serves one (query, chunk), so
 * the query's group only selects the bitmap its tile skip and hit test read; nothing past word W - 1 of a group's bitmap is read.
 * Errors, all SR_ERR_INVALID.  Before any device work: n_bits != n_docs, n_groups < 1, n_groups * W >= 2^32, a null pointer with nq > 0.
 * An entry of d_query_group outside [0, n_groups): found before any scoring (the count waits for the stream once to read the 4 nq
 * bytes), sr_last_error() names the first such query, d_lims is written as zeros and *total as 0, and no fill can follow.  The count
 * keeps the checked group ids on the handle (4 nq bytes) and its fill reads those, not d_query_group.  Pairing on the handle: three
 * kinds - unrestricted, masked, grouped; a fill needs a preceding count of its own kind with the same nq (and, grouped, the same
 * n_groups); any mix is SR_ERR_INVALID and nothing is written.  Not offered under groups: doc-sharded indexes.                      */
int sr_sparse_range_count_grouped(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                  int64_t nq, const float* d_thresholds, const uint32_t* d_group_words, int64_t n_groups,
                                  int64_t n_bits, const int32_t* d_query_group, int64_t* d_lims, int64_t* total, sr_stream stream);
int sr_sparse_range_fill_grouped(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                 int64_t nq, const float* d_thresholds, const uint32_t* d_group_words, int64_t n_groups,
                                 int64_t n_bits, const int32_t* d_query_group, const int64_t* d_lims, int64_t id_base,
                                 int64_t id_stride, float* d_out_scores, int64_t* d_out_ids, int64_t capacity, sr_stream stream);
int sr_sparse_index_destroy(sr_sparse_index* idx);
/* Measurement hook as for the dense index; algorithmic bytes = 8 B per posting of the
 * query terms that falls in the launched doc tiles (computed on the device).       */
/* Work counters of the query-block kernel (measurement hook): while enabled, every workgroup adds what it loads and applies
 * to six device counters; each call returns them (out6 may be null) and resets them.  out6[0] dense columns loaded (one =
 * 4096 floats), [1] (column, query) applications (one = 4096 unfused multiply-adds), [2] / [3] postings loaded by the one-step /
 * grouped scatter runs (8 bytes and one LDS read-modify-write each), [4] plan entries fetched, [5] (query block, doc tile)
 * workgroups.  bench.py prices the kernel's VALU and L2 bounds from these.                                                  */
int sr_sparse_index_work_counters(sr_sparse_index* idx, int enable, uint64_t* out6);
int sr_sparse_index_profile(sr_sparse_index* idx, int enable);
int sr_sparse_index_profile_read(sr_sparse_index* idx, int64_t* n_launches, double* total_ms,
                                 double* total_posting_bytes);
/* Which scoring path served the searches so far (both return the same bits): n_dense_terms = heavy
 * terms (present in at least a quarter of the docs) that also have a dense column; n_block_calls =
 * sr_sparse_search calls that ran the 4-queries-per-workgroup kernel; n_fallback_calls = those of them
 * in which at least one block of 4 queries went through the per-query kernel because a query listed
 * its terms in non-ascending order (the accumulation order the reference follows,
 * indexer.py:315-328, is the query's own).                                        */
int sr_sparse_index_block_stats(sr_sparse_index* idx, int64_t* n_dense_terms, int64_t* n_block_calls,
                                int64_t* n_fallback_calls);

/* The certified two-stage scorer (csrc/sparse_cert.hip; its index-side structures: csrc/sparse_cert_build.hip).  For an
 * index without negative values sr_sparse_index_create also builds: fp16 MFMA tiles of the heaviest terms, 4-byte packed postings, a per-term table of doc-tile boundaries and a
 * doc-major forward index.  sr_sparse_search then scores every (query, doc) approximately with a proven error bound (matrix
 * pipe for the heavy terms, 16-bit fixed-point LDS atomics for the others), keeps the k + 1024 best keys, certifies that the
 * true top-k lies among them, re-scores those candidates with the reference's exact fp32 chain
 * (scaling_retriever/indexer.py:324-340) from the forward index and returns their exact top-k: the same bits as the exact
 * kernels.  Queries it cannot certify (a negative or unordered query, more than 256 rare terms, a band of undecided keys
 * wider than 1024, fewer than k docs with a non-zero key) are re-done by the exact kernels inside the same call.
 * out8: [0] 1 if this index has the scorer, [1] heavy terms on the matrix pipe, [2] searches it ran, [3] queries it was
 * given, [4] queries re-done by the exact kernels, [5] doc tiles of 1024, [6] candidates whose exact chain the certified
 * path ran (rounded up to 16 per query), [7] query batches (of up to 8 192 queries: the scorer's per-call workspace is ~200 KB per
 * query) served by the exact kernels because that workspace did not fit in device memory.
 * Environment (read at sr_sparse_index_create): SR_SPARSE_SCORER=exact builds the index without the scorer (its side structures
 * take ~22 bytes per posting + 8 bytes per (term, 1 024-doc tile), at most half of the free device memory: 25 GB at the MS MARCO
 * shape); SR_LOG=1 prints one line per index on stderr saying what was built, with how many bytes, or why not.
 * Limits of the fast path, beyond which a query is served by the exact kernels (same results, about a quarter of the speed):
 * k <= SR_MAX_TOPK - 1024 = 3 072 (the band of extra keys: 1 024, or 2 048 / 3 072 for batches whose queries bring more than 96 / 160
 * terms outside the index's 128 heaviest ones, capped at SR_MAX_TOPK - k), <= 256 query terms (rare terms beyond the first 64 take a
 * slower walk inside the same kernel), terms strictly ascending, values >= 0, at least 8 (k + 1 024) documents in the collection.                            */
int sr_sparse_index_cert_stats(sr_sparse_index* idx, int64_t* out8);
/* Test hook for the error bound: enable = 1 / 0 switches the recording of the stage-1 keys of every (query, doc) pair on /
 * off; enable = 2 copies the last search's keys to h_keys uint16 [nq_pad][n_tiles * 1024] (nq_pad = nq rounded up to 32)
 * and the per-query constants to h_consts fp32 [nq_pad][6] = {c_q (0: query outside the fast path), s_q, rare terms in
 * stage 1, query terms, rare terms left out of stage 1 (weight below fp16's normal range), the k-th best key the scan's
 * last top-k select saw (0: none ran) - the cut below it is the scan's filter threshold}; *vscale, *T = the index-side
 * constants.  With true_fix = 65535 * s_q * (real-arithmetic score) every key obeys
 * true_fix (1 - dd) - 1.2 - 2.03 * left out <= key <= true_fix (1 + dd) + 1.2 + 1.01 * rare terms.                          */
int sr_sparse_index_cert_debug(sr_sparse_index* idx, int enable, uint16_t* h_keys, int64_t keys_capacity,
                               float* h_consts, int64_t nq_pad, float* vscale, int32_t* T);
/* Test-only hook: one of the certified scorer's buffers copied to the host as it stands (tests/test_sparse_cert_kernels_gpu.py,
 * tests/sparse_cert_cases.py hold the numpy models they are compared with).  It launches no kernel and changes none: one
 * hipDeviceSynchronize and one device-to-host copy per call, nothing when it is not called.  *n_bytes = the buffer's size; h_dst NULL:
 * the size only, otherwise capacity_bytes must hold it.  what:
 *   0  int64 [12] = {T, k-steps KS, doc tiles, e_stride, terms V, docs N, postings nnz, queries / padded queries (to 32) / k / k + band
 *      of the last search (k + band = 0: its plan found no query for the fast path), the bits of fp32 vscale}
 *   index side, built once:  1 dslot int32 [V] (dense slot, -1 = rare)   2 vmax fp32 [V]   3 d16 fp16 [tiles][32][KS][64][8] (MFMA A
 *      fragments)   4 P uint32 [nnz + 4] (packed postings, four zero words behind them)   5 S uint32 [V][tiles + 1]
 *      6 E uint32 [V][e_stride]   7 fwd_indptr int64 [N + 1]   8 fwd_tv uint64 [nnz] (term << 32 | value bits, terms ascending per doc)
 *   the last search's plan, [nq_pad] rows:  9 bfrag fp16 [nq_pad / 32][KS][64][8]   10 rare_term int32 [nq_pad][256] (-1 = none)
 *      11 rare_w fp32 [nq_pad][256]   12 elig uint8   13 c_q fp32   14 s_q fp32   15 rare terms in stage 1 int32   16 query terms int32
 *      17 rare terms left out int32
 *   the last search's certificate:  18 m_count int32 [nq_pad] (candidates re-scored, 0 = not certified)   19 ap_ids int64
 *      [nq_pad][2 (k + band)] (their doc indices, the first m_count of a row, in no order)   20 uint8 [nq] the flags of the queries the
 *      pass handed to the exact kernels (kept only while sr_sparse_index_cert_debug's recording is on)
 * A search larger than one scorer batch (8 192 queries) or one that retried a sub-batch leaves the LAST pass's plan and certificate.
 * SR_ERR_INVALID: no scorer on this index, an unknown `what`, a plan / certificate buffer before any search, a buffer too small.      */
int sr_sparse_index_cert_readout(sr_sparse_index* idx, int what, void* h_dst, int64_t capacity_bytes, int64_t* n_bytes);

/* On-device index build: doc-major postings -> CSR by term.  Replaces the per-posting Python append of
 * IndexDictOfArray.add_batch_document (scaling_retriever/utils/inverted_index.py:67-76) and the per-term concatenation of
 * merge_indexes (:108-170) behind SparseIndexer.index (scaling_retriever/indexer.py:239-308).
 * d_rows int32 [nnz] = global doc row of every posting, d_cols int32 [nnz] = term in [0, n_terms), d_vals fp32 [nnz], in
 * insertion order.  A stable radix sort by term (this library's kernels) keeps the insertion order inside a term - the
 * reference's posting order; sort_docs = 1 additionally orders every posting list by ascending doc row (needs n_docs >
 * every row), which is what sr_sparse_index_create requires of a merged multi-rank index.  Outputs: d_indptr int64
 * [n_terms + 1], d_out_rows int32 [nnz], d_out_vals fp32 [nnz] (must not alias the inputs).  Synchronises the stream.
 * Errors: SR_ERR_INVALID for a term outside [0, n_terms), a negative row, or (sort_docs) a row >= n_docs - reported when the
 * call returns; the outputs then hold the postings in no defined order (the digits are masked: never a write outside the
 * arrays).  SR_ERR_NOMEM when the ping-pong buffers (4 bytes x nnz x 4, x 6 with three or more passes) cannot be allocated.  */
/* Term of every posting of a CSR-by-term index: d_out_terms int32 [nnz][p] = t for d_indptr[t] <= p < d_indptr[t + 1]
 * (the per-term arrays of IndexDictOfArray, inverted_index.py:22-55, flattened back to triples for a re-sort).            */
int sr_sparse_csr_expand_terms(const int64_t* d_indptr, int64_t n_terms, int64_t nnz, int32_t* d_out_terms,
                               sr_stream stream);
int sr_sparse_csr_build(const int32_t* d_rows, const int32_t* d_cols, const float* d_vals, int64_t nnz,
                        int64_t n_terms, int64_t n_docs, int sort_docs, int64_t* d_indptr,
                        int32_t* d_out_rows, float* d_out_vals, sr_stream stream);

/* ------------------------------------------------------------ top-k merge ---
 * The one exchange step of doc-sharded retrieval: merge `n_lists` per-shard
 * top-k lists (after the RCCL gather) into the global top-k per query.
 * d_scores fp32 [n_lists, nq, k], d_ids int64 [n_lists, nq, k] (ids < 0 = pad; every other id must be below 2^32 and unique
 * within its query: the key holds 32 id bits and nothing on the device checks the range; no score may be NaN).
 * Outputs as sr_dense_search, in its order (pad_score fills unused slots).  1 <= k <= 2^30 with n_lists * k < 2^31; the library's workspace
 * holds n_lists * k candidates and, for k > sr_max_topk(), 2k + k / 2 more 8-byte words per query.                        */
int sr_topk_merge(const float* d_scores, const int64_t* d_ids, int n_lists, int64_t nq, int k,
                  float pad_score, float* d_out_scores, int64_t* d_out_ids, sr_stream stream);

/* ---------------------------------------------------------- hybrid fusion ---
 * The two device steps of the exact hybrid search (scaling_retriever_amd/hybrid.py) around the pair scorers.  No
 * reference counterpart: its HybridRetriever (scaling_retriever/indexer.py:859-1019) dumps the two heads' runs and fuses nothing.
 * The two indexes number documents independently: d_d2s int64 [n_d2s] maps a dense position to its sparse position (-1: the document
 * has no posting), d_s2d int64 [n_s2d] back (-1: no such document).  n_s2d + n_d2s < 2^32 (the tie below is 32 bits of a key).
 *
 * sr_hybrid_union: per query the set union of two lists of dense positions as an ascending, duplicate-free CSR.
 *   list A  d_a_indptr == NULL: d_a_ids int64 [nq, kd], any order, negative entries are padding (a dense top-k), kd <= sr_max_topk()
 *           - sorted in LDS; else d_a_ids is a CSR over d_a_indptr int64 [nq + 1] of STRICTLY ASCENDING positions of any length
 *           (range hits; kd is ignored) - only read, never staged: the union is placed by ranks, every A entry binary-searches the
 *           LDS-resident B and every B entry binary-searches A.
 *   list B  d_b_spos int64 [nq, ks] SPARSE positions with d_b_counts int32 [nq] valid entries per row (sr_sparse_search's outputs),
 *           ks <= sr_max_topk(), mapped through d_s2d inside the kernel and sorted in LDS.
 *   Outputs: d_out_indptr int64 [nq + 1]; d_out_dpos / d_out_spos / d_out_tie int64 [capacity]: the union's dense positions, their
 *   sparse positions d2s[dpos] and tie = spos where spos >= 0, else n_s2d + dpos (retrieve_fused's tie rule); *total (host) =
 *   indptr[nq].  Count, device scan, fill: no size is read back before the launches; the call waits for the stream once more at its
 *   end to read the status and the total (and frees its nq * 8 scratch bytes).  total > capacity: SR_ERR_INVALID, indptr is complete
 *   and no entry at or beyond capacity was written (nq * (kd + ks), or A's total + nq * ks, always suffices).  A sparse position of B
 *   that maps to no dense document (outside [0, n_s2d) or s2d = -1), or a position of A at or beyond n_d2s (CSR: or negative):
 *   SR_ERR_INVALID, found on the device, sr_last_error() names the first offender; the outputs are then not to be used and the
 *   library stays usable.  An A that is not ascending gives a meaningless union, but no store leaves the query's segment.  nq = 0 is
 *   legal (indptr[0] = 0).                                                                                                      */
int sr_hybrid_union(const int64_t* d_a_ids, const int64_t* d_a_indptr, int64_t kd, const int64_t* d_b_spos,
                    const int32_t* d_b_counts, int64_t ks, const int64_t* d_s2d, int64_t n_s2d, const int64_t* d_d2s,
                    int64_t n_d2s, int64_t nq, int64_t* d_out_indptr, int64_t* d_out_dpos, int64_t* d_out_spos,
                    int64_t* d_out_tie, int64_t capacity, int64_t* total, sr_stream stream);
/* sr_hybrid_rank: per query the top-k of a ragged candidate list of ANY length by (fused descending, tie ascending), where
 *   fused(p) = f32( f32(w_d * dense[p]) + f32(w_s * sparse'[p]) ),  sparse'[p] = sparse[p] where spos[p] >= 0, else 0.0f
 * - two rounded products and one rounded sum (compiled with contraction off: the device compiler would turn a*b + c*d into an fma),
 * the bits of rerank.fused_scores.  Candidates as CSR d_cand_indptr int64 [nq + 1] over d_dpos / d_spos / d_tie int64 and d_dense_scores /
 * d_sparse_scores fp32 (sr_hybrid_union's outputs and the two pair scorers' over them); ties must be distinct inside a list and lie in
 * [0, n_s2d + id_end), n_s2d + id_end < 2^32 (checked: SR_ERR_INVALID naming the first offender, found on the device).  The k best by
 * the 64-bit key (order-preserving fused bits, then the complement of tie) are found by a radix select and sorted in LDS: 1 <= k <=
 * sr_max_topk(), a larger k is SR_ERR_UNSUPPORTED.  w_d, w_s finite and >= 0.  Outputs d_out_scores fp32 / d_out_ids int64 [nq, k]
 * (fused scores, dense positions; padding -FLT_MAX, -1) and d_out_counts int32 [nq].
 * The certificate: with d_D / d_S fp32 [nq] the k'-th scores of the two searches whose lists made the candidates (S = 0.0f for a sparse
 * list shorter than k') and d_complete uint8 [nq] "the dense list held every document", every document outside both lists has fused <=
 * B = fused(D, S) (multiplying by a non-negative weight and adding are monotone under round-to-nearest), so d_out_certified int32 [nq] =
 * complete, or the list holds k candidates and its k-th fused score F_k > B - strictly: at F_k == B an outside document with a smaller
 * tie could win.  d_out_threshold fp32 [nq] = pred(d*), d* the smallest float with g(d*) = fused(d*, S) >= F_k, found by bisection
 * over the ordered image of the floats with the same three roundings; -inf where g(-FLT_MAX) >= F_k or the list holds fewer than k
 * candidates, +inf where not even g(+inf) reaches F_k.  Every document outside the sparse list with fused >= F_k has dense > that
 * threshold: what sr_dense_range_count / _fill take.  nq = 0 is legal.  Waits for the stream once, to read the status.           */
int sr_hybrid_rank(const int64_t* d_cand_indptr, const int64_t* d_dpos, const int64_t* d_spos, const int64_t* d_tie,
                   const float* d_dense_scores, const float* d_sparse_scores, int64_t nq, float w_d, float w_s, int k,
                   const float* d_D, const float* d_S, const uint8_t* d_complete, int64_t n_s2d, int64_t id_end,
                   float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, int32_t* d_out_certified,
                   float* d_out_threshold, sr_stream stream);

/* -------------------------------------------------------------- rank fusion ---
 * sr_rank_fuse (csrc/rank_fuse.hip): per query the k best distinct documents of n_lists ranked lists by a fused score
 * that is defined on the lists alone, so the result is exact by definition (no certificate, no pair scorer).  No reference counterpart.
 * d_ids int64 [n_lists, nq, depth] (id < 0 = padding), d_counts int32 [n_lists, nq] the valid prefix of each row (NULL: depth), d_scores
 * fp32 [n_lists, nq, depth], read only by SR_FUSE_MINMAX (else may be NULL).  Entry (l, q, r) is valid iff r < counts[l, q] and
 * ids[l, q, r] >= 0; its rank is r + 1, the slot's place in the row.
 *   SR_FUSE_RRF     contrib = f32( w_l / f32( c + f32(r + 1) ) ): one rounded add, one correctly rounded division.
 *   SR_FUSE_MINMAX  over the valid entries of (l, q): mn, mx the smallest and largest score, span = f32(mx - mn);
 *                   norm = f32( f32(s - mn) / span ) where span > 0, else 1.0f; contrib = f32(w_l * norm).  Scores are finite (not checked).
 * The fused score of a document starts from +0.0f and adds the contributions of the lists that hold it in ascending l, one rounded fp32
 * add each (compiled with contraction off).  A document only in lists of weight 0 is still a candidate, with fused 0.0.  Result: the k
 * best distinct documents by (fused descending, id ascending) in d_out_scores fp32 / d_out_ids int64 [nq, k] (padding -FLT_MAX, -1),
 * d_out_counts int32 [nq] = min(k, distinct documents), and, unless NULL, d_out_ranks int32 [nq, k, n_lists]: the 1-based rank of the hit
 * in each list, 0 = absent (and in padding).  No atomic decides an output byte: two calls return the same bytes.
 * h_weights is a HOST array [n_lists], finite and >= 0; c (RRF only) finite and > -1.  1 <= n_lists <= 8, 1 <= depth <= sr_max_topk(),
 * n_lists * depth <= 2 * sr_max_topk(), 1 <= k <= sr_max_topk(): anything beyond is SR_ERR_UNSUPPORTED.  A null pointer, a bad nq, weight,
 * c or method, or SR_FUSE_MINMAX without scores: SR_ERR_INVALID before any device work.  nq = 0 is legal.  Found on the device
 * (SR_ERR_INVALID, sr_last_error() names the first offender as id, list, query, entry; the outputs are then not to be used and the
 * library stays usable): a valid id >= 2^32 (the keys hold 32 id bits), and an id that occurs twice among the valid entries of one
 * (l, q) row.  Waits for the stream once, to read the status.                                                                    */
#define SR_FUSE_RRF 0
#define SR_FUSE_MINMAX 1
int sr_rank_fuse(const int64_t* d_ids, const int32_t* d_counts, const float* d_scores, int n_lists, int64_t nq, int64_t depth,
                 int method, const float* h_weights, float c, int k, float* d_out_scores, int64_t* d_out_ids,
                 int32_t* d_out_counts, int32_t* d_out_ranks, sr_stream stream);

/* --------------------------------------------------------------- evaluation ---
 * sr_eval_ranked (csrc/eval_metrics.hip): the ranking metrics of nq result lists against graded judgements, per query and
 * as means, from the arrays a search returns.  Stateless.  No reference counterpart (its utils/metrics.py hands dicts to pytrec_eval).
 * The list of query q: d_scores fp32 [nq, depth] (read by SR_EVAL_ORDER_SCORE only, else may be NULL), d_ids int64 [nq, depth] (id < 0 =
 * padding), d_counts int32 [nq] (NULL: depth), d_tie_key int32 [nq, depth] with values in [0, 65536) (NULL: all 0), d_exclude int64 [nq]
 * (NULL or a negative value: none).  Entry r is valid iff r < counts[q], ids[q, r] >= 0 and ids[q, r] != exclude[q] (BEIR's "drop the
 * hit whose id is the query's").
 * The judgements are a CSR over the same nq rows: d_qrel_indptr int64 [nq + 1] inside [0, n_qrel], d_qrel_ids int64 [n_qrel] strictly
 * ascending inside a row, d_qrel_grades int32 [n_qrel], any sign; a judged document the index does not hold carries an id no list holds.
 * Three tables depend on the judgements alone; the host computes them once and the kernel trusts them: d_n_rel int32 [nq] the number of
 * grades > 0; d_idcg double [nq, n_cuts], for cut c the positive grades sorted descending, the first c of them, summed from 0.0 in that
 * order as double(g) / log2(i + 2); d_log2 double [depth] = log2(i + 2).  The kernel computes no logarithm.
 * h_cuts: HOST int32 [n_cuts], strictly ascending, each >= 1, 0 <= n_cuts <= sr_eval_max_cuts() (16).  rr_depth >= 0.
 * Ranking: SR_EVAL_ORDER_LIST takes the valid entries in list order; SR_EVAL_ORDER_SCORE orders them by (score descending with -0.0
 * read as +0.0, tie_key descending, list position ascending); NaN is outside the contract.  With tie_key = the rank of str(doc id) among
 * the tied documents that is trec_eval's order.  recip_rank is computed on the list CUT FIRST to its first rr_depth valid entries in list
 * order (0: no cut), THEN ordered.
 * d_out double [nq, 1 + 4 n_cuts], all arithmetic in double, contraction off, `/` correctly rounded; the columns of a query that is not
 * evaluated are 0.0:
 *   [0]                  recip_rank = 1.0 / rank of the first entry with grade > 0, else 0.0
 *   [1 + j]              recall  = double(h) / double(n_rel), h = the entries with grade > 0 among the first c_j ranked ones; 0.0 if n_rel == 0
 *   [1 + n_cuts + j]     ndcg_cut = dcg / idcg, 0.0 unless idcg > 0; dcg starts from 0.0 and adds double(max(grade, 0)) / log2[i] in rank order
 *   [1 + 2 n_cuts + j]   r_cap   = double(h) / double(min(n_rel, c_j)), 0.0 if n_rel == 0
 *   [1 + 3 n_cuts + j]   map_cut = (the sum in rank order from 0.0 of double(hits so far) / double(rank) at every relevant entry) / double(n_rel)
 * d_out_flags int32 [nq]: bit 0 = evaluated (the judgement row is non-empty AND the list has a valid entry), bit 1 = n_rel[q] == 0.
 * d_out_mean double [1 + 4 n_cuts]: every column summed over the evaluated queries in ascending q from 0.0, one rounded add each, divided
 * by their number d_out_n (int64, one word); 0.0 without an evaluated query.  No atomic decides an output byte.
 * 1 <= depth <= sr_max_topk(): a larger depth is SR_ERR_UNSUPPORTED; a bad size, order, cut or pointer is SR_ERR_INVALID before any device
 * work; nq = 0 is legal.  Found on the device (SR_ERR_INVALID, the outputs are then not to be used, the library stays usable): a
 * judgement row that is not strictly ascending or leaves the arrays (sr_last_error() names the query); a tie_key outside its range
 * at a valid entry (query, entry); a JUDGED document that occurs twice among a list's valid entries (query, entry of the repeat, id).
 * Waits for the stream once, to read the status.                                                                                 */
#define SR_EVAL_ORDER_SCORE 0
#define SR_EVAL_ORDER_LIST 1
int sr_eval_max_cuts(void);
int sr_eval_ranked(const float* d_scores, const int64_t* d_ids, const int32_t* d_counts, const int32_t* d_tie_key, const int64_t* d_exclude,
                   int64_t nq, int64_t depth, const int64_t* d_qrel_indptr, const int64_t* d_qrel_ids, const int32_t* d_qrel_grades,
                   int64_t n_qrel, const int32_t* d_n_rel, const double* d_idcg, const double* d_log2, const int32_t* h_cuts, int n_cuts,
                   int order, int64_t rr_depth, double* d_out, int32_t* d_out_flags, double* d_out_mean, int64_t* d_out_n,
                   sr_stream stream);

/* sr_eval_randomization (same file): the two-sided paired randomization test.  d_diff double [n_cols, n]: the per-query differences a - b
 * of 1 to 8 metric columns over n paired queries.  Permutation b in [0, n_perm) flips the sign of query q iff bit (q & 63) of
 * mix(seed + b * W + (q >> 6)) is set, W = ceil(n / 64), in wrapping uint64 arithmetic, mix the splitmix64 step (z += 0x9E3779B97F4A7C15;
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31).  The same signs serve all columns.
 * T_b[c] = the sum over q ascending, from +0.0, of +-diff[c, q], one rounded add each; T_obs[c] the same sum without flips.
 * d_t_obs double [n_cols]; d_count_ge int64 [n_cols] = the number of b with |T_b[c]| >= |T_obs[c]|; p = (count + 1) / (n_perm + 1) is
 * the caller's.  n = 0 is legal (the counts are n_perm).  n_cols outside [1, 8], n_perm outside [1, 2^31) or a null pointer:
 * SR_ERR_INVALID before any device work.  Waits for the stream once (its partial counts are freed on return).                     */
int sr_eval_randomization(const double* d_diff, int n_cols, int64_t n, int64_t n_perm, uint64_t seed, double* d_t_obs, int64_t* d_count_ge,
                          sr_stream stream);

/* ------------------------------------------------------- diversified search ---
 * sr_dense_mmr (csrc/dense_mmr.hip): exact greedy Maximal Marginal Relevance over a candidate list per query, on the
 * rows the dense index holds (fp32 or fp16 rows, any number of segments).  No reference counterpart.
 * Input: d_ids int64 [nq, n] global doc indices as sr_dense_search returns them, d_rel fp32 [nq, n] the caller's relevance (a search's
 * scores, a fused score, ...), d_counts int32 [nq] the valid prefix of each row (NULL: n).  Entry i of query q is a candidate iff
 * i < counts[q] and ids[q, i] >= 0 (id < 0 = padding, skipped).  An id may repeat in a row: each entry is its own candidate.
 * d_ids and d_rel must be readable for all nq * n entries, padding and the entries beyond counts included (their values are ignored).
 * lambda in [0, 1]; mu = f32(1) - f32(lambda), computed once on the host.
 * Similarity: sim(i, j) = the fp32 fmaf chain from +0.0f over the stored rows i and j in the exact kernel's k order (per 8 columns
 * k = 8s + j, then 8s + 4 + j) - bit for bit what sr_dense_score_pairs returns for a query equal to row i read as fp32 and document j
 * (fp16-stored rows are widened exactly); symmetric, because the products commute.
 * Selection: pick 0 is the best candidate by (rel descending, id ascending, position ascending); its marginal value is f32(lambda * rel).
 * At pick t >= 1 every unselected candidate has m_i = the largest sim(i, j) over the selected j (m = sim > m ? sim : m, from -inf) and
 * v_i = f32( f32(lambda * rel_i) - f32(mu * m_i) ), two roundings and no contraction; the pick is the best by (v descending as floats,
 * -0.0 equal to +0.0; id ascending; position ascending).  Selection ends after k picks or when the candidates run out.  A total order
 * and no atomic on the result path: two calls return the same bytes.
 * Output [nq, k]: d_out_ids int64, d_out_rel fp32 (the pick's rel, bits untouched), d_out_mmr fp32 (v at the moment of the pick),
 * d_out_pos int32 (its position in the candidate row); d_out_counts int32 [nq] picks made; padding (-1, -FLT_MAX, -FLT_MAX, -1).
 * lambda = 1 returns the first k candidates by (rel, id); d_out_mmr never increases from pick 1 on (m_i never decreases and every
 * rounding is monotone); pick 0 may lie below pick 1 when similarities are negative.
 * Contract: rel and the rows are finite and no chain overflows - a NaN or an infinity in rel, in a row or in a similarity is outside
 * the contract (not checked).  1 <= n <= sr_mmr_max_candidates() (1024: the candidates' state lives in LDS), 1 <= k <= that cap; a bad
 * size, lambda or pointer is SR_ERR_INVALID before any device work; nq = 0 is legal.  A candidate id that is in no segment is found on
 * the device: SR_ERR_INVALID, sr_last_error() names query, entry and id, and NOTHING is selected (every output row is padding).
 * One workgroup per query runs all k steps (no host round trip in between); waits for the stream once, to read the status.       */
int sr_mmr_max_candidates(void);
int sr_dense_mmr(sr_dense_index* idx, const int64_t* d_ids, const float* d_rel, const int32_t* d_counts, int64_t nq, int64_t n, int k,
                 float lambda, int64_t* d_out_ids, float* d_out_rel, float* d_out_mmr, int32_t* d_out_pos, int32_t* d_out_counts,
                 sr_stream stream);

/* sr_sparse_mmr (csrc/sparse_mmr.hip): the same selection on the sparse head.  Stateless, like sr_sparse_feedback: the
 * documents arrive as a doc-major CSR (d_doc_indptr int64 [n_docs + 1], d_doc_cols int32 ascending inside a row, d_doc_vals fp32;
 * trusted) - what SparseIndexHIP.forward_rows() keeps.  d_ids int64 [nq, n] are document positions in [0, n_docs); d_rel, d_counts, the
 * candidate rule (i < counts[q] and id >= 0; a repeated id is its own candidate), lambda and mu as for sr_dense_mmr; 1 <= k <= n <=
 * sr_mmr_max_candidates().
 * Similarity, contraction off everywhere: ip(i, j) is s = +0.0f, then for every term t that both rows hold, in ascending t,
 * s = f32(s + f32(v_i[t] * v_j[t])) - bit for bit what sr_sparse_score_pairs returns for the query "row i" and document j; symmetric
 * (the products commute); an empty row or a pair without a common term gives +0.0f.
 *   sim_mode = SR_MMR_SIM_IP:      sim = ip.
 *   sim_mode = SR_MMR_SIM_COSINE:  norm_i = f32(sqrt(ip(i, i))), den = f32(norm_i * norm_j), sim = den > 0 ? f32(ip / den) : +0.0f, the
 *                                  square root and the division correctly rounded.  Sparse document-document inner products are far
 *                                  larger than query-document scores (about 128 terms meet, not 32): on raw inner products no lambda
 *                                  balances the two terms of v.
 * Selection, the five outputs, their padding and the order of a pick are exactly sr_dense_mmr's.  A valid entry >= n_docs is found on
 * the device (the kernel reads no row offset for it): SR_ERR_INVALID, sr_last_error() names query, entry and id, every output row is
 * padding.  A bad size, sim_mode, lambda or pointer is SR_ERR_INVALID before any device work; nq = 0 is legal.  Non-finite values are
 * outside the contract.  No atomic decides an output byte: two calls return the same bytes.  One workgroup per query runs all k picks;
 * the picked row is staged in LDS in chunks of 512 entries (the dev switch SR_MMR_SPARSE_CHUNK lowers it; the bits do not depend on
 * it).  Waits for the stream once, to read the status.                                                                            */
#define SR_MMR_SIM_IP 0
#define SR_MMR_SIM_COSINE 1
int sr_sparse_mmr(const int64_t* d_doc_indptr, const int32_t* d_doc_cols, const float* d_doc_vals, int64_t n_docs, const int64_t* d_ids,
                  const float* d_rel, const int32_t* d_counts, int64_t nq, int64_t n, int k, float lambda, int sim_mode,
                  int64_t* d_out_ids, float* d_out_rel, float* d_out_mmr, int32_t* d_out_pos, int32_t* d_out_counts, sr_stream stream);

/* ------------------------------------------------- pseudo-relevance feedback ---
 * Rocchio's rebuilt query for both heads (csrc/prf.hip).  No reference counterpart.
 * Per query, d_fb_ids int64 [nq, depth] is a ranked list (id < 0 = padding), d_counts int32 [nq] its valid prefix (NULL: depth).  Let v
 * be the valid, non-padding entries in list order: the positive set is the first p = min(n_pos, |v|) of them, the negative set the last
 * g = min(n_neg, |v| - p) in list order (never overlapping the positive set); a document that appears twice counts twice.
 * cp = f32(beta / f32(p)), cn = f32(gamma / f32(g)), fp32 divisions on the host (two tables of 64 entries in the kernel arguments).
 * For every coordinate t (a term / a column): P_t = the positive documents' values at t summed in list order from +0.0f, one rounded fp32
 * add each (a document that does not hold t adds nothing), N_t likewise for the negative set;
 *   w_t = f32( f32(alpha * q_t) + f32(cp * P_t) ), then w_t = f32( w_t - f32(cn * N_t) ), contraction off;
 * q_t absent starts from +0.0f, p = 0 / g = 0 skips its step.  1 <= n_pos <= 64, 0 <= n_neg <= 64, 1 <= depth <= sr_max_topk(), alpha,
 * beta, gamma finite and >= 0, max_terms >= 0: anything else is SR_ERR_INVALID before any device work.  nq = 0 is legal.  Values are
 * finite (not checked).  No atomic decides an output byte: two calls return the same bytes.
 *
 * sr_sparse_feedback (stateless): the queries as CSR (d_q_indptr int64 [nq + 1], d_q_cols int32 strictly ascending inside a row and in
 * [0, n_terms) - what sr_sparse_compact emits -, d_q_vals fp32) and the documents as a doc-major CSR (d_doc_indptr int64 [n_docs + 1],
 * d_doc_cols int32 ascending inside a row, d_doc_vals fp32; trusted).  Ids are document positions.  A term is kept only if w_t > 0; of the
 * kept terms the max_terms largest survive, by (w descending, term ascending), 0 = no limit; they are emitted with terms ascending - the
 * conventions of sr_sparse_compact_topm.  Output CSR d_row_ptr int64 [nq + 1], d_cols int32, d_vals fp32 with capacity, *h_nnz and
 * SR_ERR_NOMEM exactly as sr_sparse_compact (the needed size is written to *h_nnz; nothing but d_row_ptr is written when it does not fit).
 * Found on the device, SR_ERR_INVALID and nothing written: a valid entry >= n_docs (sr_last_error() names query, entry and id - every
 * valid entry is checked, used or not), query columns out of order or outside [0, n_terms) (names the query).  One workgroup per query
 * merges the query row and the at most 128 document rows in LDS while they hold at most sr_prf_max_entries() entries together (8 192;
 * the dev switch SR_PRF_MAX_ENTRIES lowers it); a query above that takes the same steps on a global-memory workspace, same bits (at most
 * 2^25 - 1 entries: SR_ERR_UNSUPPORTED beyond).  Waits for the stream twice: the plan (status, entry counts), the total.
 *
 * sr_dense_feedback: d_queries fp32 [nq, dim], ids as sr_dense_search returns them (every segment's id_base / id_stride; fp32 or fp16
 * rows, fp16 widened exactly); d_out fp32 [nq, dim] (16-byte aligned, as d_queries) := w over all columns.  An id the index does not hold
 * is found on the device: SR_ERR_INVALID naming query, entry and id, nothing is written.  Every row is read once, as 16-byte pieces.
 * Waits for the stream once, to read the status.                                                                                     */
int sr_prf_max_entries(void);
int sr_sparse_feedback(const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals, int64_t nq,
                       const int64_t* d_doc_indptr, const int32_t* d_doc_cols, const float* d_doc_vals, int64_t n_docs, int64_t n_terms,
                       const int64_t* d_fb_ids, const int32_t* d_counts, int64_t depth, int n_pos, int n_neg, float alpha, float beta,
                       float gamma, int64_t max_terms, int64_t* d_row_ptr, int32_t* d_cols, float* d_vals, int64_t capacity,
                       int64_t* h_nnz, sr_stream stream);
int sr_dense_feedback(sr_dense_index* idx, const float* d_queries, int64_t nq, const int64_t* d_fb_ids, const int32_t* d_counts,
                      int64_t depth, int n_pos, int n_neg, float alpha, float beta, float gamma, float* d_out, sr_stream stream);

/* ---------------------------------------------------------------- encoder ---
 * Replaces LlamaBiDense / LlamaBiSparse .encode / .query_encode / .doc_encode
 * (scaling_retriever/modeling/llm_encoder.py:66-70,186-196,424-443) and the
 * LlamaBiModel forward they call (modeling/bidirectional_llama.py:67-188 over
 * transformers' LlamaModel), and the same for Qwen2BiDense / Qwen2BiSparse
 * (llm_encoder.py:204-209,528-533) over Qwen2BiModel (modeling/bidrectional_qwen2.py:68-101
 * over transformers' Qwen2Model): a Llama layer whose q_proj / k_proj / v_proj carry a bias
 * (attention_bias below).                                                     */
typedef struct sr_model sr_model;

typedef struct {
    int32_t vocab_size, hidden_size, intermediate_size, num_layers;
    int32_t num_heads, num_kv_heads, head_dim;
    float rms_norm_eps;
    float rope_theta;
    int32_t rope_llama3;              /* 0 = default rope, 1 = "llama3" scaling */
    float rope_factor, rope_low_freq_factor, rope_high_freq_factor;
    int32_t rope_original_max_pos;
    int32_t tie_word_embeddings;      /* lm_head shares embed_tokens */
    int32_t has_lm_head;              /* 0: LlamaBiModel (dense), 1: LlamaBiForMNTP (sparse) */
    int32_t max_batch_tokens;         /* workspace sizing: max packed tokens per encode call */
    int32_t max_batch_seqs;
    int32_t fp32_planes;              /* fp32 regime (sr_encode_*_fp32): 0 = not available; 16 = every weight also kept as two
                                         fp16 planes of power-of-two scaled rows (22 significand bits, 3 plane products
                                         per GEMM: truncation below the fp32 accumulation's own rounding); 3 = three bf16
                                         planes (24 bits, 6 products); 2 = two bf16 planes (3 products: dropped terms up
                                         to 2^-15 of sum |a w| per output, see SR_PRECISION_BF16X3)                */
    int32_t attention_bias;           /* 1: q_proj / k_proj / v_proj carry a bias, added before the rotation (Qwen2:
                                         modeling/bidrectional_qwen2.py:68-101, llm_encoder.py:204-209,528-533); the model then
                                         needs model.layers.N.self_attn.{q,k,v}_proj.bias.  0 (Llama): those names are unknown */
} sr_model_config;

int sr_model_create(sr_model** out, const sr_model_config* cfg);
/* Copies one checkpoint tensor (HF Llama naming, e.g.
 * "model.layers.3.self_attn.q_proj.weight") from device memory into the
 * model's internal layout.  dtype = SR_DTYPE_F32 or SR_DTYPE_BF16.  A 1-D tensor (norm weights, and with
 * attention_bias = 1 the q / k / v biases) is passed as [rows, 1].  The fp32 regime adds a bias as it is, the
 * autocast regime its bf16 rounding (autocast casts an nn.Linear's bias to bf16).                            */
int sr_model_set_weight(sr_model* m, const char* name, const void* d_ptr, int dtype,
                        int64_t rows, int64_t cols, sr_stream stream);
/* Verifies all tensors were provided and fixes the weights' layout: with fp32_planes = 16, a matrix whose low fp16 plane is
 * all zero (e.g. bf16-valued weights) drops that plane's segment, so its GEMMs run 2 plane products instead of 3 with the
 * same result bits.  sr_model_set_weight on a finalized model fails (SR_ERR_INVALID).                                    */
int sr_model_finalize(sr_model* m);
/* K segments of each fp32-regime weight matrix of a finalized model: 4 per layer (qkv, o_proj, gate-up, down_proj), then the
 * lm_head if the model has one; *n = their number (4 num_layers + has_lm_head), min(capacity, *n) of them are written to the
 * host array out.  fp32_planes = 16: 2 or 3 per matrix (see sr_model_finalize); 2 / 3: 3 / 6 everywhere; 0: 0.          */
int sr_model_weight_segments(sr_model* m, int32_t* out, int64_t capacity, int64_t* n);
/* fp32_planes = 16: which layers of a finalized model run the fused SwiGLU split (the gate-up GEMM writes the down_proj's fp16
 * planes under a row scale from the bound |xn|^2 max_j |w_gate_j||w_up_j|): out[i] = 1, or 0 for a layer whose weights make that
 * bound loose (hidden_size max_j p_j >= 2^16 median_j p_j, p_j = |w_gate_j||w_up_j|) and which takes the fp32 SwiGLU output + row
 * split instead.  *n = num_layers (0 for any other fp32_planes); min(capacity, *n) values are written to the host array out.   */
int sr_model_fused_act_layers(sr_model* m, int32_t* out, int64_t capacity, int64_t* n);
/* d_input_ids / d_attention_mask: int64 [B, L] on device (the tokenizer
 * collator's output, data_collator.py:177-190).  d_out: fp32 [B, hidden].    */
int sr_encode_dense(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask,
                    int32_t B, int32_t L, float* d_out, sr_stream stream);
/* d_out: fp32 [B, vocab]. */
int sr_encode_sparse(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask,
                     int32_t B, int32_t L, float* d_out, sr_stream stream);
/* The two calls above are the reference's torch.autocast(bf16) regime (documents: indexer.py:46-52,
 * :255-256; sparse queries: :390-391): bf16 GEMM inputs, fp32 accumulation, fp32 everything else.
 * The _fp32 variants are its NO-autocast regime - dense queries (eval_dense.py:94-106, no autocast at
 * :101-102) and examples/quick_start.py: every nn.Linear is an fp32 GEMM and SDPA runs on fp32
 * operands.  Same arguments and outputs; needs a model created with fp32_planes > 0
 * (SR_ERR_INVALID otherwise).                                                */
int sr_encode_dense_fp32(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask,
                         int32_t B, int32_t L, float* d_out, sr_stream stream);
int sr_encode_sparse_fp32(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask,
                          int32_t B, int32_t L, float* d_out, sr_stream stream);
/* Both heads from ONE backbone pass - the hybrid model HybridIndexer / HybridRetriever drive
 * (`batch_sparse_reps, batch_dense_reps = self.model.encode(**inputs)`, indexer.py:764, :939):
 * d_out_sparse fp32 [B, vocab], d_out_dense fp32 [B, hidden]; fp32 = 0 autocast regime, 1 fp32 regime. */
int sr_encode_both(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask,
                   int32_t B, int32_t L, int32_t fp32, float* d_out_sparse, float* d_out_dense,
                   sr_stream stream);
/* Rows of SEVERAL collator batches in one call.  The reference's drivers hand the encoder eval_batch_size rows at a time
 * (DenseRetriever.generate_query_vecs, eval_dense.py:94-106; SparseRetrieval._generate_query_vecs, indexer.py:382-403; default 128
 * queries = ~1 100 tokens, far too few rows to fill 256-row GEMM tiles).  The host side lays the batches into ONE [B, L] matrix
 * (L = the widest batch; a narrower batch gets extra left padding, mask 0) and passes d_row_shift int32 [B]: how many columns row b
 * moved right.  Positions (RoPE, the dense head's `[-length:]` pooling) are counted from there, i.e. every row keeps the
 * position_ids it had in its own batch, and its output is bit-identical to encoding that batch alone.  d_row_shift may be NULL
 * (no shifts).  mode: 0 dense head, 1 sparse head, 2 both; fp32: 0 autocast regime, 1 fp32 regime.  d_out_sparse fp32 [B, vocab]
 * (modes 1, 2), d_out_dense fp32 [B, hidden] (modes 0, 2).                                                                      */
int sr_encode_rows(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L,
                   const int32_t* d_row_shift, int32_t mode, int32_t fp32, float* d_out_sparse, float* d_out_dense,
                   sr_stream stream);
/* Debug/test hook: last_hidden_state (after the final norm) of the packed
 * tokens of the last encode call, fp32 [n_tokens, hidden]; returns n_tokens
 * through *n_tokens.                                                         */
int sr_model_last_hidden(sr_model* m, float* d_out, int64_t capacity_rows, int64_t* n_tokens, sr_stream stream);
int sr_model_destroy(sr_model* m);

/* peft merge_and_unload for one Linear (llm_encoder.py:116-122,502-508):
 * W[out,in] += scale * B[out,r] @ A[r,in], fp32 in place, scale = alpha / r.  One grid row per output feature:
 * out_features beyond the device's maxGridSize[1] is SR_ERR_INVALID, found by the argument check ("grid limit").  */
int sr_lora_merge(float* d_W, const float* d_A, const float* d_B, int64_t out_features,
                  int64_t in_features, int32_t r, float scale, sr_stream stream);

/* nonzero -> (row, col, val) compaction of sparse reps [B, V]
 * (indexer.py:259-260 torch.nonzero + gather; _generate_query_vecs :393-399).
 * d_row_ptr int64 [B+1] receives CSR row offsets, d_cols int32 / d_vals fp32
 * [capacity] the entries (cols ascending inside a row, like torch.nonzero).
 * *h_nnz gets the total (call synchronises the stream). Returns SR_ERR_NOMEM
 * if capacity is too small (then *h_nnz holds the needed size).               */
int sr_sparse_compact(const float* d_reps, int64_t B, int64_t V, int64_t* d_row_ptr,
                      int32_t* d_cols, float* d_vals, int64_t capacity, int64_t* h_nnz,
                      sr_stream stream);
/* The same compaction under a per-row term budget.  NO reference counterpart: the reference keeps every non-zero
 * (indexer.py:259-260, :393-399); this extends those two places.  max_terms == 0: no limit, exactly sr_sparse_compact.
 * Otherwise a row keeps its min(max_terms, nnz) largest non-zeros - ordered by value descending as fp32 numbers (negative values
 * rank below every positive one; -0.0 is zero and never an entry), ties to the LOWER column - and emits them with cols ascending,
 * values unchanged; a row with nnz <= max_terms comes out as from sr_sparse_compact.  Inputs are finite (NaN: unspecified).
 * Capacity, SR_ERR_NOMEM and *h_nnz as sr_sparse_compact (the needed size is at most B * min(max_terms, V)); the call
 * synchronises the stream.  max_terms < 0 is SR_ERR_INVALID, checked before any device call.                                    */
int sr_sparse_compact_topm(const float* d_reps, int64_t B, int64_t V, int64_t max_terms,
                           int64_t* d_row_ptr, int32_t* d_cols, float* d_vals,
                           int64_t capacity, int64_t* h_nnz, sr_stream stream);

/* run.json of the retrieval drivers, written straight from the result arrays (HOST function: every pointer is host memory).
 * Replaces the per-hit Python loops + json.dump of eval_dense.py:225-241 (`qid_to_rankdata[str(qid)][str(docid)] = float(score)`)
 * and SparseRetrieval.retrieve, indexer.py:405-474,530-540 (`res[str(qid)][str(doc_ids[id_])] = float(sc)`; `json.dump(res)`):
 * the file holds byte for byte what Python's json.dump writes for that nested dict - {"qid": {"docid": score, ...}, ...},
 * ", " / ": " separators, entries in row order, scores as float.__repr__ of the fp32 value widened to double.
 * h_scores fp32 [nq, k], h_idx int64 [nq, k] = positions in the document id table (negative = padding, skipped), h_counts int32
 * [nq] or NULL = hits per row (NULL: k).  A query without a hit gets no entry, as in the reference.  Keys: decimal int64
 * (h_qid_i64 [nq] / h_doc_i64 [n_docs]) or, when the *_i64 pointer is NULL, JSON string bodies already escaped by the caller:
 * bytes + offsets [n + 1], or - offsets NULL - fixed-width NUL-padded entries of *_width bytes (a numpy 'S' array of ASCII ids
 * that need no escaping).  Keys are assumed distinct (the caller checks; a dict would merge duplicates).
 * n_threads <= 0: all hardware threads.  *bytes_written (nullable) = file size.                                             */
int sr_write_run_json(const char* path, int64_t nq, int64_t k, const float* h_scores, const int64_t* h_idx, const int32_t* h_counts,
                      const int64_t* h_qid_i64, const char* h_qid_bytes, const int64_t* h_qid_off, int64_t qid_width,
                      const int64_t* h_doc_i64, const char* h_doc_bytes, const int64_t* h_doc_off, int64_t doc_width,
                      int64_t n_docs, int32_t n_threads, int64_t* bytes_written);
/* The same file in pieces, so that the host writes piece c while the GPU searches piece c + 1 (eval_dense.py:225-241 writes after the whole
 * search): part 1 = first piece (creates the file, leaves it open-ended), 2 = a middle piece, 3 = the last piece (closes the object).
 * The finished file holds the bytes of one sr_write_run_json call over the concatenated pieces.  *bytes_written = size so far.      */
int sr_write_run_json_part(const char* path, int32_t part, int64_t nq, int64_t k, const float* h_scores, const int64_t* h_idx,
                           const int32_t* h_counts, const int64_t* h_qid_i64, const char* h_qid_bytes, const int64_t* h_qid_off,
                           int64_t qid_width, const int64_t* h_doc_i64, const char* h_doc_bytes, const int64_t* h_doc_off,
                           int64_t doc_width, int64_t n_docs, int32_t n_threads, int64_t* bytes_written);
/* Test hook: rounds of sr_write_run_json that were copied through the shared file mapping (rounds of >= 8 MB with more than
 * one thread) since the library was loaded; the other rounds are written with pwrite.                                       */
int64_t sr_run_writer_mapped_rounds(void);

/* ----------------------------------------------------- building blocks ---
 * The two MFMA kernels of the encoder, exported for per-kernel parity tests and
 * profiling (they are what sr_encode_* launches per layer).
 * sr_gemm_bf16: y = A[M,K] @ W[N,K]^T, bf16 inputs, fp32 accumulate.
 *   epilogue 0: C bf16 [M,N];  1: C fp32 [M,N] += y;  2: SwiGLU, W rows interleaved
 *   gate/up in 16-row blocks, C bf16 [M,N/2];  3: per-sequence max over token rows,
 *   C fp32 [n_seq,N] (pre-zeroed), d_seq_of int32 [M];  4: C fp32 [M,N].
 * sr_attention_varlen: bidirectional GQA attention over packed sequences with the
 *   RoPE rotation fused; d_qkv bf16 [T,(nh+2nkv)*hd], d_out bf16 [T,nh*hd],
 *   d_cu_seqlens int32 [B+1], d_pos int32 [T], d_key_valid uint8 [T],
 *   d_rope_cos/sin fp32 [max_pos, hd/2]; pass NULL for both when d_qkv is already
 *   rotated (sr_gemm_qkv_rope output) - that is the form sr_encode_* uses.  For that
 *   form the call fetches d_cu_seqlens and picks the kernel by the longest sequence, as
 *   sr_encode_* does from its own lengths: internally max_seqlen = 0 with apply_rope = 0
 *   does not occur unless every sequence is empty, and then nothing is launched.
 *   B = 0 returns SR_OK; num_heads % num_kv_heads != 0 is SR_ERR_INVALID.         */
int sr_gemm_bf16(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                 void* d_C, const int32_t* d_seq_of, sr_stream stream);
/* QKV projection with the RoPE rotation fused into the epilogue (fp32, HF rotate_half layout):
 * C bf16 [M,N]; features [0, n_rope) = q heads then k heads are rotated with the angle of
 * d_pos[m], features [n_rope, N) (v heads) are stored as is.                      */
/* The GEMM of the encoder's fp32 regime on fp16 planes (fp32_planes = 16): d_A [M, K] / d_W [N, K] fp16 plane segments of rows
 * scaled by powers of two, d_a_scale [M] / d_w_scale [N] the inverse scales; C fp32 [M, N] += (A W^T) a_scale[m] w_scale[n]. */
int sr_gemm_f16_scaled(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, const float* d_a_scale,
                       const float* d_w_scale, float* d_C, sr_stream stream);
/* Test-only hook: one of the buffers that loading (sr_model_set_weight, sr_model_finalize) and sr_model_create's RoPE tables left
 * on the device, copied to the host as it stands, in the INTERNAL row order (tests/model_load_cases.py restates the row maps and the
 * conversions; tests/test_model_load_gpu.py compares).  It launches no kernel and changes nothing: the model's mutex, one
 * hipDeviceSynchronize and one device-to-host copy per call; the product path never calls it.  Works before and after
 * sr_model_finalize; after it an fp16-plane matrix reports the 2 or 3 segments finalize left.
 * layer = -1: the model-level buffers; 0 .. num_layers - 1: that layer's.  buffer / kind:
 *   SR_READOUT_EMBED     F32 [vocab, hidden]                      SR_READOUT_NORM  F32 [hidden, 1]
 *   SR_READOUT_ROPE_COS, SR_READOUT_ROPE_SIN   F32 [8192, head_dim / 2]
 *   SR_READOUT_LM_HEAD [vocab, hidden], SR_READOUT_QKV [(nh + 2 nkv) hd, hidden], SR_READOUT_O [hidden, nh hd],
 *   SR_READOUT_GATE_UP [2 intermediate, hidden] (gate / up interleaved in 16-row blocks), SR_READOUT_DOWN [hidden, intermediate]:
 *       BF16 uint16 [rows, K];  PLANES uint16 [rows, n_seg K] (fp32_planes 2 / 3: 3 / 6 bf16 segments; 16: 3 or 2 fp16 segments);
 *       W_INV F32 [rows, 1] (fp32_planes 16 only)
 *   SR_READOUT_LN1, SR_READOUT_LN2   F32 [hidden, 1]
 *   SR_READOUT_BIAS (attention_bias = 1)   F32 [(nh + 2 nkv) hd, 1] the values, BF16_AS_F32 their bf16 roundings held as fp32
 * *n_bytes, *n_rows, *row_elems = the buffer's size, rows and elements per row.  h_dst NULL or capacity_bytes 0: the size only,
 * otherwise capacity_bytes must hold it.  SR_ERR_INVALID: a null model or size pointer, a layer out of range, a buffer / kind this
 * model does not hold (an lm_head on a dense model, planes with fp32_planes = 0, ...), a buffer too small.                        */
#define SR_READOUT_EMBED 0
#define SR_READOUT_LM_HEAD 1
#define SR_READOUT_NORM 2
#define SR_READOUT_ROPE_COS 3
#define SR_READOUT_ROPE_SIN 4
#define SR_READOUT_QKV 5
#define SR_READOUT_O 6
#define SR_READOUT_GATE_UP 7
#define SR_READOUT_DOWN 8
#define SR_READOUT_LN1 9
#define SR_READOUT_LN2 10
#define SR_READOUT_BIAS 11
#define SR_READOUT_F32 0
#define SR_READOUT_BF16 1
#define SR_READOUT_PLANES 2
#define SR_READOUT_W_INV 3
#define SR_READOUT_BF16_AS_F32 4
int sr_model_readout(sr_model* m, int32_t layer, int32_t buffer, int32_t kind, void* h_dst, int64_t capacity_bytes,
                     int64_t* n_bytes, int64_t* n_rows, int64_t* row_elems);
/* Test-only hooks: the other launches of the fp16-plane layer loop, each with the arguments the encoder fills.  Every call
 * validates its arguments before it touches a device (SR_ERR_INVALID).
 * sr_rows_split_f16: rows of d_src fp32 [T, K] -> d_planes fp16 [T, nseg K] = [f1 | f0 | f0] (nseg = 3) or [f1 | f0] (2) of
 *   row * sc, sc the power of two that puts the row's largest magnitude into [2^14, 2^15) (1 for a zero row), d_a_inv [T] = 1 / sc.
 *   d_norm_w [K] (or NULL): the row is RMS-normalised first, y = (x rsqrt(mean(x^2) + eps)) w.  d_embed + d_tok_id (with d_norm_w
 *   only): row t is gathered from d_embed[d_tok_id[t]] and written back to d_src.  d_gu_cmax (device float, or NULL) with
 *   d_act_sc / d_act_inv [T]: the forward and inverse power-of-two scale of the row's SwiGLU output from the bound
 *   B = |y|^2 cmax 1.02, B act_sc in [2^14, 2^15).  K % 4 == 0; K = 2048 / 4096 / 8192 run the register kernels.
 * sr_gu_cmax_f16: *d_cmax = max_j |w_gate_j||w_up_j| 1.001 over the I feature pairs of an interleaved gate/up matrix (gate and up
 *   rows alternate in blocks of 16) given as fp16 plane segments [2 I, nseg K] ([w0 | w1 | w0] or [w0 | w0]) and inverse row scales.
 * sr_gemm_f16_planes: the fp16-plane GEMM with any of its epilogues, K = a_nseg x features (a_nseg 2 or 3 picks the 256 x 256 loop
 *   as in the encoder).  epilogue 9: QKV + bias + RoPE, C fp32 [M, N] (d_pos, tables, n_rope, head_dim, optional d_bias);
 *   10: C fp32 [M, N] += y (= sr_gemm_f16_scaled);  11: SwiGLU, C fp32 [M, N/2];  12: per-sequence max, C fp32 [n_seq, N]
 *   pre-zeroed, d_seq_of [M] ascending, -2 = masked row;  13: SwiGLU scaled by d_out_scale[m] and written as fp16 planes
 *   C [M, out_nseg N/2] = [f1 | f0 | f0] or [f1 | f0].  Arguments an epilogue does not use are ignored.                        */
int sr_rows_split_f16(float* d_src, const float* d_embed, const int32_t* d_tok_id, const float* d_norm_w, float eps,
                      int32_t T, int32_t K, int32_t nseg, void* d_planes, float* d_a_inv, const float* d_gu_cmax,
                      float* d_act_sc, float* d_act_inv, sr_stream stream);
int sr_gu_cmax_f16(const void* d_wgu_planes, const float* d_wgu_inv, int32_t I, int32_t K, int32_t nseg, float* d_cmax,
                   sr_stream stream);
int sr_gemm_f16_planes(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t a_nseg,
                       const float* d_a_scale, const float* d_w_scale, void* d_C, const int32_t* d_pos,
                       const float* d_rope_cos, const float* d_rope_sin, int32_t n_rope, int32_t head_dim,
                       const float* d_bias, const int32_t* d_seq_of, const float* d_out_scale, int32_t out_nseg,
                       sr_stream stream);
int sr_gemm_qkv_rope(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, void* d_C,
                     const int32_t* d_pos, const float* d_rope_cos, const float* d_rope_sin,
                     int32_t n_rope, int32_t head_dim, sr_stream stream);
/* The same with a bias (Qwen2's q_proj / k_proj / v_proj, modeling/bidrectional_qwen2.py:68-101): d_bias fp32 [N], q rows then k
 * rows then v rows like d_W, added to the fp32 accumulator before the rotation; NULL = no bias (then the bits of
 * sr_gemm_qkv_rope).  fp32_out = 0: C bf16 [M,N]; 1: C fp32 [M,N], the epilogue of the fp32 regime's bf16-plane GEMM.      */
int sr_gemm_qkv_rope_bias(const void* d_A, const void* d_W, int32_t M, int32_t N, int32_t K, void* d_C,
                          const int32_t* d_pos, const float* d_rope_cos, const float* d_rope_sin,
                          int32_t n_rope, int32_t head_dim, const float* d_bias, int32_t fp32_out, sr_stream stream);
int sr_attention_varlen(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, const int32_t* d_pos,
                        const uint8_t* d_key_valid, const float* d_rope_cos, const float* d_rope_sin,
                        int32_t B, int32_t num_heads, int32_t num_kv_heads, int32_t head_dim, sr_stream stream);
/* The attention of the encoder's fp32 regime: d_qkv fp32 [T,(nh+2nkv)*hd] with q / k already rotated, fp32 scores, softmax and
 * P.V.  Exactly one output: d_out_f32 fp32 [T,nh*hd] (what fp32_planes = 16 uses), or d_out_planes bf16 [T, n_seg*nh*hd] = the
 * bf16 plane segments the o_proj GEMM consumes, fp32_planes = 3 (6 segments: planes 2 0 1 1 0 0) or 2 (3 segments: 1 0 0);
 * fp32_planes is ignored with d_out_f32.  d_qkv and d_out_f32 must be 16-byte aligned, d_out_planes 8-byte aligned (else
 * SR_ERR_INVALID).  max_seqlen = the longest sequence of the batch (it sizes the grids and the LDS of the
 * short-sequence kernel: never pass less).  head_dim 64 or 128, else SR_ERR_UNSUPPORTED and nothing is launched.  The kernel is
 * chosen per sequence (<= 64 tokens at 4 q heads per kv head: fp32 MFMA), so a sequence's bits do not depend on its batch.
 * Launch plan of the <= 64-token kernel: a sequence needs LDS for its own ceil(S / 16) blocks of 16 keys, and the encoder, which holds
 * cu_seqlens on the host, runs one launch per such class (1..4) that has a sequence.  This entry point does not know the classes: it
 * runs ONE launch with LDS for max_seqlen's class, which serves every shorter sequence too (one that needs more is skipped, never
 * overrun).  The bits are the same on every route.  Dev switch SR_ATTN_F32_LAYOUT (read per call): 0 = the form before the plan (LDS by
 * max_seqlen, q staged through LDS, element stores), 2 = a launch per class up to max_seqlen's even here (tests). */
int sr_attention_varlen_f32(const float* d_qkv, float* d_out_f32, void* d_out_planes, int32_t fp32_planes,
                            const int32_t* d_cu_seqlens, const uint8_t* d_key_valid, int32_t B, int32_t num_heads,
                            int32_t num_kv_heads, int32_t head_dim, int32_t max_seqlen, sr_stream stream);
/* Test-only hooks: what the bf16 regime (fp32_planes = 0) and the two heads launch besides the GEMMs and the attention, each with
 * the arguments the encoder fills (per-kernel tables and bounds: tests/test_bf16_regime_gpu.py, tests/bf16_regime_cases.py).  Every
 * call validates its arguments before it touches a device (SR_ERR_INVALID).
 * sr_rmsnorm_bf16: one launch of the RMSNorm kernel on d_x fp32 [T, H] (H % 4 == 0; H = 256 / 512 / 1024 / 2048 / 3072 / 4096 run
 *   the register kernels).  d_embed + d_tok_id [T] (both or neither): row t is gathered from d_embed[d_tok_id[t]] first.  d_delta bf16
 *   [T, H] (or NULL): the pending residual, x = fl(x + delta).  With either, the new row is written back to d_x.  d_norm_w [H]:
 *   y = (x rsqrt(mean(x^2) + eps)) w goes to d_xn (bf16 [T, H], round to nearest even) and / or d_xn_f32 (fp32 [T, H]); NULL = only
 *   the residual is added and both outputs must be NULL.
 * sr_dense_head_pool: the dense head's two launches.  Per token rs = rsqrt(mean(x^2) + eps), inv = 1 / max(|x rs w|, 1e-12)
 *   (d_stats: [T] pairs of fp32, scratch); d_out fp32 [B, H] = mean over the tokens t of [cu[b], cu[b + 1]) with
 *   d_pos[t] >= d_pool_start[b] of ((x rs) w) inv, summed in token order; a sequence without such a token gives zeros, T = 0 zeros
 *   everywhere.
 * sr_sparse_finish: d_out[i] = log(max(bf16(d_out[i]) scale, 0) + 1) in place over n elements, product and sum in fp32, the
 *   logarithm in double and rounded once; round_bf16 = 0 leaves out the bf16 rounding of the input (the fp32 regime).
 * sr_encode_plan: the packing plan of a [B, L] batch, as every sr_encode_* call computes it first.  mode 0 (dense) / 2 (both):
 *   row b keeps the positions [min(first key, L - len), L), pool_start = L - len; mode 1 (sparse): [first key, last key]; a row
 *   without a key keeps nothing.  d_row_shift [B] (or NULL, sr_encode_rows): positions and pool_start are counted that many
 *   columns further left (never below 0).  Written: d_span_start, d_span_len, d_pool_start, d_row_len [B], d_cu_seqlens [B + 1],
 *   *n_tokens (host), and for the n_tokens packed tokens d_tok_id (clamped into [0, vocab)), d_pos, d_key_valid (uint8) and
 *   d_seq_of (row index; -2 for a masked position inside the span unless mode 0).  capacity = elements of the four token arrays:
 *   a batch that packs to more is SR_ERR_INVALID (the [B] arrays and *n_tokens are written, the token arrays are not touched). */
int sr_rmsnorm_bf16(float* d_x, const float* d_embed, const int32_t* d_tok_id, const void* d_delta, const float* d_norm_w,
                    void* d_xn, float* d_xn_f32, float eps, int32_t T, int32_t H, sr_stream stream);
int sr_dense_head_pool(const float* d_x, const float* d_norm_w, const int32_t* d_cu_seqlens, const int32_t* d_pos,
                       const int32_t* d_pool_start, float eps, int32_t B, int32_t T, int32_t H, void* d_stats, float* d_out,
                       sr_stream stream);
int sr_sparse_finish(float* d_out, int64_t n, float scale, int32_t round_bf16, sr_stream stream);
int sr_encode_plan(const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L, int32_t mode, int32_t vocab,
                   const int32_t* d_row_shift, int32_t* d_span_start, int32_t* d_span_len, int32_t* d_pool_start,
                   int32_t* d_row_len, int32_t* d_cu_seqlens, int32_t* d_tok_id, int32_t* d_pos, uint8_t* d_key_valid,
                   int32_t* d_seq_of, int64_t capacity, int64_t* n_tokens, sr_stream stream);
/* Test-only hook: the plane split of SR_PRECISION_BF16X3 / _BF16X6 on its own (split_bf16_kernel, csrc/dense_split.hip), as
 * sr_dense_index_set_precision runs it over a segment and every split-mode search over its queries (tests/test_dense_split_gpu.py,
 * tests/dense_split_cases.py).  d_src fp32 [n], 16-byte aligned, n % 4 == 0; d_p0 and the nullable d_p1, d_p2: bf16 words [n], 8-byte
 * aligned.  p0 = bf16(v), p1 = bf16(v - p0), p2 = bf16(v - p0 - p1), every rounding to nearest even, both subtractions exact in
 * fp32; a finite v whose bf16 rounding would be infinite (|v| >= 0x7F7F8000, the top 2^-8 of the top binade) takes the largest
 * finite bf16 number of its sign as p0, so that the planes of a finite value are finite and p0 + p1 + p2 = v exactly for every
 * |v| >= 2^-110 (below that the planes lose what lies under bf16's smallest subnormal 2^-133).  Non-finite input is outside the
 * contract of the split modes.  A null d_src / d_p0, n < 0, n % 4 != 0 or a misaligned pointer is SR_ERR_INVALID before anything
 * launches; n = 0 is SR_OK.                                                                                                     */
int sr_split_bf16(const float* d_src, int64_t n, void* d_p0, void* d_p1, void* d_p2, sr_stream stream);
/* Test-only hook: the top-k protocol every search ends in (csrc/topk.hip, csrc/topk_large.hip), replayed on a caller-supplied stream of
 * (score, id) entries with the thresholds and the running set read out after every compaction (tests/test_topk_replay_gpu.py,
 * tests/topk_cases.py).  d_scores fp32 / d_ids int64 [nq, n_stream] on the device; an entry with id < 0 is no entry, every other id must
 * be below 2^32 and unique within its query, no score may be NaN.  h_steps (host): n_steps + 1 ascending offsets into the stream, step i
 * = entries [h_steps[i], h_steps[i + 1]), at most 2^22 of them.  Per step a producer appends the step's entries (filter = 1: only those
 * with score >= tau[q], as every score kernel does; 0: all), then the library's compaction runs with k, k2 (0: no second rank) and
 * select_over as the searches pass them (select_over is clamped into [k, 2k]); after the last step the final sort.  seg_n > 0: the
 * producers use the segmented candidate slots of the split-bf16 kernels - producer p takes the step's entries [p seg_group,
 * (p + 1) seg_group) and owns segment p; 1..4 survivors go to its segment, more (or p >= seg_n) behind one atomic reservation.
 * Outputs: d_out_scores / d_out_ids [nq, k] and d_out_counts [nq] as sr_dense_search writes them (pad_score, id -1); per step
 * d_trace_tau / d_trace_tau2 fp32 [n_steps, nq] (tau; the k2-th best score, tau2_init until a select has refreshed it) and
 * d_trace_run int32 [n_steps, nq] (keys held) after the compaction, d_trace_cand int32 [n_steps, nq] the candidates it found, and, unless
 * NULL, d_trace_keys uint64 [n_steps, nq, 2k]: the running set's keys (ordered score word << 32 | ~id), the first d_trace_run of each row.
 * The workspace lives for the call, which waits for the stream before it returns.  SR_ERR_INVALID before anything touches a device: a
 * null pointer (but d_trace_keys), sizes out of range, k outside [1, 2^20], k2 outside [0, k) or k2 > 0 / seg_n > 0 with k >
 * sr_max_topk(), seg_n no multiple of 4, steps that do not ascend inside [0, n_stream] or are longer than 2^22.                       */
int sr_topk_replay(const float* d_scores, const int64_t* d_ids, int64_t nq, int64_t n_stream, const int64_t* h_steps, int n_steps,
                   int k, int k2, int64_t select_over, int filter, int seg_n, int seg_group, float tau2_init, float pad_score,
                   float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, float* d_trace_tau, float* d_trace_tau2,
                   int32_t* d_trace_cand, int32_t* d_trace_run, uint64_t* d_trace_keys, sr_stream stream);

/* ------------------------------------------------------------------------------------------------------- collapsed search ---
 * sr_topk_collapse: the device step of the collapsed search (top-k distinct groups, each scored by its best passage: "MaxP", field
 * collapsing; scaling_retriever_amd/collapse.py).  No reference counterpart.  Turns every ranked row into its
 * first-occurrence-per-group row and says whether that row is provably complete.
 *   Inputs: d_scores fp32 / d_ids int64 [nq, row_len], rows as the searches return them (score descending, ties by ascending id).  The
 *   valid prefix of row q is d_counts[q] entries (int32, clamped to [0, row_len]: sr_sparse_search's counts), or with d_counts == NULL
 *   everything before the first negative id (the dense searches' padding).  row_len is any value in [0, 2^31): a row is streamed in
 *   chunks of 1024 ranks, never staged whole.  d_keys int32 [n_keys] maps an id to its group key >= 0.
 *   Outputs: d_out_scores fp32 / d_out_ids int64 / d_out_keys int32 [nq, k]: the first k entries of the valid prefix whose key did not
 *   occur earlier in the row, in row order, the rest padding (-FLT_MAX, -1, -1); d_out_counts int32 [nq] = min(k, distinct keys of the
 *   prefix); d_out_complete int32 [nq] = 1 iff out_counts[q] == k, or the valid prefix is shorter than row_len (the search had nothing
 *   more to return), or exhaustive != 0 (the caller states that the rows are whole rankings), else 0.  When complete, the row is the
 *   top-k groups of the full ranking: the order on (score, id) is total, so every passage outside the prefix ranks behind everything
 *   inside it and cannot change the first k first occurrences.
 *   1 <= k <= sr_max_topk() (the keys met so far sit in an LDS hash table of 1.5 (k + 1024) slots); a larger k: SR_ERR_UNSUPPORTED.
 *   Null pointers (d_counts may be NULL), nq < 0, row_len outside [0, 2^31), n_keys < 0, k < 1: SR_ERR_INVALID before anything touches
 *   a device.  nq == 0 and row_len == 0 are legal (row_len == 0: every row is padding with count 0, complete only when exhaustive).
 *   An id outside [0, n_keys) inside a valid prefix, or a negative key: SR_ERR_INVALID, found on the device, sr_last_error() names the
 *   first (query, position); the outputs are then not to be used and the library stays usable.  A workgroup stops reading its row
 *   behind the chunk of 1024 ranks in which it found its k-th group: entries of later chunks are NOT checked (those of that chunk are).
 *   One workgroup per query, no global atomics, the same bytes on every run; the call waits for the stream once, at its end, to read
 *   the status (and frees its nq * 4 scratch bytes).                                                                             */
int sr_topk_collapse(const float* d_scores, const int64_t* d_ids, const int32_t* d_counts, int64_t nq, int64_t row_len, int exhaustive,
                     const int32_t* d_keys, int64_t n_keys, int k, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_keys,
                     int32_t* d_out_counts, int32_t* d_out_complete, sr_stream stream);

/* ------------------------------------------------------------------------------------- hits inside a collapsed search's groups ---
 * The two device steps of collapse.group_hits (csrc/group_hits.hip): the top-m passages of every group a collapsed
 * search returned ("inner hits").  Between them run the pair scorers above, unchanged, so a hit's score is sr_dense_score_pairs /
 * sr_sparse_score_pairs of that pair bit for bit.  No reference counterpart.
 *
 * The member table (built once per key table, collapse.member_table): d_uniq_keys int32 [n_groups] STRICTLY ASCENDING group keys;
 * d_member_indptr int64 [n_groups + 1]; d_member_ids int64 [n_members], the documents of group g at indptr[g] .. indptr[g + 1], ascending.
 * Keys are arbitrary non-negative int32: a slot's key is looked up by binary search, never used as an array index.
 *
 * sr_group_members_count / _fill: which members of every (query, slot) the query's filter allows, as CSR over the nq * kg slots.
 *   d_slot_keys int32 [nq, kg]: the keys a collapsed search returned; a negative key is padding and has no members.
 *   Filter: n_masks == 0: none (d_mask_words / d_query_group unused).  Otherwise d_mask_words uint32 [n_masks, W], W = ceil(n_bits / 32),
 *   stacked bitmaps in the convention of sr_dense_search_grouped, and d_query_group int32 [nq]: query q's members are tested against
 *   bitmap d_query_group[q]; n_masks == 1 with d_query_group == NULL: the one bitmap for every query.
 *   count  writes d_out_indptr int64 [nq * kg + 1], the exclusive scan in slot order of the number of allowed members of every slot, and
 *          *total (host) = its last entry.
 *   fill   the same inputs and that d_out_indptr: d_out_ids int64 [capacity] holds at indptr[s] .. indptr[s + 1] the allowed members of
 *          slot s in ascending order; nothing is written at or beyond `capacity`.
 *   Eight lanes per slot, a ballot per eight members; no global atomics, the same bytes on every run.  Each call waits for the stream
 *   once, to read the status (and count's total), and frees its scratch (count: 4 bytes per slot).
 *   SR_ERR_INVALID before any device work: null pointers (the mask pointers only where n_masks asks for them), nq < 0, kg < 0,
 *   nq * kg >= 2^38, negative sizes, n_members >= 2^31.  SR_ERR_INVALID found on the device, the outputs then not to be used and the
 *   library usable as before - sr_last_error() names the first offender in slot order: a d_query_group entry outside [0, n_masks) ("query
 *   Q is in group G"), a non-negative slot key absent from the table ("query Q, slot J: key K"), under a mask a member id outside
 *   [0, n_bits) ("query Q, slot J: member id I"; without a mask the ids are copied unread).  nq * kg == 0: indptr[0] = 0, total 0.
 *
 * sr_segment_topm: the m best entries of every segment of a scored CSR.  d_scores fp32 / d_ids int64 [d_seg_indptr[n_segs]], segment s
 *   at d_seg_indptr[s] .. [s + 1] (int64 [n_segs + 1], starting at 0, never decreasing), of any length, ids in any order (below
 *   INT64_MAX).  With use_threshold != 0 only entries with score > threshold take part.  Order: score descending compared as floats
 *   (-0.0 and +0.0 are one score and read back as +0.0), then id ascending - the order of the searches.  d_out_scores fp32 / d_out_ids
 *   int64 [n_segs, m]: the best min(m, count) entries, then (pad_score, -1); d_out_counts int32 [n_segs] = the number of entries that
 *   took part (NOT cut to m).  One wave per segment over tiles of 64 entries, the running best one per lane, in-wave bitonic sort and
 *   merge through cross-lane exchanges; no atomics, the same bytes on every run.  1 <= m <= 64.  m outside that, null pointers, n_segs
 *   < 0: SR_ERR_INVALID before any device work; a d_seg_indptr that does not start at 0 or decreases: SR_ERR_INVALID found on the device
 *   (reads stay inside [0, d_seg_indptr[n_segs])), naming the place.  The call waits for the stream once.                            */
int sr_group_members_count(const int32_t* d_slot_keys, int64_t nq, int64_t kg, const int32_t* d_uniq_keys, int64_t n_groups,
                           const int64_t* d_member_indptr, const int64_t* d_member_ids, int64_t n_members,
                           const uint32_t* d_mask_words, int64_t n_masks, int64_t n_bits, const int32_t* d_query_group,
                           int64_t* d_out_indptr, int64_t* total, sr_stream stream);
int sr_group_members_fill(const int32_t* d_slot_keys, int64_t nq, int64_t kg, const int32_t* d_uniq_keys, int64_t n_groups,
                          const int64_t* d_member_indptr, const int64_t* d_member_ids, int64_t n_members,
                          const uint32_t* d_mask_words, int64_t n_masks, int64_t n_bits, const int32_t* d_query_group,
                          const int64_t* d_out_indptr, int64_t* d_out_ids, int64_t capacity, sr_stream stream);
int sr_segment_topm(const float* d_scores, const int64_t* d_ids, const int64_t* d_seg_indptr, int64_t n_segs, int m,
                    int use_threshold, float threshold, float pad_score, float* d_out_scores, int64_t* d_out_ids,
                    int32_t* d_out_counts, sr_stream stream);

/* ---- lexical: BM25 from token ids (csrc/token_counts.hip, csrc/bm25_weights.hip) ------------------------------------
 *
 * sr_token_counts: token rows -> a term-frequency CSR.  d_ids / d_mask int64 [B, L] row-major are a loader's input_ids /
 *   attention_mask, padding on either side; d_mask NULL = every slot is real.  A slot counts when its mask is non-zero and its id is
 *   none of the n_skip <= 16 ids of h_skip (host memory; BOS, EOS, pad).  Masked and skipped slots are not range-checked.  Row b yields
 *   its distinct counted ids ascending in d_cols (int32) with d_vals = f32(occurrences) (exact: L <= sr_token_counts_max_len() = 8192);
 *   d_row_ptr int64 [B + 1] the CSR offsets; d_len int32 [B] the number of counted slots of the row (the sum of its values: BM25's
 *   document length).  capacity, *h_nnz and SR_ERR_NOMEM exactly as sr_sparse_compact (nothing but d_row_ptr is written when it does not
 *   fit; B * L always fits).  The call reads the total and the status back and waits for the stream once.  A counted id outside
 *   [0, n_terms) is found on the device: SR_ERR_INVALID, sr_last_error() names row, position and id of the smallest (row, position),
 *   d_cols / d_vals / d_len are not written.  L above the maximum, B >= 2^24 (one workgroup per row: the launch limit), n_skip outside [0, 16], n_terms outside [1, 2^31), negative sizes,
 *   null pointers: SR_ERR_INVALID before any device call.  B == 0 or L == 0: a valid empty result (row offsets all 0, lengths 0).
 *   32-bit keys (the id, 0xFFFFFFFF for a slot that does not count) are sorted ascending, run heads flagged, a head's frequency is the
 *   distance to the end of its run, heads appended in order: rows of at most 256 slots by one wave each with the keys in registers
 *   (cross-lane exchanges, no barrier; four rows per workgroup), longer rows by a workgroup each with the keys in LDS.  The sort runs
 *   twice, for the count and for the fill.  No atomic decides an output byte: two calls return the same bytes.
 *
 * sr_bm25_weights: term frequencies -> BM25 weights on a term-major CSR (d_indptr int64 [n_terms + 1] from 0 to nnz, d_doc_ids int32
 *   [nnz], d_tf fp32 [nnz]), d_doc_len int32 [n_docs], d_idf fp32 [n_terms].  Posting p of term t with document d:
 *     K = f32(a + f32(s * f32(doc_len[d])));   w = f32(idf[t] * f32(f32(tf * numer) / f32(tf + K)))
 *   one rounded fp32 operation at a time, contraction off, the division correctly rounded.  d_out_vals fp32 [nnz] may be d_tf.  The
 *   scalars and the idf table come from the host (bm25.py: bm25_scalars, idf_table): no logarithm runs here.  One thread per posting,
 *   the term found by a search of d_indptr per wave; d_doc_len is the only gathered stream.  A document id outside [0, n_docs) is found
 *   on the device: SR_ERR_INVALID naming posting and id, the outputs then not to be used.  Null pointers, negative sizes, n_terms or
 *   n_docs >= 2^31: SR_ERR_INVALID before any device call; nnz == 0 is legal.  Waits for the stream once, to read the status.        */
int sr_token_counts_max_len(void);
int sr_token_counts(const int64_t* d_ids, const int64_t* d_mask, int64_t B, int64_t L, const int32_t* h_skip, int n_skip,
                    int64_t n_terms, int64_t* d_row_ptr, int32_t* d_cols, float* d_vals, int32_t* d_len, int64_t capacity,
                    int64_t* h_nnz, sr_stream stream);
int sr_bm25_weights(const int64_t* d_indptr, const int32_t* d_doc_ids, const float* d_tf, int64_t n_terms, int64_t nnz,
                    const int32_t* d_doc_len, int64_t n_docs, const float* d_idf, float numer, float a, float s, float* d_out_vals,
                    sr_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SR_HIP_H */
