// The dense index handle: segments and their preparation (bf16 planes, the certified filter's fp16 plane), settings, statistics.
#include "dense_index.h"
#include "dense_split.h"
#include "dense_filter.h"

// fp16 plane + per-document error terms of one segment.  Never fails the caller: a segment that cannot be filtered (values
// that are not finite or beyond 2^55, no device memory for the plane) is marked, and the index then answers with the exact
// kernel - the filter is an accelerator of the exact search, not a precondition.
int filter_prepare_segment(sr_dense_index* idx, DenseSegment& seg) {
    if (seg.f_state != 0) return SR_OK;
    seg.f_state = -1;
    if (idx->dim % 64 != 0) return SR_OK;
    if (idx->f_scratch.reserve(2, nullptr) != SR_OK) return SR_OK;
    unsigned int* const f_scratch = idx->f_scratch.p;
    unsigned int h[2] = {0, 0};
    SR_CHECK_HIP(hipMemsetAsync(f_scratch, 0, 8, nullptr));
    SR_TRY(launch_filter_absmax(seg.rows, idx->row_dtype, seg.n, idx->dim, f_scratch, nullptr));
    SR_CHECK_HIP(hipMemcpy(h, f_scratch, 8, hipMemcpyDeviceToHost));
    float absmax;
    memcpy(&absmax, &h[0], 4);
    if (h[0] >= 0x7f800000u || !sr_filter_scale_of(absmax, &seg.fsd, &seg.fisd)) return SR_OK;
    if (seg.fpl.reserve(seg.n * (int64_t)idx->dim, nullptr) != SR_OK || seg.fxy.reserve((int64_t)(filter_xy_bytes(seg.n) / sizeof(float)), nullptr) != SR_OK) {
        seg.fpl.release();
        return SR_OK;
    }
    SR_TRY(launch_filter_plane(seg.rows, idx->row_dtype, seg.n, idx->dim, seg.fsd, sr_filter_sigma(idx->dim), seg.fpl.p, seg.fxy.p,
                               reinterpret_cast<int*>(f_scratch) + 1, nullptr));
    SR_TRY(launch_filter_group_max(seg.fxy.p, seg.n, seg.fxy.p + 2 * seg.n, nullptr));
    SR_CHECK_HIP(hipMemcpy(h, f_scratch, 8, hipMemcpyDeviceToHost));
    {
        std::vector<float> gm((size_t)ceil_div64(seg.n, 128) * 2);
        SR_CHECK_HIP(hipMemcpy(gm.data(), seg.fxy.p + 2 * seg.n, gm.size() * 4, hipMemcpyDeviceToHost));
        seg.fx_max = seg.fy_max = 0.f;
        for (size_t g = 0; g < gm.size(); g += 2) {
            seg.fx_max = gm[g] > seg.fx_max ? gm[g] : seg.fx_max;
            seg.fy_max = gm[g + 1] > seg.fy_max ? gm[g + 1] : seg.fy_max;
        }
    }
    if (h[1] != 0) {                          // a non-finite error term: the segment is not filterable, its plane is of no use
        seg.fpl.release(); seg.fxy.release();
        return SR_OK;
    }
    seg.f_state = 1;
    return SR_OK;
}

static int split_segment(sr_dense_index* idx, DenseSegment& seg, int want) {
    if (seg.n_planes >= want) return SR_OK;
    const int64_t elems = seg.n * (int64_t)idx->dim;
    for (int p = seg.n_planes; p < want; ++p) {
        if (seg.pl[p].reserve(elems, nullptr) != SR_OK) {
            for (int r = seg.n_planes; r < p; ++r) seg.pl[r].release();
            sr_set_error("split precision needs %zu more bytes of device memory per plane of this segment", (size_t)elems * 2);
            return SR_ERR_NOMEM;
        }
    }
    // (re)compute all planes: cheap next to one search, and keeps the planes consistent
    SR_TRY(launch_split_bf16(static_cast<const float*>(seg.rows), seg.pl[0].p, want >= 2 ? seg.pl[1].p : nullptr, want == 3 ? seg.pl[2].p : nullptr, elems, nullptr));
    SR_CHECK_HIP(hipStreamSynchronize(nullptr));
    seg.n_planes = want;
    return SR_OK;
}

extern "C" int sr_dense_index_create(sr_dense_index** out, int dim) {
    SR_REQUIRE(out, "sr_dense_index_create: null out");
    SR_REQUIRE(dim > 0 && dim % 16 == 0, "sr_dense_index_create: dim=%d must be a positive multiple of 16", dim);
    *out = new sr_dense_index();
    (*out)->dim = dim;
    return SR_OK;
}

// one segment of rows stored as `dtype`; every check comes before the index is touched
static int dense_index_add_rows(sr_dense_index* idx, const void* d_rows, int dtype, int64_t n_rows, int64_t id_base, int64_t id_stride,
                                const char* who) {
    SR_REQUIRE(idx, "%s: null index", who);
    SR_REQUIRE(n_rows >= 0 && id_stride >= 1 && id_base >= 0, "%s: bad sizes", who);
    if (n_rows == 0) return SR_OK;
    SR_REQUIRE(d_rows, "%s: null rows", who);
    SR_REQUIRE(((uintptr_t)d_rows & 15) == 0, "%s: rows must be 16-byte aligned", who);
    SR_REQUIRE(id_base + (n_rows - 1) * id_stride < 0xffffffffll, "%s: global doc index exceeds 32 bits", who);
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_REQUIRE(idx->segs.empty() || idx->row_dtype == dtype, "%s: the index holds %s rows; an index holds fp32 rows or fp16 rows, not both", who,
               idx->row_dtype == SR_DTYPE_F16 ? "fp16" : "fp32");
    if (dtype == SR_DTYPE_F16 && planes_of(idx->precision)) {
        sr_set_error("%s: the split-bf16 precisions are not available for fp16-stored rows", who);
        return SR_ERR_UNSUPPORTED;
    }
    DenseSegment seg;
    seg.rows = d_rows; seg.n = n_rows; seg.id_base = id_base; seg.id_stride = id_stride;
    const int dtype_before = idx->row_dtype;
    idx->row_dtype = dtype;                  // the segment's preparation reads it
    int rc = SR_OK;
    if (planes_of(idx->precision)) rc = split_segment(idx, seg, planes_of(idx->precision));
    if (rc == SR_OK && idx->precision == SR_PRECISION_FP32_FILTERED) rc = filter_prepare_segment(idx, seg);
    if (rc != SR_OK) { idx->row_dtype = dtype_before; return rc; }
    idx->segs.push_back(seg);
    idx->ntotal += n_rows;
    return SR_OK;
}

extern "C" int sr_dense_index_add(sr_dense_index* idx, const float* d_rows, int64_t n_rows, int64_t id_base, int64_t id_stride) {
    return dense_index_add_rows(idx, d_rows, SR_DTYPE_F32, n_rows, id_base, id_stride, "sr_dense_index_add");
}

extern "C" int sr_dense_index_add_f16(sr_dense_index* idx, const void* d_rows_f16, int64_t n_rows, int64_t id_base, int64_t id_stride) {
    return dense_index_add_rows(idx, d_rows_f16, SR_DTYPE_F16, n_rows, id_base, id_stride, "sr_dense_index_add_f16");
}

extern "C" int sr_dense_index_row_dtype(const sr_dense_index* idx) { return idx ? idx->row_dtype : -1; }

extern "C" int sr_dense_index_owned_bytes(sr_dense_index* idx, int64_t* out) {
    SR_REQUIRE(idx && out, "sr_dense_index_owned_bytes: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    int64_t bytes = 0;
    for (const DenseSegment& seg : idx->segs) {
        const int64_t plane = seg.n * (int64_t)idx->dim * 2;
        bytes += plane * seg.n_planes;                                                   // split_segment
        if (seg.fpl.p) bytes += plane;                                                   // filter_prepare_segment
        if (seg.fxy.p) bytes += (int64_t)filter_xy_bytes(seg.n);
    }
    *out = bytes;
    return SR_OK;
}

extern "C" int64_t sr_dense_index_ntotal(const sr_dense_index* idx) { return idx ? idx->ntotal : -1; }

int64_t dense_id_end(const sr_dense_index* idx) {
    int64_t end = 0;
    for (const DenseSegment& seg : idx->segs)
        if (seg.n > 0 && seg.id_base + (seg.n - 1) * seg.id_stride + 1 > end) end = seg.id_base + (seg.n - 1) * seg.id_stride + 1;
    return end;
}
extern "C" int64_t sr_dense_index_id_end(const sr_dense_index* idx) { return idx ? dense_id_end(idx) : -1; }

extern "C" int sr_dense_index_set_workspace_limit(sr_dense_index* idx, int64_t bytes) {
    SR_REQUIRE(idx && bytes >= (1 << 20), "sr_dense_index_set_workspace_limit: bad argument");
    idx->ws_limit = bytes;
    return SR_OK;
}

extern "C" int sr_dense_index_set_batch_invariant(sr_dense_index* idx, int on) {
    SR_REQUIRE(idx, "sr_dense_index_set_batch_invariant: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->batch_invariant = on != 0;
    return SR_OK;
}

extern "C" int sr_dense_index_destroy(sr_dense_index* idx) {
    if (!idx) return SR_OK;
    idx->order.release();
    for (DenseSegment& seg : idx->segs) {
        for (int p = 0; p < 3; ++p) seg.pl[p].release();
        seg.fpl.release(); seg.fxy.release();
    }
    idx->ws.release(); idx->wsf.release(); idx->ws2.release(); idx->ws3.release();
    for (int p = 0; p < 3; ++p) idx->qpl[p].release();
    idx->qa.release(); idx->a_scores.release(); idx->a_ids.release(); idx->flags.release();
    idx->f_scratch.release();
    idx->redo_q.release(); idx->redo_idx.release(); idx->redo_scores.release(); idx->redo_ids.release();
    idx->pair_segs.release();
    if (idx->pair_status) (void)hipFree(idx->pair_status);      // allocated by pair_status_begin / subset_status_begin
    idx->mask_words.release(); idx->mask_list.release(); idx->mask_blocks.release();
    idx->grp_valid.release(); idx->grp_qoff.release(); idx->grp_counts.release();
    idx->range_tab.release(); idx->range_qoff.release(); idx->range_union.release(); idx->range_used.release();
    delete idx;
    return SR_OK;
}

extern "C" int sr_dense_index_set_precision(sr_dense_index* idx, int mode) {
    SR_REQUIRE(idx, "sr_dense_index_set_precision: null index");
    SR_REQUIRE(mode == SR_PRECISION_FP32 || mode == SR_PRECISION_BF16X3 || mode == SR_PRECISION_BF16X6 ||
                   mode == SR_PRECISION_FP32_FILTERED,
               "sr_dense_index_set_precision: unknown mode %d", mode);
    std::lock_guard<std::mutex> lock(idx->mu);
    if (planes_of(mode) && idx->row_dtype == SR_DTYPE_F16) {
        sr_set_error("sr_dense_index_set_precision: the split-bf16 precisions are not available for fp16-stored rows");
        return SR_ERR_UNSUPPORTED;
    }
    if (planes_of(mode)) {
        SR_REQUIRE(idx->dim % 64 == 0, "split precisions need dim %% 64 == 0 (dim = %d)", idx->dim);
        for (DenseSegment& seg : idx->segs) SR_TRY(split_segment(idx, seg, planes_of(mode)));
    }
    if (mode == SR_PRECISION_FP32_FILTERED)
        for (DenseSegment& seg : idx->segs) SR_TRY(filter_prepare_segment(idx, seg));
    idx->precision = mode;
    return SR_OK;
}

extern "C" int sr_dense_index_filter_stats(sr_dense_index* idx, int64_t* n_filtered, int64_t* n_fallback) {
    SR_REQUIRE(idx && n_filtered && n_fallback, "sr_dense_index_filter_stats: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *n_filtered = idx->n_filtered;
    *n_fallback = idx->n_fallback;
    return SR_OK;
}

extern "C" int sr_dense_index_filter_query_stats(sr_dense_index* idx, int64_t* n_certified, int64_t* n_redone) {
    SR_REQUIRE(idx && n_certified && n_redone, "sr_dense_index_filter_query_stats: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *n_certified = idx->nq_certified;
    *n_redone = idx->nq_redone;
    return SR_OK;
}

extern "C" int sr_dense_index_profile(sr_dense_index* idx, int enable) {
    SR_REQUIRE(idx, "sr_dense_index_profile: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    idx->prof.enabled = enable != 0;
    return SR_OK;
}

extern "C" int sr_dense_index_profile_read(sr_dense_index* idx, int64_t* n_launches, double* total_ms, double* total_flop,
                                           double* total_d_bytes) {
    SR_REQUIRE(idx && n_launches && total_ms && total_flop && total_d_bytes, "sr_dense_index_profile_read: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *total_flop = idx->prof.flop;
    *total_d_bytes = idx->prof.bytes;
    *n_launches = idx->prof.read(total_ms);
    idx->prof.flop = idx->prof.bytes = 0;
    return SR_OK;
}
