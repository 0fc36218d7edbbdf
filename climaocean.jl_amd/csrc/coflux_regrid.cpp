// coflux_regrid.cpp — the fixed sparse surface operator (include/coflux.h: cf_regrid_*; the kernels are coflux_regrid.hip).
// Create checks the CSR operator, turns the columns into halo-layout offsets (the context fixes nx, ny, hx, hy), builds the
// unit tables of the stated summation order — rows of at most 64 entries four to a wave, longer rows cut into segments of
// 256 entries — and copies everything to the device in one block; an apply is one launch, plus a small one when the
// operator has rows of several segments.
#include "coflux_ctx.hpp"

extern "C" {

int cf_regrid_create(cf_ctx* ctx, const cf_regrid_desc* desc, cf_regrid** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_regrid_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_regrid_desc.struct_size = %d, library expects %zu", desc->struct_size, sizeof(cf_regrid_desc));
    if (desc->mode != CF_REGRID_MEAN && desc->mode != CF_REGRID_SUM)
        return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: unknown mode %d", desc->mode);
    if (desc->max_workgroups < 0) return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: max_workgroups %d (≥ 0)", desc->max_workgroups);
    const int64_t n_rows = desc->n_rows, nnz = desc->nnz, limit = (int64_t)1 << 31;
    if (n_rows < 1 || nnz < 0 || n_rows >= limit || nnz >= limit)
        return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: n_rows %lld (1 … 2^31 − 1), nnz %lld (0 … 2^31 − 1)", (long long)n_rows, (long long)nnz);
    if (!desc->row_ptr || (nnz > 0 && (!desc->col || !desc->weight)))
        return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: NULL row_ptr, col or weight");
    const int64_t* rp = desc->row_ptr;
    if (rp[0] != 0) return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: row_ptr[0] = %lld (0)", (long long)rp[0]);
    for (int64_t r = 0; r < n_rows; ++r)
        if (rp[r + 1] < rp[r] || rp[r + 1] > nnz)
            return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: row_ptr[%lld] = %lld after %lld (non-decreasing, at most nnz = %lld)",
                        (long long)(r + 1), (long long)rp[r + 1], (long long)rp[r], (long long)nnz);
    if (rp[n_rows] != nnz)
        return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: row_ptr[n_rows] = %lld, nnz = %lld", (long long)rp[n_rows], (long long)nnz);
    const GridDesc& G = ctx->grid;
    const int64_t cells = (int64_t)G.nx * (int64_t)G.ny;
    if ((int64_t)G.sj * (int64_t)(G.ny + 2 * G.hy) >= ((int64_t)1 << 32))
        return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: the surface has more than 2^32 elements");
    for (int64_t k = 0; k < nnz; ++k) {
        if (desc->col[k] < 0 || (int64_t)desc->col[k] >= cells)
            return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: col[%lld] = %d (0 … %lld)", (long long)k, desc->col[k], (long long)(cells - 1));
        if (!std::isfinite(desc->weight[k]) || desc->weight[k] < 0.0)
            return fail(ctx, CF_ERR_INVALID, "cf_regrid_create: weight[%lld] = %g (finite, ≥ 0)", (long long)k, desc->weight[k]);
    }

    // the unit tables: the order of a row follows from its entry count alone (coflux_regrid.hip)
    std::vector<uint32_t> short_rows;
    std::vector<RegridSegment> segments;
    std::vector<RegridLongRow> long_rows;
    uint32_t slots = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t n = rp[r + 1] - rp[r];
        if (n <= REGRID_SHORT) {
            short_rows.push_back((uint32_t)r);
            continue;
        }
        const uint32_t n_seg = (uint32_t)((n + REGRID_SEGMENT - 1) / REGRID_SEGMENT);
        if (n_seg > 1) long_rows.push_back(RegridLongRow{(uint32_t)r, slots, n_seg, 0u});
        for (uint32_t s = 0; s < n_seg; ++s) {
            const int64_t first = rp[r] + (int64_t)s * REGRID_SEGMENT;
            const uint32_t count = (uint32_t)std::min<int64_t>(REGRID_SEGMENT, rp[r + 1] - first);
            segments.push_back(RegridSegment{(uint32_t)r, (uint32_t)first, count, n_seg > 1 ? slots++ : REGRID_NONE});
        }
    }
    while (short_rows.size() % 4 != 0) short_rows.push_back(REGRID_NONE);

    cf::Layout L;   // the device block, piece by piece
    const size_t at_weight = L.add((size_t)nnz * sizeof(double));
    const size_t at_segments = L.add(segments.size() * sizeof(RegridSegment));
    const size_t at_long = L.add(long_rows.size() * sizeof(RegridLongRow));
    const size_t at_offset = L.add((size_t)nnz * sizeof(uint32_t));
    const size_t at_row = L.add((size_t)(n_rows + 1) * sizeof(uint32_t));
    const size_t at_short = L.add(short_rows.size() * sizeof(uint32_t));
    const size_t upload = L.bytes;
    const size_t at_partial = L.add((size_t)slots * REGRID_PARTIAL * sizeof(double));   // written by every apply before it is read
    std::vector<unsigned char> host(upload, 0);
    if (nnz > 0) std::memcpy(host.data() + at_weight, desc->weight, (size_t)nnz * sizeof(double));
    if (!segments.empty()) std::memcpy(host.data() + at_segments, segments.data(), segments.size() * sizeof(RegridSegment));
    if (!long_rows.empty()) std::memcpy(host.data() + at_long, long_rows.data(), long_rows.size() * sizeof(RegridLongRow));
    uint32_t* offset = reinterpret_cast<uint32_t*>(host.data() + at_offset);
    for (int64_t k = 0; k < nnz; ++k) {
        const int64_t j = desc->col[k] / G.nx, i = desc->col[k] - j * G.nx;
        offset[k] = (uint32_t)((j + G.hy) * (int64_t)G.sj + (i + G.hx));
    }
    uint32_t* row_start = reinterpret_cast<uint32_t*>(host.data() + at_row);
    for (int64_t r = 0; r <= n_rows; ++r) row_start[r] = (uint32_t)rp[r];
    if (!short_rows.empty()) std::memcpy(host.data() + at_short, short_rows.data(), short_rows.size() * sizeof(uint32_t));

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    cf::DeviceBuffer<unsigned char> block;
    HIP_TRY(ctx, block.create(std::max<size_t>(L.bytes, 16)));
    unsigned char* const d = block.get();
    if (upload > 0) HIP_TRY(ctx, hipMemcpy(d, host.data(), upload, hipMemcpyHostToDevice));
    cf_regrid* rg = new cf_regrid();
    rg->n_rows = n_rows;
    rg->max_blocks = desc->max_workgroups;
    rg->d_block = std::move(block);
    RegridTables& T = rg->tables;
    T.weight = cf::Layout::at<const double>(d, at_weight);
    T.segments = cf::Layout::at<const RegridSegment>(d, at_segments);
    T.long_rows = cf::Layout::at<const RegridLongRow>(d, at_long);
    T.offset = cf::Layout::at<const uint32_t>(d, at_offset);
    T.row_start = cf::Layout::at<const uint32_t>(d, at_row);
    T.short_rows = cf::Layout::at<const uint32_t>(d, at_short);
    T.partial = cf::Layout::at<double>(d, at_partial);
    T.mask_kind = desc->mask ? ctx->dev.mask_kind : CF_MASK_NONE;
    T.mask = T.mask_kind == CF_MASK_NONE ? nullptr : desc->mask;
    T.z_surface = ctx->dev.z_surface;
    T.n_short_units = (uint32_t)(short_rows.size() / 4);
    T.n_segments = (uint32_t)segments.size();
    T.n_long_rows = (uint32_t)long_rows.size();
    T.mode = desc->mode;
    child_adopt(ctx, rg);
    *out = rg;
    return CF_OK;
}

int cf_regrid_destroy(cf_regrid* rg) {
    if (!rg) return CF_OK;
    child_leave(rg);
    // hipFree (in the delete; it needs no current device) waits for the buffer's device: an apply still in flight has finished before its tables go
    (void)hipSetDevice(rg->device);
    delete rg;
    return CF_OK;
}

int cf_regrid_apply(cf_regrid* rg, int32_t n_fields, const double* const* src, double* const* dst, double* coverage) {
    CHECK(live(rg, "cf_regrid_apply", "regridder"));
    cf_ctx* ctx = rg->ctx;
    if (n_fields < 1 || n_fields > CF_REGRID_MAX_FIELDS)
        return fail(ctx, CF_ERR_INVALID, "cf_regrid_apply: %d fields (1…%d)", n_fields, CF_REGRID_MAX_FIELDS);
    if (!src || !dst) return fail(ctx, CF_ERR_INVALID, "cf_regrid_apply: NULL src or dst");
    RegridFields F{};
    for (int f = 0; f < n_fields; ++f) {
        if (!src[f] || !dst[f]) return fail(ctx, CF_ERR_INVALID, "cf_regrid_apply: src[%d] or dst[%d] is NULL", f, f);
        F.src[f] = src[f];
        F.dst[f] = dst[f];
    }
    F.coverage = coverage;
    F.n_fields = n_fields;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_regrid(ctx->stream, rg->tables, F, rg->max_blocks, ctx->launch.cu_count));
    return CF_OK;
}

}  // extern "C"
