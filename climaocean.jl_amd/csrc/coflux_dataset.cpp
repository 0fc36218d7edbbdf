// coflux_dataset.cpp — a dataset staged on the device and followed in time (include/coflux.h: cf_dataset_*,
// cf_materialize_dataset_restoring, cf_attach_restoring_dataset; the kernels are coflux_dataset.hip, the host rules
// coflux_dataset_rules.hpp).  The host holds each plane when it is staged, so it knows the number of inpainting sweeps before
// the first launch (one breadth-first pass) and queues exactly that many: upload, convert, sweeps, fill, regrid — all on the
// context's stream, nothing read back.  The clock is a pure function of the time and the copied table.
#include <memory>

#include "coflux_ctx.hpp"

namespace {

// what the library chooses when the descriptor leaves sweeps_per_launch to it: the tiled form at its deepest — measured fastest
// of 1, 2, 4, 8 on 360 × 180 and 1440 × 720 planes (profiles/dataset_probe.json)
constexpr int DATASET_SWEEPS_PER_LAUNCH = INPAINT_MAX_SWEEPS;

int check_level(const cf_dataset* d, const char* fn, int32_t level) {
    if (level < 0 || level >= d->n_levels) return fail(d->ctx, CF_ERR_INVALID, "%s: level %d (0…%d)", fn, level, d->n_levels - 1);
    return CF_OK;
}

}  // namespace

int dataset_target_at(const cf_dataset* d, const char* fn, double time, DatasetTarget* out) {
    if (const int l = d->first_unstaged(); l >= 0)
        return fail(d->ctx, CF_ERR_INVALID, "%s: level %d of the dataset has not been staged (every level first)", fn, l);
    int32_t level1 = 0, level2 = 0;
    double fraction = 0.0;
    if (!cfds::time_index(d->times.data(), d->n_levels, d->period, time, &level1, &level2, &fraction))
        return fail(d->ctx, CF_ERR_INVALID, "%s: the dataset's clock %g is not finite", fn, time);
    *out = DatasetTarget{d->level(level1), d->level(level2), fraction};
    return CF_OK;
}

extern "C" {

int cf_dataset_create(cf_ctx* ctx, const cf_dataset_desc* desc, cf_dataset** out) {
    const char* fn = "cf_dataset_create";
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "%s: NULL argument", fn);
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_dataset_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_dataset_desc.struct_size = %d, library expects %zu", desc->struct_size, sizeof(cf_dataset_desc));
    if (desc->ns_x < 2 || desc->ns_y < 2 || (int64_t)desc->ns_x * desc->ns_y > ((int64_t)1 << 31))
        return fail(ctx, CF_ERR_INVALID, "%s: source shape %d x %d (≥ 2 each, at most 2^31 cells)", fn, desc->ns_x, desc->ns_y);
    if (desc->n_levels < 1 || desc->n_levels > CF_DATASET_MAX_LEVELS)
        return fail(ctx, CF_ERR_INVALID, "%s: %d levels (1…%d)", fn, desc->n_levels, CF_DATASET_MAX_LEVELS);
    if (desc->sweeps_per_launch < 0 || desc->sweeps_per_launch > INPAINT_MAX_SWEEPS)
        return fail(ctx, CF_ERR_INVALID, "%s: sweeps_per_launch %d (0…%d)", fn, desc->sweeps_per_launch, INPAINT_MAX_SWEEPS);
    if (desc->max_workgroups < 0) return fail(ctx, CF_ERR_INVALID, "%s: max_workgroups %d (≥ 0)", fn, desc->max_workgroups);
    if (std::isnan(desc->fill_value)) return fail(ctx, CF_ERR_INVALID, "%s: fill_value is NaN", fn);
    if (!cfds::times_ok(desc->times, desc->n_levels, desc->period))
        return fail(ctx, CF_ERR_INVALID, "%s: times (finite, strictly increasing) or period %g (0, or above the table's span)", fn, desc->period);
    if (!desc->weights.fi || !desc->weights.fj) return fail(ctx, CF_ERR_INVALID, "%s: interpolation weights (fi, fj) are NULL", fn);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<cf_dataset> d(new cf_dataset());
    d->ctx = ctx;   // (parent() reads the grid; the handle joins the context's list only when all of it exists)
    d->ns_x = desc->ns_x;
    d->ns_y = desc->ns_y;
    d->n_levels = desc->n_levels;
    d->periodic_x = desc->periodic_x != 0;
    d->max_sweeps = desc->max_sweeps;
    d->sweeps_per_launch = desc->sweeps_per_launch;
    d->max_blocks = desc->max_workgroups;
    d->fill_value = desc->fill_value;
    d->period = desc->period;
    d->times.assign(desc->times, desc->times + desc->n_levels);
    d->weights = desc->weights;
    const size_t cells = (size_t)d->ns_x * (size_t)d->ns_y, level_bytes = d->parent() * sizeof(double) * (size_t)d->n_levels;
    HIP_TRY(ctx, d->d_plane[0].create(cells * sizeof(double)));
    HIP_TRY(ctx, d->d_plane[1].create(cells * sizeof(double)));
    HIP_TRY(ctx, d->d_upload.create(cells * sizeof(float)));
    HIP_TRY(ctx, d->d_levels.create(level_bytes));
    for (int s = 0; s < 2; ++s) {
        HIP_TRY(ctx, d->h_upload[s].create(cells * sizeof(float)));
        HIP_TRY(ctx, d->uploaded[s].create(hipEventDisableTiming));
    }
    HIP_TRY(ctx, hipMemsetAsync(d->d_levels.get(), 0, level_bytes, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d->d_plane[0].get(), 0, cells * sizeof(double), ctx->stream));
    child_adopt(ctx, d.get());
    *out = d.release();
    return CF_OK;
}

int cf_dataset_destroy(cf_dataset* d) {
    if (!d) return CF_OK;
    if (d->ctx) (void)hipSetDevice(d->device);
    child_leave(d);
    delete d;   // (hipFree waits for the device: work still in flight on the planes and levels has finished before they go)
    return CF_OK;
}

int cf_dataset_stage(cf_dataset* d, int32_t level, const float* h_plane) {
    const char* fn = "cf_dataset_stage";
    CHECK(live(d, fn, "dataset"));
    cf_ctx* ctx = d->ctx;
    CHECK(check_level(d, fn, level));
    if (!h_plane) return fail(ctx, CF_ERR_INVALID, "%s: the plane is NULL", fn);
    const size_t cells = (size_t)d->ns_x * (size_t)d->ns_y;
    const cfds::SweepPlan plan = cfds::sweep_plan(h_plane, d->ns_x, d->ns_y, d->periodic_x, d->max_sweeps);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // upload through the slot the stage call two before used (its copy has long finished, as a rule)
    const int slot = d->upload_slot;
    HIP_TRY(ctx, hipEventSynchronize(d->uploaded[slot].get()));
    std::memcpy(d->h_upload[slot].get(), h_plane, cells * sizeof(float));
    HIP_TRY(ctx, hipMemcpyAsync(d->d_upload.get(), d->h_upload[slot].get(), cells * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(d->uploaded[slot].get(), ctx->stream));
    d->upload_slot = slot ^ 1;
    int cur = 0;
    HIP_TRY(ctx, launch_dataset_convert(ctx->stream, d->d_upload.get(), d->d_plane[cur].get(), cells, d->max_blocks));
    const int per_launch = d->sweeps_per_launch > 0 ? d->sweeps_per_launch : DATASET_SWEEPS_PER_LAUNCH;
    for (int left = plan.sweeps; left > 0;) {
        const int now = std::min(left, per_launch);
        HIP_TRY(ctx, launch_dataset_inpaint(ctx->stream, d->d_plane[cur].get(), d->d_plane[cur ^ 1].get(), d->ns_x, d->ns_y, d->periodic_x, now,
                                            d->max_blocks));
        cur ^= 1;
        left -= now;
    }
    if (plan.defaulted > 0) HIP_TRY(ctx, launch_dataset_default(ctx->stream, d->d_plane[cur].get(), cells, d->fill_value, d->max_blocks));
    HIP_TRY(ctx, launch_dataset_regrid(ctx->stream, d->d_plane[cur].get(), d->ns_x, d->ns_y, &d->weights, ctx->grid, d->level(level), d->max_blocks));
    d->current = cur;
    d->last_level = level;
    d->staged[level] = cf_dataset::Staged{true, plan.sweeps, plan.filled, plan.defaulted};
    return CF_OK;
}

int cf_dataset_level(cf_dataset* d, int32_t level, const double** d_field) {
    const char* fn = "cf_dataset_level";
    CHECK(live(d, fn, "dataset"));
    CHECK(check_level(d, fn, level));
    if (!d_field) return fail(d->ctx, CF_ERR_INVALID, "%s: d_field is NULL", fn);
    *d_field = d->level(level);
    return CF_OK;
}

int cf_dataset_read_source(cf_dataset* d, double* h_out) {
    const char* fn = "cf_dataset_read_source";
    CHECK(live(d, fn, "dataset"));
    cf_ctx* ctx = d->ctx;
    if (!h_out) return fail(ctx, CF_ERR_INVALID, "%s: h_out is NULL", fn);
    if (d->last_level < 0) return fail(ctx, CF_ERR_INVALID, "%s: no level has been staged", fn);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d->d_plane[d->current].get(), (size_t)d->ns_x * (size_t)d->ns_y * sizeof(double), hipMemcpyDeviceToHost,
                                ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CF_OK;
}

int cf_dataset_stage_info(cf_dataset* d, int32_t level, int32_t* sweeps, int64_t* filled, int64_t* defaulted) {
    const char* fn = "cf_dataset_stage_info";
    CHECK(live(d, fn, "dataset"));
    CHECK(check_level(d, fn, level));
    if (!d->staged[level].done) return fail(d->ctx, CF_ERR_INVALID, "%s: level %d has not been staged", fn, level);
    if (sweeps) *sweeps = d->staged[level].sweeps;
    if (filled) *filled = d->staged[level].filled;
    if (defaulted) *defaulted = d->staged[level].defaulted;
    return CF_OK;
}

int cf_dataset_time_index(const double* times, int32_t n, double period, double time, int32_t* level1, int32_t* level2, double* fraction) {
    const char* fn = "cf_dataset_time_index";
    if (!level1 || !level2 || !fraction) return fail(nullptr, CF_ERR_INVALID, "%s: NULL argument", fn);
    if (!cfds::times_ok(times, n, period))
        return fail(nullptr, CF_ERR_INVALID, "%s: times (n ≥ 1, finite, strictly increasing) or period %g (0, or above the table's span)", fn, period);
    if (!cfds::time_index(times, n, period, time, level1, level2, fraction)) return fail(nullptr, CF_ERR_INVALID, "%s: time %g is not finite", fn, time);
    return CF_OK;
}

int cf_dataset_evaluate(cf_dataset* d, double time, double* d_out) {
    const char* fn = "cf_dataset_evaluate";
    CHECK(live(d, fn, "dataset"));
    cf_ctx* ctx = d->ctx;
    if (!d_out) return fail(ctx, CF_ERR_INVALID, "%s: d_out is NULL", fn);
    DatasetTarget T{};
    CHECK(dataset_target_at(d, fn, time, &T));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_dataset_evaluate(ctx->stream, T.level1, T.level2, T.fraction, ctx->grid, d_out, d->max_blocks));
    return CF_OK;
}

int cf_materialize_dataset_restoring(cf_ctx* ctx, double piston_velocity, cf_dataset* d, double time, const cf_ocean_surface* ocean,
                                     double* d_buffer) {
    const char* fn = "cf_materialize_dataset_restoring";
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    CHECK(live(d, fn, "dataset"));
    if (d->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "%s: the dataset belongs to another context", fn);
    if (!ocean || !ocean->S || !d_buffer) return fail(ctx, CF_ERR_INVALID, "%s: NULL argument", fn);
    if (ctx->dev.mask_kind != CF_MASK_NONE && !ocean->mask) return fail(ctx, CF_ERR_INVALID, "ocean mask is NULL");
    DatasetTarget T{};
    CHECK(dataset_target_at(d, fn, time, &T));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_dataset_restoring(ctx->stream, ctx->dev, ctx->grid, ocean->mask, piston_velocity, T.level1, T.level2, T.fraction, ocean->S,
                                          d_buffer));
    return CF_OK;
}

int cf_attach_restoring_dataset(cf_ctx* ctx, cf_dataset* d, double time_origin, double step_seconds) {
    const char* fn = "cf_attach_restoring_dataset";
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!d) {
        ctx->restoring_dataset = Attachment{};
        return CF_OK;
    }
    if (d->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "%s: the dataset belongs to another context", fn);
    if (!std::isfinite(time_origin) || !std::isfinite(step_seconds))
        return fail(ctx, CF_ERR_INVALID, "%s: time origin %g and step %g (finite)", fn, time_origin, step_seconds);
    if (const int l = d->first_unstaged(); l >= 0)
        return fail(ctx, CF_ERR_INVALID, "%s: level %d of the dataset has not been staged (every level first)", fn, l);
    ctx->restoring_dataset = Attachment{d, StepSchedule{1, time_origin, step_seconds}, 0.0};
    return CF_OK;
}

}  // extern "C"
