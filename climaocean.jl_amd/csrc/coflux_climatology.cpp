// coflux_climatology.cpp — calendar-binned means of surface fields accumulated on the device (include/coflux.h:
// cf_climatology_*, cf_calendar_bin, cf_attach_climatology; the kernels are coflux_climatology.hip).  The host keeps the total
// weight of every collection since the reset and of each bin, turns a collection of (bin, weight) into the two pairs of
// running-mean coefficients by the averagers' rule (RunningWeight, coflux_collect.hpp), and looks a step's time up in the
// calendar table; the device does one launch per collection.  The handle owns no device resource: every array is the caller's.
#include "coflux_ctx.hpp"

namespace {

// CF_ERR_INVALID unless (edges, bin_of_interval, n_edges) is a calendar table; `fn` names the entry point
int check_calendar(cf_ctx* ctx, const char* fn, const double* edges, const int32_t* bin_of_interval, int32_t n_edges) {
    if (!edges || !bin_of_interval) return fail(ctx, CF_ERR_INVALID, "%s: edges or bin_of_interval is NULL", fn);
    if (n_edges < 2) return fail(ctx, CF_ERR_INVALID, "%s: n_edges = %d (at least 2)", fn, n_edges);
    for (int32_t k = 0; k < n_edges; ++k) {
        if (!std::isfinite(edges[k])) return fail(ctx, CF_ERR_INVALID, "%s: edges[%d] is not finite", fn, k);
        if (k > 0 && !(edges[k] > edges[k - 1]))
            return fail(ctx, CF_ERR_INVALID, "%s: edges[%d] = %.17g is not above edges[%d] = %.17g (strictly increasing)", fn, k, edges[k],
                        k - 1, edges[k - 1]);
        if (k + 1 < n_edges && bin_of_interval[k] < -1)
            return fail(ctx, CF_ERR_INVALID, "%s: bin_of_interval[%d] = %d (−1 or a bin)", fn, k, bin_of_interval[k]);
    }
    return CF_OK;
}

// the lookup on a checked table of n edges: t_r = rint(time) (ties to even), then k with edges[k] ≤ t_r < edges[k + 1]
bool lookup(const double* edges, const int32_t* bin_of_interval, size_t n, double time, int32_t* bin) {
    if (!std::isfinite(time)) return false;
    const double t = std::nearbyint(time);   // the default rounding mode: to nearest, ties to even
    if (t < edges[0] || !(t < edges[n - 1])) return false;
    const size_t k = (size_t)(std::upper_bound(edges, edges + n, t) - edges) - 1;
    *bin = bin_of_interval[k];
    return true;
}

}  // namespace

int cf_climatology::collect(int32_t bin, double w) {
    const GridDesc& G = ctx->grid;
    const RunningWeight::Blend T = weight.next(w), B = bin_weight[bin].next(w);
    const size_t parent = (size_t)G.sj * (size_t)(G.ny + 2 * G.hy);
    ClimatologyFields F{};
    for (int f = 0; f < n_fields; ++f) {
        F.src[f] = src[f];
        F.total[f] = total[f];
        F.bin[f] = bins[f] + parent * (size_t)bin;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_climatology(ctx->stream, F, n_fields, G, T.store, B.store, ClimatologyBlend{T.c_prev, T.c_new, B.c_prev, B.c_new},
                                    max_blocks));
    weight.add(w);
    bin_weight[bin].add(w);
    return CF_OK;
}

int cf_climatology::check_entry(const cfck::Entry& E, const char* fn) const {
    if ((int)E.n_entries != n_bins)
        return fail(ctx, CF_ERR_INVALID, "%s: section \"%s\" has %u bins in the image, the climatology has %d", fn, E.name, E.n_entries, n_bins);
    return CF_OK;
}

// an attached climatology whose calendar table does not cover a step it would collect: nothing is launched
int cf_climatology::admit(const Attachment& at, const char* fn, int64_t first_step, int nsteps) const {
    int32_t bin;
    for (int64_t step = first_step; step < first_step + nsteps; ++step)
        if (at.when.due(step) && !lookup(edges.data(), bin_of_interval.data(), edges.size(), at.when.stamp(step), &bin))
            return fail(ctx, CF_ERR_INVALID, "%s: step %lld at time %.17g lies outside the attached climatology's calendar table "
                        "[%.17g, %.17g)", fn, (long long)step, at.when.stamp(step), edges.front(), edges.back());
    return CF_OK;
}

// the averagers' rule, into the bin the calendar gives the step's time (−1: outside the analysis window, nothing is collected;
// the table covers the step: admit)
int cf_climatology::collect_step(const Attachment& at, int64_t step) {
    int32_t bin = -1;
    lookup(edges.data(), bin_of_interval.data(), edges.size(), at.when.stamp(step), &bin);
    return bin >= 0 ? collect(bin, at.when.stride * at.step_weight) : CF_OK;
}

extern "C" {

int cf_climatology_create(cf_ctx* ctx, const cf_climatology_desc* desc, cf_climatology** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_climatology_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_climatology_desc.struct_size = %d, library expects %zu", desc->struct_size, sizeof(cf_climatology_desc));
    if (desc->n_fields < 1 || desc->n_fields > CF_CLIMATOLOGY_MAX_FIELDS)
        return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: %d fields (1…%d)", desc->n_fields, CF_CLIMATOLOGY_MAX_FIELDS);
    if (desc->n_bins < 1 || desc->n_bins > CF_CLIMATOLOGY_MAX_BINS)
        return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: %d bins (1…%d)", desc->n_bins, CF_CLIMATOLOGY_MAX_BINS);
    if (desc->max_workgroups < 0) return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: max_workgroups %d (≥ 0)", desc->max_workgroups);
    if (desc->reserved[0] != 0 || desc->reserved[1] != 0) return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: reserved is not 0");
    const int n = desc->n_fields;
    for (int f = 0; f < n; ++f)
        if (!desc->sources[f] || !desc->bins[f])
            return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: field %d has a NULL source or bins", f);
    // the averager's parent-array rule: an output — a total (one parent array) or a bin block (n_bins of them) — shares no byte
    // with a source's parent array or with another output
    const GridDesc& G = ctx->grid;
    const uintptr_t parent = (uintptr_t)G.sj * (uintptr_t)(G.ny + 2 * G.hy) * sizeof(double), block = parent * (uintptr_t)desc->n_bins;
    struct Output {
        const void* p;
        uintptr_t bytes;
        const char* what;
        int field;
    };
    std::vector<Output> outputs;
    for (int f = 0; f < n; ++f) {
        if (desc->totals[f]) outputs.push_back(Output{desc->totals[f], parent, "total", f});
        outputs.push_back(Output{desc->bins[f], block, "bin block", f});
    }
    for (size_t a = 0; a < outputs.size(); ++a) {
        const Output& A = outputs[a];
        for (int g = 0; g < n; ++g)
            if (ranges_overlap(A.p, A.bytes, desc->sources[g], parent))
                return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: the %s of field %d overlaps source %d", A.what, A.field, g);
        for (size_t b = a + 1; b < outputs.size(); ++b)
            if (ranges_overlap(A.p, A.bytes, outputs[b].p, outputs[b].bytes))
                return fail(ctx, CF_ERR_INVALID, "cf_climatology_create: the %s of field %d overlaps the %s of field %d", A.what, A.field,
                            outputs[b].what, outputs[b].field);
    }
    cf_climatology* c = new cf_climatology();
    c->n_fields = n;
    c->n_bins = desc->n_bins;
    c->max_blocks = desc->max_workgroups;
    for (int f = 0; f < n; ++f) {
        c->src[f] = desc->sources[f];
        c->total[f] = desc->totals[f];
        c->bins[f] = desc->bins[f];
    }
    child_adopt(ctx, c);
    *out = c;
    return CF_OK;
}

int cf_climatology_destroy(cf_climatology* c) {
    if (!c) return CF_OK;
    child_leave(c);
    delete c;
    return CF_OK;
}

int cf_climatology_reset(cf_climatology* c) {
    CHECK(live(c, "cf_climatology_reset", "climatology"));
    c->weight.reset();
    for (RunningWeight& b : c->bin_weight) b.reset();
    return CF_OK;
}

int cf_climatology_collect(cf_climatology* c, int32_t bin, double weight) {
    CHECK(live(c, "cf_climatology_collect", "climatology"));
    if (bin < -1 || bin >= c->n_bins) return fail(c->ctx, CF_ERR_INVALID, "cf_climatology_collect: bin %d (−1…%d)", bin, c->n_bins - 1);
    if (!c->weight.accepts(weight))
        return fail(c->ctx, CF_ERR_INVALID, "cf_climatology_collect: weight %g (> 0 and finite)", weight);
    if (bin < 0) return CF_OK;
    return c->collect(bin, weight);
}

int cf_climatology_weights(cf_climatology* c, double* total, int64_t* samples, double* bin_totals, int64_t* bin_samples) {
    CHECK(live(c, "cf_climatology_weights", "climatology"));
    if (total) *total = c->weight.total;
    if (samples) *samples = c->weight.samples;
    for (int b = 0; b < c->n_bins; ++b) {
        if (bin_totals) bin_totals[b] = c->bin_weight[b].total;
        if (bin_samples) bin_samples[b] = c->bin_weight[b].samples;
    }
    return CF_OK;
}

int cf_climatology_extremes(cf_climatology* c, int32_t field, double* d_min, double* d_max, int32_t* d_argmin, int32_t* d_argmax) {
    CHECK(live(c, "cf_climatology_extremes", "climatology"));
    cf_ctx* ctx = c->ctx;
    if (field < 0 || field >= c->n_fields) return fail(ctx, CF_ERR_INVALID, "cf_climatology_extremes: field %d (0…%d)", field, c->n_fields - 1);
    ClimatologyBinList L{};
    for (int b = 0; b < c->n_bins; ++b)
        if (c->bin_weight[b].samples > 0) L.bin[L.n++] = (uint8_t)b;
    if (L.n == 0) return fail(ctx, CF_ERR_INVALID, "cf_climatology_extremes: field %d has no available bins (nothing collected since the reset)", field);
    if (!d_min && !d_max && !d_argmin && !d_argmax) return CF_OK;
    const GridDesc& G = ctx->grid;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_climatology_extremes(ctx->stream, c->bins[field], (size_t)G.sj * (size_t)(G.ny + 2 * G.hy), L, G, d_min, d_max, d_argmin,
                                             d_argmax, c->max_blocks));
    return CF_OK;
}

int cf_calendar_bin(const double* edges, const int32_t* bin_of_interval, int32_t n_edges, double time, int32_t* bin) {
    if (!bin) return fail(nullptr, CF_ERR_INVALID, "cf_calendar_bin: bin is NULL");
    CHECK(check_calendar(nullptr, "cf_calendar_bin", edges, bin_of_interval, n_edges));
    if (!lookup(edges, bin_of_interval, (size_t)n_edges, time, bin))
        return fail(nullptr, CF_ERR_INVALID, "cf_calendar_bin: time %.17g lies outside the table [%.17g, %.17g)", time, edges[0], edges[n_edges - 1]);
    return CF_OK;
}

int cf_attach_climatology(cf_ctx* ctx, cf_climatology* c, int32_t stride, double step_weight, double time_origin, double step_seconds,
                          const double* edges, const int32_t* bin_of_interval, int32_t n_edges) {
    const char* fn = "cf_attach_climatology";
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!c) {
        ctx->attached[cf_ctx::AT_CLIMATOLOGY] = Attachment{};
        return CF_OK;
    }
    if (c->ctx != ctx) return fail(ctx, CF_ERR_INVALID, "%s: the climatology belongs to another context", fn);
    if (stride < 1 || !(step_weight > 0.0) || !std::isfinite(step_weight * stride))
        return fail(ctx, CF_ERR_INVALID, "%s: stride %d (≥ 1), step weight %g (> 0 and finite)", fn, stride, step_weight);
    if (!std::isfinite(time_origin) || !std::isfinite(step_seconds))
        return fail(ctx, CF_ERR_INVALID, "%s: time origin %g and step %g (finite)", fn, time_origin, step_seconds);
    CHECK(check_calendar(ctx, fn, edges, bin_of_interval, n_edges));
    for (int32_t k = 0; k + 1 < n_edges; ++k)
        if (bin_of_interval[k] >= c->n_bins)
            return fail(ctx, CF_ERR_INVALID, "%s: bin_of_interval[%d] = %d, the climatology has %d bins", fn, k, bin_of_interval[k], c->n_bins);
    c->edges.assign(edges, edges + n_edges);
    c->bin_of_interval.assign(bin_of_interval, bin_of_interval + (n_edges - 1));
    ctx->attached[cf_ctx::AT_CLIMATOLOGY] = Attachment{c, StepSchedule{stride, time_origin, step_seconds}, step_weight};
    return CF_OK;
}

}  // extern "C"
