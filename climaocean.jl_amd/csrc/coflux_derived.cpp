// coflux_derived.cpp — cf_average_create_derived (include/coflux.h): checks a term table, numbers its distinct source arrays
// and hands back a cf_average whose collections go to the kernel of coflux_derived.hip (cf_average::collect,
// coflux_average.cpp, chooses the launch).  Nothing is allocated on the device.
#include "coflux_ctx.hpp"

namespace {

bool reads_b(int kind) {
    return kind == CF_TERM_PRODUCT || kind == CF_TERM_KINETIC_ENERGY || kind == CF_TERM_EAST || kind == CF_TERM_NORTH;
}
bool rotates(int kind) { return kind == CF_TERM_EAST || kind == CF_TERM_NORTH; }
// which operand a term reads at [i+1] / [j+1]
bool a_east(int kind, int flags) {
    return kind == CF_TERM_CENTER_X || kind == CF_TERM_CENTER_X_SQUARE || kind == CF_TERM_KINETIC_ENERGY ||
           (rotates(kind) && !(flags & CF_TERM_AT_CENTERS));
}
bool a_north(int kind) { return kind == CF_TERM_CENTER_Y || kind == CF_TERM_CENTER_Y_SQUARE; }
bool b_north(int kind, int flags) { return kind == CF_TERM_KINETIC_ENERGY || (rotates(kind) && !(flags & CF_TERM_AT_CENTERS)); }

}  // namespace

extern "C" int cf_average_create_derived(cf_ctx* ctx, const cf_average_desc* desc, cf_average** out) {
    if (!ctx) return fail(nullptr, CF_ERR_INVALID, "ctx is NULL");
    if (!out || !desc) return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: NULL argument");
    *out = nullptr;
    if (desc->struct_size != (int32_t)sizeof(cf_average_desc))
        return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: struct_size %d (expected %d)", desc->struct_size,
                    (int)sizeof(cf_average_desc));
    if (desc->max_workgroups < 0 || desc->reserved != 0)
        return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: max_workgroups %d (≥ 0), reserved %d (0)", desc->max_workgroups,
                    desc->reserved);
    const int n = desc->n_terms;
    if (n < 1 || n > CF_AVERAGE_MAX_FIELDS || !desc->terms)
        return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: %d terms (1…%d, a host array)", n, CF_AVERAGE_MAX_FIELDS);
    const GridDesc& G = ctx->grid;
    DerivedArgs A{};
    A.n_terms = n;
    A.cos_slot = A.sin_slot = -1;
    A.max_blocks = desc->max_workgroups;
    auto slot = [&](const double* p) {   // the number of a source array, or −1: the table is full
        for (int s = 0; s < A.n_src; ++s)
            if (A.src[s] == p) return s;
        if (A.n_src == CF_DERIVED_MAX_SOURCES) return -1;
        A.src[A.n_src] = p;
        return A.n_src++;
    };
    for (int t = 0; t < n; ++t) {
        const cf_average_term& T = desc->terms[t];
        if (T.kind < CF_TERM_FIELD || T.kind > CF_TERM_NORTH)
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: term %d has the unknown kind %d", t, T.kind);
        if ((T.flags & ~CF_TERM_AT_CENTERS) || (T.flags && !rotates(T.kind)))
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: term %d (kind %d) has the flags 0x%x", t, T.kind, T.flags);
        if (!T.a || !T.mean || (reads_b(T.kind) && !T.b))
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: term %d (kind %d) has a NULL pointer", t, T.kind);
        if (rotates(T.kind) && (!desc->cos_rotation || !desc->sin_rotation))
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: term %d rotates, cos_rotation / sin_rotation is NULL", t);
        if (!std::isfinite(T.scale)) return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: term %d has the scale %g", t, T.scale);
        const bool ae = a_east(T.kind, T.flags), an = a_north(T.kind), bn = b_north(T.kind, T.flags);
        if ((ae && G.hx < 1) || ((an || bn) && G.hy < 1))
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: term %d (kind %d) reads a neighbour, the halo is (%d, %d)", t,
                        T.kind, G.hx, G.hy);
        const int a = slot(T.a), b = reads_b(T.kind) ? slot(T.b) : a;
        if (rotates(T.kind)) {
            A.cos_slot = slot(desc->cos_rotation);
            A.sin_slot = slot(desc->sin_rotation);
        }
        if (a < 0 || b < 0 || (rotates(T.kind) && (A.cos_slot < 0 || A.sin_slot < 0)))
            return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: more than %d distinct source arrays", CF_DERIVED_MAX_SOURCES);
        A.kind[t] = (uint8_t)T.kind;
        A.flags[t] = (uint8_t)T.flags;
        A.a[t] = (uint8_t)a;
        A.b[t] = (uint8_t)b;
        A.scale[t] = T.scale;
        A.mean[t] = T.mean;
        if (ae) A.need_x |= 1u << a;
        if (an) A.need_y |= 1u << a;
        if (bn) A.need_y |= 1u << b;
    }
    auto overlap = [&](const void* p, const void* q) { return fields_overlap(G, p, q); };
    for (int t = 0; t < n; ++t) {
        for (int s = 0; s < A.n_src; ++s)
            if (overlap(A.mean[t], A.src[s]))
                return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: mean %d overlaps a source or rotation array", t);
        for (int u = 0; u < t; ++u)
            if (overlap(A.mean[t], A.mean[u])) return fail(ctx, CF_ERR_INVALID, "cf_average_create_derived: means %d and %d overlap", u, t);
    }
    cf_average* a = new cf_average();
    a->args = A;
    child_adopt(ctx, a);
    *out = a;
    return CF_OK;
}
