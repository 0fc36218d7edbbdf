// Host-visible launchers of the gfx950 kernels (coflux_interp.hip, coflux_solver.hip,
// coflux_solver_libm.hip, coflux_net.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "coflux_device.hpp"

namespace coflux {

// The experiment options of cf_set_option (CF_OPT_INTERP_TILE_CAP, CF_OPT_INTERP_TILE_ROWS, CF_OPT_AO_CHUNK: scheduling only,
// never results) are accepted only in a process started with COFLUX_EXPERIMENTS=1; the variable is read once per process.
inline bool experiments_enabled() {
    static const bool enabled = [] {
        const char* e = std::getenv("COFLUX_EXPERIMENTS");
        return e != nullptr && e[0] == '1';
    }();
    return enabled;
}

struct LoopParams;
struct IceParams;
struct HaloRider;

struct LaunchCfg {
    int solver;              // CF_SOLVER_*
    int interp_cap;          // float2 entries per variable of a wave's LDS-staged JRA55 tile
    int interp_rows;         // CF_OPT_INTERP_TILE_ROWS: rows of 64 cells per wave tile, 1 / 2 / 4 (0 = automatic, by surface size)
    int ao_chunk;            // wet cells per solver workgroup: 256 / 512 / 768 (0 = automatic)
    int cu_count;            // compute units of the device (sizes the automatic chunk)
    const double* d_tables;  // device copy of the solver tables (coflux_tables.cpp)
    const DevParams* d_params;  // device copy of DevParams (the solver stages it in LDS)
    uint8_t* d_trip;            // per-wet-cell trip count of the previous call (scheduling hint) or NULL
    const int* d_chunk_begins;  // cost-balanced chunk table of the solver (coflux_solver.hip), n_chunks + 1 entries
    int n_chunks;
    int chunk_south, chunk_north;  // chunks [0, chunk_south) read the south halo rows, [chunk_north, n_chunks) the north ones (HaloRider)
    const uint32_t* d_wet_pos;  // static wet lists of the chunks, fixed stride (coflux_solver.hip), or NULL
    uint32_t* d_lean_sorted;    // the lean ocean kernel's lists: every chunk's wet cells ordered by last call's trip counts (coflux_solver_lean.hip)
    const int* d_lean_info;     // per chunk: wet cells listed, fingerprint of the wet set (x, y), 0
    int lean_hints;             // 1: the lean ocean kernel re-orders its lists by trip count at the end of every call
    int certified;              // CF_OPT_SOLVER_PATH: 1 = the certified reduced-iteration solve wherever it applies (lean_certified_applies)
    int latency_layout;         // CF_OPT_LATENCY_LAYOUT: 0 never, 1 automatic (COARE profile on chunk plans of at most two workgroups per CU), 2 always
    int keep_land;              // CF_OPT_LAND_ZEROS, per launch: 1 = the ocean solve leaves the land of a chunk whose list is valid as it is.  Never
                                // set in a context's own copy: cf_update_state sets it in the copy it hands to the launches of a marked step
};

// the exact path's kernels for one or two waves per SIMD (coflux_solver_slab.hip) carry this launch
bool lean_line_applies(const LaunchCfg& L, const LoopParams& C, bool coare);

// CF_SOLVER_PATH_CERTIFIED runs in the lean ocean kernel under the convergence stop rule with index-ordered lists; everywhere
// else the exact path runs.
bool lean_certified_applies(const LaunchCfg& L, const LoopParams& C);

hipError_t launch_interpolate(hipStream_t st, const LaunchCfg& L, const GridDesc& G, const cf_atmos_source* s,
                              const cf_interp_weights* w, const cf_exchange_fields* e);
hipError_t launch_ao_fluxes(hipStream_t st, const LaunchCfg& L, const DevParams& P, const LoopParams& C,
                            const GridDesc& G, const cf_ocean_surface* o, const cf_exchange_fields* e,
                            const cf_interface_fluxes* f, const cf_sea_ice_fields* ice = nullptr,
                            const cf_net_ocean_fluxes* net = nullptr, const double* land = nullptr);
hipError_t launch_net_stress(hipStream_t st, const DevParams& P, const GridDesc& G, const cf_ocean_surface* o,
                             const cf_interface_fluxes* f, const cf_sea_ice_fields* ice, const cf_net_ocean_fluxes* n,
                             bool keep_land = false);   // keep_land: land cells are neither read nor written (CF_OPT_LAND_ZEROS)
hipError_t build_wet_lists(hipStream_t st, const DevParams* d_params, const GridDesc& G, const void* mask, int nchunks,
                           const int* d_begins, uint32_t* d_wet_pos, uint8_t* d_trip, int* d_scratch, int* overflow_out);
hipError_t build_lean_lists(hipStream_t st, int nchunks, const uint32_t* d_wet_pos, const int* d_begins, uint32_t* d_sorted, int* d_info);
hipError_t launch_ly_fluxes_with_tail(hipStream_t st, const LaunchCfg& L, const DevParams& P, const LoopParams& C, const GridDesc& G,
                                      const cf_ocean_surface* o, const cf_exchange_fields* e, const cf_interface_fluxes* f,
                                      const cf_sea_ice_fields* ice, const cf_net_ocean_fluxes* net, const double* land,
                                      const cf_atmos_source* next_src, const cf_interp_weights* w, const cf_exchange_fields* next_out,
                                      int tail_rows, int tail_blocks);
hipError_t launch_ao_fluxes_lean(hipStream_t st, const LaunchCfg& L, const DevParams& P, const LoopParams& C, const GridDesc& G,
                                 const cf_ocean_surface* o, const cf_exchange_fields* e, const cf_interface_fluxes* f,
                                 const cf_sea_ice_fields* ice = nullptr, const cf_net_ocean_fluxes* net = nullptr, const double* land = nullptr,
                                 const cf_atmos_source* next_src = nullptr, const cf_interp_weights* w = nullptr,
                                 const cf_exchange_fields* next_out = nullptr, int tail_rows = 0, int tail_blocks = 0,
                                 const HaloRider* halo = nullptr);
// the step's peer-direct halo rows can ride in the ocean solver's launch (exact path of the lean kernel, with tail workgroups)
bool lean_halo_rides(const LaunchCfg& L, const LoopParams& C);
size_t wet_list_capacity(int ncells);
int wet_list_stride();
hipError_t launch_ao_fluxes_libm(hipStream_t st, const DevParams& P, const GridDesc& G, const cf_ocean_surface* o,
                                 const cf_exchange_fields* e, const cf_interface_fluxes* f);
hipError_t launch_net_fluxes(hipStream_t st, const DevParams& P, const GridDesc& G, const cf_ocean_surface* o,
                             const cf_exchange_fields* e, const cf_interface_fluxes* f, const cf_sea_ice_fields* ice,
                             const cf_interp_weights* w, const cf_net_ocean_fluxes* n, const double* land = nullptr);
hipError_t launch_interpolate_land(hipStream_t st, const GridDesc& G, const cf_land_source* s, const cf_interp_weights* w, double* out);
hipError_t launch_salinity_restoring(hipStream_t st, const DevParams& P, const GridDesc& G, const void* mask, double vp,
                                     const double* target, const double* S, double* out);
void interpolate_grid(const LaunchCfg& L, const GridDesc& G, int* rows_out, int* blocks_out);
hipError_t launch_interpolate_and_stress(hipStream_t st, const LaunchCfg& L, const DevParams& P, const GridDesc& G,
                                         const cf_atmos_source* s, const cf_interp_weights* w, const cf_exchange_fields* e,
                                         const cf_ocean_surface* o, const cf_interface_fluxes* f, const cf_sea_ice_fields* ice,
                                         const cf_net_ocean_fluxes* n);
hipError_t launch_interpolate_background(hipStream_t st, const GridDesc& G, const cf_atmos_source* s,
                                         const cf_interp_weights* w, const cf_exchange_fields* e);
// The ocean solve of this step as workgroups of ANOTHER launch (the sea-ice interface solve's: ice_ocean_kernel): the round-3
// ocean kernel's argument block, filled by make_ocean_rider exactly as launch_ao_fluxes_lean fills it (fused net fluxes).
struct OceanRider {
    alignas(16) unsigned char args[1536];
    int n_chunks = 0;
    bool coare = false, valid = false;
};
hipError_t make_ocean_rider(const LaunchCfg& L, const DevParams& P, const LoopParams& C, const GridDesc& G, const cf_ocean_surface* o,
                            const cf_exchange_fields* e, const cf_interface_fluxes* f, const cf_sea_ice_fields* ice,
                            const cf_net_ocean_fluxes* net, const double* land, OceanRider* out);
// what may ride in the tail workgroups of the sea-ice interface launch (launch_ai_fluxes)
struct AiTail {
    const OceanRider* ocean = nullptr;              // this step's ocean solve (then the stresses cannot ride: they need its ρτ)
    const cf_atmos_source* next_src = nullptr;      // the next step's interpolation …
    const cf_interp_weights* w = nullptr;
    const cf_exchange_fields* next_out = nullptr;
    int interp_rows = 0, interp_blocks = 0;
    const DevParams* d_ocean_params = nullptr;      // … and this step's face stresses (compute_net_ocean_fluxes!)
    const cf_ocean_surface* stress_ocean = nullptr;
    const cf_interface_fluxes* stress_fluxes = nullptr;
    const cf_sea_ice_fields* stress_ice = nullptr;
    const cf_net_ocean_fluxes* stress_net = nullptr;
};
hipError_t launch_ai_fluxes(hipStream_t st, const LaunchCfg& L, const DevParams& P, const LoopParams& C, const IceParams& I,
                            const GridDesc& G, const cf_sea_ice_state* ice, const cf_ocean_surface* o,
                            const cf_exchange_fields* e, const cf_interface_fluxes* f, const double* d_tables,
                            const DevParams* d_params, uint8_t* d_trip, const AiTail* tail = nullptr, const NetIceOut* net_ice = nullptr);
// build_chunk_table / cf_debug_chunk_plan: `wet_per_chunk` = AO_PLAN_TAIL asks for the automatic plan of a launch that carries
// tail workgroups (CF_OPT_MERGED_PREFETCH = 2)
constexpr int AO_PLAN_TAIL = -2;
hipError_t build_chunk_table(hipStream_t st, const DevParams* d_params, const GridDesc& G, const void* mask, int cu_count,
                             int wet_per_chunk, int* d_sums, int* d_begins, int* d_meta, int* wet_per_chunk_out,
                             int* nchunks_out);
int chunk_table_capacity(int ncells);
int chunk_sums_capacity(int ncells);
hipError_t launch_net_sea_ice_fluxes(hipStream_t st, const DevParams& P, const GridDesc& G, const void* mask,
                                     const cf_sea_ice_state* ice, double albedo, double emissivity, double eps_sigma,
                                     double T_offset, const cf_exchange_fields* e, const cf_interface_fluxes* f,
                                     const double* frazil, const double* interface_heat, const cf_net_sea_ice_fluxes* out);
hipError_t launch_sea_ice_albedo(hipStream_t st, const cf_sea_ice_albedo_params& A, const GridDesc& G, const double* hi,
                                 const double* hs, const double* Ts, double* out);
hipError_t launch_sea_ice_ocean_fluxes(hipStream_t st, const DevParams& P, const cf_ice_ocean_params& Q, const GridDesc& G,
                                       const cf_ocean_surface* o, const double* conc, const double* tx, const double* ty,
                                       const cf_ice_ocean_fluxes* out);
// cf_prepare_coupled_step (coflux_net.hip): the three jobs of the one launch; a job whose output is null is absent
struct PrepareArgs {
    const float* friver;      // land freshwater → land_out on W
    const float* licalvf;
    int32_t ns_x, ns_y, level1, level2;
    double tf;
    double* land_out;
    cf_ice_ocean_params Q;    // ice–ocean exchange and frazil → Qio, Jsio[, Qfr, ustar] on I
    const double* T;
    const double* conc;
    const double* tx;
    const double* ty;
    double* Qio;
    double* Jsio;
    double* Qfr;
    double* ustar;
    double vp;                // restoring buffer → restoring on I
    const double* target;     // S★, or level1 of a staged dataset …
    const double* target2;    // … whose level2 and fraction these are (fraction 0.0: target alone is read)
    double fraction;
    double* restoring;
    const double* S;          // read once for both interior jobs, like the mask
    const void* mask;
};
hipError_t launch_prepare_coupled_step(hipStream_t st, const DevParams& P, const GridDesc& G, const cf_interp_weights* w,
                                       const PrepareArgs& A);
// cf_dataset_* (coflux_dataset.hip): a plane of the dataset's grid converted to f64, inpainted by `sweeps` nearest-neighbour sweeps
// in one launch (1: one thread per cell; 2 … INPAINT_MAX_SWEEPS: overlapped LDS tiles — same bits), its remaining NaNs given the
// fill value, interpolated onto W of an ocean-grid array; S★ from two levels on W; the restoring buffer with S★ formed per cell.
// max_blocks: cf_dataset_desc.max_workgroups (0: the kernels' own cap)
constexpr int INPAINT_MAX_SWEEPS = 8;
hipError_t launch_dataset_convert(hipStream_t st, const float* in, double* out, size_t n, int max_blocks);
hipError_t launch_dataset_default(hipStream_t st, double* plane, size_t n, double fill, int max_blocks);
hipError_t launch_dataset_inpaint(hipStream_t st, const double* p, double* q, int ns_x, int ns_y, bool periodic, int sweeps, int max_blocks);
hipError_t launch_dataset_regrid(hipStream_t st, const double* plane, int ns_x, int ns_y, const cf_interp_weights* w, const GridDesc& G,
                                 double* out, int max_blocks);
hipError_t launch_dataset_evaluate(hipStream_t st, const double* level1, const double* level2, double fraction, const GridDesc& G, double* out,
                                   int max_blocks);
hipError_t launch_dataset_restoring(hipStream_t st, const DevParams& P, const GridDesc& G, const void* mask, double vp, const double* level1,
                                    const double* level2, double fraction, const double* S, double* out);
constexpr int SALINITY_PARTIAL_BLOCKS = 512;
hipError_t launch_salinity_partial_sums(hipStream_t st, const DevParams& P, const GridDesc& G, const double* flux,
                                        const double* additional, const double* area, const void* mask, double* partial,
                                        int nblocks, double* sums);
hipError_t launch_salinity_subtract(hipStream_t st, const GridDesc& G, double* flux, const double* sums, double* mean_out);
hipError_t launch_debug_eval(hipStream_t st, const LaunchCfg& L, int fn, int n, const double* x, double* y);
// cf_normalize_salinity_flux_exact (coflux_exact_sum.hip): the wet interior's Σ fl(fl(flux + additional) · area) and Σ area into the
// accumulator pair (2 · XS_WORDS words, integer atomics), then one workgroup that joins the reduction world's pairs, rounds once
// into sums[0 … 1] and zeroes the pair; `nonfinite` (or NULL): the NaN / +Inf / −Inf term counts of the first sum
constexpr int EXACT_SUM_BLOCKS = 512;
struct ReduceWorld;
hipError_t launch_exact_sums(hipStream_t st, const DevParams& P, const GridDesc& G, const double* flux, const double* additional,
                             const double* area, const void* mask, unsigned long long* accumulator);
hipError_t launch_exact_finish(hipStream_t st, unsigned long long* accumulator, const ReduceWorld& W, unsigned long long seq, int* d_status,
                               double* sums, unsigned long long* nonfinite);
struct PeerMailbox;
struct PeerFields;
struct FoldFields;
hipError_t launch_peer_halo(hipStream_t st, const PeerMailbox& M, const PeerFields& F, const GridDesc& G, int rows,
                            unsigned long long seq, int* d_status);
// the exchange launch of the rank that owns the tripolar fold: workgroup 0 exchanges with the south neighbour, 1 + F.n · rows
// workgroups fold the north halo rows of the exchange's own fields (coflux_halo.hip: peer_halo_fold_kernel)
hipError_t launch_peer_halo_fold(hipStream_t st, const PeerMailbox& M, const FoldFields& F, const GridDesc& G, int rows,
                                 unsigned long long seq, int* d_status);
hipError_t launch_fold_north(hipStream_t st, const FoldFields& F, const GridDesc& G, int rows);
// the two launches of a tile world's exchange (coflux_halo.hip): the x-halo columns, then the rows full width — on the top row of
// a tripolar world with px > 1 the north side sends the fold partner its rows mirrored and signed (fold.cols > 0)
struct TileMailbox;
struct TileFold;
hipError_t launch_tile_halo_x(hipStream_t st, const TileMailbox& M, const PeerFields& F, const GridDesc& G, int wcols, int ecols,
                              unsigned long long seq, int* d_status);
hipError_t launch_tile_halo_y(hipStream_t st, const TileMailbox& M, const FoldFields& F, const GridDesc& G, int rows, const TileFold& fold,
                              unsigned long long seq, int* d_status);
hipError_t launch_copy(hipStream_t st, void* dst, const void* src, size_t bytes);
// cf_average_collect (coflux_average.hip): every field's interior mean m ← f (store) or m ← (m · c_prev) + (f · c_new), one launch
struct AverageFields {
    const double* src[CF_AVERAGE_MAX_FIELDS];
    double* mean[CF_AVERAGE_MAX_FIELDS];
};
hipError_t launch_average(hipStream_t st, const AverageFields& F, int nfields, const GridDesc& G, bool store, double c_prev,
                          double c_new);
// cf_climatology_collect (coflux_climatology.hip): per field the source enters the total's running mean (total[f] NULL: this
// field keeps none) and ONE bin's (bin[f] already points at that bin's parent array), each stored or blended with its own
// coefficients, one launch; max_blocks: cf_climatology_desc.max_workgroups (0: the kernel's own cap)
struct ClimatologyFields {
    const double* src[CF_CLIMATOLOGY_MAX_FIELDS];
    double* total[CF_CLIMATOLOGY_MAX_FIELDS];
    double* bin[CF_CLIMATOLOGY_MAX_FIELDS];
};
struct ClimatologyBlend {
    double total_prev, total_new, bin_prev, bin_new;
};
hipError_t launch_climatology(hipStream_t st, const ClimatologyFields& F, int nfields, const GridDesc& G, bool store_total,
                              bool store_bin, const ClimatologyBlend& C, int max_blocks);
// cf_climatology_extremes (coflux_climatology.hip): per interior cell Julia's min / max over the n listed bins of one field's
// block, in list order (the host lists the non-empty bins ascending); any output may be NULL
struct ClimatologyBinList {
    int32_t n;
    uint8_t bin[CF_CLIMATOLOGY_MAX_BINS];
};
hipError_t launch_climatology_extremes(hipStream_t st, const double* bins, size_t parent, const ClimatologyBinList& L, const GridDesc& G,
                                       double* d_min, double* d_max, int32_t* d_argmin, int32_t* d_argmax, int max_blocks);
// cf_average_collect of a derived averager (coflux_derived.hip): the distinct source arrays of the terms (rotation arrays
// included) are numbered by the host; term t reads slots a[t] / b[t]; bit s of need_x / need_y: some term reads slot s at
// [i+1] / [j+1]; cos_slot / sin_slot: −1 without an EAST / NORTH term
struct DerivedArgs {
    const double* src[CF_DERIVED_MAX_SOURCES];
    double* mean[CF_AVERAGE_MAX_FIELDS];
    double scale[CF_AVERAGE_MAX_FIELDS];
    uint8_t kind[CF_AVERAGE_MAX_FIELDS], flags[CF_AVERAGE_MAX_FIELDS], a[CF_AVERAGE_MAX_FIELDS], b[CF_AVERAGE_MAX_FIELDS];
    int32_t n_src, n_terms;
    uint32_t need_x, need_y;
    int32_t cos_slot, sin_slot;
    int32_t max_blocks, pad;   // cf_average_desc.max_workgroups (0: the kernel's own cap); the launcher reads it, the kernel does not
};
hipError_t launch_derived_average(hipStream_t st, const DerivedArgs& A, const GridDesc& G, bool store, double c_prev, double c_new);
// cf_average_collect of a budget averager (coflux_budget.hip): the inputs of compute_net_ocean_fluxes!'s cell in a fixed
// numbering; in[s] is NULL where no requested kind reads input s or the caller has none (the cell then sees 0.0), so the
// pointer table is the load mask.  term t averages kind[t] (CF_BUDGET_*) times scale[t] into mean[t].
enum BudgetInput {
    BUDGET_IN_S, BUDGET_IN_TS, BUDGET_IN_MP, BUDGET_IN_QS, BUDGET_IN_QL, BUDGET_IN_QC, BUDGET_IN_QV, BUDGET_IN_MV,
    BUDGET_IN_ICE, BUDGET_IN_QIO, BUDGET_IN_JSIO, BUDGET_IN_LAND, BUDGET_IN_FRAZIL, BUDGET_INPUTS
};
struct BudgetArgs {
    const double* in[BUDGET_INPUTS];
    const void* mask;
    const double* latitude;    // read only with reads_albedo and CF_ALBEDO_LATITUDE_DEPENDENT
    double* mean[CF_AVERAGE_MAX_FIELDS];
    double scale[CF_AVERAGE_MAX_FIELDS];
    uint8_t kind[CF_AVERAGE_MAX_FIELDS];
    int32_t n_terms, separable;
    int32_t reads_albedo;      // some requested kind reads Qts
    int32_t max_blocks;        // cf_budget_desc.max_workgroups (0: the kernel's own cap); the launcher reads it, the kernel does not
};
hipError_t launch_budget_average(hipStream_t st, const DevParams& P, const BudgetArgs& A, const GridDesc& G, bool store, double c_prev,
                                 double c_new);
// cf_integrals_collect (coflux_integrals.hip): one record of area-weighted, masked, regional integrals; the distinct `a` / `b`
// arrays of the entries are numbered (field slots) by the host
// interior cells per tile of the summation order (a constant of the record's bits; A/B builds may set it: 512 · 1 / 2 / 4)
#ifndef COFLUX_INTEGRALS_TILE
#define COFLUX_INTEGRALS_TILE 1024
#endif
constexpr int INTEGRALS_TILE = COFLUX_INTEGRALS_TILE;
struct IntegralArgs {
    const double* field[CF_INTEGRALS_MAX_FIELDS];
    const double* area;
    const void* mask;
    const uint8_t* region;
    double* partial;                  // [tiles][bucket] per-tile sums
    const uint32_t* entry;            // device, [CF_INTEGRALS_MAX_ENTRIES]: kind | slot of a << 8 | slot of b << 16 | region mask << 24 (0: unused)
    const double* threshold;          // device, [CF_INTEGRALS_MAX_ENTRIES]
    double z_surface;
    int32_t mask_kind, n_fields, n_entries;
};
int integrals_bucket(int n_entries);          // the compile-time entry count an integrator of n_entries runs with: 8 / 16 / 32
unsigned integrals_tiles(const GridDesc& G);
// the tile kernel on min(tiles, max_blocks) workgroups (0: one per tile), then the combination into record[0 … n_entries)
hipError_t launch_integrals(hipStream_t st, const IntegralArgs& K, const GridDesc& G, double* record, int max_blocks);

// cf_monitor_collect (coflux_monitor.hip): extrema, non-finite counts and the state hash of up to CF_MONITOR_MAX_ENTRIES fields.
// Every reduction is exact (integer keys, integer sums, a wrapping sum), so the partition of the cells is free: `slices`
// slices of the interior per entry, one partial per (entry, slice), combined by a single-workgroup launch.
// (the argument bundle and the partials' layout: coflux_kernel_types.hpp)
struct MonitorArgs;
int monitor_slices(const GridDesc& G, int n_entries);   // the library's partition (a function of the surface and the entry count)
// the pass on min(n_entries · slices, max_blocks) workgroups (0: one per (entry, slice)), then the combination into
// record[0 … n_entries) and the status (`record_index`: the record's number since the last reset)
hipError_t launch_monitor(hipStream_t st, const MonitorArgs& K, const GridDesc& G, cf_monitor_value* record, int64_t record_index,
                          int max_blocks);

// cf_regrid_apply (coflux_regrid.hip): a fixed sparse surface operator on up to CF_REGRID_MAX_FIELDS fields in one pass.
// The host (coflux_regrid.cpp) turns the CSR operator into the tables below at create; all of them are device arrays.
constexpr int REGRID_SHORT = 64;        // rows of at most this many entries: one 16-lane group each, four rows per wave
constexpr int REGRID_SEGMENT = 256;     // longer rows: segments of this many consecutive entries, one wave each
constexpr int REGRID_PARTIAL = CF_REGRID_MAX_FIELDS + 1;   // doubles per segment partial: N of every field, then D
constexpr uint32_t REGRID_NONE = 0xffffffffu;
struct RegridSegment {                  // one wave's work on a long row
    uint32_t row, start, count, slot;   // entries [start, start + count); slot REGRID_NONE: the row's only segment, finished here
};
struct RegridLongRow {                  // a row of several segments, finished by the combination launch
    uint32_t row, first_slot, n_segments, reserved;
};
struct RegridTables {
    const uint32_t* offset;             // [nnz] halo-layout element offset of the entry's source cell
    const double* weight;               // [nnz]
    const uint32_t* row_start;          // [n_rows + 1]
    const uint32_t* short_rows;         // [4 · n_short_units] row index or REGRID_NONE (padding of the last unit)
    const RegridSegment* segments;      // [n_segments]
    const RegridLongRow* long_rows;     // [n_long_rows]
    double* partial;                    // [slots][REGRID_PARTIAL]
    const void* mask;
    double z_surface;
    uint32_t n_short_units, n_segments, n_long_rows;
    int32_t mask_kind, mode;
};
struct RegridFields {
    const double* src[CF_REGRID_MAX_FIELDS];
    double* dst[CF_REGRID_MAX_FIELDS];
    double* coverage;
    int32_t n_fields;
};
// the row kernel (instantiated for 1 / 4 / 8 / 16 ≥ n_fields fields) on min(ceil(units / 4), max_blocks) workgroups (0: 8 per
// compute unit), then the combination of the rows of several segments
hipError_t launch_regrid(hipStream_t st, const RegridTables& T, const RegridFields& F, int max_blocks, int cu_count);

}  // namespace coflux
