// coflux_ctx.hpp — the context object behind the C ABI and the error plumbing shared by its translation units (every .cpp
// of this directory but coflux_tables.cpp).  Internal: nothing here crosses the ABI.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/coflux.h"
#include "coflux_checkpoint.hpp"
#include "coflux_checkpoint_image.hpp"
#include "coflux_collect.hpp"
#include "coflux_dataset_rules.hpp"
#include "coflux_fast.hpp"
#include "coflux_kernel_types.hpp"
#include "coflux_kernels.h"
#include "coflux_owned.hpp"
#include "coflux_request_ahead.hpp"
#include "coflux_tables.h"

using namespace coflux;

// CF_OPT_LAND_ZEROS of a fresh context: 1 = automatic; an A/B build sets 0 (tools/make_variant.sh everystep -DCF_LAND_ZEROS_DEFAULT=0)
#ifndef CF_LAND_ZEROS_DEFAULT
#define CF_LAND_ZEROS_DEFAULT 1
#endif
static_assert(CF_LAND_ZEROS_DEFAULT == 0 || CF_LAND_ZEROS_DEFAULT == 1, "the experiment value is not a default");

struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommCuDevice)(const ncclComm_t, int*) = nullptr;
};

// What the step loops know of an attached handle (cf_ctx::attached): the handle and when it is due; a collection of an averager
// or the climatology weighs stride · step_weight.  Steps are numbered globally (StepSchedule, coflux_collect.hpp).
struct cf_child;
struct Attachment {
    cf_child* handle = nullptr;
    StepSchedule when;
    double step_weight = 0.0;
    bool collects(int64_t step) const { return handle && when.due(step); }
};

// One section of a checkpoint image as its handle lays it out (plan_section): n_entries, count and bytes of the directory entry,
// how many of the payload's bytes the device holds, the runs of them (the payload starts at image offset `offset`) and the
// host-kept bytes that follow them
struct SectionPlan {
    uint32_t section;
    uint64_t offset;
    cfck::Entry& entry;
    uint64_t& device_bytes;
    std::vector<unsigned char>& tail;
    std::vector<CheckpointSegment>& segments;
};

// What every handle made on a context is (averagers, climatologies, integrators, monitors, regridders, snapshot windows,
// checkpoints): it may outlive the context.  cf_destroy orphans every child (orphan_children); calls that need the context then
// fail through live(), destroy still works.  The step loops and the checkpoint ask the handle itself; the defaults are those of
// a handle that is never attached or registered.
struct cf_child {
    cf_ctx* ctx = nullptr;   // NULL once the context is destroyed
    int device = 0;
    virtual ~cf_child() = default;
    // attached as `at`: CF_ERR_INVALID (the refusal of `fn`) unless the steps [first_step, first_step + nsteps) may run — asked
    // before anything is launched — and the collection of a due step
    virtual int admit(const Attachment& /*at*/, const char* /*fn*/, int64_t /*first_step*/, int /*nsteps*/) const { return CF_OK; }
    virtual int collect_step(const Attachment& /*at*/, int64_t /*step*/) { return CF_OK; }
    // registered with a checkpoint (coflux_checkpoint.cpp): the section's kind (cfck::KIND_*); its layout — as the handle stands
    // now or, with `image_count`, as an image with so many records states it (whose host-kept bytes the caller takes from the
    // image); the payload bytes it can grow to; CF_ERR_INVALID unless an image's entry fits the handle; the host-kept bytes back
    virtual uint32_t section_kind() const { return cfck::KINDS; }
    virtual void plan_section(const SectionPlan&, const int64_t* /*image_count*/) const {}
    virtual uint64_t section_room() const { return 0; }
    virtual int check_entry(const cfck::Entry&, const char* /*fn*/) const { return CF_OK; }
    virtual void load_tail(const std::vector<unsigned char>&, int64_t /*count*/) {}
};

// Ownership: every stream, event, device buffer and IPC mapping below is a cf:: owner (coflux_owned.hpp) and releases itself
// with the context; LaunchCfg, PeerMailbox and the kernels' arguments carry raw pointers filled from get().  Resources that
// only make sense together sit in one struct, built aside and moved in only when all of it was created.
struct cf_ctx {
    int device = 0;
    GridDesc grid{};
    cf_flux_params params{};
    DevParams dev{};
    cf::Stream own_stream;
    hipStream_t stream = nullptr;
    LoopParams fast{};
    cf::DeviceBuffer<DevParams> d_params;
    LaunchCfg launch = [] {
        LaunchCfg L{};
        L.solver = CF_SOLVER_TABLES;
        L.interp_cap = 128;
        L.cu_count = 256;
        return L;
    }();
    struct WetLists {                          // regrown as a unit by ensure_chunk_table
        cf::DeviceBuffer<uint8_t> d_trip;          // trip count of the previous call per wet-list entry
        cf::DeviceBuffer<uint32_t> d_wet_pos;      // static wet lists of the solver's chunks
        cf::DeviceBuffer<uint32_t> d_lean_sorted;  // the lean ocean kernel's sorted lists (same capacity as d_wet_pos)
        cf::DeviceBuffer<int> d_lean_info;         // per chunk: listed wet cells + fingerprint (4 ints)
        cf::DeviceBuffer<uint8_t> d_trip_ice;      // trip counts of the sea-ice interface solve per wet-list entry
        size_t entries = 0;                        // entries allocated in d_wet_pos / d_trip / d_trip_ice
    } wet;
    bool trip_hints = true;
    bool lean_hints = false;         // the lean ocean kernel sorts its lists by trip count only when CF_OPT_TRIP_HINTS = 1
    int merged_prefetch = 0;         // CF_OPT_MERGED_PREFETCH: a requested next-step interpolation rides in the face-stress launch
    double certified_budget = 8e-7;  // CF_OPT_CERTIFIED_BUDGET
    int fused_net = 2;               // cf_update_state: net fluxes in the solver's epilogue + a stress kernel: 0 never, 1 when possible, 2 with the lean ocean kernel
    // cost-balanced chunk table of the solver, rebuilt when the wet mask (pointer / kind / surface z) changes
    cf::DeviceBuffer<int> d_chunk_sums, d_chunk_begins, d_chunk_meta;
    const void* chunk_mask = nullptr;
    int chunk_mask_kind = -1;
    double chunk_z_surface = 0.0;
    int chunk_wet = 0;      // wet cells per chunk actually used
    bool chunk_valid = false;
    cf::DeviceBuffer<double> d_reduce;  // [2·SALINITY_PARTIAL_BLOCKS partial sums][2 totals]
    // atmosphere–sea-ice formulation (cf_set_sea_ice_formulation)
    bool ice_ready = false;
    cf_flux_params ice_params{};
    cf_sea_ice_params ice_props{};
    DevParams ice_dev{};
    LoopParams ice_loop{};
    IceParams ice_kernel{};
    bool ice_orbit_shortcut = true;  // CF_OPT_ICE_ORBIT_SHORTCUT
    bool ice_free_zero = false;      // CF_OPT_ICE_FREE_CELLS = CF_ICE_FREE_ZERO
    const double* d_land_freshwater = nullptr;   // cf_set_land_freshwater (borrowed)
    bool ice_albedo_ccsm3 = false;   // cf_set_sea_ice_albedo: SeaIceAlbedo(hi, hs, Ts) wherever no albedo field is given
    cf_sea_ice_albedo_params ice_albedo{};
    cf::DeviceBuffer<double> d_ice_albedo;  // the albedo field of the current step (computed by the library)
    cf::DeviceBuffer<double> d_ice_tables;
    cf::DeviceBuffer<DevParams> d_ice_params;
    // halo rows travel on their own stream so that they overlap the interpolation kernel, which
    // does not read the ocean state; consumers of the ocean fields wait on ev_comm_done
    struct CommLane {
        cf::Stream stream;
        cf::Event ev_main_idle, ev_comm_done;
    } comm_lane;
    bool comm_pending = false;
    cf::DeviceBuffer<double> d_tables;
    int tables_kind = -1;
    std::string error;
    std::mutex error_mutex;  // cf_window_wait_slot may fail on a reader thread while the stepping thread reads the text
    // auxiliary stream: the next step's interpolation runs here while the current step's solver runs on `stream`
    // (cf_prefetch_atmosphere_state).  The context owns the HIP objects; who is on the lane, who waits to get there and every
    // counter of cf_debug_prefetch_stats are `ahead`'s (coflux_request_ahead.hpp), whose record k owns done[k]
    struct AuxLane {
        cf::Stream stream;
        cf::Event ev_gate;   // recorded on `stream` at the point after which a requested set is free to be overwritten
        cf::Event done[2];
    } aux;
    AheadLedger ahead;
    // peer-direct halo rows (coflux_halo.hip)
    PeerMailbox peer{};                                  // raw views of the three below
    cf::DeviceBuffer<char> peer_mine;                    // this context's mailbox (fine-grained)
    cf::IpcMapping peer_south_map, peer_north_map;       // a neighbour's, where it was opened through HIP IPC
    int peer_max_fields = 0, peer_max_rows = 0;
    bool peer_connected = false;
    unsigned long long peer_seq = 0;
    cf::DeviceBuffer<int> d_peer_status;
    // the tile world (cf_peer_tile_*; coflux_tiles.cpp): a context is slab-connected (above) or tile-connected, never both
    struct TileWorld {
        TileMailbox M{};                                 // raw views of `mine` and `maps`
        cf::DeviceBuffer<char> mine;                     // this context's tile mailbox (fine-grained)
        cf::IpcMapping maps[TILE_MAX_RANKS];             // the other ranks' this rank exchanges with, opened once each, by rank
        TileNote note{};                                 // what `mine` was exported for
        TilePlace place{};
        bool connected = false, tripolar = false;
        unsigned long long seq = 0, column_launches = 0, folds_sent = 0;   // cf_peer_tile_stats
    } tile;
    // cf_debug_fold_counts: fold_north_kernel launches, and exchange launches whose north side was the fold (peer_halo_fold_kernel)
    long long fold_launch_count = 0, fold_exchange_count = 0;
    // the exact sums of cf_normalize_salinity_flux_exact (coflux_exact_sum.hip) and their reduction world (cf_peer_reduce_*)
    cf::DeviceBuffer<unsigned long long> d_exact;        // [2 · XS_WORDS: the accumulator pair][2 doubles: the sums][3: non-finite counts]
    ReduceWorld reduce{nullptr, nullptr, 0, 1};          // raw views of the three below
    cf::DeviceBuffer<char> reduce_mine;                  // this context's reduce mailbox (fine-grained)
    cf::IpcMapping reduce_maps[REDUCE_MAX_RANKS];        // the other ranks', where they were opened through HIP IPC
    cf::DeviceBuffer<char*> d_reduce_peers;              // device table of the REDUCE_MAX_RANKS mailboxes
    bool reduce_connected = false;
    unsigned long long reduce_seq = 0;                   // reductions issued over the world (every rank counts the same)
    // the peer-direct exchange as riders of the solver launch (CF_OPT_HALO_IN_SOLVER_LAUNCH; coflux_lean_kernel.hpp, HALO)
    int halo_in_launch = 0;
    unsigned long long halo_in_launch_count = 0;            // exchanges that rode in a solver launch (cf_peer_halo_stats)
    cf::DeviceBuffer<unsigned long long> d_halo_counters;   // [0,1] fields sent south / north, [2,3] fields received from there
    unsigned long long halo_expect_sent[2] = {0, 0}, halo_expect_done[2] = {0, 0};
    struct HaloRequest {                                    // cf_time_steps asked for this step's rows: the next solver launch carries
        bool valid = false;                                 // them, or cf_update_state issues the stand-alone kernel in front of it
        PeerFields F{};
        int rows = 0;
    } halo_request;
    // CF_OPT_LAND_ZEROS: which launches write zero_interface_state into the land cells.  cf_time_steps opens `step_loop` for the
    // length of one call (LandZeroScope: closed on every way out, so that a failed call cannot leave it open for a later
    // cf_update_state of the host); cf_update_state marks a step "land kept" only inside an open loop whose previous step went the
    // way `last_way` says
    int land_zeros = CF_LAND_ZEROS_DEFAULT;
    struct StepLoop {
        bool open = false;
        unsigned last_way = 0;     // 0: no step of this call yet; else 1 | fused << 1 | kernel family << 2 of the previous step's solver launch
        int zero_launches = 0;     // solver launches of the last call that wrote the land zeros (cf_debug_land_zero_launches)
    } step_loop;
    // RCCL
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    // per-kernel event recorder (cf_profile_enable): 4 events per recorded update_state
    std::vector<cf::Event> prof_events;
    int prof_capacity = 0, prof_count = 0;
    // every averager, integrator, monitor, regridder and window made on this context (cf_destroy orphans them)
    std::vector<cf_child*> children;
    // the checkpoint handles among them: cf_sync reports a restore whose device-side hashes do not match (coflux_checkpoint.cpp)
    std::vector<struct cf_checkpoint*> checkpoints;
    // what the step loops collect behind every step, in this order: the time averages in slot order (cf_attach_average_slot; slot 0
    // is cf_attach_average's), the calendar-binned means (cf_attach_climatology), then the series recorders: surface integrals
    // (cf_attach_integrals) and the monitor (cf_attach_monitor)
    enum { AT_CLIMATOLOGY = CF_ATTACHED_AVERAGES_MAX, AT_INTEGRALS, AT_MONITOR, AT_COUNT };
    Attachment attached[AT_COUNT];
    // the dataset the coupled loop's restoring job follows (cf_attach_restoring_dataset): not collected — step s restores toward
    // S★ at when.time_origin + s · when.step_seconds
    Attachment restoring_dataset;
};

// One cf_time_steps call's step loop, as CF_OPT_LAND_ZEROS sees it: open for exactly the scope's lifetime
struct LandZeroScope {
    cf_ctx* ctx;
    explicit LandZeroScope(cf_ctx* c) : ctx(c) {
        ctx->step_loop = cf_ctx::StepLoop{};
        ctx->step_loop.open = true;
    }
    ~LandZeroScope() {
        ctx->step_loop.open = false;   // (zero_launches stays: cf_debug_land_zero_launches reads the last call's)
        ctx->step_loop.last_way = 0;
    }
    LandZeroScope(const LandZeroScope&) = delete;
    LandZeroScope& operator=(const LandZeroScope&) = delete;
};

// One cf_time_steps / cf_time_steps_coupled call as CF_OPT_HALO_IN_SOLVER_LAUNCH sees it: a step's halo request is consumed by the
// cf_update_state of its own iteration or dropped here — a call that fails between the two must not leave it, with the
// caller's pointers, to the next cf_update_state on the context
struct HaloRequestScope {
    cf_ctx* ctx;
    explicit HaloRequestScope(cf_ctx* c) : ctx(c) { ctx->halo_request = cf_ctx::HaloRequest{}; }
    ~HaloRequestScope() { ctx->halo_request = cf_ctx::HaloRequest{}; }
    HaloRequestScope(const HaloRequestScope&) = delete;
    HaloRequestScope& operator=(const HaloRequestScope&) = delete;
};

// time averages: what cf_average_create (coflux_average.cpp), cf_average_create_derived (coflux_derived.cpp) and
// cf_average_create_budget (coflux_budget.cpp) hand back differs in the arguments of a collection's launch only
struct PlainAverageArgs {
    int nfields;
    AverageFields fields;
};
struct cf_average : cf_child {
    std::variant<PlainAverageArgs, DerivedArgs, BudgetArgs> args;
    RunningWeight weight;    // of the window
    int collect(double w);   // one collection (cf_average_collect without the argument checks of the ABI entry)
    int collect_step(const Attachment& at, int64_t) override { return collect(at.when.stride * at.step_weight); }
    uint32_t section_kind() const override { return cfck::KIND_AVERAGE; }
    void plan_section(const SectionPlan& P, const int64_t*) const override {
        P.entry.bytes = RunningWeight::BYTES;
        P.tail.resize(RunningWeight::BYTES);
        weight.put(P.tail.data());
    }
    void load_tail(const std::vector<unsigned char>& tail, int64_t) override { weight.get(tail.data()); }
};

// calendar-binned means (coflux_climatology.cpp): the pointers are the caller's, the weights are host bookkeeping — the handle
// owns no device resource
struct cf_climatology : cf_child {
    int n_fields = 0, n_bins = 0, max_blocks = 0;
    const double* src[CF_CLIMATOLOGY_MAX_FIELDS] = {};
    double* total[CF_CLIMATOLOGY_MAX_FIELDS] = {};
    double* bins[CF_CLIMATOLOGY_MAX_FIELDS] = {};
    RunningWeight weight;       // of every collection since the reset
    RunningWeight bin_weight[CF_CLIMATOLOGY_MAX_BINS];
    std::vector<double> edges;               // while attached: a copy of the caller's calendar table (cf_attach_climatology)
    std::vector<int32_t> bin_of_interval;
    int collect(int32_t bin, double w);   // one collection into bin ≥ 0 (cf_climatology_collect without the argument checks)
    int admit(const Attachment& at, const char* fn, int64_t first_step, int nsteps) const override;   // the table covers every due step
    int collect_step(const Attachment& at, int64_t step) override;
    uint32_t section_kind() const override { return cfck::KIND_CLIMATOLOGY; }
    void plan_section(const SectionPlan& P, const int64_t*) const override {
        P.entry.n_entries = (uint32_t)n_bins;
        P.entry.bytes = RunningWeight::BYTES + 16 * (uint64_t)n_bins;
        P.tail.resize((size_t)P.entry.bytes);
        put_binned_weights(P.tail.data(), weight, bin_weight, n_bins);
    }
    int check_entry(const cfck::Entry& E, const char* fn) const override;
    void load_tail(const std::vector<unsigned char>& tail, int64_t) override { get_binned_weights(tail.data(), &weight, bin_weight, n_bins); }
};

// a dataset staged on the device (coflux_dataset.cpp): the handle owns its planes, its levels and the upload lane
struct cf_dataset : cf_child {
    int ns_x = 0, ns_y = 0, n_levels = 0, max_sweeps = -1, sweeps_per_launch = 0, max_blocks = 0;
    bool periodic_x = false;
    double fill_value = 0.0, period = 0.0;
    std::vector<double> times;
    cf_interp_weights weights{};              // borrowed device arrays
    cf::DeviceBuffer<double> d_plane[2];      // the sweeps' p and q
    cf::DeviceBuffer<float> d_upload;         // the plane as it arrived
    cf::DeviceBuffer<double> d_levels;        // n_levels parent arrays back to back
    cf::PinnedBuffer<float> h_upload[2];      // two slots: a stage call returns while its copy is still in flight
    cf::Event uploaded[2];
    int upload_slot = 0, current = 0;         // current: which plane holds the most recently staged level, inpainted
    int last_level = -1;
    struct Staged {
        bool done = false;
        int32_t sweeps = 0;
        int64_t filled = 0, defaulted = 0;
    } staged[CF_DATASET_MAX_LEVELS];
    size_t parent() const { return (size_t)ctx->grid.sj * (size_t)(ctx->grid.ny + 2 * ctx->grid.hy); }
    double* level(int l) const { return d_levels.get() + parent() * (size_t)l; }
    int first_unstaged() const {
        for (int l = 0; l < n_levels; ++l)
            if (!staged[l].done) return l;
        return -1;
    }
};
// S★ of `d` at `time` as the kernels take it: CF_ERR_INVALID (the refusal of `fn`) unless every level is staged and the time finite
struct DatasetTarget {
    const double* level1;
    const double* level2;
    double fraction;
};
int dataset_target_at(const cf_dataset* d, const char* fn, double time, DatasetTarget* out);

struct cf_regrid : cf_child {
    RegridTables tables{};
    int64_t n_rows = 0;
    int max_blocks = 0;
    cf::DeviceBuffer<unsigned char> d_block;  // the one allocation behind every table
};

// sets the thread-local and the context's last-error text and returns `code`
int cf_fail(cf_ctx* ctx, int code, const char* fmt, ...);
#define fail cf_fail

#define HIP_TRY(ctx, expr)                                                                              \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(ctx, CF_ERR_HIP, "%s:%d: %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
    } while (0)

#define CHECK(call)            \
    do {                       \
        int rc_ = (call);      \
        if (rc_ != CF_OK) return rc_; \
    } while (0)

// coflux_steps.cpp: the stand-alone peer-direct exchange kernel for `F` (counts the exchange in ctx->peer_seq)
extern "C" __attribute__((visibility("hidden"))) int cf_peer_halo_launch_now(cf_ctx* ctx, const PeerFields* F, int rows);
// coflux_steps.cpp, for coflux_tiles.cpp: a mailbox behind an IPC handle (this process's own are found by their handle and used
// as they are), the book of this process's own, and what the fold of `rows` rows needs of the grid
extern "C" __attribute__((visibility("hidden"))) int cf_peer_map_mailbox(cf_ctx* ctx, const void* handle, char** out, cf::IpcMapping* mapping);
void cf_peer_remember_local(const void* handle, char* mailbox, int device);
void cf_peer_forget_local(const char* mailbox);
extern "C" __attribute__((visibility("hidden"))) int check_fold_geometry(cf_ctx* ctx, int rows);
// coflux_tiles.cpp: what one tile exchange of `nfields` × `rows` needs of the context and of the call (`fn` names the caller),
// and the exchange itself — the x-phase, the y-phase, on a world one tile wide the local fold (counts it in ctx->tile.seq)
int check_tile_exchange(cf_ctx* ctx, const char* fn, int nfields, int rows, int fold_north);
int tile_exchange_launch(cf_ctx* ctx, const FoldFields* F, int rows, int fold_north);
// coflux_checkpoint.cpp: waits for the restores of ctx's checkpoint handles that are still unchecked and compares their hashes
int checkpoint_settle_restores(cf_ctx* ctx);
// coflux_steps.cpp: queues what a transition of ctx->ahead answered with (AheadLedger::Work)
extern "C" __attribute__((visibility("hidden"))) int cf_ahead_perform(cf_ctx* ctx, const AheadLedger::Work* work);
// coflux_abi.cpp: the argument checks of cf_prepare_coupled_step, of the cf_update_state of every step of a schedule and of the
// cf_update_state_sea_ice of a coupled step loop, without their launches (cf_time_steps and cf_time_steps_coupled validate a
// whole call before its first launch)
extern "C" __attribute__((visibility("hidden"))) int check_coupled_prepare(cf_ctx* ctx, const cf_coupled_prepare* p);
// coflux_abi.cpp: cf_prepare_coupled_step whose restoring job reads S★ from two levels of a dataset — p->target_salinity is
// level1, `level2` and `fraction` the rest (fraction 0.0: cf_prepare_coupled_step itself)
extern "C" __attribute__((visibility("hidden"))) int prepare_coupled_step_levels(cf_ctx* ctx, const cf_coupled_prepare* p, const double* level2,
                                                                                 double fraction);
extern "C" __attribute__((visibility("hidden"))) int check_step_arguments(cf_ctx* ctx, const cf_atmos_source* src, const cf_interp_weights* w,
                                                                          const cf_run_schedule* S, const cf_interface_fluxes* fluxes,
                                                                          const cf_net_ocean_fluxes* net);
extern "C" __attribute__((visibility("hidden"))) int check_coupled_update(cf_ctx* ctx, const cf_atmos_source* src, const cf_interp_weights* w,
                                                                          const cf_run_schedule* S, const cf_interface_fluxes* fluxes,
                                                                          const cf_net_ocean_fluxes* net, const cf_interface_fluxes* ai_fluxes);

// whether two ocean-grid fields (halos included) at p and q share bytes: what the averagers refuse between a mean and anything else
inline bool fields_overlap(const GridDesc& G, const void* p, const void* q) {
    const uintptr_t bytes = (uintptr_t)G.sj * (uintptr_t)(G.ny + 2 * G.hy) * sizeof(double), x = (uintptr_t)p, y = (uintptr_t)q;
    return x < y + bytes && y < x + bytes;
}

// the same for two byte ranges of their own lengths (a block of several parent arrays, a uint8 mask)
inline bool ranges_overlap(const void* p, uintptr_t bytes_p, const void* q, uintptr_t bytes_q) {
    const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
    return x < y + bytes_q && y < x + bytes_p;
}

// The child handles: `child` joins ctx's list / leaves it and whichever attachment holds it (a no-op once orphaned) / cf_destroy
// orphans them all
inline void child_adopt(cf_ctx* ctx, cf_child* child) {
    child->ctx = ctx;
    child->device = ctx->device;
    ctx->children.push_back(child);
}
inline void child_leave(cf_child* child) {
    cf_ctx* ctx = child->ctx;
    if (!ctx) return;
    ctx->children.erase(std::remove(ctx->children.begin(), ctx->children.end(), child), ctx->children.end());
    for (Attachment& at : ctx->attached)
        if (at.handle == child) at = Attachment{};
    if (ctx->restoring_dataset.handle == child) ctx->restoring_dataset = Attachment{};
}
inline void orphan_children(cf_ctx* ctx) {
    for (cf_child* child : ctx->children) child->ctx = nullptr;
    ctx->children.clear();
    ctx->checkpoints.clear();
    for (Attachment& at : ctx->attached) at = Attachment{};
    ctx->restoring_dataset = Attachment{};
}
// CF_ERR_INVALID unless `child` is a handle whose context is alive: live(a, "cf_average_reset", "averager")
inline int live(const cf_child* child, const char* fn, const char* kind) {
    if (!child) return fail(nullptr, CF_ERR_INVALID, "%s: %s is NULL", fn, kind);
    if (!child->ctx) return fail(nullptr, CF_ERR_INVALID, "%s: the %s's context has been destroyed", fn, kind);
    return CF_OK;
}
