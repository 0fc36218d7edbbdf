// coflux_request_ahead.hpp — the books of the atmosphere states requested AHEAD of their step (include/coflux.h:
// cf_prefetch_atmosphere_state, a pipelined cf_time_steps, cf_discard_prefetched_atmosphere_state, cf_window_commit).  Plain
// host bookkeeping without HIP: every transition of a request's life is one method below, which books it and answers with the
// stream work it implies (Work) for the caller to queue — cf_ahead_perform, coflux_steps.cpp.  WHICH launch carries a request
// that leaves with a step stays the launch code's decision (coflux_abi.cpp); it tells the ledger by leave_main.
// tests/request_ahead_driver.cpp holds this header against tests/prefetch_model.py on the CPU.
#pragma once
#include <cstdint>

#include "../../include/coflux.h"

// Whether the atmosphere state requested ahead from (a, wa) is the one a step asks for with (b, wb): the same source arrays and
// shape, levels and time fraction, through the same map.  Levels and fraction alone do not say so: two snapshot windows, a
// re-bound in-memory atmosphere or a second weight map give another field under the same clock.
inline bool same_interpolation(const cf_atmos_source& a, const cf_interp_weights& wa, const cf_atmos_source& b, const cf_interp_weights& wb) {
    for (int v = 0; v < CF_JRA55_NVARS; ++v)
        if (a.data[v] != b.data[v]) return false;
    return a.ns_x == b.ns_x && a.ns_y == b.ns_y && a.n_levels == b.n_levels && a.level1 == b.level1 && a.level2 == b.level2 &&
           a.time_fraction == b.time_fraction && wa.separable == wb.separable && wa.fi == wb.fi && wa.fj == wb.fj &&
           wa.cos_rot == wb.cos_rot && wa.sin_rot == wb.sin_rot && wa.latitude == wb.latitude;
}

struct AheadLedger {
    // A request is booked in one record from the moment it is accepted until it ends; record k owns the auxiliary lane's
    // done[k] event for that time.  An exchange set (identified by its u pointer) has at most one record, and at most one
    // record is WAITING: request() sends an earlier one off before it books the next.
    enum State : uint8_t {
        FREE,
        WAITING,     // requested, not launched: it leaves with the next step into another set, or on the auxiliary stream
        LEFT_AUX,    // launched on the auxiliary stream: done[k] is recorded behind it, whoever touches the set next waits on it
        LEFT_MAIN,   // launched on the context's stream (tail, merged, a launch of its own): stream order, no event
    };
    // the launch a request left in: the launched_* counter of cf_prefetch_stats of the same name
    enum Route { AUX, TAIL, MERGED, ICE_TAIL, OWN };
    struct Record {
        State state = FREE;
        bool gated = false;         // the lane's gate event has been recorded for it (not for a deferred request under
                                    // CF_OPT_MERGED_PREFETCH: stream order gates it, a flush to the auxiliary stream records it late)
        cf_atmos_source src{};      // what is interpolated: the source's arrays and shape, the levels and the fraction …
        cf_interp_weights w{};      // … through which map …
        cf_exchange_fields out{};   // … into which exchange set
    };
    // What the caller queues for a transition, in this order
    struct Work {
        int launch_aux = -1;        // record k leaves on the auxiliary stream: (gate_late: the gate event on the context's stream,) the
        bool gate_late = false;     //   lane waits on the gate, the background interpolation of `launched`, done[k] behind it
        Record launched;            //   a copy of the request that leaves: the same transition may book record k anew (request)
        unsigned wait_done = 0;     // bit k: the context's stream waits on done[k]
        bool gate_now = false;      // the gate event on the context's stream
    };
    // … and what the transition answers besides.  rec NULL: refused, two other sets are pending (the waiting one has still been
    // sent off); interpolate: nothing was pending for the step's set, or not what it asks for; needed: the call requests its
    // first step's state itself
    struct Booked { Work work; const Record* rec = nullptr; };
    struct Stepped { Work work; bool interpolate = true; };
    struct FirstStep { Work work; bool needed = true; };

    // record k, read-only: every change goes through a method below
    const Record& operator[](int k) const { return rec[k]; }
    int index(const Record* r) const { return (int)(r - rec); }

    // the counters of cf_debug_prefetch_stats, written in this file and nowhere else;
    // requests = consumed + mismatched + voided + superseded + discarded + pending after every method
    const cf_prefetch_stats& stats() const { return stats_; }

    // cf_prefetch_atmosphere_state and the requests of cf_time_steps.  `mode`: CF_OPT_MERGED_PREFETCH.  A state of the same set
    // that no step asked for is superseded, now: the set never has two states on the books.  The set written was last read by
    // kernels already queued on the context's stream, so everything queued so far gates the request — but for a deferred one
    // under a merged mode, which leaves inside a launch of that stream (an event per step would only put a barrier packet into
    // the queue).  !defer: the caller sends it off at once (leave_aux).
    Booked request(const cf_atmos_source& src, const cf_interp_weights& w, const cf_exchange_fields& out, int mode, bool defer) {
        Booked B{leave_aux()};   // at most one request waits for a solver launch
        Record* r = find(out.u);
        if (!r) r = find_free();
        if (!r) return B;   // refused here, where nothing has been launched or booked for it
        if (r->state != FREE) end(*r, stats_.superseded, B.work);
        ++stats_.requests;
        ++stats_.pending;
        r->state = WAITING;
        r->gated = B.work.gate_now = !(defer && mode != 0);
        r->src = src;
        r->w = w;
        r->out = out;
        B.rec = r;
        return B;
    }

    // The waiting request, if any, leaves on the auxiliary stream: cf_sync, another request, a step into its own set, a step
    // under CF_OPT_MERGED_PREFETCH = 0 (right behind its solver launch)
    Work leave_aux() {
        Work W;
        for (Record& r : rec)
            if (r.state == WAITING) {
                W.launch_aux = index(&r);
                W.gate_late = !r.gated;   // (a later gate than needed: still ordered)
                r.gated = true;
                r.state = LEFT_AUX;
                W.launched = r;
                ++counter(AUX);
            }
        return W;
    }

    // The waiting request when it is for another set than `key` — the one a step into `key` may carry in its launches — else NULL
    const Record* waiting_for_other_set(const double* key) const {
        for (const Record& r : rec)
            if (r.state == WAITING && r.out.u != key) return &r;
        return nullptr;
    }
    // … and has just been launched on the context's stream, in the launch `route` names
    void leave_main(const Record* waiting, Route route) {
        rec[index(waiting)].state = LEFT_MAIN;
        ++counter(route);
    }

    // A step into set `key` that asks for (src, w).  A request into `key` itself that still waits is sent off first; what is
    // pending for the set then ends: consumed when it is what the step asks for, else mismatched (the wait also orders its
    // writes before the step's own)
    Stepped step(const double* key, const cf_atmos_source& src, const cf_interp_weights& w) {
        Stepped S;
        if (Record* r = find(key)) {
            if (r->state == WAITING) S.work = leave_aux();
            S.interpolate = !same_interpolation(r->src, r->w, src, w);
            end(*r, S.interpolate ? stats_.mismatched : stats_.consumed, S.work);
        }
        if (S.interpolate) ++stats_.step_interpolations;
        return S;
    }

    // The first step of a pipelined cf_time_steps call: its state is pending already (a continuing call requested it; still
    // waiting, it is sent off), or the call has to request it
    FirstStep first_step_of_call(const double* key, const cf_atmos_source& src, const cf_interp_weights& w) {
        FirstStep F;
        const Record* r = find(key);
        F.needed = !(r && same_interpolation(r->src, r->w, src, w));
        if (!F.needed && r->state == WAITING) F.work = leave_aux();
        return F;
    }

    // cf_window_commit: a state computed — or to be computed — from the snapshot in `slot` is void
    Work commit_slot(int slot) {
        Work W;
        for (Record& r : rec)
            if (r.state != FREE && (r.src.level1 == slot || r.src.level2 == slot)) end(r, stats_.voided, W);
        return W;
    }
    // cf_discard_prefetched_atmosphere_state: everything pending, launched or not
    Work discard() {
        Work W;
        for (Record& r : rec)
            if (r.state != FREE) end(r, stats_.discarded, W);
        return W;
    }

    // cf_set_stream: a state launched ON the context's stream is consumed by stream order alone — another stream has to wait for it
    bool any_left_on_main() const { return rec[0].state == LEFT_MAIN || rec[1].state == LEFT_MAIN; }

  private:
    Record rec[2];
    cf_prefetch_stats stats_{};

    Record* find(const double* key) {
        for (Record& r : rec)
            if (r.state != FREE && r.out.u == key) return &r;
        return nullptr;
    }
    Record* find_free() {
        for (Record& r : rec)
            if (r.state == FREE) return &r;
        return nullptr;
    }
    // one that went out on the auxiliary stream: whatever the context's stream does to its set next is ordered behind that kernel
    void end(Record& r, uint64_t& outcome, Work& W) {
        if (r.state == LEFT_AUX) W.wait_done |= 1u << index(&r);
        r.state = FREE;
        ++outcome;
        --stats_.pending;
    }
    uint64_t& counter(Route route) {
        using C = cf_prefetch_stats;
        static constexpr uint64_t C::*of[] = {&C::launched_aux, &C::launched_tail, &C::launched_merged, &C::launched_ice_tail, &C::launched_own};
        return stats_.*of[route];
    }
};
