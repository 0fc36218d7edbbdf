// coflux_collect.hpp — the two host rules every collected diagnostic follows, stated once: the weight of a running mean
// (cf_average, and cf_climatology for its total and for each bin) and the schedule by which the step loops collect an attached
// handle.  Plain C++: no HIP header, no context (the image's byte order comes from coflux_checkpoint_image.hpp, inline), so that
// tests/collect_rules_driver.cpp builds and runs alone.
#pragma once
#include <cmath>

#include "coflux_checkpoint_image.hpp"

// The total weight a running mean has received and in how many collections.  A collection of weight w blends the mean as
// m ← (m · c_prev) + (f · c_new); the first one since the reset stores f.  All in double, in this order of operations: the
// climatology's total holds bit for bit what a cf_average fed the same weights holds because both come through here.
struct RunningWeight {
    double total = 0.0;
    int64_t samples = 0;
    struct Blend {
        bool store;
        double c_prev, c_new;
    };
    bool accepts(double w) const { return w > 0.0 && std::isfinite(w) && std::isfinite(total + w); }
    Blend next(double w) const {
        const double sum = total + w;
        const bool store = samples == 0;
        return Blend{store, store ? 0.0 : total / sum, store ? 1.0 : w / sum};
    }
    void add(double w) {
        total += w;
        ++samples;
    }
    void reset() { *this = RunningWeight{}; }

    // the checkpoint form: the total's bits, then the samples
    static constexpr size_t BYTES = 16;
    void put(unsigned char* at) const {
        cfck::put_f64(at, total);
        cfck::put64(at + 8, (uint64_t)samples);
    }
    void get(const unsigned char* at) {
        total = cfck::get_f64(at);
        samples = (int64_t)cfck::get64(at + 8);
    }
};

// A binned mean's weights in a checkpoint, BYTES + 16 · n bytes: the weight of everything, all bin totals, then all bin samples
inline void put_binned_weights(unsigned char* at, const RunningWeight& all, const RunningWeight* bin, int n) {
    all.put(at);
    for (int b = 0; b < n; ++b) {
        cfck::put_f64(at + RunningWeight::BYTES + 8 * (size_t)b, bin[b].total);
        cfck::put64(at + RunningWeight::BYTES + 8 * (size_t)(n + b), (uint64_t)bin[b].samples);
    }
}
inline void get_binned_weights(const unsigned char* at, RunningWeight* all, RunningWeight* bin, int n) {
    all->get(at);
    for (int b = 0; b < n; ++b) {
        bin[b].total = cfck::get_f64(at + RunningWeight::BYTES + 8 * (size_t)b);
        bin[b].samples = (int64_t)cfck::get64(at + RunningWeight::BYTES + 8 * (size_t)(n + b));
    }
}

// When the step loops collect an attached handle.  Steps are numbered globally, so a run split into several calls collects the
// same steps and stamps them with the same times.
struct StepSchedule {
    int32_t stride = 1;
    double time_origin = 0.0, step_seconds = 0.0;
    bool due(int64_t step) const { return (step + 1) % stride == 0; }
    double stamp(int64_t step) const { return time_origin + (double)(step + 1) * step_seconds; }
    // of the steps [first_step, first_step + nsteps): those that are due
    int64_t collections(int64_t first_step, int nsteps) const { return (first_step + nsteps) / stride - first_step / stride; }
};
