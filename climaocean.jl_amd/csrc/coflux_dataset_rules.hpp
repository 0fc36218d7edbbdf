// coflux_dataset_rules.hpp — the two host rules of a staged dataset (cf_dataset_*, include/coflux.h), stated once: the clock
// that turns a time into two levels and a fraction (cf_dataset_time_index) and the number of inpainting sweeps a plane needs,
// known before the first launch (cf_dataset_stage).  Plain C++: no HIP header, no context, nothing else of the library, so
// that tests/dataset_rules_driver.cpp builds and runs alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cfds {

// a table of level times: n ≥ 1 finite, strictly increasing values; period 0 (clamped) or above times[n − 1] − times[0] (cyclical)
inline bool times_ok(const double* times, int32_t n, double period) {
    if (!times || n < 1) return false;
    for (int32_t k = 0; k < n; ++k) {
        if (!std::isfinite(times[k])) return false;
        if (k > 0 && !(times[k] > times[k - 1])) return false;
    }
    if (!std::isfinite(period) || period < 0.0) return false;
    if (period > 0.0 && !(period > times[n - 1] - times[0])) return false;
    return true;
}

// The clock on a checked table.  Cyclical: r = fmod(time − times[0], period), + period when negative, τ = times[0] + r; k with
// times[k] ≤ τ < times[k + 1] gives (k, k + 1, (τ − times[k]) / (times[k + 1] − times[k])), and τ ≥ times[n − 1] gives
// (n − 1, 0, (τ − times[n − 1]) / (times[0] + period − times[n − 1])).  Clamped: below times[0] (0, 0, 0.0), at or beyond
// times[n − 1] (n − 1, n − 1, 0.0).  One level: always (0, 0, 0.0).  False for a time that is not finite.
inline bool time_index(const double* times, int32_t n, double period, double time, int32_t* level1, int32_t* level2, double* fraction) {
    if (!std::isfinite(time)) return false;
    *level1 = *level2 = 0;
    *fraction = 0.0;
    if (n == 1) return true;
    double tau = time;
    if (period > 0.0) {
        double r = std::fmod(time - times[0], period);
        if (r < 0.0) r += period;
        tau = times[0] + r;
        if (tau >= times[n - 1]) {
            *level1 = n - 1;
            *level2 = 0;
            *fraction = (tau - times[n - 1]) / (times[0] + period - times[n - 1]);
            return true;
        }
    } else {
        if (tau < times[0]) return true;
        if (tau >= times[n - 1]) {
            *level1 = *level2 = n - 1;
            return true;
        }
    }
    const int32_t k = (int32_t)(std::upper_bound(times, times + n, tau) - times) - 1;
    *level1 = k;
    *level2 = k + 1;
    *fraction = (tau - times[k]) / (times[k + 1] - times[k]);
    return true;
}

// What the inpainting of one plane (ns_y rows of ns_x, NaN = missing) will do, from one multi-source breadth-first pass: a NaN
// cell at 4-connected distance d from the nearest cell that is not NaN (x wraps when periodic, y never does) receives its value
// in sweep d.  depth: the largest such distance (0 without a NaN, and for a plane with no valid cell at all); sweeps:
// min(max_sweeps, depth), or depth when max_sweeps < 0; filled: NaN cells with d ≤ sweeps; defaulted: the NaN cells left.
struct SweepPlan {
    int32_t depth = 0, sweeps = 0;
    int64_t filled = 0, defaulted = 0;
};
inline SweepPlan sweep_plan(const float* plane, int32_t ns_x, int32_t ns_y, bool periodic_x, int32_t max_sweeps) {
    SweepPlan P;
    const size_t n = (size_t)ns_x * (size_t)ns_y;
    std::vector<int32_t> dist(n, -1);
    std::vector<uint32_t> queue;
    queue.reserve(n);
    for (size_t c = 0; c < n; ++c)
        if (!std::isnan(plane[c])) {
            dist[c] = 0;
            queue.push_back((uint32_t)c);
        }
    const int64_t missing = (int64_t)(n - queue.size());
    for (size_t head = 0; head < queue.size(); ++head) {
        const uint32_t c = queue[head];
        const int32_t j = (int32_t)(c / (uint32_t)ns_x), i = (int32_t)(c - (uint32_t)j * (uint32_t)ns_x);
        const int32_t d = dist[c] + 1;
        auto visit = [&](int32_t ii, int32_t jj) {
            const size_t at = (size_t)jj * (size_t)ns_x + (size_t)ii;
            if (dist[at] < 0) {
                dist[at] = d;
                queue.push_back((uint32_t)at);
            }
        };
        if (i > 0) visit(i - 1, j);
        else if (periodic_x) visit(ns_x - 1, j);
        if (i + 1 < ns_x) visit(i + 1, j);
        else if (periodic_x) visit(0, j);
        if (j > 0) visit(i, j - 1);
        if (j + 1 < ns_y) visit(i, j + 1);
    }
    if (!queue.empty()) P.depth = dist[queue.back()];   // breadth first: the last cell reached is a farthest one
    P.sweeps = max_sweeps < 0 ? P.depth : std::min(max_sweeps, P.depth);
    for (size_t c = 0; c < n; ++c)
        if (dist[c] > 0 && dist[c] <= P.sweeps) ++P.filled;
    P.defaulted = missing - P.filled;
    return P;
}

}  // namespace cfds
