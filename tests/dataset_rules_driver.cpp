// dataset_rules_driver.cpp — answers questions about the host rules of a staged dataset (csrc/coflux_dataset_rules.hpp, the
// only header of the library included here) on stdin, one per line, one answer line each (tests/test_dataset_cpu.py):
//   time <n> <period> <time> <times[0]> … <times[n-1]>     doubles as 16 hex digits  →  "<level1> <level2> <fraction hex>" | "invalid"
//   plan <ns_x> <ns_y> <periodic> <max_sweeps> <cells …>   floats as 8 hex digits    →  "<depth> <sweeps> <filled> <defaulted>"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "coflux_dataset_rules.hpp"

static double f64_of(const std::string& s) {
    const uint64_t u = std::stoull(s, nullptr, 16);
    double v;
    std::memcpy(&v, &u, 8);
    return v;
}
static float f32_of(const std::string& s) {
    const uint32_t u = (uint32_t)std::stoul(s, nullptr, 16);
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, word;
        in >> what;
        if (what == "time") {
            int n;
            std::string period, time;
            in >> n >> period >> time;
            std::vector<double> times;
            while (in >> word) times.push_back(f64_of(word));
            int32_t l1 = -1, l2 = -1;
            double f = -1.0;
            if ((int)times.size() != n || !cfds::times_ok(times.empty() ? nullptr : times.data(), n, f64_of(period)) ||
                !cfds::time_index(times.data(), n, f64_of(period), f64_of(time), &l1, &l2, &f)) {
                std::printf("invalid\n");
                continue;
            }
            uint64_t u;
            std::memcpy(&u, &f, 8);
            std::printf("%d %d %016" PRIx64 "\n", l1, l2, u);
        } else if (what == "plan") {
            int ns_x, ns_y, periodic, max_sweeps;
            in >> ns_x >> ns_y >> periodic >> max_sweeps;
            std::vector<float> plane;
            while (in >> word) plane.push_back(f32_of(word));
            if ((int)plane.size() != ns_x * ns_y) {
                std::printf("invalid\n");
                continue;
            }
            const cfds::SweepPlan P = cfds::sweep_plan(plane.data(), ns_x, ns_y, periodic != 0, max_sweeps);
            std::printf("%d %d %lld %lld\n", P.depth, P.sweeps, (long long)P.filled, (long long)P.defaulted);
        } else {
            std::printf("invalid\n");
        }
    }
    return 0;
}
