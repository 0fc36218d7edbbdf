// collect_rules_driver.cpp — a stand-alone program over csrc/coflux_collect.hpp alone (no HIP, no libcoflux): it reads one
// command per line from its standard input and answers each with one line; doubles travel as the 16 hex digits of their bits.
//     weights <w | reset>...           per weight: accepts store c_prev c_new total samples   (an accepted weight is added)
//     collections <stride> <first> <n> StepSchedule::collections, then the count of due() steps in [first, first + n)
//     stamp <origin> <seconds> <step>  StepSchedule::stamp
//     weight <total> <samples>         the 16 checkpoint bytes, then (total, samples) read back from them
//     tail <n> <total> <samples> (<bin total> <bin samples>) × n
//                                      the climatology tail's bytes, then the same bytes written from what was read back
// Every byte buffer is a heap block of exactly its size: a byte written or read beyond it is a report of the sanitizer.
// tests/test_collect_rules_cpu.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "coflux_collect.hpp"

static double f64(const std::string& hex) {
    const unsigned long long bits = std::strtoull(hex.c_str(), nullptr, 16);
    double v;
    std::memcpy(&v, &bits, 8);
    return v;
}
static unsigned long long bits_of(double v) {
    unsigned long long bits;
    std::memcpy(&bits, &v, 8);
    return bits;
}
static void print_bytes(const std::vector<unsigned char>& b) {
    for (unsigned char c : b) std::printf("%02x", c);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        in >> cmd;
        if (cmd == "weights") {
            RunningWeight W;
            while (in >> tok) {
                if (tok == "reset") {
                    W.reset();
                    continue;
                }
                const double w = f64(tok);
                const bool ok = W.accepts(w);
                const RunningWeight::Blend c = W.next(w);
                if (ok) W.add(w);
                std::printf("%d %d %016llx %016llx %016llx %lld ", (int)ok, (int)c.store, bits_of(c.c_prev), bits_of(c.c_new), bits_of(W.total),
                            (long long)W.samples);
            }
        } else if (cmd == "collections") {
            StepSchedule S;
            long long first, n, due = 0;
            in >> S.stride >> first >> n;
            for (long long s = first; s < first + n; ++s) due += S.due(s);
            std::printf("%lld %lld", (long long)S.collections(first, (int)n), due);
        } else if (cmd == "stamp") {
            StepSchedule S;
            std::string origin, seconds;
            long long step;
            in >> origin >> seconds >> step;
            S.time_origin = f64(origin);
            S.step_seconds = f64(seconds);
            std::printf("%016llx", bits_of(S.stamp(step)));
        } else if (cmd == "weight") {
            RunningWeight W, back;
            long long samples;
            in >> tok >> samples;
            W.total = f64(tok);
            W.samples = samples;
            std::vector<unsigned char> bytes(RunningWeight::BYTES);
            W.put(bytes.data());
            back.get(bytes.data());
            print_bytes(bytes);
            std::printf(" %016llx %lld", bits_of(back.total), (long long)back.samples);
        } else if (cmd == "tail") {
            int n;
            in >> n;
            std::vector<RunningWeight> bins((size_t)n + 1), back((size_t)n + 1);   // [0]: the weight of everything
            for (RunningWeight& b : bins) {
                long long samples;
                in >> tok >> samples;
                b.total = f64(tok);
                b.samples = samples;
            }
            std::vector<unsigned char> bytes(RunningWeight::BYTES + 16 * (size_t)n), again(bytes.size());
            put_binned_weights(bytes.data(), bins[0], bins.data() + 1, n);
            get_binned_weights(bytes.data(), &back[0], back.data() + 1, n);
            put_binned_weights(again.data(), back[0], back.data() + 1, n);
            print_bytes(bytes);
            std::printf(" ");
            print_bytes(again);
        } else {
            std::fprintf(stderr, "unknown command: %s\n", line.c_str());
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}
