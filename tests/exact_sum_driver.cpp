// exact_sum_driver.cpp — csrc/coflux_exact_sum.hpp alone, for tests/test_exact_sum_cpu.py: compiled with
// -fsanitize=address,undefined and run once as a subprocess.  Every input line is one question,
//     sum <part> | <part> | …        a part: tokens <16 hex digits of a double>[*<repeat count>]
// and every answer one line: each part goes into an accumulator of its own, the accumulators are merged digit-wise, and the line
// holds the bits of the rounded sum, then the merged accumulator's 67 digits and 3 counters (decimal).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "coflux_exact_sum.hpp"

using namespace coflux;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        in >> word;
        if (word != "sum") {
            std::printf("?\n");
            continue;
        }
        XsAccumulator total, part;
        xs_clear(&total);
        xs_clear(&part);
        while (in >> word) {
            if (word == "|") {
                xs_merge(&total, &part);
                xs_clear(&part);
                continue;
            }
            const size_t star = word.find('*');
            const uint64_t u = std::strtoull(word.substr(0, star).c_str(), nullptr, 16);
            const unsigned long long repeat = star == std::string::npos ? 1ull : std::strtoull(word.c_str() + star + 1, nullptr, 10);
            for (unsigned long long n = 0; n < repeat; ++n) xs_add(&part, xs_double(u));
        }
        xs_merge(&total, &part);
        std::printf("%016" PRIx64, xs_bits(xs_round(&total)));
        for (int k = 0; k < XS_DIGITS; ++k) std::printf(" %" PRId64, total.digit[k]);
        for (int k = 0; k < XS_COUNTERS; ++k) std::printf(" %" PRIu64, total.nonfinite[k]);
        std::printf("\n");
    }
    return 0;
}
