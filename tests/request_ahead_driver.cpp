// request_ahead_driver.cpp — a stand-alone program over csrc/coflux_request_ahead.hpp alone (no HIP, no libcoflux): it reads
// one command per line from its standard input, applies it to the ledger of the current case and answers with one line.
// Sources, weight maps and exchange sets are small integers that stand in for pointers (never dereferenced); the time
// fraction travels as the 16 hex digits of its bits.
//     case                                                   a fresh ledger
//     request <src> <map> <set> <l1> <l2> <tf> <mode> <defer>    AheadLedger::request
//     first <set> <src> <map> <l1> <l2> <tf>                     AheadLedger::first_step_of_call
//     step <set> <src> <map> <l1> <l2> <tf>                      AheadLedger::step
//     leave_aux                                              AheadLedger::leave_aux
//     leave_main <set> <route 1…4>                           waiting_for_other_set(set), then leave_main(it, route)
//     commit <slot> | discard                                AheadLedger::commit_slot | discard
// The answer: the Work the transition returned as words in the order it is to be queued — L<k> the launch of record k on the
// auxiliary stream (gL<k>: behind a late gate) followed by :<src>:<map>:<set>:<l1>:<l2>:<tf> of the request it launches, W<k> a wait of the context's stream on done[k], G the gate now — then "|", the
// transition's own answer (request: the record booked or "refused"; first: needed 0/1; step: interpolate 0/1; leave_main: the
// record, or "none" where nothing waits for another set), "|", the 13 counters in the order of cf_prefetch_stats from
// `pending` on, any_left_on_main() and the state of both records (F free, W waiting, A left on the auxiliary stream, M on the
// context's).  tests/test_request_ahead_cpu.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "coflux_request_ahead.hpp"

template <class T>
static T* fake(long id) {
    return reinterpret_cast<T*>(static_cast<uintptr_t>(id) * 64);
}
static long id_of(const void* p) {
    return (long)(reinterpret_cast<uintptr_t>(p) / 64);
}
static cf_atmos_source source(std::istream& in, long id) {
    cf_atmos_source s{};
    for (int v = 0; v < CF_JRA55_NVARS; ++v) s.data[v] = fake<const float>(100 * id + v + 1);
    std::string tf;
    in >> s.level1 >> s.level2 >> tf;
    const unsigned long long bits = std::strtoull(tf.c_str(), nullptr, 16);
    std::memcpy(&s.time_fraction, &bits, 8);
    s.ns_x = 640, s.ns_y = 320, s.n_levels = 4;
    return s;
}
static cf_interp_weights map_of(long id) {
    cf_interp_weights w{};
    w.separable = (int)(id % 2);
    w.fi = fake<const double>(1000 + id);
    w.fj = fake<const double>(2000 + id);
    return w;
}
static void print_work(const AheadLedger::Work& W) {
    if (W.launch_aux >= 0) {
        const AheadLedger::Record& r = W.launched;   // what the launch would read and write: <src>:<map>:<set>:<l1>:<l2>:<tf>
        unsigned long long bits;
        std::memcpy(&bits, &r.src.time_fraction, 8);
        std::printf("%sL%d:%ld:%ld:%ld:%d:%d:%016llx ", W.gate_late ? "g" : "", W.launch_aux, (id_of(r.src.data[0]) - 1) / 100,
                    id_of(r.w.fi) - 1000, id_of(r.out.u), r.src.level1, r.src.level2, bits);
    }
    for (int k = 0; k < 2; ++k)
        if (W.wait_done >> k & 1) std::printf("W%d ", k);
    if (W.gate_now) std::printf("G ");
    std::printf("| ");
}

int main() {
    auto ledger = std::make_unique<AheadLedger>();
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        long src, map, set;
        in >> cmd;
        AheadLedger& L = *ledger;
        if (cmd == "case") {
            ledger = std::make_unique<AheadLedger>();
            std::printf("\n");
            continue;
        } else if (cmd == "request") {
            in >> src >> map >> set;
            const cf_atmos_source s = source(in, src);
            int mode, defer;
            in >> mode >> defer;
            cf_exchange_fields out{};
            out.u = fake<double>(set);
            const AheadLedger::Booked B = L.request(s, map_of(map), out, mode, defer != 0);
            print_work(B.work);
            if (B.rec) std::printf("%d", L.index(B.rec));
            else std::printf("refused");
        } else if (cmd == "first" || cmd == "step") {
            in >> set >> src >> map;
            const cf_atmos_source s = source(in, src);
            if (cmd == "first") {
                const AheadLedger::FirstStep F = L.first_step_of_call(fake<double>(set), s, map_of(map));
                print_work(F.work);
                std::printf("%d", (int)F.needed);
            } else {
                const AheadLedger::Stepped S = L.step(fake<double>(set), s, map_of(map));
                print_work(S.work);
                std::printf("%d", (int)S.interpolate);
            }
        } else if (cmd == "leave_aux") {
            print_work(L.leave_aux());
        } else if (cmd == "leave_main") {
            int route;
            in >> set >> route;
            print_work(AheadLedger::Work{});
            if (const AheadLedger::Record* r = L.waiting_for_other_set(fake<double>(set))) {
                std::printf("%d", L.index(r));
                L.leave_main(r, (AheadLedger::Route)route);
            } else {
                std::printf("none");
            }
        } else if (cmd == "commit") {
            int slot;
            in >> slot;
            print_work(L.commit_slot(slot));
        } else if (cmd == "discard") {
            print_work(L.discard());
        } else {
            std::fprintf(stderr, "unknown command: %s\n", line.c_str());
            return 2;
        }
        const cf_prefetch_stats& c = L.stats();
        std::printf(" | %d %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %d ", c.pending, (unsigned long long)c.requests,
                    (unsigned long long)c.launched_aux, (unsigned long long)c.launched_tail, (unsigned long long)c.launched_merged,
                    (unsigned long long)c.launched_ice_tail, (unsigned long long)c.launched_own, (unsigned long long)c.consumed,
                    (unsigned long long)c.mismatched, (unsigned long long)c.voided, (unsigned long long)c.superseded,
                    (unsigned long long)c.discarded, (unsigned long long)c.step_interpolations, (int)L.any_left_on_main());
        for (int k = 0; k < 2; ++k) std::printf("%c", "FWAM"[L[k].state]);
        std::printf("\n");
    }
    return 0;
}
