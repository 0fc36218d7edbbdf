// tile_geometry_driver.cpp — csrc/coflux_tile_geometry.hpp alone (plain C++, no HIP): tests/test_tile_world_cpu.py builds this with
// -fsanitize=address,undefined and compares what it prints with the Python statement of the same world.
//   world <px> <py> <rank> <tripolar> <nxl>  →  "refused" or "p q W E S N sideW sideE sideS sideN top partner"
//   note <max_fields> <max_rows> <max_cols> <sj> <ny> <hx> <hy>  →  "x_slot y_slot bytes offW offE offS offN", after writing the
//        first and the last double of both parities of every slot of a heap block of exactly `bytes` bytes
//   agree <side> <7 ints of mine> <7 ints of theirs>  →  0 or 1
// One command per line of standard input.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "coflux_tile_geometry.hpp"

using namespace coflux;

static TileNote read_note(std::istream& in) {
    TileNote n{};
    n.magic = TILE_MAGIC;
    in >> n.max_fields >> n.max_rows >> n.max_cols >> n.sj >> n.ny >> n.hx >> n.hy;
    return n;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "world") {
            int px, py, rank, tripolar, nxl;
            in >> px >> py >> rank >> tripolar >> nxl;
            char why[200];
            if (tile_world_refusal(px, py, rank, tripolar, nxl, why, sizeof why)) {
                std::cout << "refused\n";
                continue;
            }
            const TilePlace T = tile_place(px, py, rank, tripolar);
            std::cout << T.p << ' ' << T.q;
            for (int s = 0; s < 4; ++s) std::cout << ' ' << T.neighbour[s];
            for (int s = 0; s < 4; ++s) std::cout << ' ' << T.remote_side[s];
            std::cout << ' ' << T.top_row << ' ' << T.partner_north << '\n';
        } else if (what == "note") {
            const TileNote n = read_note(in);
            const size_t bytes = tile_mailbox_bytes(n);
            char* block = static_cast<char*>(std::malloc(bytes));
            std::memset(block, 0, TILE_DATA_OFFSET);
            std::memcpy(block + TILE_NOTE_OFFSET, &n, sizeof n);
            for (int s = 0; s < 4; ++s) {
                const size_t slot = s < TILE_S ? tile_x_slot(n) : tile_y_slot(n);
                double* first = reinterpret_cast<double*>(block + tile_slot_offset(n, s));
                for (int parity = 0; parity < 2; ++parity) {
                    first[(size_t)parity * slot] = 1.0 + s;
                    first[(size_t)parity * slot + slot - 1] = 2.0 + s;
                }
            }
            std::cout << tile_x_slot(n) << ' ' << tile_y_slot(n) << ' ' << bytes;
            for (int s = 0; s < 4; ++s) std::cout << ' ' << tile_slot_offset(n, s);
            std::cout << '\n';
            std::free(block);
        } else if (what == "agree") {
            int side;
            in >> side;
            const TileNote mine = read_note(in), theirs = read_note(in);
            char text[160];
            tile_note_text(theirs, text, sizeof text);
            std::cout << (tile_notes_agree(mine, theirs, side) ? 1 : 0) << ' ' << text << '\n';
        } else if (what == "columns") {
            int ring, sends_fold, west, east;
            in >> ring >> sends_fold;
            tile_phase_columns(ring, sends_fold != 0, &west, &east);
            std::cout << west << ' ' << east << '\n';
        } else {
            return 2;
        }
    }
    return 0;
}
