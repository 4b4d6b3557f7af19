// Host check of K1's shared row term (cvx_proj_amd/csrc/apap_row_term.h): the predicate that decides whether a block shares
// the term, and the side table's indexing, walked over every block fill on the CPU.  Build and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cvx_proj_amd/csrc tools/row_term_check.cpp -o row_term_check && ./row_term_check
// 1. Blocks of 64 and 128 lanes (one tile, two tiles) holding 1 .. width cells (the lanes past the last cell repeat it, as
//    cell_vertex's clamp does), their vy laid out as one row, two rows with the change at every position, three rows with the
//    two changes at every pair of positions, and the patterns A B A (shares) and A C B (does not): the vote of the kernel -
//    row_is_shared on every lane's bit pattern against A (the first lane's) and B (row_second_value) - must be true exactly
//    when a memcmp of the bytes finds no third value.  The row values include +0.0 / -0.0, neighbours one ulp apart, NaNs of two payloads and inf.
// 2. The side table: the 128 owners of a chunk write every (keypoint, value) entry of their buffer exactly once, inside the
//    table; every (buffer, step, keypoint of the step, value) is read inside it, from the entry its keypoint's owner wrote.
//    The table is a heap block of exactly kRowBytes and is accessed through the byte offsets, so that AddressSanitizer sees a
//    stray one.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "apap_row_term.h"

using namespace apap;

static long long bits(double v) {
    long long b;
    std::memcpy(&b, &v, 8);
    return b;
}

static long checked = 0;

// `vy` of the block's cells (cells <= width); returns the kernel's vote and checks it against the bytes
static bool vote(const std::vector<double> &vy, int width) {
    const int cells = (int)vy.size();
    std::vector<double> lanes(width);
    for (int l = 0; l < width; ++l) lanes[l] = vy[l < cells ? l : cells - 1];     // cell_vertex's clamp
    std::vector<long long> lane_bits(width);
    for (int l = 0; l < width; ++l) lane_bits[l] = bits(lanes[l]);
    const long long a = lane_bits[0], b = row_second_value(lane_bits.data(), width);
    double bv;
    std::memcpy(&bv, &b, 8);
    std::vector<double> distinct;       // by memcmp
    for (int l = 0; l < width; ++l) {
        bool known = false;
        for (const double &d : distinct) known = known || std::memcmp(&d, &lanes[l], 8) == 0;
        if (!known) distinct.push_back(lanes[l]);
    }
    const bool bytes = distinct.size() <= 2;
    bool all = true;
    for (int l = 0; l < width; ++l) {
        all = all && row_is_shared(bits(lanes[l]), a, b);
        if (row_is_shared(bits(lanes[l]), a, b)) {      // the value a sharing cell reads is its own vy, bit for bit
            const double v = row_value(bits(lanes[l]), a) == 0 ? lanes[0] : bv;
            if (std::memcmp(&v, &lanes[l], 8) != 0) {
                std::fprintf(stderr, "row_value picks another value: lane %d of %d, %d cells\n", l, width, cells);
                std::exit(1);
            }
        }
    }
    if (all != bytes) {
        std::fprintf(stderr, "vote %d, bytes %d: width %d, %d cells\n", all, bytes, width, cells);
        std::exit(1);
    }
    ++checked;
    return all;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    double nan1 = std::numeric_limits<double>::quiet_NaN(), nan2;
    long long nb = bits(nan1) | 0x1234;
    std::memcpy(&nan2, &nb, 8);
    // triples (r0, r1, r2) of row values; all three pairwise different as BYTES
    const double rows[][3] = {{10.0, 20.0, 30.0},   {0.0, -0.0, 1.0},       {1.0, std::nextafter(1.0, 2.0), std::nextafter(1.0, 0.0)},
                              {nan1, nan2, 5.0},    {inf, -inf, nan1},      {-0.0, 0.0, nan2}};
    for (const auto &r : rows) {
        for (int width : {64, 128}) {
            for (int cells = 1; cells <= width; ++cells) {
                std::vector<double> vy(cells, r[0]);
                if (!vote(vy, width)) return 2;                                     // one row: A == B
                for (int p = 1; p < cells; ++p) {                                   // two rows, the change at p
                    for (int i = 0; i < cells; ++i) vy[i] = i < p ? r[0] : r[1];
                    if (!vote(vy, width)) return 3;
                    for (int q = p + 1; q < cells; ++q) {                           // three rows, changes at p and q: no sharing
                        for (int i = 0; i < cells; ++i) vy[i] = i < p ? r[0] : i < q ? r[2] : r[1];
                        if (vote(vy, width)) return 4;                              // A C B
                        for (int i = 0; i < cells; ++i) vy[i] = i < p ? r[0] : i < q ? r[1] : r[0];
                        if (!vote(vy, width)) return 5;                             // A B A
                    }
                }
            }
        }
    }

    // the side table
    unsigned char *table = static_cast<unsigned char *>(std::malloc(kRowBytes));
    for (int buffer = 0; buffer < 2; ++buffer) {
        std::memset(table, 0, kRowBytes);
        for (int t = 0; t < kRowOwners; ++t) {
            const int off = row_term_off(buffer, row_owner_keypoint(t), row_owner_value(t));
            if (off % 8 != 0) return 6;
            double tag;
            std::memcpy(&tag, table + off, 8);
            if (tag != 0.0) return 7;                               // written twice
            tag = 1000.0 + 2 * row_owner_keypoint(t) + row_owner_value(t);
            std::memcpy(table + off, &tag, 8);
        }
        for (int i = 0; i < kRowBytes / 2; i += 8) {                // every entry of this buffer, none of the other
            double own, other;
            std::memcpy(&own, table + buffer * (kRowBytes / 2) + i, 8);
            std::memcpy(&other, table + (1 - buffer) * (kRowBytes / 2) + i, 8);
            if (own == 0.0 || other != 0.0) return 8;
        }
        for (int step = 0; step < kRowChunk / 4; ++step)
            for (int kgrp = 0; kgrp < 4; ++kgrp)
                for (int value = 0; value < 2; ++value) {
                    double tag;
                    std::memcpy(&tag, table + row_read_off(buffer, step, kgrp, value), 8);
                    if (tag != 1000.0 + 2 * (4 * step + kgrp) + value) return 9;
                    ++checked;
                }
    }
    std::free(table);
    std::printf("row_term_check: ok (%ld block fills and reads)\n", checked);
    return 0;
}
