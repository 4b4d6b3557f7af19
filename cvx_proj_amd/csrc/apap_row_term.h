// K1's shared row term (k_assemble_mfma, float64 weights): which blocks share it, who writes which entry of the side table
// and who reads it.  Plain functions of integers, host and device, so that tools/row_term_check.cpp can walk every block fill
// on the CPU.
//
// The weight chain starts from x = fma(dx, dx, fma(dy, dy, 1e-300)) with dy = vy - sy.  The inner term depends on the keypoint
// and on the cell's vy alone, and the cells of a block lie on one or two mesh rows: a block whose every cell has the vy of its
// first cell (A) or the first other vy in cell order (B: on a mesh the last cell's) computes the term once per (keypoint, value) into
//     double s_row[2][kRowChunk][2]      [chunk buffer][keypoint of the chunk][0: A, 1: B]
// and its lanes read it from there.  Everything is decided on bit patterns: +0.0 and -0.0 are two values, a NaN is equal to
// itself, and no float compare takes part.
#pragma once

#if defined(__HIP__)
#define APAP_ROW_HD __host__ __device__
#else
#define APAP_ROW_HD
#endif

namespace apap {

constexpr int kRowChunk = 64;                   // keypoints per chunk buffer (k_assemble_mfma's kChunk)
constexpr int kRowOwners = 2 * kRowChunk;       // threads 0 .. 127 of the block write one entry each per chunk
constexpr int kRowBytes = 2 * kRowChunk * 2 * 8;

// B of a block whose cells (the clamped lanes of an overhang included) have these vy bits, bits[0] being A: the first that
// is not A, or A where there is none.  (The kernel finds it with a ballot per 64 cells; this is the rule it follows.)
APAP_ROW_HD constexpr long long row_second_value(const long long *bits, int n) {
    for (int i = 1; i < n; ++i)
        if (bits[i] != bits[0]) return bits[i];
    return bits[0];
}
// A cell with these vy bits can take its term from the table of a block with these A and B; the block shares the term when
// all its cells can.
APAP_ROW_HD constexpr bool row_is_shared(long long vy_bits, long long a_bits, long long b_bits) {
    return vy_bits == a_bits || vy_bits == b_bits;
}
// Which of the two values such a cell reads (A where A == B).
APAP_ROW_HD constexpr int row_value(long long vy_bits, long long a_bits) { return vy_bits == a_bits ? 0 : 1; }

// Byte offset of s_row[buffer][keypoint][value].
APAP_ROW_HD constexpr int row_term_off(int buffer, int keypoint, int value) { return (buffer * kRowChunk + keypoint) * 16 + value * 8; }
// The entry thread t < kRowOwners writes: keypoint t & 63 of the chunk, value t >> 6 (wave 0 writes A's terms, wave 1 B's).
APAP_ROW_HD constexpr int row_owner_keypoint(int t) { return t & (kRowChunk - 1); }
APAP_ROW_HD constexpr int row_owner_value(int t) { return t / kRowChunk; }
// The entry a lane reads at step `step` of a chunk (4 keypoints a step; kgrp = lane >> 4 is the lane's keypoint of the step):
// a per-lane constant, row_term_off(0, kgrp, value), plus the step's immediate.
constexpr int kRowStepBytes = 4 * 16;
APAP_ROW_HD constexpr int row_read_off(int buffer, int step, int kgrp, int value) {
    return row_term_off(buffer, 0, 0) + row_term_off(0, kgrp, value) + step * kRowStepBytes;
}

}  // namespace apap
