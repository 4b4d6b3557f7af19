// Host check of the image pyramid's two host-only entry points (cvx_proj_amd/csrc/apap_pyramid.hip): apap_pyramid_layout and
// apap_pyramid_level_caps against the definition of include/apap_hip.h "image pyramid", restated here, with the output arrays
// in heap blocks of exactly the size the header names, so that a sanitizer sees any write past them.  Touches no device.
// Build and run (the host side under the sanitizers; the kernels of the source are compiled but never launched):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all tools/pyramid_layout_check.cpp cvx_proj_amd/csrc/apap_pyramid.hip \
//       -o pyramid_layout_check && ./pyramid_layout_check
// Ranges: every pair of sides (s, s), (s, 32), (s, s + 37) for s = 32 .. 300, and 32768; n_levels 1 .. 16; both half_steps;
// max_corners 1 .. 300, 600, 2000, 2^31 - 1.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../include/apap_hip.h"

namespace apap {   // what the library's other sources define: the messages are not under test here
int fail(int code, const char *, ...) { return code; }
int hip_fail(int, const char *) { return APAP_ERR_HIP; }
}  // namespace apap

static long long checked = 0;

static void expect(bool ok, const char *what, int a, int b, int c, int d) {
    if (!ok) {
        std::fprintf(stderr, "FAILED %s at (%d, %d, %d, %d)\n", what, a, b, c, d);
        std::exit(1);
    }
    ++checked;
}

static void check_layout(int h, int w, int n_levels, int half) {
    // exactly n_levels (+ 1) entries each
    std::unique_ptr<int[]> hs(new int[n_levels]), ws(new int[n_levels]), num(new int[n_levels]), shift(new int[n_levels]);
    std::unique_ptr<long long[]> off(new long long[n_levels + 1]);
    const int n = apap_pyramid_layout(h, w, n_levels, half, hs.get(), ws.get(), off.get(), num.get(), shift.get());
    expect(n >= 1 && n <= n_levels, "count", h, w, n_levels, half);
    long long at = 0;
    int l = 0;
    for (; l < n_levels; ++l) {
        const bool odd = half && (l & 1);
        const int k = half ? l / 2 : l;
        int lh = odd ? (3 * h) / 4 : h, lw = odd ? (3 * w) / 4 : w;
        for (int i = 0; i < k; ++i) {
            lh = (lh + 1) / 2;
            lw = (lw + 1) / 2;
        }
        if (lh < APAP_PYRAMID_MIN_SIDE || lw < APAP_PYRAMID_MIN_SIDE) break;
        expect(l < n && hs[l] == lh && ws[l] == lw && off[l] == at && num[l] == (odd ? 3 : 1) && shift[l] == (odd ? k + 2 : k), "level", h, w,
               n_levels * 2 + half, l);
        at += ((long long)lh * lw + 255) / 256 * 256;
    }
    expect(l == n && off[n] == at, "end", h, w, n_levels, half);
    expect(apap_pyramid_layout(h, w, n_levels, half, nullptr, nullptr, nullptr, nullptr, nullptr) == n, "null outputs", h, w, n_levels, half);
}

static void check_caps(int max_corners, int n_levels, int half) {
    std::unique_ptr<int[]> caps(new int[n_levels]);
    expect(apap_pyramid_level_caps(max_corners, n_levels, half, caps.get()) == APAP_OK, "caps rc", max_corners, n_levels, half, 0);
    for (int l = 0; l < n_levels; ++l) {
        const bool odd = half && (l & 1);
        const int k = half ? l / 2 : l;
        long long share = odd ? 9ll * max_corners : (long long)max_corners;
        for (int i = 0; i < (odd ? 2 * k + 4 : 2 * k); ++i) share /= 2;
        long long want = share < 16 ? 16 : share;
        if (want > max_corners) want = max_corners;
        expect(caps[l] == (int)want, "cap", max_corners, n_levels, half, l);
    }
}

int main() {
    std::vector<int> sides;
    for (int s = 32; s <= 300; ++s) sides.push_back(s);
    sides.push_back(32768);
    for (int s : sides)
        for (int other : {s, 32, s == 32768 ? 32768 : s + 37})
            for (int half = 0; half < 2; ++half)
                for (int n_levels = 1; n_levels <= APAP_PYRAMID_MAX_LEVELS; ++n_levels) {
                    check_layout(s, other, n_levels, half);
                    check_layout(other, s, n_levels, half);
                }
    std::vector<int> corners;
    for (int c = 1; c <= 300; ++c) corners.push_back(c);
    for (int c : {600, 2000, 2147483647}) corners.push_back(c);
    for (int c : corners)
        for (int half = 0; half < 2; ++half)
            for (int n_levels = 1; n_levels <= APAP_PYRAMID_MAX_LEVELS; ++n_levels) check_caps(c, n_levels, half);
    // the refusals write nothing and return 0 / APAP_ERR_INVALID_ARG
    int one = 0;
    expect(apap_pyramid_layout(31, 100, 6, 1, &one, &one, nullptr, &one, &one) == 0 && one == 0, "small side", 31, 100, 6, 1);
    expect(apap_pyramid_layout(100, 32769, 6, 1, &one, &one, nullptr, &one, &one) == 0 && one == 0, "large side", 100, 32769, 6, 1);
    expect(apap_pyramid_layout(100, 100, 0, 1, &one, &one, nullptr, &one, &one) == 0, "no level", 100, 100, 0, 1);
    expect(apap_pyramid_layout(100, 100, 17, 1, &one, &one, nullptr, &one, &one) == 0, "too many levels", 100, 100, 17, 1);
    expect(apap_pyramid_level_caps(0, 6, 1, &one) == APAP_ERR_INVALID_ARG && one == 0, "no corner", 0, 6, 1, 0);
    expect(apap_pyramid_level_caps(10, 17, 1, &one) == APAP_ERR_INVALID_ARG && one == 0, "caps levels", 10, 17, 1, 0);
    expect(apap_pyramid_level_caps(10, 6, 1, nullptr) == APAP_ERR_INVALID_ARG, "caps null", 10, 6, 1, 0);
    std::printf("pyramid_layout_check: %lld checks passed\n", checked);
    return 0;
}
