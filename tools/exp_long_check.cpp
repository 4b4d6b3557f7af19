// Host check of K1's long exp table and short weight chain (cvx_proj_amd/csrc/apap_exp_long.h): the table's layout, the
// equality of the two chains bit for bit wherever the short one may run, and the limit.  Build and run:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I cvx_proj_amd/csrc \
//       tools/exp_long_check.cpp -o exp_long_check && ./exp_long_check cvx_proj_amd/csrc/apap_kernels.hip
// The argument is the source that holds kExp2Tab: its 512 hexadecimal constants are read from the text, so the table checked
// is the one the kernels carry (without it: exp2(i / 512) of the C library, which the algebra below does not depend on).
// fract, fma, ldexp, the conversion and max are IEEE operations: the host's results are the device's.
// 1. The table, a heap block of exactly kExpLong doubles filled the way ExpTableStage::publish_long fills it (256 threads:
//    kExp2Tab[t] and kExp2Tab[256 + t] in place, one entry beyond per thread): every entry written exactly once, equal to
//    exp_long_entry, and for every j < kExpLong the entry of j, s[kExpLong - 1 - j], is twice
//    ldexp(kExp2Tab[(-j) & 511], (-j) >> 9), bit for bit.
// 2. The chains, for gamma2 in {0, 0.25, 0.81, the value whose limit lies just under a table boundary}: yu at every j, one
//    ulp below and above it, at the limit's neighbours, and 10^7 seeded values over [0, kExpLong).  Whenever yu < ylim the
//    full chain (mask, shift, ldexp, max) and the short one give the same 64 bits, and the product is above gamma2 strictly;
//    the first yu >= ylim - ylim itself - is never taken (the predicate is yu < ylim, and the limit is below the table's end
//    and below the yu where the clamp sets in).
// 3. The bound: random boxes of cells, cells inside them, keypoints and scales - whenever
//    (max(|x - x0|, |x - x1|)^2 + max(|y - y0|, |y - y1|)^2 + 1e-300) s^2 < ylim^2, the chain's own yu = sqrt(dx^2 + dy^2 +
//    1e-300) s, taken one part in 2^40 too large (the device's square root is within an ulp), is below ylim; NaN and infinite
//    keypoints, boxes and scales fail the compare.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "apap_exp_long.h"

using namespace apap;

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

static int fail(const char *what, double a = 0.0, double b = 0.0) {
    std::fprintf(stderr, "exp_long_check: %s (%a, %a)\n", what, a, b);
    return 1;
}

static std::vector<double> read_table(const char *path) {
    std::vector<double> T;
    if (!path) {
        for (int i = 0; i < kExpTabN; ++i) T.push_back(std::exp2((double)i / kExpTabN));
        return T;
    }
    std::ifstream in(path);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string text = ss.str();
    size_t at = text.find("kExp2Tab[kExpN] = {");
    if (at == std::string::npos) return T;
    const size_t end = text.find("};", at);
    at = text.find('{', at) + 1;
    while (at < end) {
        const size_t x = text.find("0x", at);
        if (x == std::string::npos || x >= end) break;
        char *stop = nullptr;
        T.push_back(std::strtod(text.c_str() + x, &stop));
        at = (size_t)(stop - text.c_str());
    }
    return T;
}

// the bound of k1_mfma_tiles' chunk_proved, operation for operation
static bool bound_passes(double x, double y, double x0, double x1, double y0, double y1, double k2, double lim) {
    const double ax = std::fmax(std::fabs(x - x0), std::fabs(x - x1));
    const double ay = std::fmax(std::fabs(y - y0), std::fabs(y - y1));
    const double d2 = std::fma(ax, ax, std::fma(ay, ay, 1e-300));
    return d2 * k2 < lim;
}

int main(int argc, char **argv) {
    const std::vector<double> T = read_table(argc > 1 ? argv[1] : nullptr);
    if ((int)T.size() != kExpTabN) return fail("kExp2Tab: 512 constants expected");
    for (int i = 0; i < kExpTabN; ++i)
        if (!(T[i] >= 1.0 && T[i] < 2.0) || (i && !(T[i] > T[i - 1]))) return fail("kExp2Tab: not increasing in [1, 2)", i, T[i]);
    if (std::fabs(T[256] - std::sqrt(2.0)) > 1e-15) return fail("kExp2Tab[256] is not sqrt(2)", T[256]);

    // 1. the table
    double *s = static_cast<double *>(std::malloc(kExpLong * sizeof(double)));
    std::vector<int> written(kExpLong, 0);
    for (int tid = 0; tid < 256; ++tid) {
        const double v[2] = {T[tid], T[tid + 256]};                     // ExpTableStage<256>::fetch
        for (int i = 0; i < 2; ++i) {                                   // publish(s + kExpLongZero, tid)
            s[kExpLongZero + ((tid + i * 256) & (kExpTabN - 1))] = v[i];
            ++written[kExpLongZero + ((tid + i * 256) & (kExpTabN - 1))];
        }
        if (tid == 0) s[kExpLong - 1] = 2.0, ++written[kExpLong - 1];
        else if (256 - tid <= kExpLongZero) s[kExpLongZero - (256 - tid)] = 0.5 * v[1], ++written[kExpLongZero - (256 - tid)];
    }
    for (int a = 0; a < kExpLong; ++a) {
        if (written[a] != 1) return fail("an entry of the long table is not written exactly once", a, written[a]);
        if (bits(s[a]) != bits(exp_long_entry(T.data(), a))) return fail("publish_long and exp_long_entry disagree", a, s[a]);
    }
    for (int j = 0; j < kExpLong; ++j) {
        const double tab3 = std::ldexp(T[(-j) & (kExpTabN - 1)], (-j) >> 9);
        if (bits(s[kExpLong - 1 - j]) != bits(2.0 * tab3)) return fail("the entry of j is not twice the ldexp form", j, s[kExpLong - 1 - j]);
        if (!(tab3 > 0.25 && tab3 <= 1.0)) return fail("tab3 outside (2^-2, 1]", j, tab3);
    }

    // 2. the chains
    double g_edge = std::exp2(-300.0 / (1.0 - 0x1p-20) / 512.0);        // its limit: the largest one below 300
    while (exp_long_limit(g_edge) >= 300.0) g_edge = std::nextafter(g_edge, 1.0);
    while (exp_long_limit(std::nextafter(g_edge, 0.0)) < 300.0) g_edge = std::nextafter(g_edge, 0.0);
    const double gammas[] = {0.0, 0.25, 0.81, g_edge};
    long compared = 0, refused = 0;
    for (double gamma2 : gammas) {
        const double ylim = exp_long_limit(gamma2);
        if (!(ylim > 0.0 && ylim < (double)kExpLong)) return fail("limit outside (0, kExpLong)", gamma2, ylim);
        if (gamma2 > 0.0 && !(ylim < -512.0 * std::log2(gamma2))) return fail("limit not below the clamp's yu", gamma2, ylim);
        auto one = [&](double yu) -> int {
            if (!(yu >= 0.0) || !(yu < ylim)) {     // the kernel's predicate: never taken
                ++refused;
                return 0;
            }
            const double full = exp_chain_full(yu, s, gamma2), brief = exp_chain_short(yu, s);
            if (bits(full) != bits(brief)) return fail("the chains differ", yu, gamma2);
            if (!(brief > gamma2)) return fail("the clamp is not idle strictly", yu, gamma2);
            ++compared;
            return 0;
        };
        for (int j = 0; j < kExpLong; ++j) {
            if (one((double)j) || one(std::nextafter((double)j, 1e9))) return 1;
            if (j && one(std::nextafter((double)j, 0.0))) return 1;
        }
        const long before = refused;
        if (one(std::nextafter(ylim, 0.0)) || refused != before) return fail("the last yu below the limit is not taken", ylim);
        if (one(ylim) || refused != before + 1) return fail("the limit itself is taken", ylim);
        if (one(std::nextafter(ylim, 1e9)) || refused != before + 2) return fail("a yu above the limit is taken", ylim);
        std::mt19937_64 rng(20240 + (uint64_t)(gamma2 * 1000));
        std::uniform_real_distribution<double> u(0.0, (double)kExpLong);
        for (long k = 0; k < 10000000; ++k)
            if (one(u(rng))) return 1;
    }
    if (bits(gammas[3]) == bits(0.0) || !(exp_long_limit(gammas[3]) > 299.99)) return fail("the edge gamma2", gammas[3], exp_long_limit(gammas[3]));
    // limits that are 0: the switch, gamma >= 1, a clamp too close to 1 for the margin, and what is no number
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double g : {1.0, 4.0, inf, nan, -1.0, std::nextafter(1.0, 0.0), 1.0 - 0x1p-30})
        if (exp_long_limit(g) != 0.0) return fail("a limit that should be 0", g, exp_long_limit(g));
    if (bits(exp_long_limit(0.0)) != bits((1.0 - 0x1p-20) * kExpLong)) return fail("the limit of gamma2 = 0");
    if (bits(exp_long_limit(0.25)) != bits((1.0 - 0x1p-20) * kExpLong)) return fail("the limit of gamma2 = 0.25 (the table's end)");

    // 3. the bound
    std::mt19937_64 rng(77);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    long bounded = 0, passed = 0;
    for (long k = 0; k < 2000000; ++k) {
        const double size = std::exp2(24.0 * u01(rng) - 8.0);           // boxes and offsets from 2^-8 to 2^16
        const double x0 = (u01(rng) - 0.5) * size, x1 = x0 + u01(rng) * size, y0 = (u01(rng) - 0.5) * size, y1 = y0 + u01(rng) * size;
        const double x = (u01(rng) - 0.5) * 3.0 * size, y = (u01(rng) - 0.5) * 3.0 * size;
        const double ylim = exp_long_limit(k % 3 == 0 ? 0.0 : k % 3 == 1 ? 0.25 : 0.81);
        const double scale = ylim / size * std::exp2(4.0 * u01(rng) - 2.0);
        const bool ok = bound_passes(x, y, x0, x1, y0, y1, scale * scale, ylim * ylim);
        passed += ok;
        for (int corner = 0; corner < 5 && ok; ++corner) {              // the four corners and a cell inside
            const double vx = corner == 4 ? x0 + u01(rng) * (x1 - x0) : (corner & 1) ? x1 : x0;
            const double vy = corner == 4 ? y0 + u01(rng) * (y1 - y0) : (corner & 2) ? y1 : y0;
            const double dx = vx - x, dy = vy - y;
            const double yu = std::sqrt(std::fma(dx, dx, std::fma(dy, dy, 1e-300))) * scale * (1.0 + 0x1p-40);
            if (!(yu < ylim)) return fail("the bound passes a keypoint whose yu reaches the limit", yu, ylim);
            ++bounded;
        }
    }
    if (passed < 100000 || passed > 1900000) return fail("the bound's sweep is one-sided", (double)passed);
    const double lim = exp_long_limit(0.25) * exp_long_limit(0.25);
    if (!bound_passes(1.0, 2.0, 0.0, 3.0, 0.0, 3.0, 1.0, lim)) return fail("a plain keypoint fails the bound");
    for (double bad : {nan, inf, -inf}) {
        if (bound_passes(bad, 2.0, 0.0, 3.0, 0.0, 3.0, 1.0, lim) || bound_passes(1.0, bad, 0.0, 3.0, 0.0, 3.0, 1.0, lim))
            return fail("a keypoint that is no finite number passes the bound", bad);
        if (bound_passes(1.0, 2.0, 0.0, 3.0, 0.0, 3.0, std::fabs(bad) /* the scale enters as a square */, lim) ||
            bound_passes(1.0, 2.0, 0.0, 3.0, 0.0, 3.0, 1.0, bad == inf ? nan : bad))
            return fail("a scale or limit that is no finite number passes the bound", bad);
        if (bound_passes(1.0, 2.0, bad, bad, 0.0, 3.0, 1.0, lim)) return fail("a box that is no finite number passes the bound", bad);
    }
    if (bound_passes(1.0, 2.0, 0.0, 3.0, 0.0, 3.0, 1.0, 0.0)) return fail("a limit of 0 passes");
    if (bound_passes(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e307, lim)) return fail("the 1e-300 of the chain is not in the bound");

    std::free(s);
    std::printf("exp_long_check: ok (%d entries, %ld chain pairs equal, %ld refused, %ld bounded distances)\n", kExpLong, compared,
                refused, bounded);
    return 0;
}
