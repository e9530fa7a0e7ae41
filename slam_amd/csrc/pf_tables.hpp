// pf_tables.hpp -- the three host-made tables of the particle filter (docs/PARTICLE_FILTER.md section 2): every value that a
// libm decides is computed here, on the host, and handed to the device and to the numpy restatement alike.  Plain C++: no HIP,
// no device, no library state, so that it can be compiled alone (tests/cpp/pf_tables_check.cpp runs it under the host
// sanitizers).  Each maker answers 0 with the table written, or -1 with nothing written and *why naming the refusal.
#pragma once
#include <cmath>
#include <cstdint>

namespace slam {

constexpr int kPfMinAngles = 1 << 6, kPfMaxAngles = 1 << 16; // A: a power of two
constexpr int kPfMinGaussBits = 4, kPfMaxGaussBits = 16;     // b
constexpr int kPfMaxWeightLen = 1 << 16, kPfMaxWeightShift = 14; // (L - 1) << shift stays below 2^30
constexpr uint32_t kPfWeightOne = 65536;                     // 16.16 fixed point

// cs[2 k], cs[2 k + 1] = cos, sin(2 pi k / A), n = 2 A doubles; the four quadrant entries are exactly (+-1, 0), (0, +-1)
inline int pf_angle_table(int n_angles, double *cs, int n, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!cs) return *why = "null table", -1;
    if (n_angles < kPfMinAngles || n_angles > kPfMaxAngles || (n_angles & (n_angles - 1)))
        return *why = "n_angles must be a power of two from 2^6 to 2^16", -1;
    if (n != 2 * n_angles) return *why = "the table has 2 n_angles entries", -1;
    const int    A = n_angles;
    const double step = (2.0 * 3.14159265358979323846) / (double)A;
    for (int k = 0; k < A; ++k) cs[2 * k] = std::cos(step * (double)k), cs[2 * k + 1] = std::sin(step * (double)k);
    const int q = A / 4;
    cs[0] = 1.0, cs[1] = 0.0;
    cs[2 * q] = 0.0, cs[2 * q + 1] = 1.0;
    cs[4 * q] = -1.0, cs[4 * q + 1] = 0.0;
    cs[6 * q] = 0.0, cs[6 * q + 1] = -1.0;
    return 0;
}

// G[i] = Phi^-1((i + 1/2) / 2^b), n = 2^b doubles.  The upper half is found by Newton's iteration on the upper tail
// Q(x) = erfc(x / sqrt 2) / 2 = (2^b - i - 1/2) / 2^b, a dyadic number that a double holds exactly: Q is convex there and the
// start 0 lies left of the root, so the iterates rise to it without overshoot.  The lower half is the upper one negated, entry
// for entry: G[i] == -G[2^b - 1 - i] exactly.
inline int pf_gauss_table(int bits, double *G, int n, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!G) return *why = "null table", -1;
    if (bits < kPfMinGaussBits || bits > kPfMaxGaussBits) return *why = "gauss_bits must be 4..16", -1;
    const int N = 1 << bits;
    if (n != N) return *why = "the table has 2^gauss_bits entries", -1;
    const double inv_sqrt2 = 0.70710678118654752440, inv_sqrt_2pi = 0.39894228040143267794;
    for (int i = N / 2; i < N; ++i) {
        const double q = ((double)(N - i) - 0.5) / (double)N; // the upper tail's mass, in (0, 1/2)
        double       x = 0.0;
        for (int it = 0; it < 200; ++it) {
            const double f = 0.5 * std::erfc(x * inv_sqrt2) - q;          // > 0 left of the root
            const double d = f / (inv_sqrt_2pi * std::exp(-0.5 * x * x)); // Newton's step, -f / Q'
            const double nx = x + d;
            if (!(nx > x)) break; // the step no longer moves x (or turned back in the last place)
            x = nx;
        }
        G[i] = x;
        G[N - 1 - i] = -x;
    }
    return 0;
}

// wtab[j] = (uint32_t)rint(65536 exp(-(double)(j << shift) / scale)), j < L: wtab[0] == 65536 and no entry above it.
// scale must be positive and finite (a zero, negative or NaN scale has no quotient at j = 0; an infinite one has no decay).
inline int pf_weight_table(double scale, int shift, int L, uint32_t *wtab, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!wtab) return *why = "null table", -1;
    if (L < 2 || L > kPfMaxWeightLen) return *why = "weight_len must be 2..65536", -1;
    if (shift < 0 || shift > kPfMaxWeightShift) return *why = "weight_shift must be 0..14", -1;
    if (!std::isfinite(scale) || !(scale > 0.0)) return *why = "weight_scale must be positive and finite", -1;
    for (int j = 0; j < L; ++j) {
        const double d = (double)((int64_t)j << shift);
        const double v = std::rint(65536.0 * std::exp(-d / scale)); // in [0, 65536]: d / scale >= 0 (or +inf), never NaN
        wtab[j] = v >= 65536.0 ? kPfWeightOne : (uint32_t)v;
    }
    return 0;
}

// what slam_pf_set_tables asks of a weight table given from outside
inline bool pf_weight_table_ok(const uint32_t *wtab, int L)
{
    if (!wtab || L < 2 || L > kPfMaxWeightLen || wtab[0] != kPfWeightOne) return false;
    for (int j = 0; j < L; ++j)
        if (wtab[j] > kPfWeightOne) return false;
    return true;
}

} // namespace slam
