// pf_tables_check.cpp -- slam_amd/csrc/pf_tables.hpp alone, as a program of its own: tests/test_pf_cases.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it.  Every table is allocated at exactly its size, so a write past
// either end is the sanitizer's to find; every refusal must leave its table untouched.  Prints "ok" and returns 0, or names the
// check that failed.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "pf_tables.hpp"

static int failures = 0;

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                \
        }                                                              \
    } while (0)

template <class T>
static bool untouched(const T *p, int n, T mark)
{
    for (int i = 0; i < n; ++i)
        if (std::memcmp(&p[i], &mark, sizeof(T)) != 0) return false;
    return true;
}

static double phi(double x) { return 0.5 * std::erfc(-x / std::sqrt(2.0)); }

int main()
{
    const char *why = nullptr;
    // ---- the angle table
    for (int A : {64, 4096, 65536}) {
        std::unique_ptr<double[]> cs(new double[2 * (size_t)A]);
        CHECK(slam::pf_angle_table(A, cs.get(), 2 * A, &why) == 0 && why[0] == 0);
        const int q = A / 4;
        CHECK(cs[0] == 1.0 && cs[1] == 0.0 && cs[2 * q] == 0.0 && cs[2 * q + 1] == 1.0);
        CHECK(cs[4 * q] == -1.0 && cs[4 * q + 1] == 0.0 && cs[6 * q] == 0.0 && cs[6 * q + 1] == -1.0);
        for (int k = 0; k < A; ++k) CHECK(std::fabs(cs[2 * k] * cs[2 * k] + cs[2 * k + 1] * cs[2 * k + 1] - 1.0) < 1e-15);
        CHECK(std::fabs(cs[2 * (A / 8)] - std::sqrt(0.5)) < 1e-15 && std::fabs(cs[2 * (A / 8) + 1] - std::sqrt(0.5)) < 1e-15);
    }
    for (int A : {0, -64, 32, 63, 65, 96, 131072, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
        double one[2] = {7.0, 7.0};
        CHECK(slam::pf_angle_table(A, one, 2, &why) == -1 && why[0] != 0 && untouched(one, 2, 7.0));
    }
    for (int off : {-1, 1}) { // a length off by one either way, the table allocated at that length
        const int                 n = 2 * 64 + off;
        std::unique_ptr<double[]> cs(new double[n]);
        for (int i = 0; i < n; ++i) cs[i] = 7.0;
        CHECK(slam::pf_angle_table(64, cs.get(), n, &why) == -1 && untouched(cs.get(), n, 7.0));
    }
    CHECK(slam::pf_angle_table(64, nullptr, 128, &why) == -1 && slam::pf_angle_table(64, nullptr, 128, nullptr) == -1);
    // ---- the Gaussian table
    for (int b : {4, 12, 16}) {
        const int                 N = 1 << b;
        std::unique_ptr<double[]> G(new double[N]);
        CHECK(slam::pf_gauss_table(b, G.get(), N, &why) == 0);
        double worst = 0.0;
        for (int i = 0; i < N; ++i) {
            CHECK(G[i] == -G[N - 1 - i] && std::isfinite(G[i]));
            CHECK(i == 0 || G[i] > G[i - 1]);
            const double e = std::fabs(phi(G[i]) - ((double)i + 0.5) / (double)N);
            worst = e > worst ? e : worst;
        }
        CHECK(worst <= 1e-12);
        CHECK(G[N / 2] > 0.0 && G[N - 1] < 6.0);
    }
    for (int b : {3, 17, 0, -1, 31, 32, 64, std::numeric_limits<int>::max()}) {
        double one[1] = {7.0};
        CHECK(slam::pf_gauss_table(b, one, 1, &why) == -1 && why[0] != 0 && untouched(one, 1, 7.0));
    }
    for (int off : {-1, 1}) {
        const int                 n = 16 + off;
        std::unique_ptr<double[]> G(new double[n]);
        for (int i = 0; i < n; ++i) G[i] = 7.0;
        CHECK(slam::pf_gauss_table(4, G.get(), n, &why) == -1 && untouched(G.get(), n, 7.0));
    }
    CHECK(slam::pf_gauss_table(4, nullptr, 16, &why) == -1);
    // ---- the weight table
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double scale : {1024.0, 1.0, DBL_MAX, DBL_MIN, 4.9406564584124654e-324, 1e-300, 1e300})
        for (int shift : {0, 4, 14})
            for (int L : {2, 3, 1024, 65536}) {
                std::unique_ptr<uint32_t[]> w(new uint32_t[L]);
                CHECK(slam::pf_weight_table(scale, shift, L, w.get(), &why) == 0);
                CHECK(w[0] == 65536u && slam::pf_weight_table_ok(w.get(), L));
                for (int j = 1; j < L; ++j) CHECK(w[j] <= w[j - 1]);
            }
    for (double scale : {0.0, -0.0, -1.0, inf, -inf, nan, -DBL_MAX}) {
        uint32_t w[2] = {7u, 7u};
        CHECK(slam::pf_weight_table(scale, 4, 2, w, &why) == -1 && why[0] != 0 && untouched(w, 2, 7u));
    }
    for (int shift : {-1, 15, 31, 32, 64}) {
        uint32_t w[2] = {7u, 7u};
        CHECK(slam::pf_weight_table(1024.0, shift, 2, w, &why) == -1 && untouched(w, 2, 7u));
    }
    for (int L : {1, 0, -5, 65537, std::numeric_limits<int>::max()}) {
        uint32_t w[1] = {7u};
        CHECK(slam::pf_weight_table(1024.0, 4, L, w, &why) == -1 && untouched(w, 1, 7u));
    }
    CHECK(slam::pf_weight_table(1024.0, 4, 2, nullptr, &why) == -1);
    {
        uint32_t good[3] = {65536u, 65536u, 0u}, high[3] = {65536u, 65537u, 0u}, low[3] = {65535u, 1u, 0u};
        CHECK(slam::pf_weight_table_ok(good, 3) && !slam::pf_weight_table_ok(high, 3) && !slam::pf_weight_table_ok(low, 3));
        CHECK(!slam::pf_weight_table_ok(nullptr, 3) && !slam::pf_weight_table_ok(good, 1));
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
