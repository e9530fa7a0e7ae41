// sc_oracle.cpp -- the scalar restatement of the scan-context contract (docs/SCAN_CONTEXT.md) that slam_kf_sc_* is held
// against: one point, one cell, one shift at a time, nothing shared with slam_amd/csrc/kf_sc.hip.  The mutation switches
// restate the contract wrongly on purpose, one decision each; tests/test_sc_oracle.py shows that every one of them changes
// a case of tests/sc_cases.py, i.e. that the cases reach the decision.
#include <cmath>
#include <cstdint>
#include <cstdlib>

enum {
    MUT_NONE = 0,
    MUT_RING_STRICT = 1,    // edge2[k] < r2: a point on a ring edge stays in the ring inside
    MUT_SECTOR_STRICT = 2,  // py c[k] > px s[k]: a point on a sector boundary stays in the sector before
    MUT_QUADRANT_TURN = 3,  // the second quadrant turned the wrong way: (px, py) = (-x, y)
    MUT_TIE_HIGHEST = 4,    // of equal distances the highest shift
    MUT_ROLL_DIRECTION = 5, // b[(c + s) mod S]
    MUT_H_NO_PLUS_ONE = 6   // h = the height bin itself: bin 0 reads as an empty cell
};

extern "C" {

// the tables from this translation unit's own libm
void sco_tables(int n_rings, int n_sectors, double max_range, double *edge2, double *c, double *sn)
{
    for (int k = 0; k < n_rings; ++k) {
        const double e = (k + 1) * (max_range / n_rings);
        edge2[k] = e * e;
    }
    for (int k = 0; k < n_sectors / 4; ++k) {
        c[k] = std::cos(2.0 * M_PI * k / n_sectors);
        sn[k] = std::sin(2.0 * M_PI * k / n_sectors);
    }
}

// out: n_rings * n_sectors bytes, ring-major
void sco_descriptor(const float *xyz, int n, int stride, int n_rings, int n_sectors, double z_min, double z_step, const double *edge2, const double *c,
                    const double *sn, int mutation, uint8_t *out)
{
    const double inv_step = 1.0 / z_step;
    const int    per = n_sectors / 4;
    for (int i = 0; i < n_rings * n_sectors; ++i) out[i] = 0;
    for (int i = 0; i < n; ++i) {
        const float x = xyz[(size_t)stride * i], y = xyz[(size_t)stride * i + 1], z = xyz[(size_t)stride * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) continue;
        const double r2 = (double)x * (double)x + (double)y * (double)y;
        int          ring = 0;
        for (int k = 0; k < n_rings; ++k)
            if (mutation == MUT_RING_STRICT ? edge2[k] < r2 : edge2[k] <= r2) ++ring;
        if (ring >= n_rings) continue;
        int sector;
        if (x == 0.0f && y == 0.0f)
            sector = 0;
        else {
            int   q;
            float px, py;
            if (x > 0 && y >= 0)
                q = 0, px = x, py = y;
            else if (x <= 0 && y > 0) {
                q = 1, px = y, py = -x;
                if (mutation == MUT_QUADRANT_TURN) px = -x, py = y;
            } else if (x < 0 && y <= 0)
                q = 2, px = -x, py = -y;
            else
                q = 3, px = -y, py = x;
            int j = 0;
            for (int k = 1; k < per; ++k) {
                const double l = (double)py * c[k], r = (double)px * sn[k];
                if (mutation == MUT_SECTOR_STRICT ? l > r : l >= r) ++j;
            }
            sector = q * per + j;
        }
        const double t = std::floor(((double)z - z_min) * inv_step);
        int          bin = t < 0.0 ? 0 : t > 254.0 ? 254 : (int)t;
        const int    h = mutation == MUT_H_NO_PLUS_ONE ? bin : 1 + bin;
        uint8_t     *cell = out + ring * n_sectors + sector;
        if (h > *cell) *cell = (uint8_t)h;
    }
}

// out: distance, shift, n_query, n_candidate, n_both
void sco_match(const uint8_t *a, const uint8_t *b, int n_rings, int n_sectors, int mutation, int *out)
{
    auto from = [&](int col, int s) { return mutation == MUT_ROLL_DIRECTION ? (col + s) % n_sectors : ((col - s) % n_sectors + n_sectors) % n_sectors; };
    long best = -1;
    int  best_s = 0;
    for (int s = 0; s < n_sectors; ++s) {
        long D = 0;
        for (int r = 0; r < n_rings; ++r)
            for (int col = 0; col < n_sectors; ++col) D += std::abs((int)a[r * n_sectors + col] - (int)b[r * n_sectors + from(col, s)]);
        if (best < 0 || D < best || (mutation == MUT_TIE_HIGHEST && D == best)) best = D, best_s = s;
    }
    int na = 0, nb = 0, both = 0;
    for (int r = 0; r < n_rings; ++r)
        for (int col = 0; col < n_sectors; ++col) {
            const int x = a[r * n_sectors + col], y = b[r * n_sectors + from(col, best_s)];
            na += x != 0, nb += y != 0, both += (x != 0 && y != 0);
        }
    out[0] = (int)best, out[1] = best_s, out[2] = na, out[3] = nb, out[4] = both;
}

} // extern "C"
