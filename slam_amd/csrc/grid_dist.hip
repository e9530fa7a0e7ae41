// grid_dist.hip -- exact squared distance to the nearest obstacle cell of an occupancy plane, capped at R cells, and the
// inflated costmap read off it through a byte table (docs/GRID_DIST.md).  The reference has no counterpart (MLS's robot_size
// only sets a height): the definition is the brute-force restatement of tests/grid_dist_cases.py, and the planes are held to it
// bit for bit.  All integer on the device; the only floating point is the host's table (grid_cost_table.hpp).
//
// Two kernels, both over WINDOW-order planes data[x + size_x * y]:
//   gdist_rows_kernel   one workgroup per row.  The row's obstacle bits, 64 cells per word by wave ballot, go to LDS (at most
//                       512 words); then every cell finds its nearest obstacle of the row from those words by count-leading /
//                       count-trailing zeros over its own word and at most ceil(R / 64) + 1 words on each side: g(x, y) =
//                       min |x - x'| capped at R + 1, one byte, in a plane whose rows are padded to whole words (64-byte rows,
//                       so a tile row below is one aligned line).  Beside it two bytes per (row, word): does any cell of the
//                       word have g <= R, and the largest g of the word's cells.
//   gdist_cols_kernel   one workgroup per tile of 64 columns x kTileH rows, lanes along x.  LDS has room for the tile's g with R
//                       rows of halo above and below ((kTileH + 2R) x 64 bytes), but the halo is filled only as far as the
//                       tile's largest row distances make any cell look (best <= g^2); rows outside the plane, and rows none
//                       of whose cells has an obstacle within R, enter as R + 1 without a load.  Every cell walks dy = 0, +-1,
//                       +-2 ... with best = min(best, g(x, y +- dy)^2 + dy^2) from best = R^2 + 1 until dy^2 >= best: nothing
//                       further out can be nearer, so the stop is exact.  A tile all of whose rows are such rows writes FAR
//                       without loading anything.  The cost byte is looked up in the table (global memory, at most 64 518
//                       bytes) in the same pass.
// Nothing wraps: a row's words end at the window's edge and the rows beyond the plane hold R + 1.
#include <memory>

#include "device_mem.hpp"
#include "grid_cost_table.hpp"
#include "grid_dist.hpp"

using namespace slam;

namespace {

constexpr int kTileH = 128;     // rows of a column tile (tests/grid_dist_cases.py names it: TILE_H)
constexpr int kMaxWords = 512;  // 64-cell words of a row: size_x <= 32767

__global__ __launch_bounds__(256) void gdist_rows_kernel(const int8_t *occ, int sx, int n_words, int R, int unknown_is_obstacle,
                                                         uint8_t *g, uint8_t *row_meta)
{
    __shared__ unsigned long long words[kMaxWords];
    const int     y = blockIdx.x, pitch = n_words * 64;
    const int8_t *row = occ + (size_t)sx * y;
    // (pitch is a multiple of 64 and the stride one of 64: the lanes of a wavefront stay on one word and leave the loop together)
    for (int x = threadIdx.x; x < pitch; x += 256) {
        bool obstacle = false;
        if (x < sx) {
            const int8_t o = row[x];
            obstacle = o == 100 || (unknown_is_obstacle && o == -1);
        }
        const unsigned long long m = __ballot(obstacle); // cells at and beyond size_x: no bit
        if ((threadIdx.x & 63) == 0) words[x >> 6] = m;
    }
    __syncthreads();
    const int reach = (R + 63) / 64 + 1; // an obstacle j words away is at least 64 j - 63 cells away
    for (int x = threadIdx.x; x < pitch; x += 256) {
        const int                w = x >> 6, b = x & 63;
        const unsigned long long cur = words[w];
        int                      dl = R + 1, dr = R + 1;
        const unsigned long long ml = cur & (~0ull >> (63 - b)); // bits 0 .. b: this cell and those to its left
        if (ml) {
            dl = b - (63 - __clzll((long long)ml));
        } else {
            for (int j = 1; j <= reach && w - j >= 0; ++j) {
                const unsigned long long v = words[w - j];
                if (v) {
                    dl = x - (64 * (w - j) + 63 - __clzll((long long)v));
                    break;
                }
            }
        }
        const unsigned long long mr = cur & (~0ull << b); // bits b .. 63
        if (mr) {
            dr = (__ffsll((long long)mr) - 1) - b;
        } else {
            for (int j = 1; j <= reach && w + j < n_words; ++j) {
                const unsigned long long v = words[w + j];
                if (v) {
                    dr = 64 * (w + j) + (__ffsll((long long)v) - 1) - x;
                    break;
                }
            }
        }
        int d = min(min(dl, dr), R + 1);
        if (x >= sx) d = R + 1; // the padding of the last word
        g[(size_t)y * pitch + x] = (uint8_t)d;
        const unsigned long long near = __ballot(d <= R);
        int                      gmax = x < sx ? d : 0; // the largest row distance of the word's cells
        for (int off = 32; off > 0; off >>= 1) gmax = max(gmax, __shfl_xor(gmax, off));
        if ((threadIdx.x & 63) == 0) {
            row_meta[((size_t)y * n_words + w) * 2] = near ? 1 : 0;
            row_meta[((size_t)y * n_words + w) * 2 + 1] = (uint8_t)gmax;
        }
    }
}

struct CostRule {
    const uint8_t *table;  // [R * R + 2], null: no cost plane
    const int8_t  *occ;
    int            unknown_is_obstacle, unknown_cost, unknown_keep_from;
};

__global__ __launch_bounds__(256) void gdist_cols_kernel(const uint8_t *g, const uint8_t *row_meta, int sx, int sy, int n_words, int R,
                                                         CostRule rule, uint16_t *dist2, uint8_t *cost)
{
    extern __shared__ uint32_t tile32[]; // [(kTileH + 2R) * 16]: row r of the tile is plane row y0 - R + r
    __shared__ int s_need[2];
    const int      w = blockIdx.x, y0 = blockIdx.y * kTileH, pitch = n_words * 64;
    const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned far2 = (unsigned)(R * R + 1);
    if (threadIdx.x < 2) s_need[threadIdx.x] = 0;
    __syncthreads();
    // How far beyond the tile its cells look.  A cell's answer is at most its own row distance squared, so no cell of a row
    // whose largest row distance is gmax <= R looks gmax or more rows away; a row with a cell that has no obstacle within R in
    // its row looks R rows away (best starts at R^2 + 1).
    for (int c = threadIdx.x; c < kTileH; c += 256) {
        const int y = y0 + c;
        if (y < sy) {
            const int reach = min((int)row_meta[((size_t)y * n_words + w) * 2 + 1], R + 1) - 1;
            atomicMax(&s_need[0], reach - c);                // rows above the tile
            atomicMax(&s_need[1], reach - (kTileH - 1 - c)); // rows below it
        }
    }
    __syncthreads();
    const int r_lo = R - s_need[0], r_hi = R + kTileH + s_need[1]; // 0 <= r_lo, r_hi <= kTileH + 2R: reach <= R
    // the rows [r_lo, r_hi) of the tile: rows outside the plane, and rows none of whose cells has an obstacle within R (their
    // g is R + 1 throughout), enter as R + 1 without a load; when every row is such a row nothing is loaded and all is FAR
    int any = 0;
    for (int r = r_lo + (int)threadIdx.x; r < r_hi; r += 256) {
        const int yy = y0 - R + r;
        if (yy >= 0 && yy < sy) any |= row_meta[((size_t)yy * n_words + w) * 2];
    }
    any = __syncthreads_or(any);
    if (any) {
        for (int i = r_lo * 16 + (int)threadIdx.x; i < r_hi * 16; i += 256) {
            const int yy = y0 - R + (i >> 4);
            uint32_t  v = (uint32_t)(R + 1) * 0x01010101u;
            if (yy >= 0 && yy < sy && row_meta[((size_t)yy * n_words + w) * 2])
                v = *reinterpret_cast<const uint32_t *>(g + (size_t)yy * pitch + (size_t)w * 64 + 4 * (i & 15));
            tile32[i] = v;
        }
        __syncthreads();
    }
    const uint8_t *tile = reinterpret_cast<const uint8_t *>(tile32);
    const int      x = w * 64 + lane, y_end = min(y0 + kTileH, sy);
    for (int y = y0 + wave; y < y_end; y += 4) {
        unsigned best = x < sx ? far2 : 0; // (the padding lanes of the last word do not walk)
        if (any) {
            // dy = 0, +-1, +-2 ... until dy^2 >= best: nothing further out can be nearer, so the stop is exact.  It comes at
            // dy <= min(g0, R + 1) - 1, this row's reach at most: rows r_lo .. r_hi - 1 only.
            const int      c = R + (y - y0);
            const unsigned g0 = tile[c * 64 + lane];
            best = min(best, g0 * g0);
            for (unsigned dy = 1; dy * dy < best; ++dy) {
                const unsigned a = tile[(c - (int)dy) * 64 + lane], b = tile[(c + (int)dy) * 64 + lane];
                const unsigned m = min(a, b);
                best = min(best, m * m + dy * dy);
            }
        }
        if (x < sx) {
            const size_t i = (size_t)y * sx + x;
            dist2[i] = best < far2 ? (uint16_t)best : (uint16_t)SLAM_GDIST_FAR;
            if (rule.table) {
                int c8 = rule.table[best]; // best <= R^2 + 1: the last entry answers FAR
                if (!rule.unknown_is_obstacle && rule.occ[i] == -1 && c8 < rule.unknown_keep_from) c8 = rule.unknown_cost;
                cost[i] = (uint8_t)c8;
            }
        }
    }
}

} // namespace

struct slam_gdist {
    slam_gdist_params prm;
    int               sx = 0, sy = 0, n_words = 0;
    size_t            cells = 0;
    OwnedArray<uint8_t>  d_g;       // [sy][n_words * 64] row distances
    OwnedArray<uint8_t>  d_row_meta; // [sy][n_words][2]: any cell with an obstacle within R in its row; the largest row distance
    OwnedArray<uint16_t> d_dist2;   // [cells]
    OwnedArray<uint8_t>  d_cost;    // [cells]
    OwnedArray<uint8_t>  d_table;   // [R * R + 2]
    OwnedArray<int8_t>   d_occ;     // [cells] staging of slam_gdist_compute
    bool has_table = false, computed = false, cost_computed = false;
};

namespace slam {

void gdist_size(const slam_gdist *h, int *size_x, int *size_y)
{
    *size_x = h->sx;
    *size_y = h->sy;
}

int gdist_compute_on(slam_gdist *h, const int8_t *d_occ, hipStream_t st)
{
    const int R = h->prm.max_cells;
    hipLaunchKernelGGL(gdist_rows_kernel, dim3(h->sy), dim3(256), 0, st, d_occ, h->sx, h->n_words, R, h->prm.unknown_is_obstacle ? 1 : 0,
                       h->d_g.get(), h->d_row_meta.get());
    CostRule rule;
    rule.table = h->has_table ? h->d_table.get() : nullptr;
    rule.occ = d_occ;
    rule.unknown_is_obstacle = h->prm.unknown_is_obstacle ? 1 : 0;
    rule.unknown_cost = h->prm.unknown_cost;
    rule.unknown_keep_from = h->prm.unknown_keep_from;
    const size_t lds = (size_t)(kTileH + 2 * R) * 64;
    hipLaunchKernelGGL(gdist_cols_kernel, dim3(h->n_words, (h->sy + kTileH - 1) / kTileH), dim3(256), lds, st, h->d_g.get(),
                       h->d_row_meta.get(), h->sx, h->sy, h->n_words, R, rule, h->d_dist2.get(), h->d_cost.get());
    SLAM_HIP(hipGetLastError());
    h->computed = true;
    h->cost_computed = h->has_table;
    return SLAM_OK;
}

} // namespace slam

extern "C" {

void slam_gdist_default_params(slam_gdist_params *p)
{
    if (!p) return;
    p->max_cells = 32; // a starting value, not tuned
    p->unknown_is_obstacle = 0;
    p->unknown_cost = 255;      // costmap_2d NO_INFORMATION
    p->unknown_keep_from = 253; // costmap_2d INSCRIBED_INFLATED_OBSTACLE
}

int slam_grid_inflation_table(double resolution, double inscribed_radius, double inflation_radius, double cost_scaling, int max_cells,
                              uint8_t *table, int n)
{
    const char *why = "";
    if (grid_inflation_table(resolution, inscribed_radius, inflation_radius, cost_scaling, max_cells, table, n, &why) != 0) {
        set_error("slam_grid_inflation_table: %s", why);
        return SLAM_E_INVALID;
    }
    return SLAM_OK;
}

int slam_grid_likelihood_table(double resolution, double sigma, int max_cells, uint8_t *table, int n)
{
    const char *why = "";
    if (grid_likelihood_table(resolution, sigma, max_cells, table, n, &why) != 0) {
        set_error("slam_grid_likelihood_table: %s", why);
        return SLAM_E_INVALID;
    }
    return SLAM_OK;
}

int slam_gdist_create(int size_x, int size_y, const slam_gdist_params *p, slam_gdist_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_gdist_create: null out pointer");
    slam_gdist_params prm;
    if (p)
        prm = *p;
    else
        slam_gdist_default_params(&prm);
    SLAM_REQUIRE(size_x > 0 && size_y > 0 && size_x <= 32767 && size_y <= 32767, SLAM_E_INVALID,
                 "slam_gdist_create: size must be 1..32767 cells");
    SLAM_REQUIRE(prm.max_cells >= 1 && prm.max_cells <= kGdistMaxCells, SLAM_E_INVALID, "slam_gdist_create: max_cells must be 1..254");
    SLAM_REQUIRE(prm.unknown_cost >= 0 && prm.unknown_cost <= 255 && prm.unknown_keep_from >= 0 && prm.unknown_keep_from <= 255,
                 SLAM_E_INVALID, "slam_gdist_create: unknown_cost and unknown_keep_from must be 0..255");
    *out = nullptr;
    SLAM_TRY(require_device());
    std::unique_ptr<slam_gdist> h(new (std::nothrow) slam_gdist());
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_gdist_create: out of host memory");
    h->prm = prm;
    h->sx = size_x;
    h->sy = size_y;
    h->n_words = (size_x + 63) / 64;
    h->cells = (size_t)size_x * size_y;
    const int R = prm.max_cells;
    SLAM_TRY(h->d_g.alloc((size_t)h->n_words * 64 * size_y));
    SLAM_TRY(h->d_row_meta.alloc((size_t)h->n_words * size_y * 2));
    SLAM_TRY(h->d_dist2.alloc(h->cells * sizeof(uint16_t)));
    SLAM_TRY(h->d_cost.alloc(h->cells));
    SLAM_TRY(h->d_table.alloc((size_t)R * R + 2));
    SLAM_TRY(h->d_occ.alloc(h->cells));
    *out = h.release();
    return SLAM_OK;
}

void slam_gdist_destroy(slam_gdist_t *h) { delete h; } // (the frees wait for the device)

int slam_gdist_set_table(slam_gdist_t *h, const uint8_t *table, int n)
{
    SLAM_REQUIRE(h, SLAM_E_INVALID, "slam_gdist_set_table: null handle");
    if (!table && n == 0) {
        h->has_table = false;
        h->cost_computed = false;
        return SLAM_OK;
    }
    const int R = h->prm.max_cells;
    SLAM_REQUIRE(table && n == R * R + 2, SLAM_E_INVALID, "slam_gdist_set_table: the table has max_cells * max_cells + 2 = %d bytes, not %d",
                 R * R + 2, n);
    SLAM_HIP(hipDeviceSynchronize()); // a compute still in flight reads the old table
    SLAM_HIP(hipMemcpy(h->d_table.get(), table, (size_t)n, hipMemcpyHostToDevice));
    h->has_table = true;
    h->cost_computed = false; // the cost plane belongs to the table it was computed with
    return SLAM_OK;
}

int slam_gdist_compute_dev(slam_gdist_t *h, const int8_t *d_occ, slam_stream_t stream)
{
    SLAM_REQUIRE(h && d_occ, SLAM_E_INVALID, "slam_gdist_compute_dev: bad arguments");
    return gdist_compute_on(h, d_occ, as_stream(stream));
}

int slam_gdist_compute(slam_gdist_t *h, const int8_t *occ)
{
    SLAM_REQUIRE(h && occ, SLAM_E_INVALID, "slam_gdist_compute: bad arguments");
    SLAM_HIP(hipMemcpy(h->d_occ.get(), occ, h->cells, hipMemcpyHostToDevice));
    SLAM_TRY(gdist_compute_on(h, h->d_occ.get(), nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_gdist_read(slam_gdist_t *h, uint16_t *dist2, uint8_t *cost)
{
    SLAM_REQUIRE(h && (dist2 || cost), SLAM_E_INVALID, "slam_gdist_read: bad arguments");
    SLAM_REQUIRE(!cost || h->has_table, SLAM_E_INVALID, "slam_gdist_read: no cost plane without a table (slam_gdist_set_table)");
    SLAM_REQUIRE(h->computed, SLAM_E_INVALID, "slam_gdist_read: nothing has been computed");
    SLAM_REQUIRE(!cost || h->cost_computed, SLAM_E_INVALID, "slam_gdist_read: the table was set after the last compute");
    SLAM_HIP(hipDeviceSynchronize()); // whichever stream the last compute went to
    if (dist2) SLAM_HIP(hipMemcpy(dist2, h->d_dist2.get(), h->cells * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (cost) SLAM_HIP(hipMemcpy(cost, h->d_cost.get(), h->cells, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_gdist_planes_dev(slam_gdist_t *h, uint16_t **d_dist2, uint8_t **d_cost)
{
    SLAM_REQUIRE(h, SLAM_E_INVALID, "slam_gdist_planes_dev: null handle");
    if (d_dist2) *d_dist2 = h->d_dist2.get();
    if (d_cost) *d_cost = h->has_table ? h->d_cost.get() : nullptr;
    return SLAM_OK;
}

} // extern "C"
