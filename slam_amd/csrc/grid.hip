// grid.hip -- occupancy-grid update on gfx950 behind the C-ABI.
//
// Reference path (under /root/reference/mls):
//   MLS::addToOccupancy  src/mls.cpp:59-150   endpoint binning: obstacle +1.0, ground -0.3
//   Grid::operator()     include/mls/mls.h:76-85   toroidal wrap
//   MLS::setPose         src/mls.cpp:408-479  rolling window
// plus the north-star Bresenham free-space traversal, which the reference does
// not have; its definition is oracle/slam_oracle.c
// ogrid_raycast and the closed form in bres_y() below.
//
// Data layout in HBM (DESIGN.md "Grid"): two int32 planes [hits | misses] of
// size_x*size_y cells each, contiguous (one RCCL all-reduce merges both), in
// toroidal STORAGE order; a f64 evidence plane (Cluster::num_pts) and an int8
// occupancy plane derived from the counts by finalize.  The reference's
// per-cell `Cell` object (vector<Cluster> + deque, mls.h:37-51) is not
// reproduced: in occupancy mode only clusters[0].num_pts and `drivable` are
// ever touched.
//
// Here: endpoints, finalize, fold, roll, the in-order mode, the handle and the C-ABI.  The raycast's device code is
// grid_raycast.hpp, the row ranges grid_rows.hpp, what every kernel is handed grid_view.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "device_mem.hpp"
#include "grid_dist.hpp"
#include "grid_raycast.hpp"
#include "grid_view.hpp"

using namespace slam;

namespace {

// ------------------------------------------------------------- endpoints
// MLS::addToOccupancy's two loops (mls.cpp:73-106 obstacle points, :110-142 ground points) as counts: one workgroup takes
// kEndpointsPerBlock consecutive points, lanes take consecutive points (coalesced, and runs of equal cells stay inside a
// wavefront).  The rows it touched and the number of points it accepted leave the workgroup ONCE: the range words and the
// update counter are single addresses, and same-address atomics retire one at a time (11 ns each) -- with one pair per
// wavefront, the thousands of wavefronts that start together right after a reset (range empty: every one of them widens
// it) cost 70 us on config 2's 276 k endpoints, four times the kernel's own work (round 4, bench.py's endpoint leg).
constexpr int kEndpointsPerBlock = 1024;

__global__ __launch_bounds__(256) void endpoints_kernel(GridView g, const float *obs, int n_obs,
                                                        const float *gnd, int n_gnd, int stride)
{
    __shared__ int      s_lo[4], s_nhi[4];
    __shared__ unsigned s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int       lo = kNoRow, nhi = kNoRow; // lowest row, minus the highest
    unsigned  cnt = 0;
#pragma unroll
    for (int k = 0; k < kEndpointsPerBlock / 256; ++k) {
        const int i = blockIdx.x * kEndpointsPerBlock + k * 256 + (int)threadIdx.x;
        bool      did = false;
        int       key = -1;
        if (i < n_obs + n_gnd) {
            const bool   is_obs = i < n_obs;
            const float *p = is_obs ? obs + (size_t)i * stride : gnd + (size_t)(i - n_obs) * stride;
            int cx, cy;
            if (point_cell(g, p[0], p[1], &cx, &cy)) {
                const int s = storage_index(g, cx, cy), row = s / g.sx;
                did = true;
                key = (is_obs ? 0 : g.sx * g.sy) + s; // word of [hits | misses] this point counts in
                lo = min(lo, row);
                nhi = min(nhi, -row);
                ++cnt;
            }
        }
        // Consecutive points of a scan or of a lidar ring fall into the same cell in runs (beams 0.25 degrees apart are
        // centimetres apart at the wall): the first lane of a run adds the run's length, one atomic per run instead of one
        // per point (mls.cpp:99 / :135 as counts: integer sums, any grouping gives the same planes).
        const int                prev = __shfl_up(key, 1);
        const bool               head = did && (lane == 0 || prev != key);
        const unsigned long long heads = __ballot(head || !did); // a dropped point ends a run too
        if (head) {
            const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
            const int                len = after ? __builtin_ctzll(after) + 1 : 64 - lane;
            atomicAdd(&g.hits[key], len);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        nhi = min(nhi, __shfl_xor(nhi, off));
        cnt += (unsigned)__shfl_xor((int)cnt, off);
    }
    if (lane == 0) s_lo[wave] = lo, s_nhi[wave] = nhi, s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
        nhi = min(min(s_nhi[0], s_nhi[1]), min(s_nhi[2], s_nhi[3]));
        cnt = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (lo != kNoRow) rows_widen_touched(g.dirty, lo, nhi);
        if (cnt) atomicAdd(&g.updates[(blockIdx.x * 7u + blockIdx.y * 7919u) & (kUpdateSlots - 1)], (unsigned long long)cnt);
    }
}

// --------------------------------------------------------------- row ranges
// (grid_rows.hpp: what the touched and the changed rows are, and every transition of the two)

// (a fixed launch whose workgroups stride over the rows of the range: sizing the launch for the whole grid and leaving
// the rows outside the range to empty workgroups cost as much as the memset it replaces -- 16 000 empty workgroups, 9 us)
constexpr int kRangeBlocks = 1024;

__global__ __launch_bounds__(256) void reset_rows_kernel(int32_t *planes, size_t cells, int sx, int sy, const RowRanges *ranges)
{
    int lo, hi;
    rows_touched(*ranges, sy, &lo, &hi);
    if (hi < lo) return;
    const int  per_row = (sx + 1023) / 1024; // 256 threads x 4 ints
    const long items = (long)(hi - lo + 1) * per_row;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const int row = lo + (int)(it / per_row), x = ((int)(it % per_row) * 256 + threadIdx.x) * 4;
        for (int k = 0; k < 4; ++k)
            if (x + k < sx) {
                planes[(size_t)row * sx + x + k] = 0;
                planes[cells + (size_t)row * sx + x + k] = 0;
            }
    }
}

// One transition of the ranges, by one thread.  (A launch of its own: letting the range kernels' last workgroup do it -- a
// completion counter, one atomic and a fence per workgroup -- made each of them 12 us slower; 1024 same-address atomics again.)
enum class RowStep { Retire, Fold, Finalized, AllChanged, Mark };

__global__ void ranges_step_kernel(RowRanges *ranges, RowStep step, int lo, int hi, int sy)
{
    if (threadIdx.x || blockIdx.x) return;
    const RowRanges r = *ranges;
    switch (step) {
    case RowStep::Retire: *ranges = rows_retire(r); break;
    case RowStep::Fold: *ranges = rows_fold(r, lo, hi); break;
    case RowStep::Finalized: *ranges = rows_finalized(r); break;
    case RowStep::AllChanged: *ranges = rows_all_changed(r, sy); break;
    case RowStep::Mark: *ranges = rows_mark(r, lo, hi); break;
    }
}

// --------------------------------------------------------------- finalize
// SURVEY 8(a) G3 on the summed counts, window order out (mls.h:167-175 data[x + size_x*y]).
struct FinalizeRule {
    double  inc, dec, minp; // slam_grid_params: occupancy_increment, occupancy_decrement, min_cluster_points
    double *num_pts;        // evidence out
    int8_t *occ;            // occupancy out
};

__device__ inline void cell_value(int h, int m, const FinalizeRule f, double &v, int8_t &o)
{
    v = f.inc * (double)h;
    o = -1;
    if (h > 0 && v > f.minp) o = 100; // mls.cpp:101-105
    v = v - f.dec * (double)m;
    if (m > 0 && v < f.minp) o = 0; // mls.cpp:137-141
}

__device__ inline void finalize_cell(const GridView &g, int x, int y, const FinalizeRule f)
{
    const int s = storage_index(g, x, y);
    const int h = g.hits[s] + (g.acc_hits ? g.acc_hits[s] : 0), m = g.misses[s] + (g.acc_misses ? g.acc_misses[s] : 0);
    double    v;
    int8_t    o;
    cell_value(h, m, f, v, o);
    f.num_pts[x + (size_t)g.sx * y] = v;
    f.occ[x + (size_t)g.sx * y] = o;
}

// Four consecutive cells of one storage row per thread, where the row length and the toroidal x origin are multiples of
// four (any non-rolling grid): 16-byte loads of both count planes, 2 x 16-byte stores of the evidence, one 4-byte store of
// the occupancy -- the rows kernels stream 17 B per cell and were bound by the requests in flight per thread, not by HBM
// (one cell per thread: 8.0 us for config 2's 602 rows; four: see DESIGN.md 4.3).  RESET: the counts just folded go back to
// zero (slam_grid_finalize_reset).
template <bool RESET>
__device__ inline void finalize_quad(const GridView &g, int srow, int ix0, int y, const FinalizeRule f)
{
    const size_t s0 = (size_t)srow * g.sx + ix0;
    int4         h = *reinterpret_cast<const int4 *>(g.hits + s0), m = *reinterpret_cast<const int4 *>(g.misses + s0);
    const bool   any = (h.x | h.y | h.z | h.w | m.x | m.y | m.z | m.w) != 0;
    if (g.acc_hits) {
        const int4 ah = *reinterpret_cast<const int4 *>(g.acc_hits + s0), am = *reinterpret_cast<const int4 *>(g.acc_misses + s0);
        h.x += ah.x, h.y += ah.y, h.z += ah.z, h.w += ah.w;
        m.x += am.x, m.y += am.y, m.z += am.z, m.w += am.w;
    }
    double v[4];
    int8_t o[4];
    cell_value(h.x, m.x, f, v[0], o[0]);
    cell_value(h.y, m.y, f, v[1], o[1]);
    cell_value(h.z, m.z, f, v[2], o[2]);
    cell_value(h.w, m.w, f, v[3], o[3]);
    int x0 = ix0 - g.ox; // the window cells stored there (storage_index's inverse): the four do not straddle the seam
    x0 += x0 < 0 ? g.sx : 0;
    const size_t w0 = (size_t)x0 + (size_t)g.sx * y;
    *reinterpret_cast<double2 *>(f.num_pts + w0) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2 *>(f.num_pts + w0 + 2) = make_double2(v[2], v[3]);
    *reinterpret_cast<unsigned *>(f.occ + w0) = (unsigned)(unsigned char)o[0] | ((unsigned)(unsigned char)o[1] << 8) |
                                               ((unsigned)(unsigned char)o[2] << 16) | ((unsigned)(unsigned char)o[3] << 24);
    if (RESET && any) {
        *reinterpret_cast<int4 *>(g.hits + s0) = make_int4(0, 0, 0, 0);
        *reinterpret_cast<int4 *>(g.misses + s0) = make_int4(0, 0, 0, 0);
    }
}

// the rows lo..hi of the planes: one cell per thread, or (quads) four
template <bool RESET>
__device__ inline void finalize_rows(const GridView &g, int lo, int hi, const FinalizeRule f)
{
    const bool quads = (g.sx & 3) == 0 && (g.ox & 3) == 0;
    const int  per_thread = quads ? 4 : 1;
    const int  per_row = (g.sx + 256 * per_thread - 1) / (256 * per_thread);
    const long items = (long)(hi - lo + 1) * per_row;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const int srow = lo + (int)(it / per_row), ix = ((int)(it % per_row) * 256 + (int)threadIdx.x) * per_thread;
        if (ix >= g.sx) continue;
        int y = srow - g.oy; // the window row stored there (storage_index's inverse)
        y += y < 0 ? g.sy : 0;
        if (quads) {
            finalize_quad<RESET>(g, srow, ix, y, f);
        } else { // here ix counts WINDOW cells of the row (any order covers the row)
            finalize_cell(g, ix, y, f);
            if (RESET) {
                const int s = storage_index(g, ix, y);
                if (g.hits[s]) g.hits[s] = 0;
                if (g.misses[s]) g.misses[s] = 0;
            }
        }
    }
}

// every row (after the in-order mode, whose evidence lives in planes of its own): the same fixed launch, striding over all of them
__global__ __launch_bounds__(256) void finalize_all_rows_kernel(GridView g, FinalizeRule f)
{
    finalize_rows<false>(g, 0, g.sy - 1, f);
}

// only the storage rows whose counts were touched or changed since the last finalize (the hull of the two ranges): a fixed
// launch striding over them
__global__ __launch_bounds__(256) void finalize_rows_kernel(GridView g, FinalizeRule f, const RowRanges *ranges)
{
    int lo, hi;
    rows_due(*ranges, g.sy, &lo, &hi);
    if (hi < lo) return;
    finalize_rows<false>(g, lo, hi, f);
}

// slam_grid_finalize_reset: finalize_rows_kernel that also zeroes the counts it has just folded (what slam_grid_reset_counts
// would do next) and retires the ranges -- one launch where the batch step had four (finalize_rows, ranges_set, reset_rows,
// ranges_retire).  The rows it covers are the hull of the touched and the changed rows, as in finalize_rows_kernel.  Afterwards
// the touched rows are "changed" (their counts are zero again while their evidence still shows this batch: the next finalize
// must visit them) and nothing is touched: that state goes into the OTHER range buffer (`next`; every workgroup reads `ranges`,
// nobody reads `next` during this launch), which the host makes the grid's current one for everything enqueued behind.
__global__ __launch_bounds__(256) void finalize_reset_rows_kernel(GridView g, FinalizeRule f, const RowRanges *ranges, RowRanges *next)
{
    const RowRanges r = *ranges;
    int             lo, hi;
    rows_due(r, g.sy, &lo, &hi);
    if (blockIdx.x == 0 && threadIdx.x == 0) *next = rows_retire(rows_finalized(r));
    if (hi < lo) return;
    finalize_rows<true>(g, lo, hi, f);
}

__global__ __launch_bounds__(256) void gather_counts_kernel(GridView g, int32_t *hits_w, int32_t *misses_w)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.sx) return;
    const int s = storage_index(g, x, y);
    hits_w[x + (size_t)g.sx * y] = g.hits[s] + (g.acc_hits ? g.acc_hits[s] : 0);
    misses_w[x + (size_t)g.sx * y] = g.misses[s] + (g.acc_misses ? g.acc_misses[s] : 0);
}

// slam_grid_fold: rows [row_lo, row_hi] of the count planes are added to the accumulator planes and zeroed
__global__ __launch_bounds__(256) void fold_rows_kernel(int32_t *planes, int32_t *acc, size_t cells, int sx, int row_lo, int n_rows)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)n_rows * sx;
    if (i >= n) return;
    const size_t k = (size_t)row_lo * sx + i;
    for (int p = 0; p < 2; ++p) {
        const size_t j = p * cells + k;
        const int    v = planes[j];
        if (v) {
            acc[j] += v;
            planes[j] = 0;
        }
    }
}

// MLS::setPose roll, mls.cpp:461-468: cells that rolled into the window are cleared
__global__ __launch_bounds__(256) void roll_clear_kernel(GridView g, int dx, int dy, double *num_pts,
                                                         int8_t *occ_state)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.sx) return;
    if (x < -dx || x >= g.sx - dx || y < -dy || y >= g.sy - dy) {
        const int s = storage_index(g, x, y);
        g.hits[s] = 0;
        g.misses[s] = 0;
        if (g.acc_hits) {
            const_cast<int32_t *>(g.acc_hits)[s] = 0;
            const_cast<int32_t *>(g.acc_misses)[s] = 0;
        }
        num_pts[s] = 0.0;
        occ_state[s] = -1;
    }
}

// in-order single scan: per touched cell replay the reference's += / -= sequence
// per-scan delta of a cell: hits in the high, misses in the low 32 bits of one 64-bit word,
// so exactly one point sees the cell untouched and lists it
__global__ __launch_bounds__(256) void inorder_count_kernel(GridView g, const float *obs, int n_obs,
                                                            const float *gnd, int n_gnd, int stride,
                                                            unsigned long long *delta, int *touched,
                                                            int *n_touched)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_obs + n_gnd) return;
    const bool   is_obs = i < n_obs;
    const float *p = is_obs ? obs + (size_t)i * stride : gnd + (size_t)(i - n_obs) * stride;
    int cx, cy;
    if (!point_cell(g, p[0], p[1], &cx, &cy)) return;
    const int s = storage_index(g, cx, cy);
    const unsigned long long old = atomicAdd(&delta[s], is_obs ? (1ull << 32) : 1ull);
    atomicAdd(is_obs ? &g.hits[s] : &g.misses[s], 1);
    if (old == 0ull) { // the first point of the scan in this cell
        const int row = s / g.sx;
        rows_widen_touched(g.dirty, row, -row);
        const int k = atomicAdd(n_touched, 1);
        touched[k] = s;
    }
}

__global__ __launch_bounds__(256) void inorder_apply_kernel(GridView g, FinalizeRule f, unsigned long long *delta,
                                                            const int *touched, const int *n_touched,
                                                            unsigned long long *updates)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned  did = 0;
    if (i < *n_touched) {
        const int s = touched[i];
        const unsigned long long d = delta[s];
        delta[s] = 0ull; // each touched cell is listed once: no other thread reads it
        const int h = (int)(d >> 32), m = (int)(d & 0xffffffffull);
        {
            double v = f.num_pts[s]; // (here the rule's planes are the mode's own, in storage order)
            int8_t o = f.occ[s];
            for (int k = 0; k < h; ++k) v = __dadd_rn(v, f.inc); // mls.cpp:99, one += per point
            if (h > 0 && v > f.minp) o = 100;                    // monotone: last test decides
            for (int k = 0; k < m; ++k) v = __dsub_rn(v, f.dec); // mls.cpp:135
            if (m > 0 && v < f.minp) o = 0;
            f.num_pts[s] = v;
            f.occ[s] = o;
            did = (unsigned)(h + m);
        }
    }
    block_add_updates(updates, did);
}

__global__ __launch_bounds__(256) void window_from_storage_kernel(GridView g, const double *num_s,
                                                                  const int8_t *occ_s, double *num_w,
                                                                  int8_t *occ_w)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= g.sx) return;
    const int s = storage_index(g, x, y);
    num_w[x + (size_t)g.sx * y] = num_s[s];
    occ_w[x + (size_t)g.sx * y] = occ_s[s];
}

// How the tiled raycast is launched: resolved once, in slam_grid_create, from slam_grid_params (and in the measuring build
// from the SLAM_RAYCAST_* environment)
struct RaycastShape {
    int  chunk;     // 64-beam blocks a workgroup takes from a tile's list at a time
    int  wg_per_cu; // persistent raycast workgroups per CU
    bool merge;     // lanes on one cell add once (SLAM_RAYCAST_TILED_MERGE)
    int  ablate;    // debug: SLAM_RAYCAST_ABLATE bit mask (timing experiments only)
};

} // namespace

struct slam_grid {
    slam_grid_params prm;
    GridView         gv;
    size_t           cells = 0;
    OwnedArray<int32_t> d_planes;  // [hits | misses]
    OwnedArray<double>  d_num_w;   // window order, written by finalize
    OwnedArray<int8_t>  d_occ_w;   // window order, written by finalize
    OwnedArray<double>  d_num_s;   // storage order, in-order mode state
    OwnedArray<int8_t>  d_occ_s;   // storage order, in-order mode state
    OwnedArray<unsigned long long> d_delta; // [cells] per-scan deltas of the in-order mode
    OwnedArray<int>     d_touched; // [2*cap_points] + counter
    OwnedArray<unsigned long long> d_updates;
    OwnedArray<RowRanges> d_dirty;  // [2] see GridView::dirty
    OwnedArray<int32_t> d_acc;      // [hits | misses] accumulator planes (slam_grid_enable_accumulator)
    OwnedArray<Beam>    d_beams;
    OwnedArray<int4>    d_chunk_box;
    OwnedArray<int>     d_tile_cnt; // [n_tiles] overlapping chunks per tile
    OwnedArray<int>     d_tile_off; // [n_tiles+1] where each tile's list starts (grids beyond kMaxLdsTiles tiles)
    OwnedArray<int>     d_cursor;   // [n_tiles+1] blocks of each tile's list handed out so far; behind them, the launch's tile write-backs
    OwnedArray<int>     d_items;    // chunk ids bucketed by tile
    int              n_cu = 256;
    RaycastShape     shape{};
    DevMem           d_stage;             // host-API staging
    bool             state_from_inorder = false;
    long             shift_x = 0, shift_y = 0; // cells the rolling window has moved since creation (sum of setPose's dx, dy)

    // Two range buffers: slam_grid_finalize_reset reads the current one (gv.dirty) and starts the other, which the host
    // then makes current for every call enqueued from there on (one stream at a time per handle: the header's contract).
    RowRanges *other_ranges() const { return gv.dirty == d_dirty.get() ? d_dirty.get() + 1 : d_dirty.get(); }
    void       make_current(RowRanges *r) { gv.dirty = r; }
};

namespace {

// The grid's growing buffers: at least a quarter more than before and never below 4 KB.  (The free waits for the device:
// callers with varying sizes reserve up front, slam_grid_reserve.)
int reserve(DevMem &b, size_t bytes) { return b.reserve(bytes, std::max(b.cap + b.cap / 4, (size_t)4096)); }

int reserve_beams(slam_grid *g, size_t n)
{
    SLAM_TRY(reserve(g->d_beams, n * sizeof(Beam)));
    const size_t chunks = (n + kBlock - 1) / kBlock + kChunk / kBlock;
    SLAM_TRY(reserve(g->d_chunk_box, chunks * sizeof(int4)));
    if (g->prm.raycast_impl != SLAM_RAYCAST_GLOBAL) {
        const size_t n_tiles = (size_t)((g->gv.sx + kTile - 1) / kTile) * ((g->gv.sy + kTile - 1) / kTile);
        if (!g->d_tile_cnt) { // the three together or none of them
            OwnedArray<int> cnt, off, cursor;
            SLAM_TRY(cnt.alloc(n_tiles * sizeof(int)));
            SLAM_TRY(off.alloc((n_tiles + 1) * sizeof(int)));
            SLAM_TRY(cursor.alloc((n_tiles + 1) * sizeof(int)));
            g->d_tile_cnt = std::move(cnt), g->d_tile_off = std::move(off), g->d_cursor = std::move(cursor);
        }
        SLAM_TRY(reserve(g->d_items, (chunks * n_tiles) * sizeof(int)));
    }
    return SLAM_OK;
}

RaycastShape raycast_shape(const slam_grid_params &p)
{
    RaycastShape s;
    // (a visit's log holds at least two chunks and at most kMaxAccBlocks / kChunkMin)
    s.chunk = p.raycast_seg_items > 0 ? std::min(std::max(p.raycast_seg_items, kChunkMin), kMaxAccBlocks / 2) : kChunkDefault;
    // Persistent raycast workgroups per CU where the caller did not say: two (thirty-two wavefronts, 2 x 75 KB of LDS).  A
    // workgroup's walk is a chain of dependent integer steps and LDS adds: the second workgroup's wavefronts issue in its gaps
    // (tools/raycast_time.py, chunks of 16 blocks: config 2 0.110 ms per call with two against 0.131 with one; config 4's share
    // 0.274 against 0.322).
    s.wg_per_cu = p.raycast_wg_per_cu > 0 ? std::min(p.raycast_wg_per_cu, 8) : 2;
    s.merge = p.raycast_impl == SLAM_RAYCAST_TILED_MERGE;
    s.ablate = 0;
#ifdef SLAM_MEASURE
    if (const char *e = getenv("SLAM_RAYCAST_MERGE")) s.merge = atoi(e) != 0;
    if (const char *e = getenv("SLAM_RAYCAST_SEG")) s.chunk = std::min(std::max(kChunkMin, atoi(e)), kMaxAccBlocks / 2);
    if (const char *e = getenv("SLAM_RAYCAST_ABLATE")) s.ablate = atoi(e);
    if (const char *e = getenv("SLAM_RAYCAST_WGPCU")) s.wg_per_cu = std::max(1, atoi(e));
#endif
    return s;
}

// ... and how many workgroups in all: the whole chip, unless the caller caps it (slam_grid_params::raycast_max_workgroups: a
// raycast that runs beside registrations holds every CU it has a workgroup on for as long as the launch lasts)
int raycast_workgroups(const slam_grid *g)
{
    const int all = g->shape.wg_per_cu * g->n_cu;
    return g->prm.raycast_max_workgroups > 0 ? std::min(all, g->prm.raycast_max_workgroups) : all;
}

int walk_beams(slam_grid *g, int n, hipStream_t st)
{
    const int n_chunks = (n + kBlock - 1) / kBlock; // culling blocks
    if (g->prm.raycast_impl != SLAM_RAYCAST_GLOBAL) {
        const int tiles_x = (g->gv.sx + kTile - 1) / kTile, tiles_y = (g->gv.sy + kTile - 1) / kTile;
        const int n_tiles = tiles_x * tiles_y;
        const bool rows = n_tiles <= kMaxLdsTiles; // every tile's list in a row of its own, or one behind the other
        if (rows) {
            // one pass over the block boxes; the raycast workgroups work the prefix of the tile counts out themselves
            hipLaunchKernelGGL(tile_items_wg_kernel, dim3(n_tiles), dim3(1024), 0, st, g->d_chunk_box, n_chunks, tiles_x,
                               g->gv.sx, g->gv.sy, g->d_tile_cnt, g->d_items, g->d_cursor);
        } else {
            const dim3 tgrid((n_tiles * 64 + 255) / 256);
            hipLaunchKernelGGL((tile_items_kernel<0>), tgrid, dim3(256), 0, st, g->d_chunk_box, n_chunks, tiles_x,
                               n_tiles, g->gv.sx, g->gv.sy, g->d_tile_cnt, g->d_tile_off, g->d_items);
            hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kTileThreads), 0, st, g->d_tile_cnt, n_tiles, g->d_tile_off, g->d_cursor);
            hipLaunchKernelGGL((tile_items_kernel<1>), tgrid, dim3(256), 0, st, g->d_chunk_box, n_chunks, tiles_x,
                               n_tiles, g->gv.sx, g->gv.sy, g->d_tile_cnt, g->d_tile_off, g->d_items);
        }
        // persistent workgroups (75 KB of LDS each)
        hipLaunchKernelGGL(g->shape.merge ? raycast_tiled_kernel<true> : raycast_tiled_kernel<false>, dim3(raycast_workgroups(g)),
                           dim3(kTileThreads), 0, st, g->gv, g->d_beams, n, g->d_items, rows ? (const int *)nullptr : g->d_tile_off.get(),
                           n_tiles, g->d_cursor, tiles_x, g->shape.chunk, g->shape.ablate, g->d_tile_cnt, rows ? n_chunks : 0);
    } else {
        hipLaunchKernelGGL(raycast_global_kernel, dim3((n + 255) / 256), dim3(256), 0, st, g->gv, g->d_beams, n);
    }
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// A raycast of n beams: room for them, the entry point's pre-pass (its kChunk-thread launch over `grid` workgroups, which
// leaves the integer beams and the block boxes), the walk.
template <class PrePass>
int raycast_beams(slam_grid *g, int n, hipStream_t st, PrePass launch_pre_pass)
{
    SLAM_TRY(reserve_beams(g, (size_t)n));
    launch_pre_pass(dim3((n + kChunk - 1) / kChunk));
    SLAM_HIP(hipGetLastError());
    return walk_beams(g, n, st);
}

dim3 grid2d(const slam_grid *g) { return dim3((g->gv.sx + 255) / 256, g->gv.sy); }

// the finalize rule as the grid's parameters have it, writing the window-order planes (or the in-order mode's own)
FinalizeRule finalize_rule(const slam_grid *g, bool inorder_planes = false)
{
    return {g->prm.occupancy_increment, g->prm.occupancy_decrement, (double)g->prm.min_cluster_points,
            inorder_planes ? g->d_num_s.get() : g->d_num_w.get(), inorder_planes ? g->d_occ_s.get() : g->d_occ_w.get()};
}

int step_ranges(slam_grid *g, hipStream_t st, RowStep step, int lo = 0, int hi = 0)
{
    hipLaunchKernelGGL(ranges_step_kernel, dim3(1), dim3(64), 0, st, g->gv.dirty, step, lo, hi, g->gv.sy);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

} // namespace

extern "C" {

void slam_grid_default_params(slam_grid_params *p)
{
    if (!p) return;
    p->max_range = 75.0;          // mls.h:161
    p->occupancy_increment = 1.0; // mls.h:188
    p->occupancy_decrement = 0.3; // mls.h:189
    p->min_cluster_points = 10;   // mls.h:165
    p->rolling = 1;               // local_mapper.cpp:29 MLS(200,200,0.2,true)
    p->raycast_impl = SLAM_RAYCAST_TILED;
    p->raycast_seg_items = 0;
    p->raycast_wg_per_cu = 0;
    p->raycast_max_workgroups = 0;
}

int slam_grid_create(int size_x, int size_y, double resolution, const slam_grid_params *params,
                     slam_grid_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_grid_create: null out pointer");
    *out = nullptr;
    SLAM_REQUIRE(size_x > 0 && size_y > 0 && size_x <= 32767 && size_y <= 32767 && resolution > 0,
                 SLAM_E_INVALID, "slam_grid_create: size must be 1..32767 cells and resolution > 0");
    SLAM_TRY(require_device());
    slam_grid *g = new (std::nothrow) slam_grid();
    SLAM_REQUIRE(g, SLAM_E_NOMEM, "slam_grid_create: out of host memory");
    if (params)
        g->prm = *params;
    else
        slam_grid_default_params(&g->prm);
    g->cells = (size_t)size_x * size_y;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            g->n_cu = std::max(1, prop.multiProcessorCount);
    }
    g->shape = raycast_shape(g->prm);
    std::unique_ptr<slam_grid> guard(g); // an early return gives the handle and its buffers back
    SLAM_TRY(g->d_planes.alloc(2 * g->cells * sizeof(int32_t)));
    SLAM_TRY(g->d_num_w.alloc(g->cells * sizeof(double)));
    SLAM_TRY(g->d_occ_w.alloc(g->cells));
    SLAM_TRY(g->d_num_s.alloc(g->cells * sizeof(double)));
    SLAM_TRY(g->d_occ_s.alloc(g->cells));
    SLAM_TRY(g->d_updates.alloc(kUpdateSlots * sizeof(unsigned long long)));
    SLAM_TRY(g->d_dirty.alloc(2 * sizeof(RowRanges)));
    GridView &v = g->gv;
    v.sx = size_x;
    v.sy = size_y;
    v.ox = v.oy = 0;
    v.res = resolution;
    v.max_range = g->prm.max_range;
    v.pose_x = v.pose_y = 0.0;
    v.rolling = g->prm.rolling ? 1 : 0;
    v.hits = g->d_planes;
    v.misses = g->d_planes + g->cells; // (endpoints_kernel addresses both planes through `hits` with an int key: misses == hits + cells,
                                       // and 2 * cells fits an int -- slam_grid_create refuses grids of 2^30 cells or more)
    v.updates = g->d_updates;
    v.dirty = g->d_dirty;
    v.acc_hits = v.acc_misses = nullptr;
    SLAM_TRY(slam_grid_clear(g, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    *out = guard.release();
    return SLAM_OK;
}

void slam_grid_destroy(slam_grid_t *g) { delete g; }

int slam_grid_clear(slam_grid_t *g, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    hipStream_t st = as_stream(stream);
    SLAM_HIP(hipMemsetAsync(g->d_planes, 0, 2 * g->cells * sizeof(int32_t), st));
    SLAM_HIP(hipMemsetAsync(g->d_num_w, 0, g->cells * sizeof(double), st));
    SLAM_HIP(hipMemsetAsync(g->d_num_s, 0, g->cells * sizeof(double), st));
    SLAM_HIP(hipMemsetAsync(g->d_occ_w, 0xff, g->cells, st)); // -1 = unknown (mls.cpp:26)
    SLAM_HIP(hipMemsetAsync(g->d_occ_s, 0xff, g->cells, st));
    SLAM_HIP(hipMemsetAsync(g->d_updates, 0, kUpdateSlots * sizeof(unsigned long long), st));
    SLAM_HIP(hipMemsetAsync(g->d_dirty, kNoRow & 0xff, 2 * sizeof(RowRanges), st)); // rows_empty(), both buffers
    if (g->d_acc) SLAM_HIP(hipMemsetAsync(g->d_acc, 0, 2 * g->cells * sizeof(int32_t), st));
    g->state_from_inorder = false;
    return SLAM_OK;
}

int slam_grid_reset_counts(slam_grid_t *g, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(reset_rows_kernel, dim3(kRangeBlocks), dim3(256), 0, st, g->d_planes, g->cells, g->gv.sx, g->gv.sy, g->gv.dirty);
    return step_ranges(g, st, RowStep::Retire);
}

int slam_grid_enable_accumulator(slam_grid_t *g)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    if (g->d_acc) return SLAM_OK;
    SLAM_TRY(g->d_acc.alloc(2 * g->cells * sizeof(int32_t)));
    SLAM_HIP(hipMemset(g->d_acc, 0, 2 * g->cells * sizeof(int32_t)));
    g->gv.acc_hits = g->d_acc;
    g->gv.acc_misses = g->d_acc + g->cells;
    return SLAM_OK;
}

int slam_grid_fold(slam_grid_t *g, int row_lo, int row_hi, slam_stream_t stream)
{
    SLAM_REQUIRE(g && g->d_acc, SLAM_E_INVALID, "slam_grid_fold: needs slam_grid_enable_accumulator");
    hipStream_t st = as_stream(stream);
    if (row_hi >= row_lo) {
        SLAM_REQUIRE(row_lo >= 0 && row_hi < g->gv.sy, SLAM_E_INVALID, "slam_grid_fold: rows %d..%d outside the grid", row_lo, row_hi);
        const size_t n = (size_t)(row_hi - row_lo + 1) * g->gv.sx;
        hipLaunchKernelGGL(fold_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g->d_planes, g->d_acc, g->cells,
                           g->gv.sx, row_lo, row_hi - row_lo + 1);
        SLAM_HIP(hipGetLastError());
    }
    // the folded rows have changed since the last finalize (by updates, by a merge): they and whatever else was touched
    // stay due for it; the touched range starts again
    if (row_hi >= row_lo) return step_ranges(g, st, RowStep::Fold, row_lo, row_hi);
    // nothing to fold: as before, the touched range starts again (there is nothing in it that holds counts... or the caller said so)
    return step_ranges(g, st, RowStep::Retire);
}

int slam_grid_mark_rows(slam_grid_t *g, int row_lo, int row_hi, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    if (row_hi < row_lo) return SLAM_OK;
    SLAM_REQUIRE(row_lo >= 0 && row_hi < g->gv.sy, SLAM_E_INVALID, "slam_grid_mark_rows: rows %d..%d outside the grid", row_lo, row_hi);
    return step_ranges(g, as_stream(stream), RowStep::Mark, row_lo, row_hi);
}

int slam_grid_dirty_rows_dev(slam_grid_t *g, int32_t **d_range)
{
    SLAM_REQUIRE(g && d_range, SLAM_E_INVALID, "slam_grid_dirty_rows_dev: bad arguments");
    *d_range = &g->gv.dirty->touched_lo; // the touched pair (the buffer in use as of the calls enqueued so far: slam_grid_finalize_reset alternates between two)
    return SLAM_OK;
}

int slam_grid_dirty_rows(slam_grid_t *g, int *row_lo, int *row_hi)
{
    SLAM_REQUIRE(g && row_lo && row_hi, SLAM_E_INVALID, "slam_grid_dirty_rows: bad arguments");
    RowRanges r;
    SLAM_HIP(hipMemcpy(&r, g->gv.dirty, sizeof r, hipMemcpyDeviceToHost));
    rows_reported(r, row_lo, row_hi);
    return SLAM_OK;
}

int slam_grid_set_min_cluster_points(slam_grid_t *g, int v)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    g->prm.min_cluster_points = v;
    // the threshold enters every cell's occupancy: all rows are due at the next finalize
    return step_ranges(g, nullptr, RowStep::AllChanged);
}

int slam_grid_set_max_range(slam_grid_t *g, double v)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    g->prm.max_range = v;
    g->gv.max_range = v;
    return SLAM_OK;
}

int slam_grid_get_pose(slam_grid_t *g, double *x, double *y)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    if (x) *x = g->gv.pose_x;
    if (y) *y = g->gv.pose_y;
    return SLAM_OK;
}

int slam_grid_set_pose(slam_grid_t *g, double x, double y, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    GridView &v = g->gv;
    if (!v.rolling) { // mls.cpp:411-415
        v.pose_x = x;
        v.pose_y = y;
        return SLAM_OK;
    }
    const double xdiff = x - v.pose_x, ydiff = y - v.pose_y; // mls.cpp:419-424
    const int    dx = (int)std::round(xdiff / v.res), dy = (int)std::round(ydiff / v.res);
    if (dx == 0 && dy == 0) return SLAM_OK;
    // Grid::shiftOrigin, mls.h:87-97 (one wrap, as there; larger jumps clear everything anyway)
    auto wrap = [](int o, int d, int n) {
        long v2 = ((long)o + d) % n;
        if (v2 < 0) v2 += n;
        return (int)v2;
    };
    v.ox = wrap(v.ox, dx, v.sx);
    v.oy = wrap(v.oy, dy, v.sy);
    v.pose_x += dx * v.res; // mls.cpp:430-431
    v.pose_y += dy * v.res;
    g->shift_x += dx;
    g->shift_y += dy;
    hipLaunchKernelGGL(roll_clear_kernel, grid2d(g), dim3(256), 0, as_stream(stream), v, dx, dy, g->d_num_s,
                       g->d_occ_s);
    // the window moved over the storage: every row of the evidence / occupancy planes (window order) is due
    return step_ranges(g, as_stream(stream), RowStep::AllChanged);
}

int slam_grid_add_endpoints_dev(slam_grid_t *g, const float *d_obs, int n_obs, const float *d_gnd, int n_gnd,
                                int stride, slam_stream_t stream)
{
    SLAM_REQUIRE(g && n_obs >= 0 && n_gnd >= 0 && stride >= 2, SLAM_E_INVALID,
                 "slam_grid_add_endpoints_dev: bad arguments");
    const int n = n_obs + n_gnd;
    if (n == 0) return SLAM_OK;
    hipLaunchKernelGGL(endpoints_kernel, dim3((n + kEndpointsPerBlock - 1) / kEndpointsPerBlock), dim3(256), 0, as_stream(stream), g->gv, d_obs,
                       n_obs, d_gnd, n_gnd, stride);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

static int stage_points(slam_grid *g, const float *obs, int n_obs, const float *gnd, int n_gnd, int stride,
                        float **d_obs, float **d_gnd)
{
    const size_t bo = (size_t)n_obs * stride * sizeof(float), bg = (size_t)n_gnd * stride * sizeof(float);
    SLAM_TRY(reserve(g->d_stage, bo + bg + 16));
    *d_obs = g->d_stage.as<float>();
    *d_gnd = *d_obs + (size_t)n_obs * stride;
    if (bo) SLAM_HIP(hipMemcpyAsync(*d_obs, obs, bo, hipMemcpyHostToDevice, nullptr));
    if (bg) SLAM_HIP(hipMemcpyAsync(*d_gnd, gnd, bg, hipMemcpyHostToDevice, nullptr));
    return SLAM_OK;
}

int slam_grid_add_endpoints(slam_grid_t *g, const float *obs, int n_obs, const float *gnd, int n_gnd,
                            int stride)
{
    SLAM_REQUIRE(g && n_obs >= 0 && n_gnd >= 0 && stride >= 2 && (obs || !n_obs) && (gnd || !n_gnd),
                 SLAM_E_INVALID, "slam_grid_add_endpoints: bad arguments");
    SLAM_TRY(require_device());
    float *d_obs, *d_gnd;
    SLAM_TRY(stage_points(g, obs, n_obs, gnd, n_gnd, stride, &d_obs, &d_gnd));
    SLAM_TRY(slam_grid_add_endpoints_dev(g, d_obs, n_obs, d_gnd, n_gnd, stride, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_grid_raycast_dev(slam_grid_t *g, const float *d_origin_xy, const float *d_end_xy, int n,
                          slam_stream_t stream)
{
    SLAM_REQUIRE(g && n >= 0 && (n == 0 || (d_origin_xy && d_end_xy)), SLAM_E_INVALID,
                 "slam_grid_raycast_dev: bad arguments");
    if (n == 0) return SLAM_OK;
    hipStream_t st = as_stream(stream);
    return raycast_beams(g, n, st, [&](dim3 grid) {
        hipLaunchKernelGGL(beams_from_rays_kernel, grid, dim3(kChunk), 0, st, g->gv, reinterpret_cast<const float2 *>(d_origin_xy),
                           reinterpret_cast<const float2 *>(d_end_xy), n, g->d_beams, g->d_chunk_box);
    });
}

int slam_grid_raycast(slam_grid_t *g, const float *origin_xy, const float *end_xy, int n)
{
    SLAM_REQUIRE(g && n >= 0 && (n == 0 || (origin_xy && end_xy)), SLAM_E_INVALID,
                 "slam_grid_raycast: bad arguments");
    SLAM_TRY(require_device());
    if (n == 0) return SLAM_OK;
    float *d_o, *d_e;
    SLAM_TRY(stage_points(g, origin_xy, n, end_xy, n, 2, &d_o, &d_e));
    SLAM_TRY(slam_grid_raycast_dev(g, d_o, d_e, n, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_grid_reserve(slam_grid_t *g, int max_beams)
{
    SLAM_REQUIRE(g && max_beams >= 0, SLAM_E_INVALID, "slam_grid_reserve: bad arguments");
    return max_beams ? reserve_beams(g, (size_t)max_beams) : SLAM_OK;
}

int slam_grid_raycast_scans_dev(slam_grid_t *g, const double *d_pts, const int32_t *d_scan_off, int n_scans,
                                int n_points, const double *d_R, const double *d_t, slam_stream_t stream)
{
    SLAM_REQUIRE(g && n_scans >= 0 && n_points >= 0 && d_scan_off && d_R && d_t, SLAM_E_INVALID,
                 "slam_grid_raycast_scans_dev: bad arguments");
    if (n_scans == 0 || n_points == 0) return SLAM_OK;
    hipStream_t st = as_stream(stream);
    return raycast_beams(g, n_points, st, [&](dim3 grid) {
        hipLaunchKernelGGL(beams_from_scans_kernel, grid, dim3(kChunk), 0, st, g->gv, reinterpret_cast<const double2 *>(d_pts),
                           d_scan_off, n_scans, d_R, d_t, n_points, g->d_beams, g->d_chunk_box);
    });
}

int slam_grid_finalize(slam_grid_t *g, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    // (after the in-order mode, whose evidence lives in planes of its own, every row is recomputed)
    if (g->state_from_inorder)
        hipLaunchKernelGGL(finalize_all_rows_kernel, dim3(kRangeBlocks), dim3(256), 0, as_stream(stream), g->gv, finalize_rule(g));
    else
        hipLaunchKernelGGL(finalize_rows_kernel, dim3(kRangeBlocks), dim3(256), 0, as_stream(stream), g->gv, finalize_rule(g), g->gv.dirty);
    SLAM_TRY(step_ranges(g, as_stream(stream), RowStep::Finalized));
    g->state_from_inorder = false;
    return SLAM_OK;
}

int slam_grid_finalize_reset(slam_grid_t *g, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    // A stream that is being captured into a hipGraph records this call's kernel arguments once: the switch between the two
    // range buffers below happens on the HOST, per call, and a replay would read the same stale buffer every time (rows never
    // reset or never folded, silently).  Captured, the call is the two-step form, whose arguments do not change from call to call.
    bool capturing = false;
    if (stream) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(as_stream(stream), &cap) == hipSuccess)
            capturing = cap != hipStreamCaptureStatusNone;
        else
            (void)hipGetLastError();
    }
    if (g->state_from_inorder || capturing) { // (the in-order mode keeps its evidence in planes of its own: the two steps as they are)
        SLAM_TRY(slam_grid_finalize(g, stream));
        return slam_grid_reset_counts(g, stream);
    }
    RowRanges *next = g->other_ranges();
    hipLaunchKernelGGL(finalize_reset_rows_kernel, dim3(kRangeBlocks), dim3(256), 0, as_stream(stream), g->gv, finalize_rule(g),
                       g->gv.dirty, next);
    SLAM_HIP(hipGetLastError());
    g->make_current(next);
    return SLAM_OK;
}

// MLS::addToMap's cloud transform (mls.cpp:34-53: tf::poseMsgToEigen + pcl::transformPointCloud): every point turned by the pose's
// rotation and offset by t, computed in double and stored as float -- the arithmetic of the adapter's host loop term by term
// (products and sums rounded one by one, no contraction), so the floats are the host's.
namespace {
struct CloudTransform {
    double r[9], t[3];
};
__global__ __launch_bounds__(256) void transform_cloud_kernel(const float *in, int n, int stride, CloudTransform T, float *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = in[(size_t)i * stride], py = in[(size_t)i * stride + 1], pz = in[(size_t)i * stride + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        out[3 * (size_t)i + k] = (float)__dadd_rn(
            __dadd_rn(__dadd_rn(__dmul_rn(T.r[3 * k], px), __dmul_rn(T.r[3 * k + 1], py)), __dmul_rn(T.r[3 * k + 2], pz)), T.t[k]);
}
} // namespace

int slam_grid_transform_cloud_dev(const float *d_in_xyz, int n, int stride, const double R[9], const double t[3], float *d_out_xyz,
                                  slam_stream_t stream)
{
    SLAM_REQUIRE(n >= 0 && stride >= 3 && R && t && ((d_in_xyz && d_out_xyz) || n == 0), SLAM_E_INVALID,
                 "slam_grid_transform_cloud_dev: bad arguments");
    SLAM_TRY(require_device());
    if (n == 0) return SLAM_OK;
    CloudTransform T;
    for (int k = 0; k < 9; ++k) T.r[k] = R[k];
    for (int k = 0; k < 3; ++k) T.t[k] = t[k];
    hipLaunchKernelGGL(transform_cloud_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), d_in_xyz, n, stride, T, d_out_xyz);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_grid_add_scan_inorder_dev(slam_grid_t *g, const float *d_obs, int n_obs, const float *d_gnd, int n_gnd, int stride,
                                   slam_stream_t stream)
{
    SLAM_REQUIRE(g && n_obs >= 0 && n_gnd >= 0 && stride >= 2 && (d_obs || !n_obs) && (d_gnd || !n_gnd), SLAM_E_INVALID,
                 "slam_grid_add_scan_inorder_dev: bad arguments");
    SLAM_TRY(require_device());
    const int n = n_obs + n_gnd;
    if (n == 0) return SLAM_OK;
    hipStream_t st = as_stream(stream);
    if (!g->d_delta) {
        SLAM_TRY(g->d_delta.alloc(g->cells * sizeof(unsigned long long)));
        SLAM_HIP(hipMemsetAsync(g->d_delta, 0, g->cells * sizeof(unsigned long long), st));
    }
    SLAM_TRY(reserve(g->d_touched, ((size_t)n + 1) * sizeof(int)));
    int *counter = g->d_touched + n;
    SLAM_HIP(hipMemsetAsync(counter, 0, sizeof(int), st));
    hipLaunchKernelGGL(inorder_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, g->gv, d_obs, n_obs, d_gnd, n_gnd, stride,
                       g->d_delta, g->d_touched, counter);
    hipLaunchKernelGGL(inorder_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, st, g->gv, finalize_rule(g, true), g->d_delta,
                       g->d_touched, counter, g->d_updates);
    SLAM_HIP(hipGetLastError());
    g->state_from_inorder = true;
    return SLAM_OK;
}

int slam_grid_add_scan_inorder(slam_grid_t *g, const float *obs, int n_obs, const float *gnd, int n_gnd,
                               int stride)
{
    SLAM_REQUIRE(g && n_obs >= 0 && n_gnd >= 0 && stride >= 2 && (obs || !n_obs) && (gnd || !n_gnd),
                 SLAM_E_INVALID, "slam_grid_add_scan_inorder: bad arguments");
    SLAM_TRY(require_device());
    if (n_obs + n_gnd == 0) return SLAM_OK;
    float *d_obs, *d_gnd;
    SLAM_TRY(stage_points(g, obs, n_obs, gnd, n_gnd, stride, &d_obs, &d_gnd));
    SLAM_TRY(slam_grid_add_scan_inorder_dev(g, d_obs, n_obs, d_gnd, n_gnd, stride, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_grid_read_counts(slam_grid_t *g, int32_t *hits, int32_t *misses)
{
    SLAM_REQUIRE(g && hits && misses, SLAM_E_INVALID, "slam_grid_read_counts: bad arguments");
    SLAM_TRY(require_device());
    DevMem scratch; // (freed on every way out; hipFree waits for the launch)
    SLAM_TRY(scratch.alloc(2 * g->cells * sizeof(int32_t)));
    int32_t *tmp = scratch.as<int32_t>();
    hipLaunchKernelGGL(gather_counts_kernel, grid2d(g), dim3(256), 0, nullptr, g->gv, tmp, tmp + g->cells);
    SLAM_HIP(hipMemcpy(hits, tmp, g->cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    SLAM_HIP(hipMemcpy(misses, tmp + g->cells, g->cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

static int sync_window_state(slam_grid *g, hipStream_t st = nullptr)
{
    if (g->state_from_inorder) {
        hipLaunchKernelGGL(window_from_storage_kernel, grid2d(g), dim3(256), 0, st, g->gv, g->d_num_s,
                           g->d_occ_s, g->d_num_w, g->d_occ_w);
        SLAM_HIP(hipGetLastError());
    }
    return SLAM_OK;
}

int slam_grid_read_occupancy(slam_grid_t *g, int8_t *occ)
{
    SLAM_REQUIRE(g && occ, SLAM_E_INVALID, "slam_grid_read_occupancy: bad arguments");
    SLAM_TRY(require_device());
    SLAM_TRY(sync_window_state(g));
    SLAM_HIP(hipMemcpy(occ, g->d_occ_w, g->cells, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// The distance field (grid_dist.hip) of the plane slam_grid_read_occupancy returns: after the in-order mode that mode's state,
// brought into window order on `stream` first, otherwise what the last finalize left.
int slam_grid_distance_field(slam_grid_t *g, slam_gdist_t *h, slam_stream_t stream)
{
    SLAM_REQUIRE(g && h, SLAM_E_INVALID, "slam_grid_distance_field: null handle");
    int sx = 0, sy = 0;
    gdist_size(h, &sx, &sy);
    SLAM_REQUIRE(sx == g->gv.sx && sy == g->gv.sy, SLAM_E_INVALID, "slam_grid_distance_field: the grid is %d x %d cells, the distance field %d x %d",
                 g->gv.sx, g->gv.sy, sx, sy);
    SLAM_TRY(sync_window_state(g, as_stream(stream)));
    return gdist_compute_on(h, g->d_occ_w, as_stream(stream));
}

int slam_grid_read_num_pts(slam_grid_t *g, double *num_pts)
{
    SLAM_REQUIRE(g && num_pts, SLAM_E_INVALID, "slam_grid_read_num_pts: bad arguments");
    SLAM_TRY(require_device());
    SLAM_TRY(sync_window_state(g));
    SLAM_HIP(hipMemcpy(num_pts, g->d_num_w, g->cells * sizeof(double), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_grid_total_updates(slam_grid_t *g, uint64_t *n)
{
    SLAM_REQUIRE(g && n, SLAM_E_INVALID, "slam_grid_total_updates: bad arguments");
    SLAM_TRY(require_device());
    std::vector<unsigned long long> v(kUpdateSlots, 0);
    SLAM_HIP(hipMemcpy(v.data(), g->d_updates, kUpdateSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    uint64_t sum = 0;
    for (unsigned long long x : v) sum += x;
    *n = sum;
    return SLAM_OK;
}

int slam_grid_info(slam_grid_t *g, int *size_x, int *size_y, double *resolution, int *origin_x, int *origin_y)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    if (size_x) *size_x = g->gv.sx;
    if (size_y) *size_y = g->gv.sy;
    if (resolution) *resolution = g->gv.res;
    if (origin_x) *origin_x = g->gv.ox;
    if (origin_y) *origin_y = g->gv.oy;
    return SLAM_OK;
}

int slam_grid_window_cell(slam_grid_t *g, int *cell_x, int *cell_y)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    if (cell_x) *cell_x = (int)g->shift_x;
    if (cell_y) *cell_y = (int)g->shift_y;
    return SLAM_OK;
}

int slam_grid_raycast_stats(slam_grid_t *g, int *n_tiles, int *n_items, int *n_segments)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "null handle");
    const int tiles = ((g->gv.sx + kTile - 1) / kTile) * ((g->gv.sy + kTile - 1) / kTile);
    if (n_tiles) *n_tiles = tiles;
    if (n_items) *n_items = 0;
    if (n_segments) *n_segments = 0;
    if (!g->d_tile_off) return SLAM_OK; // no tiled raycast has run yet
    SLAM_HIP(hipDeviceSynchronize());
    std::vector<int> cnt((size_t)tiles);
    SLAM_HIP(hipMemcpy(cnt.data(), g->d_tile_cnt, sizeof(int) * (size_t)tiles, hipMemcpyDeviceToHost));
    long items = 0;
    for (int c : cnt) items += c;
    if (n_items) *n_items = (int)items;
    if (n_segments) SLAM_HIP(hipMemcpy(n_segments, g->d_cursor + tiles, sizeof(int), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_grid_counts_dev(slam_grid_t *g, int32_t **d_planes, size_t *n_ints)
{
    SLAM_REQUIRE(g && d_planes, SLAM_E_INVALID, "slam_grid_counts_dev: bad arguments");
    *d_planes = g->d_planes;
    if (n_ints) *n_ints = 2 * g->cells;
    return SLAM_OK;
}

} // extern "C"
