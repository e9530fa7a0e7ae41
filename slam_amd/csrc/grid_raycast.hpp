// grid_raycast.hpp -- device side of the occupancy grid's raycast (grid.hip includes it, nobody else): beams as integer
// cells, the per-tile work list, and the two walks.
//
// Raycast, tiled implementation: a pre-pass turns every beam into integer
// (x0,y0,x1,y1) cells once; each workgroup owns one 128x128-cell tile for a
// slice of the beams, accumulates hit/miss counts for that tile in LDS (ds_add,
// 16+16 bit packed per cell), and writes the tile back with coalesced global
// atomics -- one per touched cell per workgroup instead of one per traversed
// cell per beam.  Each beam's cells inside a tile come from the closed form of
// the integer Bresenham line, so clipping to the tile cannot change them.
#pragma once
#include "grid_clip.hpp"
#include "grid_view.hpp"

using namespace slam;

namespace {

struct Beam { // integer Bresenham endpoints in window cells; x0 < 0 marks a dropped beam
    short x0, y0, x1, y1;
};
constexpr Beam kDroppedBeam = {-1, 0, 0, 0};

constexpr int kTile = 128;             // cells per tile side
#ifndef SLAM_WALK_UNROLL
#define SLAM_WALK_UNROLL 4
#endif
constexpr int kWalkUnroll = SLAM_WALK_UNROLL; // steps per trip of the raycast walk loop
// Lanes of a block walk STAGGERED: lane j takes (j % kWalkStagger) single steps before the lock-step trips begin (round 5).  The 64
// beams of a block are adjacent beams of ONE scan: near the sensor they run through the same cells, and in lock-step from the same
// start they are on the same cell in the same instruction -- LDS atomics of one instruction to one address are served one after the
// other (bank-conflict share 55 %, VALU busy 35 %).  Staggered, neighbours are a cell or more apart along the beam when they add:
// the raycast call of config 2 0.1325 -> 0.0983 ms with one workgroup per CU, 0.110 -> 0.090 with two (VALU busy 56 %); the pipelined
// step 0.304 -> 0.295 ms.  Measured (tools/exp/stagger_ab.sh, ms per call with one workgroup per CU): steps ahead 2 / 3 / 4 / 6 / 8 /
// 12 / 16 / 32 -> 0.120 / 0.112 / 0.105 / 0.100 / 0.098 / 0.100 / 0.104 / 0.130; whole trips of delay instead (4 steps each), 2 / 4 /
// 6 / 8 / 16-fold -> 0.115 / 0.103 / 0.103 / 0.106 / 0.122.  Bit-exact either way: the adds commute.
#ifndef SLAM_WALK_STAGGER
#define SLAM_WALK_STAGGER 8
#endif
constexpr int kWalkStagger = SLAM_WALK_STAGGER;
constexpr int kTileStride = kTile + 1; // LDS row pitch in words: vertical neighbours fall on adjacent banks
constexpr int kTileThreads = 1024;
constexpr int kChunk = 1024;           // beams per pre-pass workgroup
constexpr int kBlock = 64;             // beams per culling block = one wavefront

__device__ inline Beam make_beam(const GridView &g, float ox, float oy, float ex, float ey)
{
    Beam b = kDroppedBeam;
    int  x1, y1, x0, y0;
    if (!point_cell(g, ex, ey, &x1, &y1)) return b;
    if (!cell_coord(ox, g.res, g.sx / 2, &x0)) return b;
    if (!cell_coord(oy, g.res, g.sy / 2, &y0)) return b;
    if (x0 < 0 || y0 < 0 || x0 >= g.sx || y0 >= g.sy) return b;
    b.x0 = (short)x0;
    b.y0 = (short)y0;
    b.x1 = (short)x1;
    b.y1 = (short)y1;
    return b;
}

// Stores the lane's integer beam and, per wavefront, the bounding box of its
// 64 beams (the culling unit of the tiled raycast: 64 consecutive beams of a
// scan are a narrow wedge).  Wave reduction only: no LDS, no atomics.
__device__ inline void store_beam_and_box(const Beam &b, bool in_range, int i, Beam *beams, int4 *block_box)
{
    if (in_range) beams[i] = b;
    const bool ok = in_range && b.x0 >= 0;
    int lo_x = ok ? min((int)b.x0, (int)b.x1) : 0x7fffffff, lo_y = ok ? min((int)b.y0, (int)b.y1) : 0x7fffffff;
    int hi_x = ok ? max((int)b.x0, (int)b.x1) : -1, hi_y = ok ? max((int)b.y0, (int)b.y1) : -1;
    for (int off = 32; off > 0; off >>= 1) {
        lo_x = min(lo_x, __shfl_xor(lo_x, off));
        lo_y = min(lo_y, __shfl_xor(lo_y, off));
        hi_x = max(hi_x, __shfl_xor(hi_x, off));
        hi_y = max(hi_y, __shfl_xor(hi_y, off));
    }
    if ((threadIdx.x & 63) == 0) block_box[i >> 6] = make_int4(lo_x, lo_y, hi_x, hi_y);
}

__global__ __launch_bounds__(kChunk) void beams_from_rays_kernel(GridView g, const float2 *origin,
                                                                 const float2 *end, int n, Beam *beams,
                                                                 int4 *block_box)
{
    const int  i = blockIdx.x * kChunk + threadIdx.x;
    const bool in = i < n;
    Beam       b = kDroppedBeam;
    if (in) {
        const float2 o = origin[i], e = end[i];
        b = make_beam(g, o.x, o.y, e.x, e.y);
    }
    store_beam_and_box(b, in, i, beams, block_box);
}

__global__ __launch_bounds__(kChunk) void beams_from_scans_kernel(GridView g, const double2 *pts,
                                                                  const int *scan_off, int n_scans,
                                                                  const double *R, const double *t, int n,
                                                                  Beam *beams, int4 *block_box)
{
    const int  i = blockIdx.x * kChunk + threadIdx.x;
    const bool in = i < n;
    Beam       b = kDroppedBeam;
    if (in) {
        // scan of point i: the last s with scan_off[s] <= i.  Scans of a batch are about the same size, so the
        // proportional guess is right or one off: a few steps from there instead of log2(n_scans) dependent loads
        // (the bisection below takes over for ragged batches)
        int lo = (int)(((long long)i * n_scans) / max(n, 1));
        lo = min(max(lo, 0), n_scans - 1);
        int steps = 0;
        while (steps < 4 && scan_off[lo] > i) --lo, ++steps;
        while (steps < 4 && lo + 1 < n_scans && scan_off[lo + 1] <= i) ++lo, ++steps;
        if (scan_off[lo] > i || (lo + 1 < n_scans && scan_off[lo + 1] <= i)) {
            lo = 0;
            int hi = n_scans - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (scan_off[mid] <= i)
                    lo = mid;
                else
                    hi = mid - 1;
            }
        }
        const double *Rs = R + 4 * (size_t)lo, *ts = t + 2 * (size_t)lo;
        const double2 P = pts[i];
        // end point formed as icpPointToPoint.cpp:69-70 forms its query; a rolling window is centred on
        // curPose, so map-frame points are taken relative to it (mls.cpp:36-47 shifts the cloud the same way)
        const double cx = g.rolling ? g.pose_x : 0.0, cy = g.rolling ? g.pose_y : 0.0;
        const double gx = __dadd_rn(__dadd_rn(__dmul_rn(Rs[0], P.x), __dmul_rn(Rs[1], P.y)), ts[0]);
        const double gy = __dadd_rn(__dadd_rn(__dmul_rn(Rs[2], P.x), __dmul_rn(Rs[3], P.y)), ts[1]);
        const float  ex = (float)(g.rolling ? __dsub_rn(gx, cx) : gx), ey = (float)(g.rolling ? __dsub_rn(gy, cy) : gy);
        const float  ox = (float)(g.rolling ? __dsub_rn(ts[0], cx) : ts[0]);
        const float  oy = (float)(g.rolling ? __dsub_rn(ts[1], cy) : ts[1]);
        b = make_beam(g, ox, oy, ex, ey);
    }
    store_beam_and_box(b, in, i, beams, block_box);
}

// one global atomic per traversed cell (baseline implementation)
__global__ __launch_bounds__(256) void raycast_global_kernel(GridView g, const Beam *beams, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned  did = 0;
    int       rlo = 0, rhi = -1;
    if (i < n) {
        const Beam b = beams[i];
        if (b.x0 >= 0) {
            const int  dx = abs(b.x1 - b.x0), dy = abs(b.y1 - b.y0);
            const int  sx = b.x1 > b.x0 ? 1 : -1, sy = b.y1 > b.y0 ? 1 : -1;
            const bool xm = dx >= dy; // the major axis takes a step per cell, the minor one where the error term says so
            const int  du = xm ? dx : dy, dv = xm ? dy : dx;
            int        x = b.x0, y = b.y0, e = du;
            for (int k = 0; k < du; ++k) {
                atomicAdd(&g.misses[storage_index(g, x, y)], 1);
                e += 2 * dv;
                const bool minor = e >= 2 * du;
                e -= minor ? 2 * du : 0;
                x += xm || minor ? sx : 0;
                y += !xm || minor ? sy : 0;
            }
            did = du + 1;
            atomicAdd(&g.hits[storage_index(g, b.x1, b.y1)], 1);
            const int ra = storage_index(g, 0, b.y0) / g.sx, rb = storage_index(g, 0, b.y1) / g.sx;
            const bool wraps = (ra <= rb) != (b.y0 <= b.y1); // the beam crosses the toroidal seam: every row may be touched
            rlo = wraps ? 0 : min(ra, rb);
            rhi = wraps ? g.sy - 1 : max(ra, rb);
        }
    }
    mark_dirty_rows(g.dirty, rlo, rhi);
    block_add_updates(g.updates, did);
}

// Work list for the tiled raycast, built without atomics (so its order is
// deterministic): for every tile the 64-beam blocks whose bounding box overlaps it.
//   tile_items_wg : one workgroup per tile, ballot + popcount over the block boxes; the ids go to the tile's own
//                row of `items` (n_blocks ids wide, so no prefix sum is needed first), the count to cnt[], and the
//                tile's cursor (the next block of its list to hand out) back to 0
//   the raycast workgroups take blocks from a tile's list through that cursor, a chunk at a time.
//   Grids of more than kMaxLdsTiles tiles keep the three-kernel form (count, scan, fill).

__device__ inline bool box_overlaps_tile(const int4 cb, int tx0, int ty0, int tx1, int ty1)
{
    return cb.z >= tx0 && cb.x <= tx1 && cb.w >= ty0 && cb.y <= ty1; // empty boxes have z = w = -1
}

constexpr int kMaxLdsTiles = 2048; // segment offsets of that many tiles fit beside the LDS tile (8 KB)

// Grids of more than kMaxLdsTiles tiles.  FILL: 0 = count only, 1 = write the ids at tile_off[t]
template <int FILL>
__global__ __launch_bounds__(256) void tile_items_kernel(const int4 *block_box, int n_blocks, int tiles_x,
                                                         int n_tiles, int sx, int sy, int *cnt,
                                                         const int *tile_off, int *items)
{
    const int t = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (t >= n_tiles) return;
    const int tx0 = (t % tiles_x) * kTile, ty0 = (t / tiles_x) * kTile;
    const int tx1 = min(tx0 + kTile, sx) - 1, ty1 = min(ty0 + kTile, sy) - 1;
    int       c = 0;
    const int base_out = FILL == 1 ? tile_off[t] : 0;
    for (int base = 0; base < n_blocks; base += 256) { // four independent box loads in flight per lane
        int4 cb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = base + 64 * j + lane;
            cb[j] = ch < n_blocks ? block_box[ch] : make_int4(0, 0, -1, -1);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool               ov = box_overlaps_tile(cb[j], tx0, ty0, tx1, ty1);
            const unsigned long long m = __ballot(ov);
            if (FILL && ov) items[base_out + c + __popcll(m & ((1ull << lane) - 1ull))] = base + 64 * j + lane;
            c += __popcll(m);
        }
    }
    if (FILL != 1 && lane == 0) cnt[t] = c;
}

// The single-pass form with one workgroup of 16 wavefronts per tile: every lane looks at up to four block boxes per
// trip (all loads in flight at once), the wavefronts' match counts go through LDS, and the ids land in the tile's row
// in ascending block order as before (17 dependent trips of one wavefront per tile took 11 us on config 2).
__global__ __launch_bounds__(1024) void tile_items_wg_kernel(const int4 *block_box, int n_blocks, int tiles_x, int sx,
                                                             int sy, int *cnt, int *items, int *cursor)
{
    __shared__ int s_cnt[4][16], s_base;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        s_base = 0;
        cursor[t] = 0;                       // the tile's list is handed out from its start
        if (t == 0) cursor[gridDim.x] = 0;   // behind the cursors: tile write-backs of the launch (slam_grid_raycast_stats)
    }
    const int tx0 = (t % tiles_x) * kTile, ty0 = (t / tiles_x) * kTile;
    const int tx1 = min(tx0 + kTile, sx) - 1, ty1 = min(ty0 + kTile, sy) - 1;
    const int base_out = t * n_blocks;
    for (int base = 0; base < n_blocks; base += 4096) {
        int4 cb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = base + 1024 * j + tid;
            cb[j] = ch < n_blocks ? block_box[ch] : make_int4(0, 0, -1, -1);
        }
        unsigned long long m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = __ballot(box_overlaps_tile(cb[j], tx0, ty0, tx1, ty1));
            if (lane == 0) s_cnt[j][wave] = __popcll(m[j]);
        }
        __syncthreads(); // the counts of this trip (and s_base of the previous one) are visible
        int total = 0; // ids are ordered by (j, wave, lane) = ascending block id
#pragma unroll
        for (int j = 0; j < 4; ++j)
            for (int w = 0; w < 16; ++w) {
                const int c = s_cnt[j][w];
                total += c;
            }
        int run = s_base;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int mine = run;
            for (int w = 0; w < 16; ++w) {
                const int c = s_cnt[j][w];
                mine += w < wave ? c : 0;
                run += c;
            }
            if ((m[j] >> lane) & 1ull)
                items[base_out + mine + __popcll(m[j] & ((1ull << lane) - 1ull))] = base + 1024 * j + tid;
        }
        __syncthreads(); // everyone has read s_cnt and s_base
        if (tid == 0) s_base += total;
    }
    __syncthreads();
    if (tid == 0) cnt[t] = s_base;
}

// Exclusive prefix of the tile counts, by one workgroup of kTileThreads threads: off[t] = cnt[0] + .. + cnt[t - 1] (where
// tile t's list starts), off[n_tiles] = the total.  Wave __shfl_up, the wave sums through LDS, a carry from trip to trip.
// The caller puts a barrier between this and whoever reads off[] written by another thread.
__device__ inline void scan_tile_counts(const int *cnt, int n_tiles, int *off)
{
    __shared__ int s_wsum[kTileThreads / 64], s_carry;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n_tiles; base += kTileThreads) {
        const int i = base + tid;
        const int v = i < n_tiles ? cnt[i] : 0;
        int       x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_wsum[tid >> 6] = x;
        __syncthreads();
        int w = 0;
        for (int k = 0; k < (tid >> 6); ++k) w += s_wsum[k];
        const int incl = s_carry + w + x;
        if (i < n_tiles) off[i] = incl - v;
        __syncthreads();
        if (tid == kTileThreads - 1) s_carry = incl;
        __syncthreads();
    }
    if (tid == 0) off[n_tiles] = s_carry;
}

// grids of more than kMaxLdsTiles tiles: where each tile's list starts (the total behind the last), and the cursors back to 0
__global__ __launch_bounds__(kTileThreads) void tile_scan_kernel(const int *cnt, int n_tiles, int *tile_off, int *cursor)
{
    scan_tile_counts(cnt, n_tiles, tile_off);
    for (int i = threadIdx.x; i <= n_tiles; i += kTileThreads) cursor[i] = 0; // (behind the cursors: tile write-backs of the launch)
}

// Tiled raycast.  A persistent workgroup works on ONE tile at a time: it zeroes a 128x128 tile of packed
// (hits<<16 | misses) counters in LDS, takes 64-beam blocks from the tile's work list a chunk at a time (the tile's
// cursor: one global atomic per chunk), its 16 wavefronts pull the chunk's blocks from an LDS counter, and it keeps
// accumulating in the same LDS tile for as long as the tile has blocks left -- the tile is written back (coalesced
// global atomics) once, when the workgroup leaves it.  Workgroups start spread over the tiles in proportion to the
// tiles' lists (a prefix over the tile counts in LDS) and, when their tile runs dry, move to the tile with the most
// blocks left.  (Round 2 cut the lists into fixed segments of one tile, each zeroed and written back by whoever took it:
// 8.5 write-backs per tile on config 2 -- 30 % of the kernel's instructions and 40 MB of atomic traffic per launch;
// a workgroup that stays is one write-back per workgroup and tile.)
// Within a block every lane owns one beam: it clips the beam's Bresenham step
// range [0, du] to the tile exactly -- the cell of step i has the closed form
//   (u0 + su*i, v0 + sv*floor((2*i*dv + du) / (2*du))),
// so the clipped range and the error term at its first step are two small
// integer divisions, not a walk -- and then all lanes step their beams in
// lock-step with the integer error update (4 integer ops + one ds_add per
// cell).  Clipping by closed form is what makes the tiling invisible in the
// result: the cells are exactly those of the unclipped line.
constexpr int kChunkMin = 8;      // (the visit's chunk log in LDS is sized for it)
constexpr int kChunkDefault = 16; // blocks a workgroup takes from a tile's list at a time, where the caller leaves it to the library
constexpr int kMaxAccBlocks = 1023; // blocks accumulated in the packed LDS counters before a write-back is forced: 64 * 1023 misses of the
                                    // sensor's cell cannot carry into the hit half

template <bool MERGE>
__global__ __launch_bounds__(kTileThreads, 8) void raycast_tiled_kernel(GridView g, const Beam *beams, int n,
                                                                        const int *items, const int *tile_off,
                                                                        int n_tiles, int *cursor, int tiles_x, int chunk,
                                                                        int ablate_arg, const int *cnt, int item_stride)
{
#ifdef SLAM_MEASURE // timing experiments only (tools/ablate.sh): bits switch parts of the kernel off -- wrong counts
    const int ablate = ablate_arg;
#else
    constexpr int ablate = 0;
    (void)ablate_arg;
#endif
    __shared__ __attribute__((aligned(16))) unsigned tile[kTile * kTileStride];
    __shared__ int s_ticket, s_done, s_end;
    __shared__ unsigned long long s_desc[kMaxAccBlocks / kChunkMin]; // the visit's chunk log
    __shared__ int s_off[kMaxLdsTiles + 1];
    __shared__ unsigned long long s_best[kTileThreads / 64];

    const int tid = threadIdx.x, lane = tid & 63;
    // (tile_off != null: a grid of more than kMaxLdsTiles tiles; its lists lie one behind the other and their starts were
    // scanned by tile_scan_kernel.  Otherwise every tile has a row of its own and the prefix is worked out here.)
    const bool in_lds = tile_off == nullptr;
    if (in_lds) {
        scan_tile_counts(cnt, n_tiles, s_off);
        __syncthreads();
    }
    const auto list_start = [&](int t) { return in_lds ? s_off[t] : tile_off[t]; };
    const int  total = list_start(n_tiles);
    unsigned   did = 0;
    int        d_lo = kNoRow, d_hi = -1; // storage rows this lane wrote back
    if (total <= 0 || (ablate & 8)) {
        mark_dirty_rows(g.dirty, d_lo, d_hi);
        block_add_updates(g.updates, did);
        return;
    }
    // where this workgroup starts: the tile that holds its share of all blocks (the last t with list_start(t) <= pos)
    int cur;
    {
        const int pos = (int)(((long long)blockIdx.x * total) / gridDim.x);
        int       lo = 0, hi = n_tiles - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (list_start(mid) <= pos)
                lo = mid;
            else
                hi = mid - 1;
        }
        cur = lo;
    }
    for (int i = tid * 4; i < kTile * kTileStride; i += kTileThreads * 4)
        *reinterpret_cast<uint4 *>(&tile[i]) = make_uint4(0u, 0u, 0u, 0u);

    // writes the LDS tile of tile t back (coalesced: consecutive lanes -> consecutive x of one row) and zeroes it
    const auto flush = [&](int t) {
        const int tx0 = (t % tiles_x) * kTile, ty0 = (t / tiles_x) * kTile;
        for (int i = (ablate & 2) ? kTile * kTile : tid; i < kTile * kTile; i += kTileThreads) {
            const int      lx = i & (kTile - 1), ly = i / kTile;
            const unsigned v = tile[ly * kTileStride + lx];
            if (!v) continue;
            tile[ly * kTileStride + lx] = 0u;
            const int s = storage_index(g, tx0 + lx, ty0 + ly);
            if (ablate & 128) {
                // measurement only (tools/raycast_interleave.sh): what the write-back would cost with {misses, hits} interleaved
                // per cell -- ONE 8-byte atomic per touched cell, the planes' memory taken as cells x 8 bytes (wrong counts)
                atomicAdd(reinterpret_cast<unsigned long long *>(g.hits) + s, ((unsigned long long)(v >> 16) << 32) | (v & 0xffffu));
            } else {
                if (v & 0xffffu) atomicAdd(&g.misses[s], (int)(v & 0xffffu));
                if (v >> 16) atomicAdd(&g.hits[s], (int)(v >> 16));
            }
            int row = ty0 + ly + g.oy; // the storage row of s (storage_index without its division)
            row -= row >= g.sy ? g.sy : 0;
            d_lo = min(d_lo, row);
            d_hi = max(d_hi, row);
        }
        if (tid == 0) atomicAdd(&cursor[n_tiles], 1); // statistics: tile write-backs of the launch
    };

    // One VISIT = the stay of this workgroup on one tile between two write-backs.  Within a visit there is no barrier: a
    // wavefront draws a ticket T from an LDS counter; ticket T is block T % chunk of the visit's chunk T / chunk, and chunk c
    // is the range [base_c, base_c + np_c) of the tile's list that a global atomic on the tile's cursor handed out,
    // published as one 64-bit LDS word {1, np, base}.  Chunks 0 and 1 come from one atomic at the start of the visit; the
    // wavefront that draws the first ticket of chunk c fetches chunk c + 2 -- two chunks of walks ahead of its use, the
    // atomic in flight while the wavefront walks its own block -- once it has seen chunks c and c + 1 full: fetches are
    // therefore issued one after the other's return, the bases grow with c, and the first chunk that is not full ends the
    // list for every later ticket (s_end).  Descriptors are a log, not a ring (one per chunk of the visit: never overwritten
    // while anybody may read them); a visit ends where the log does (kMaxAccBlocks blocks, the limit of the packed LDS
    // counters) or where the tile's list does.  A wavefront never waits while it owes a publication (settle).
    const int  kMaxChunks = kMaxAccBlocks / chunk; // chunks per visit (host: chunk <= kMaxAccBlocks / 2, so at least two)
    const auto publish = [&](int c, int base, int np) { // lane 0 of the fetching wavefront
        __hip_atomic_store(&s_desc[c], (1ull << 48) | ((unsigned long long)(unsigned)np << 32) | (unsigned)base, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
        if (np < chunk) { // the tile's list ends in (np > 0) or before (np == 0) this chunk
            atomicMin(&s_end, np > 0 ? c + 1 : c);
            s_done = 1;
        }
    };
    for (;;) {
        __syncthreads(); // the last visit's walks are in the tile and written back; nobody reads its descriptors any more
        for (int c = tid; c < kMaxChunks; c += kTileThreads) s_desc[c] = 0ull;
        if (tid == 0) {
            s_ticket = 0;
            s_done = 0;
            s_end = kMaxChunks;
        }
        __syncthreads();
        const int t = cur;
        if (tid == 0) { // the visit's first two chunks
            const int have_t = cnt[t];
            const int k = atomicAdd(&cursor[t], 2 * chunk);
            const int np0 = max(0, min(chunk, have_t - k));
            publish(0, k, np0);
            if (np0 == chunk) publish(1, k + chunk, max(0, min(chunk, have_t - k - chunk)));
        }
        const int tile_base = in_lds ? t * item_stride : tile_off[t];
        const int tx0 = (t % tiles_x) * kTile, ty0 = (t / tiles_x) * kTile;
        const int tx1 = min(tx0 + kTile, g.sx) - 1, ty1 = min(ty0 + kTile, g.sy) - 1;

        int  fetch_c = -1, fetch_k = 0; // this wavefront owes the publication of chunk fetch_c; lane 0's atomic returned fetch_k
        auto settle = [&]() {
            if (fetch_c >= 0 && lane == 0) publish(fetch_c, fetch_k, max(0, min(chunk, cnt[t] - fetch_k)));
            fetch_c = -1;
        };
        // descriptor of chunk c, or 0 when the list ends before it
        auto wait_desc = [&](int c) -> unsigned long long {
            for (;;) {
                if (c >= __hip_atomic_load(&s_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return 0ull;
                const unsigned long long d = __hip_atomic_load(&s_desc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (d != 0ull) return d;
                if (fetch_c >= 0)
                    settle(); // never wait while owing: the chunk awaited may hang on this very publication
                else
                    __builtin_amdgcn_s_sleep(1);
            }
        };
        // a wavefront's next block: its beams are requested before the current block is walked (hides the two dependent
        // loads).  Returns false at the end of the visit.
        auto grab = [&](int2 *raw) -> bool {
            int T = 0;
            if (lane == 0) T = atomicAdd(&s_ticket, 1);
            T = __builtin_amdgcn_readfirstlane(T);
            const int c = T / chunk, idx = T - c * chunk;
            if (c >= kMaxChunks) return false; // the visit's log is full: write back, then the same tile again
            const unsigned long long d = wait_desc(c);
            const int np = (int)((d >> 32) & 0xffffu), base = (int)(unsigned)(d & 0xffffffffull);
            if (idx >= np) return false; // the tile's list ends before this block
            if (idx == 0 && np == chunk && c + 2 < kMaxChunks) {
                // first ticket of a full chunk: if the next chunk is full too, fetch the one after it
                const unsigned long long d1 = wait_desc(c + 1);
                if ((int)((d1 >> 32) & 0xffffu) == chunk) {
                    settle(); // (one fetch at a time per wavefront)
                    if (lane == 0) fetch_k = atomicAdd(&cursor[t], chunk);
                    fetch_c = c + 2;
                }
            }
            const int bi = items[tile_base + base + idx] * kBlock + lane;
            *raw = bi < n ? *reinterpret_cast<const int2 *>(&beams[bi]) : make_int2(-1, 0);
            return true;
        };
        int2 raw = make_int2(-1, 0), raw_next = make_int2(-1, 0);
        bool have = grab(&raw);
        while (have) {
            const bool have_next = grab(&raw_next);

            // ---- clip this lane's beam to the tile
            int rem = 0, a = 0, e = 0, dv2 = 0, den = 1, step_u = 0, step_v = 0, to_end = 0;
            const int x0 = (short)(raw.x & 0xffff), y0 = raw.x >> 16;
            const int x1 = (short)(raw.y & 0xffff), y1 = raw.y >> 16;
            const bool maybe = x0 >= 0 && max(x0, x1) >= tx0 && min(x0, x1) <= tx1 && max(y0, y1) >= ty0 &&
                               min(y0, y1) <= ty1; // (a live beam and clip_box_meets_tile)
            if (__any(maybe) && !(ablate & 16)) {
                // (grid_clip.hpp; the reciprocals are the device's own, 1 ulp is ample: see floor_div_small)
                const float    rden = __builtin_amdgcn_rcpf((float)clip_den(x0, y0, x1, y1));
                const float    rdv2 = __builtin_amdgcn_rcpf((float)clip_dv2(x0, y0, x1, y1));
                const TileClip c = clip_beam_to_tile(x0, y0, x1, y1, tx0, ty0, tx1, ty1, kTileStride, rden, rdv2, maybe, ablate);
                rem = c.rem, a = c.a, e = c.e, dv2 = c.dv2, den = c.den, step_u = c.step_u, step_v = c.step_v, to_end = c.to_end;
                did += (unsigned)rem;
            }
            if (ablate & 1) rem = 0;
            // ---- the end cell's hit if the beam ends in this tile (its last step here is then the end cell),
            // then all lanes step their beams' misses together.  Per step: one ds_add and five integer
            // instructions -- the cell is kept as a byte offset, the error term biased by 2^32 - den so that the
            // carry of `+= dv2` is the test `e + dv2 >= den` -- in trips of kWalkUnroll steps for the lanes that
            // have that many left (no per-step predicate), then the remainders.
            const bool hit_here = rem > 0 && to_end < rem;
            if (hit_here) atomicAdd(&tile[(y1 - ty0) * kTileStride + (x1 - tx0)], 0x10000u);
            int            miss = rem - (hit_here ? 1 : 0);
            unsigned char *tb = reinterpret_cast<unsigned char *>(tile);
            int            a4 = a * 4;
            const int      su4 = step_u * 4, sv4 = step_v * 4;
            const unsigned bias = 0u - (unsigned)den, udv2 = (unsigned)dv2;
            unsigned       eu = (unsigned)e + bias;
            const auto     advance = [&]() {
                const unsigned e2 = eu + udv2;
                const bool     carry = e2 < eu; // e + dv2 >= den
                a4 += su4 + (carry ? sv4 : 0);
                eu = e2 + (carry ? bias : 0u);
            };
            // MERGE: 64 consecutive beams of a scan leave the sensor through the same cells for their first ~230
            // steps (adjacent beams are 0.25 degrees apart), and LDS atomics of one instruction to one address are
            // served one after the other.  Lanes are ordered by angle, so lanes on the same cell are neighbours: the
            // first lane of a run adds the run's length, the others add nothing.  A step on which every lane has a
            // cell of its own (the far field) costs the compare only.
            const auto add_miss = [&]() {
                if (!MERGE) {
                    atomicAdd(reinterpret_cast<unsigned *>(tb + a4), 1u);
                    return;
                }
                const int  prev = __builtin_amdgcn_update_dpp(-1, a4, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
                const bool leader = a4 != prev; // also after a lane that is not stepping (its value does not arrive)
                const unsigned long long on = __ballot(true), lead = __ballot(leader);
                if (lead == on) {
                    atomicAdd(reinterpret_cast<unsigned *>(tb + a4), 1u);
                } else {
                    const unsigned long long ends = lead | ~on; // a run ends before the next leader or idle lane
                    const unsigned long long rest = lane == 63 ? 0ull : ends >> (lane + 1);
                    const unsigned run = rest ? (unsigned)__builtin_ctzll(rest) + 1u : (unsigned)(64 - lane);
                    if (leader) atomicAdd(reinterpret_cast<unsigned *>(tb + a4), run);
                }
            };
#pragma unroll
            for (int k = 0; k < kWalkStagger - 1; ++k) { // the stagger: lane j is j % kWalkStagger cells ahead when the trips begin
                if (lane % kWalkStagger > k && miss > 0) {
                    add_miss();
                    advance();
                    --miss;
                }
            }
            while (__any(miss >= kWalkUnroll)) {
                if (miss >= kWalkUnroll) {
#pragma unroll
                    for (int k = 0; k < kWalkUnroll; ++k) {
                        add_miss();
                        advance();
                    }
                    miss -= kWalkUnroll;
                }
            }
#pragma unroll
            for (int k = 0; k < kWalkUnroll - 1; ++k) {
                if (miss > k) add_miss();
                advance(); // a finished lane's cell is not used again
            }
            settle(); // (after the walk: the fetch's round trip is behind it by now)
            have = have_next;
            raw = raw_next;
        }
        settle(); // nothing fetched may stay unpublished: others wait for it
        __syncthreads(); // every wavefront has found the end of the visit
        flush(t);
        if (s_done == 0) continue; // the visit's log was full and the tile has blocks left: the same tile again, fresh counters
        // this tile has nothing left to hand out: on to the tile with the most blocks left, if any
        unsigned long long best = 0ull;
        for (int u = tid; u < n_tiles; u += kTileThreads) {
            const int have_u = cnt[u];
            const int taken = __hip_atomic_load(&cursor[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int left = have_u - min(have_u, taken);
            const unsigned long long key = ((unsigned long long)(unsigned)left << 32) | (unsigned)u;
            best = left > 0 && key > best ? key : best;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        if (lane == 0) s_best[tid >> 6] = best;
        __syncthreads();
        best = 0ull;
        for (int w = 0; w < kTileThreads / 64; ++w) best = s_best[w] > best ? s_best[w] : best;
        if (best == 0ull) break; // every list is handed out (what is still being walked belongs to others)
        cur = (int)(unsigned)(best & 0xffffffffull);
    }
    mark_dirty_rows(g.dirty, d_lo, d_hi);
    block_add_updates(g.updates, did);
}

} // namespace
