// csm.hip -- correlative scan matcher (slam_csm_*, docs/CSM.md): per-class u8 score tables T on one global lattice, their
// D x D sliding maximum W, and an exact two-level search over (angle, y, x) candidates.
//
// A match is six launches on the caller's stream and no host wait: every bound U (csm_coarse_kernel, which also keeps the
// largest per scan), the top block at full resolution (csm_blocks_kernel: its best score is the lower bound L), the blocks
// with U >= L appended to a list (csm_select_kernel), those blocks at full resolution (csm_blocks_kernel again, a fixed
// grid striding over the list), and the answer (csm_finish_kernel).  Scores are int32 sums of table bytes; the reduction is
// an atomicMax on score << 32 | ~flat_index, so neither the list's order nor the order of the workgroups shows in the result.
// The one floating-point step, point -> cell at an angle, is spelled with __dmul_rn / __dadd_rn and an IEEE division; cos and
// sin come from the host (slam_csm_angles).
//
// slam_csm_match_post* add the posterior of that answer (docs/CSM.md section 6) in four more launches: the candidates within
// a score margin of the winner, enumerated exactly from the same bounds, summed into int64 moments and a second-mode key.
#include <cmath>
#include <cstring>
#include <new>

#include "common.hpp"
#include "device_mem.hpp"

using namespace slam;

namespace {

constexpr int    kChunk = 1024;           // scan points staged in LDS at a time (8 KB)
constexpr int    kNo = -(1 << 30);        // staged row of a point that scores nothing: no row + b reaches the table
constexpr int    kTileRows = 8;           // candidates along b per lane of the tile kernel
constexpr int    kTileW = 64, kTileH = 4 * kTileRows;
constexpr int    kCoarsePer = 2;          // blocks per lane of the coarse kernel
constexpr int    kBlockPer = 4;           // candidates per lane of the block kernel: D * D <= 64 * kBlockPer
constexpr int    kMaxD = 16, kMaxK = 64;
constexpr double kCellLimit = 1073741824.0; // 2^30
constexpr size_t kMaxTableBytes = (size_t)1 << 28;

struct Tab {
    const uint8_t *v;
    int            ox, oy, w, h; // w = 0: no table
};

struct Geom {
    Tab    T[2], W[2];
    double res;
    int    half_x, half_y, nx, ny, nth, D, nbx, nby;
};

// one scan of a batch; off == nullptr: the single scan [0, n) with n_ga points of class GA
struct Scans {
    const double  *pts;
    const int32_t *off, *nga;
    int            n, n_ga;
    const double  *t0, *cs;
};

// the posterior (docs/CSM.md section 6)
constexpr int kPostSums = 11; // n_within, m0, m1[3], m2[6]
constexpr int kPostTable = 257; // weights: deficit d of margin M reads entry d * 256 / M

struct PostAcc {
    long long          sum[kPostSums];
    unsigned long long second; // score << 32 | ~flat of the best candidate outside the exclusion box; 0 = none
    int                margin, pad;
};

struct PostCfg {
    int    margin_per_point, excl_xy, excl_theta;
    double theta_step;
};

__device__ inline bool cell_of(double v, double res, int &c)
{
    const double f = floor(v / res);
    if (!(fabs(f) <= kCellLimit)) return false; // NaN, infinite or beyond the lattice
    c = (int)f;
    return true;
}

__device__ inline void scan_range(const Scans &S, int s, int &first, int &n, int &n_ga)
{
    if (S.off) {
        first = S.off[s];
        n = S.off[s + 1] - first;
        n_ga = S.nga[s];
    } else {
        first = 0, n = S.n, n_ga = S.n_ga;
    }
    n = n < 0 ? 0 : n;
    n_ga = n_ga < 0 ? 0 : (n_ga > n ? n : n_ga);
}

// the cell of scan point i at (c, s, t0); false: the point is not counted
__device__ inline bool point_cell(const Tab *tabs, const double *pts, int first, int i, int n_ga, double c, double s, double tx, double ty,
                                  double res, int &cx, int &cy)
{
    if (tabs[i < n_ga ? 0 : 1].w == 0) return false;
    const double px = pts[2 * (size_t)(first + i)], py = pts[2 * (size_t)(first + i) + 1];
    const double qx = __dadd_rn(__dsub_rn(__dmul_rn(c, px), __dmul_rn(s, py)), tx);
    const double qy = __dadd_rn(__dadd_rn(__dmul_rn(s, px), __dmul_rn(c, py)), ty);
    return cell_of(qx, res, cx) && cell_of(qy, res, cy);
}

// Points [base, base + cn) of the scan into LDS as (column, row) of candidate (0, 0) in the table of their class (`tabs`: T or W).
__device__ inline void stage(const Geom &G, const Tab *tabs, const double *pts, int first, int base, int cn, int n_ga, double c, double s,
                             double tx, double ty, int2 *cells, int threads)
{
    for (int j = threadIdx.x; j < cn; j += threads) {
        int  cx, cy;
        int2 out = make_int2(0, kNo);
        if (point_cell(tabs, pts, first, base + j, n_ga, c, s, tx, ty, G.res, cx, cy)) {
            const Tab      &t = tabs[base + j < n_ga ? 0 : 1];
            const long long rx = (long long)cx - t.ox - G.half_x, ry = (long long)cy - t.oy - G.half_y;
            if (rx > kNo && rx < -(long long)kNo && ry > kNo && ry < -(long long)kNo) out = make_int2((int)rx, (int)ry);
        }
        cells[j] = out;
    }
}

// The walk every search kernel makes over a scan at (c, s, t0): the points staged kChunk at a time by the workgroup's
// `threads` lanes, then every lane over all of them, class GA before class NGA: body(cell, table of its class).
template <class Body>
__device__ __forceinline__ void walk(const Geom &G, const Tab *tabs, const double *pts, int first, int n, int n_ga, double c, double s, double tx,
                                     double ty, int2 *cells, int threads, Body body)
{
    for (int base = 0; base < n; base += kChunk) {
        const int cn = n - base < kChunk ? n - base : kChunk;
        __syncthreads();
        stage(G, tabs, pts, first, base, cn, n_ga, c, s, tx, ty, cells, threads);
        __syncthreads();
        const int split = n_ga - base < 0 ? 0 : (n_ga - base > cn ? cn : n_ga - base);
        for (int cl = 0; cl < 2; ++cl) {
            const Tab t = tabs[cl];
            const int j1 = cl ? cn : split;
            for (int j = cl ? split : 0; j < j1; ++j) body(cells[j], t);
        }
    }
}

// (cos, sin) of angle k of scan s
__device__ inline double2 cos_sin(const Geom &G, const Scans &S, int s, int k)
{
    return make_double2(S.cs[((size_t)s * G.nth + k) * 2], S.cs[((size_t)s * G.nth + k) * 2 + 1]);
}

// the flat index of candidate (k, b, a) and back
__device__ inline unsigned flat_of(const Geom &G, int k, int b, int a) { return ((unsigned)k * G.ny + b) * G.nx + a; }

__device__ inline void unflat(const Geom &G, unsigned flat, int &k, int &b, int &a) { k = flat / (G.nx * G.ny), b = flat / G.nx % G.ny, a = flat % G.nx; }

__device__ inline unsigned long long key_of(int score, unsigned flat) { return ((unsigned long long)(unsigned)score << 32) | (unsigned)~flat; }

__device__ inline unsigned long long wave_max(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---------------------------------------------------------------- tables
__global__ void csm_model_cells_kernel(const double *m, int n, double res, int2 *cells, int *bbox)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int  cx, cy;
    int2 out = make_int2(0, kNo); // kNo in y: the point takes no part
    if (cell_of(m[2 * (size_t)i], res, cx) && cell_of(m[2 * (size_t)i + 1], res, cy)) {
        out = make_int2(cx, cy);
        atomicMin(&bbox[0], cx), atomicMax(&bbox[1], cx), atomicMin(&bbox[2], cy), atomicMax(&bbox[3], cy);
    }
    cells[i] = out;
}

// one thread per (point, stamp entry): every write lies inside the window, which is the bounding box widened by K
__global__ void csm_scatter_kernel(const int2 *cells, int n, const uint8_t *stamp, int K, int ox, int oy, int w, int h, unsigned *plane)
{
    const int       S = 2 * K + 1;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)n * S * S) return;
    const int  p = (int)(g / (S * S)), e = (int)(g % (S * S));
    const int2 c = cells[p];
    const unsigned v = stamp[e];
    if (c.y == kNo || v == 0) return;
    const int col = c.x + e % S - K - ox, row = c.y + e / S - K - oy;
    if (col >= 0 && col < w && row >= 0 && row < h) atomicMax(&plane[(size_t)row * w + col], v);
}

__global__ void csm_pack_kernel(const unsigned *plane, size_t n, uint8_t *T)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) T[i] = (uint8_t)plane[i];
}

// W[u, v] = max over 0 <= i, j < D of T[u + i, v + j]; W's window is T's widened by D - 1 towards smaller indices
__global__ void csm_slide_kernel(const uint8_t *T, int w, int h, int D, uint8_t *W)
{
    const int    ww = w + D - 1, wh = h + D - 1;
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)ww * wh) return;
    const int u = (int)(g % ww) - (D - 1), v = (int)(g / ww) - (D - 1); // in T's window
    int       best = 0;
    for (int j = 0; j < D; ++j)
        for (int i = 0; i < D; ++i) {
            const int x = u + i, y = v + j;
            if (x >= 0 && x < w && y >= 0 && y < h) {
                const int t = T[(size_t)y * w + x];
                best = t > best ? t : best;
            }
        }
    W[g] = (uint8_t)best;
}

// ---------------------------------------------------------------- the exhaustive form
// One workgroup per (tile of 64 a x 32 b, angle, scan): lanes along a, every lane kTileRows rows of b.  For one point a wave
// reads consecutive bytes of kTileRows table rows; the point is an LDS broadcast.  Writes the volume and / or offers the best key.
__global__ __launch_bounds__(256) void csm_tiles_kernel(Geom G, Scans S, int32_t *vol, unsigned long long *best)
{
    __shared__ int2 cells[kChunk];
    const int       tiles_x = (G.nx + kTileW - 1) / kTileW;
    const int       k = blockIdx.y, s = blockIdx.z;
    int             first, n, n_ga;
    scan_range(S, s, first, n, n_ga);
    if (n < 5) return;
    const int     a = (blockIdx.x % tiles_x) * kTileW + (threadIdx.x & 63);
    const int     b0 = (blockIdx.x / tiles_x) * kTileH + (threadIdx.x >> 6) * kTileRows;
    const double  tx = S.t0[2 * s], ty = S.t0[2 * s + 1];
    const double2 cs = cos_sin(G, S, s, k);
    int           acc[kTileRows];
#pragma unroll
    for (int r = 0; r < kTileRows; ++r) acc[r] = 0;
    walk(G, G.T, S.pts, first, n, n_ga, cs.x, cs.y, tx, ty, cells, 256, [&](int2 q, const Tab &t) {
        const int col = q.x + a, row0 = q.y + b0;
        if ((unsigned)col < (unsigned)t.w) {
#pragma unroll
            for (int r = 0; r < kTileRows; ++r)
                if ((unsigned)(row0 + r) < (unsigned)t.h) acc[r] += t.v[(size_t)(row0 + r) * t.w + col];
        }
    });
    unsigned long long key = 0;
    if (a < G.nx) {
#pragma unroll
        for (int r = 0; r < kTileRows; ++r)
            if (b0 + r < G.ny) {
                const unsigned flat = flat_of(G, k, b0 + r, a);
                if (vol) vol[flat] = acc[r];
                const unsigned long long kk = key_of(acc[r], flat);
                key = kk > key ? kk : key;
            }
    }
    if (best) {
        key = wave_max(key);
        if ((threadIdx.x & 63) == 0 && key) atomicMax(&best[s], key);
    }
}

// ---------------------------------------------------------------- the two-level form
// One wave per (group of 128 blocks, angle, scan): U of kCoarsePer blocks per lane, and the scan's largest (U, block).
__global__ __launch_bounds__(64) void csm_coarse_kernel(Geom G, Scans S, int32_t *U, unsigned long long *top)
{
    __shared__ int2 cells[kChunk];
    const int       nb = G.nbx * G.nby, groups = (nb + 64 * kCoarsePer - 1) / (64 * kCoarsePer);
    const int       k = blockIdx.x / groups, grp = blockIdx.x % groups, s = blockIdx.y;
    int             first, n, n_ga;
    scan_range(S, s, first, n, n_ga);
    if (n < 5) return;
    const double  tx = S.t0[2 * s], ty = S.t0[2 * s + 1];
    const double2 cs = cos_sin(G, S, s, k);
    int           blk[kCoarsePer], dx[kCoarsePer], dy[kCoarsePer], acc[kCoarsePer];
#pragma unroll
    for (int r = 0; r < kCoarsePer; ++r) {
        blk[r] = (grp * kCoarsePer + r) * 64 + threadIdx.x;
        dx[r] = (blk[r] % G.nbx) * G.D, dy[r] = (blk[r] / G.nbx) * G.D; // (a block beyond nb reads rows that may exist: it is not written)
        acc[r] = 0;
    }
    walk(G, G.W, S.pts, first, n, n_ga, cs.x, cs.y, tx, ty, cells, 64, [&](int2 q, const Tab &t) {
#pragma unroll
        for (int r = 0; r < kCoarsePer; ++r) {
            const int col = q.x + dx[r], row = q.y + dy[r];
            if ((unsigned)col < (unsigned)t.w && (unsigned)row < (unsigned)t.h) acc[r] += t.v[(size_t)row * t.w + col];
        }
    });
    unsigned long long key = 0;
#pragma unroll
    for (int r = 0; r < kCoarsePer; ++r)
        if (blk[r] < nb) {
            const unsigned f = (unsigned)k * nb + blk[r];
            U[(size_t)s * G.nth * nb + f] = acc[r];
            const unsigned long long kk = key_of(acc[r], f);
            key = kk > key ? kk : key;
        }
    key = wave_max(key);
    if (threadIdx.x == 0 && key) atomicMax(&top[s], key);
}

// Block f = (k N_by + B) N_bx + A at full resolution by one wave: lane c of D * D holds candidates c, c + 64, ... in its
// kBlockPer registers, candidate (a, b) = (A D + c % D, B D + c / D) with score sc; a = -1: there is none (beyond D * D, or
// missing from a ragged block).
__device__ __forceinline__ void eval_block(const Geom &G, const Scans &S, int s, int first, int n, int n_ga, double tx, double ty, unsigned f,
                                           int2 *cells, int &k, int (&a)[kBlockPer], int (&b)[kBlockPer], int (&sc)[kBlockPer])
{
    const int nb = G.nbx * G.nby, A = (f % nb) % G.nbx, B = (f % nb) / G.nbx;
    k = f / nb;
    const double2 cs = cos_sin(G, S, s, k);
#pragma unroll
    for (int r = 0; r < kBlockPer; ++r) {
        const int cnd = r * 64 + threadIdx.x;
        a[r] = A * G.D + cnd % G.D, b[r] = B * G.D + cnd / G.D, sc[r] = 0;
        if (cnd >= G.D * G.D || a[r] >= G.nx || b[r] >= G.ny) a[r] = -1;
    }
    walk(G, G.T, S.pts, first, n, n_ga, cs.x, cs.y, tx, ty, cells, 64, [&](int2 q, const Tab &t) {
#pragma unroll
        for (int r = 0; r < kBlockPer; ++r) {
            const int col = q.x + a[r], row = q.y + b[r];
            if (a[r] >= 0 && (unsigned)col < (unsigned)t.w && (unsigned)row < (unsigned)t.h) sc[r] += t.v[(size_t)row * t.w + col];
        }
    });
}

// One wave per block (eval_block), its best candidate offered to the scan's key.  list == nullptr: the scan's top block alone
// (grid.x = 1); else the wave strides over the scan's list.
__global__ __launch_bounds__(64) void csm_blocks_kernel(Geom G, Scans S, const unsigned long long *top, const int32_t *list, const int32_t *count,
                                                        unsigned long long *best)
{
    __shared__ int2 cells[kChunk];
    const int       s = blockIdx.y;
    int             first, n, n_ga;
    scan_range(S, s, first, n, n_ga);
    if (n < 5) return;
    const int    items = list ? count[s] : 1;
    const double tx = S.t0[2 * s], ty = S.t0[2 * s + 1];
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        int k, a[kBlockPer], b[kBlockPer], sc[kBlockPer];
        const unsigned f = list ? (unsigned)list[(size_t)s * G.nth * G.nbx * G.nby + it] : ~(unsigned)top[s];
        eval_block(G, S, s, first, n, n_ga, tx, ty, f, cells, k, a, b, sc);
        unsigned long long key = 0;
#pragma unroll
        for (int r = 0; r < kBlockPer; ++r)
            if (a[r] >= 0) {
                const unsigned long long kk = key_of(sc[r], flat_of(G, k, b[r], a[r]));
                key = kk > key ? kk : key;
            }
        key = wave_max(key);
        if (threadIdx.x == 0 && key) atomicMax(&best[s], key);
    }
}

// The blocks of every scan that are evaluated next, appended to its list in any order.  kKeepMatch: every block whose bound
// reaches the lower bound L = best (>=: a tie with the best so far must survive), the top block excepted: it gave L.
// kKeepWithin: every block that can hold a candidate with S >= S* - M, that is U >= S* - M, the top block included.
// kKeepAll: every block (the exhaustive form has no bounds to read).
enum Keep { kKeepMatch, kKeepWithin, kKeepAll };

__global__ void csm_select_kernel(Geom G, Scans S, Keep keep, const int32_t *U, const unsigned long long *top, const unsigned long long *best,
                                  const PostAcc *acc, int32_t *list, int32_t *count)
{
    const int per = G.nth * G.nbx * G.nby, s = blockIdx.y;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    int       first, n, n_ga;
    scan_range(S, s, first, n, n_ga);
    if (n < 5 || f >= per) return;
    const int score = (int)(best[s] >> 32);
    bool      in = true;
    if (keep == kKeepMatch) in = U[(size_t)s * per + f] >= score && (unsigned)f != ~(unsigned)top[s];
    if (keep == kKeepWithin) in = U[(size_t)s * per + f] >= (long long)score - acc[s].margin;
    if (in) list[(size_t)s * per + atomicAdd(&count[s], 1)] = f;
}

// The points of the scan that have a cell at (c, s, t0), counted by a workgroup of 256; every lane gets the count.
__device__ inline int points_counted(const Geom &G, const Scans &S, int first, int n, int n_ga, double2 cs, double tx, double ty)
{
    __shared__ int counted;
    if (threadIdx.x == 0) counted = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        int cx, cy;
        mine += point_cell(G.T, S.pts, first, i, n_ga, cs.x, cs.y, tx, ty, G.res, cx, cy) ? 1 : 0;
    }
    atomicAdd(&counted, mine);
    __syncthreads();
    return counted;
}

// the answer of scan s: the winner's indices, the points counted at its angle, the pose
__global__ __launch_bounds__(256) void csm_finish_kernel(Geom G, Scans S, const unsigned long long *best, const int32_t *count, int all_blocks,
                                                         const double *R0, double *R, double *t, slam_csm_result *res)
{
    const int s = blockIdx.x;
    int       first, n, n_ga;
    scan_range(S, s, first, n, n_ga);
    slam_csm_result out = {0, 0, 0, -1, 0, 0, 0};
    if (n < 5) {
        if (threadIdx.x == 0) { // (R and t may be the arrays of the initial pose)
            for (int i = 0; i < 4; ++i) R[4 * s + i] = R0[4 * s + i];
            t[2 * s] = S.t0[2 * s], t[2 * s + 1] = S.t0[2 * s + 1];
            if (res) res[s] = out;
        }
        return;
    }
    unflat(G, ~(unsigned)best[s], out.k, out.b, out.a);
    out.score = (int)(best[s] >> 32);
    const double  tx = S.t0[2 * s], ty = S.t0[2 * s + 1];
    const double2 cs = cos_sin(G, S, s, out.k);
    // (its barriers also put every lane's read of t0 before the write of t, which may be the same array)
    out.n_points = points_counted(G, S, first, n, n_ga, cs, tx, ty);
    if (threadIdx.x == 0) {
        out.max_score = 255 * out.n_points;
        out.blocks_evaluated = all_blocks ? all_blocks : count[s] + 1;
        R[4 * s] = cs.x, R[4 * s + 1] = -cs.y, R[4 * s + 2] = cs.y, R[4 * s + 3] = cs.x;
        t[2 * s] = __dadd_rn(tx, __dmul_rn((double)(out.a - G.half_x), G.res));
        t[2 * s + 1] = __dadd_rn(ty, __dmul_rn((double)(out.b - G.half_y), G.res));
        if (res) res[s] = out;
    }
}

// ---------------------------------------------------------------- the posterior (docs/CSM.md section 6)
// After a match: the margin M from the points counted at the winning angle (csm_post_prepare_kernel), every block whose bound
// reaches S* - M (csm_select_kernel), those blocks at full resolution into eleven int64 sums and the second mode's key
// (csm_post_accumulate_kernel), and the f64 finish (csm_post_finish_kernel).  Integer sums: any order gives the same bits.
__device__ inline long long wave_sum(long long v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// scan s: clears its sums, its second-mode key and its list counter, and sets M = margin_per_point * n_points
__global__ __launch_bounds__(256) void csm_post_prepare_kernel(Geom G, Scans S, PostCfg C, const unsigned long long *best, PostAcc *acc, int32_t *count)
{
    const int s = blockIdx.x;
    int       first, n, n_ga, counted = 0;
    scan_range(S, s, first, n, n_ga);
    if (n >= 5) {
        int k, b, a;
        unflat(G, ~(unsigned)best[s], k, b, a);
        counted = points_counted(G, S, first, n, n_ga, cos_sin(G, S, s, k), S.t0[2 * s], S.t0[2 * s + 1]);
    }
    if (threadIdx.x == 0) {
        PostAcc z;
        for (int i = 0; i < kPostSums; ++i) z.sum[i] = 0;
        z.second = 0, z.margin = C.margin_per_point * counted, z.pad = 0;
        acc[s] = z;
        count[s] = 0;
    }
}

// One wave per listed block (eval_block), then every lane's candidates into the weight and the eleven terms.  A wave keeps
// the sums of all the items it strides over and adds them to the scan's once.
__global__ __launch_bounds__(64) void csm_post_accumulate_kernel(Geom G, Scans S, PostCfg C, const unsigned long long *best, const int32_t *list,
                                                                 const int32_t *count, const uint32_t *wtab, PostAcc *acc)
{
    __shared__ int2 cells[kChunk];
    const int       s = blockIdx.y;
    int             first, n, n_ga;
    scan_range(S, s, first, n, n_ga);
    if (n < 5) return;
    const int items = count[s];
    if ((int)blockIdx.x >= items) return;
    const double tx = S.t0[2 * s], ty = S.t0[2 * s + 1];
    const int    top = (int)(best[s] >> 32), M = acc[s].margin;
    int          wk, wb, wa;
    unflat(G, ~(unsigned)best[s], wk, wb, wa);
    long long          sum[kPostSums];
    unsigned long long key = 0;
#pragma unroll
    for (int i = 0; i < kPostSums; ++i) sum[i] = 0;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        int k, a[kBlockPer], b[kBlockPer], sc[kBlockPer];
        eval_block(G, S, s, first, n, n_ga, tx, ty, (unsigned)list[(size_t)s * G.nth * G.nbx * G.nby + it], cells, k, a, b, sc);
#pragma unroll
        for (int r = 0; r < kBlockPer; ++r) {
            const int d = top - sc[r];
            if (a[r] < 0 || d > M) continue;
            const int       j = M > 0 && d > 0 ? (int)(((long long)d * 256) / M) : 0;
            const long long w = wtab[j], o[3] = {a[r] - wa, b[r] - wb, k - wk};
            sum[0] += 1, sum[1] += w;
            sum[2] += w * o[0], sum[3] += w * o[1], sum[4] += w * o[2];
            sum[5] += w * o[0] * o[0], sum[6] += w * o[0] * o[1], sum[7] += w * o[0] * o[2];
            sum[8] += w * o[1] * o[1], sum[9] += w * o[1] * o[2], sum[10] += w * o[2] * o[2];
            if (o[0] > C.excl_xy || o[0] < -C.excl_xy || o[1] > C.excl_xy || o[1] < -C.excl_xy || o[2] > C.excl_theta || o[2] < -C.excl_theta) {
                const unsigned long long kk = key_of(sc[r], flat_of(G, k, b[r], a[r]));
                key = kk > key ? kk : key;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kPostSums; ++i) sum[i] = wave_sum(sum[i]);
    key = wave_max(key);
    if (threadIdx.x == 0) {
        for (int i = 0; i < kPostSums; ++i)
            if (sum[i]) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[s].sum[i]), (unsigned long long)sum[i]);
        if (key) atomicMax(&acc[s].second, key);
    }
}

// one lane per scan: the sums into mean and covariance, every operation rounded on its own
__global__ void csm_post_finish_kernel(Geom G, Scans S, PostCfg C, int n_scans, const unsigned long long *best, const PostAcc *acc, const int32_t *count,
                                       slam_csm_posterior *post)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_scans) return;
    int first, n, n_ga;
    scan_range(S, s, first, n, n_ga);
    slam_csm_posterior out;
    out.valid = 0, out.n_within = 0, out.margin = 0, out.blocks_evaluated = 0;
    out.second_score = -1, out.second_k = 0, out.second_a = 0, out.second_b = 0;
    out.m0 = 0;
    for (int i = 0; i < 3; ++i) out.m1[i] = 0, out.mean[i] = 0.0;
    for (int i = 0; i < 6; ++i) out.m2[i] = 0, out.cov[i] = 0.0;
    if (n >= 5) {
        const PostAcc &a = acc[s];
        out.valid = 1, out.n_within = (int)a.sum[0], out.margin = a.margin, out.blocks_evaluated = count[s];
        if (a.second) {
            out.second_score = (int)(a.second >> 32);
            unflat(G, ~(unsigned)a.second, out.second_k, out.second_b, out.second_a);
        }
        out.m0 = a.sum[1];
        for (int i = 0; i < 3; ++i) out.m1[i] = a.sum[2 + i];
        for (int i = 0; i < 6; ++i) out.m2[i] = a.sum[5 + i];
        const double f0 = (double)out.m0, u[3] = {G.res, G.res, C.theta_step};
        double       mc[3];
        for (int i = 0; i < 3; ++i) {
            mc[i] = (double)out.m1[i] / f0;
            out.mean[i] = __dmul_rn(mc[i], u[i]);
        }
        int ij = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j, ++ij) {
                const double cc = __dsub_rn((double)out.m2[ij] / f0, __dmul_rn(mc[i], mc[j]));
                out.cov[ij] = __dmul_rn(__dmul_rn(cc, u[i]), u[j]);
            }
    }
    post[s] = out;
}

// ---------------------------------------------------------------- the pose-set scorer (docs/GRID_MATCH.md section 3)
// Every pose has a rotation of its own, so no cell is shared between poses as walk shares them between translations: the raw
// points are staged instead, kChunk at a time (16 KB), lanes lie along poses with (c, s, tx, ty) in registers, and a point is
// an LDS broadcast.  One wave per workgroup: no cross-lane reduction, no atomics, the same bits on every run.  A lane takes
// kPosePer points at a time: their cells first, then their table bytes together, so that kPosePer loads are in flight and not
// one (a point without a byte -- no cell, or a cell outside the table -- reads byte 0 of the table and adds nothing).
constexpr int kPosePer = 4;

__global__ __launch_bounds__(64) void csm_score_poses_kernel(Geom G, const double *pts, int n, int n_ga, const double *poses, int n_poses,
                                                             int32_t *score, int32_t *counted)
{
    __shared__ double raw[2 * kChunk];
    const int  p = blockIdx.x * 64 + threadIdx.x;
    const bool live = p < n_poses;
    double     c = 0.0, s = 0.0, tx = 0.0, ty = 0.0;
    if (live) c = poses[4 * (size_t)p], s = poses[4 * (size_t)p + 1], tx = poses[4 * (size_t)p + 2], ty = poses[4 * (size_t)p + 3];
    int acc = 0, cnt = 0;
    for (int base = 0; base < n; base += kChunk) {
        const int cn = n - base < kChunk ? n - base : kChunk;
        __syncthreads();
        for (int j = threadIdx.x; j < 2 * cn; j += 64) raw[j] = pts[2 * (size_t)base + j];
        __syncthreads();
        if (!live) continue;
        const int split = n_ga - base < 0 ? 0 : (n_ga - base > cn ? cn : n_ga - base);
        for (int cl = 0; cl < 2; ++cl) {
            const Tab t = G.T[cl];
            const int j1 = cl ? cn : split;
            if (t.w == 0) continue; // a class without a table: point_cell counts none of its points
            for (int j = cl ? split : 0; j < j1; j += kPosePer) {
                unsigned at[kPosePer];
                bool     in[kPosePer];
#pragma unroll
                for (int r = 0; r < kPosePer; ++r) {
                    int cx, cy;
                    at[r] = 0, in[r] = false;
                    if (j + r < j1 && point_cell(G.T, raw, 0, j + r, split, c, s, tx, ty, G.res, cx, cy)) {
                        ++cnt;
                        const long long col = (long long)cx - t.ox, row = (long long)cy - t.oy;
                        if ((unsigned long long)col < (unsigned long long)t.w && (unsigned long long)row < (unsigned long long)t.h)
                            at[r] = (unsigned)row * (unsigned)t.w + (unsigned)col, in[r] = true; // w h <= 2^28
                    }
                }
#pragma unroll
                for (int r = 0; r < kPosePer; ++r) {
                    const int v = t.v[at[r]];
                    acc += in[r] ? v : 0;
                }
            }
        }
    }
    if (live) score[p] = acc, counted[p] = cnt;
}

inline unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

inline int tile_count(const Geom &G) { return ((G.nx + kTileW - 1) / kTileW) * ((G.ny + kTileH - 1) / kTileH); }

// workgroups striding over one scan's list in csm_blocks_kernel and csm_post_accumulate_kernel
inline int list_stride(int n_scans)
{
    const int stride = 4096 / n_scans;
    return stride < 8 ? 8 : (stride > 1024 ? 1024 : stride);
}

} // namespace

struct slam_csm {
    slam_csm_params P;
    struct Table {
        int    ox = 0, oy = 0, w = 0, h = 0;
        DevMem T, W;
    } tab[2];
    bool plane = false; // made from a byte plane (slam_csm_create_from_plane*): tab[0] alone exists and both classes read it
    // scratch of a match, for max_scans scans: the bounds, the survivor list, and the keys: every scan's top key, then every
    // scan's best key, then the list counters
    DevMem U, list, keys;
    int    max_scans = 0;
    // staging of the host forms
    DevMem pts, small, poses;
    // the posterior (slam_csm_set_post_params): the 257 weights and one PostAcc per scan
    slam_csm_post_params PP = {0, 0.0, 0, 0};
    bool                 post_set = false;
    DevMem               wtab, post;

    static size_t       key_bytes(int scans) { return (2 * sizeof(unsigned long long) + sizeof(int32_t)) * (size_t)scans; }
    unsigned long long *top() const { return keys.as<unsigned long long>(); }
    unsigned long long *best() const { return top() + max_scans; }
    int32_t            *count() const { return reinterpret_cast<int32_t *>(best() + max_scans); }

    int  nth() const { return 2 * P.half_theta + 1; }
    int  nx() const { return 2 * P.half_x + 1; }
    int  ny() const { return 2 * P.half_y + 1; }
    int  nbx() const { return (nx() + P.block - 1) / P.block; }
    int  nby() const { return (ny() + P.block - 1) / P.block; }
    Geom geom() const
    {
        Geom g;
        for (int c = 0; c < 2; ++c) {
            const int D1 = P.block - 1;
            const Table &t = tab[plane ? 0 : c];
            g.T[c] = Tab{t.T.as<uint8_t>(), t.ox, t.oy, t.w, t.h};
            g.W[c] = t.w ? Tab{t.W.as<uint8_t>(), t.ox - D1, t.oy - D1, t.w + D1, t.h + D1} : Tab{nullptr, 0, 0, 0, 0};
        }
        g.res = P.resolution, g.half_x = P.half_x, g.half_y = P.half_y, g.nx = nx(), g.ny = ny(), g.nth = nth(), g.D = P.block;
        g.nbx = nbx(), g.nby = nby();
        return g;
    }
};

namespace {

int check_window(int half_x, int half_y, int half_theta, double theta_step, int D)
{
    SLAM_REQUIRE(half_x >= 0 && half_y >= 0 && half_theta >= 0 && half_x <= 16383 && half_y <= 16383 && half_theta <= 16383 && std::isfinite(theta_step),
                 SLAM_E_INVALID, "slam_csm: half_x, half_y and half_theta lie in 0 .. 16383 and theta_step is finite");
    const double cand = (2.0 * half_x + 1) * (2.0 * half_y + 1) * (2.0 * half_theta + 1);
    SLAM_REQUIRE(cand < 2147483648.0, SLAM_E_INVALID, "slam_csm: %.0f candidates do not fit a 31-bit index", cand);
    return SLAM_OK;
}

int check_params(slam_csm_params &p)
{
    SLAM_REQUIRE(p.resolution > 0 && std::isfinite(p.resolution) && p.sigma > 0 && std::isfinite(p.sigma), SLAM_E_INVALID,
                 "slam_csm: resolution and sigma must be positive");
    if (p.kernel_cells <= 0) {
        const double k = std::ceil(3.0 * p.sigma / p.resolution - 1e-9);
        SLAM_REQUIRE(k <= kMaxK, SLAM_E_INVALID, "slam_csm: 3 sigma is %.0f cells, the stamp holds at most %d", k, kMaxK);
        p.kernel_cells = k < 0 ? 0 : (int)k;
    }
    SLAM_REQUIRE(p.kernel_cells <= kMaxK, SLAM_E_INVALID, "slam_csm: kernel_cells at most %d", kMaxK);
    SLAM_REQUIRE(p.block >= 1 && p.block <= kMaxD, SLAM_E_INVALID, "slam_csm: block lies in 1 .. %d", kMaxD);
    return check_window(p.half_x, p.half_y, p.half_theta, p.theta_step, p.block);
}

// T and W of class c from n model points on the device; waits
int build_table(slam_csm *s, int c, const double *d_m, int n, const uint8_t *d_stamp, hipStream_t st)
{
    if (n <= 3) return SLAM_OK; // icpPointToPoint.cpp:59,93: ICP does not use such a class either
    const int K = s->P.kernel_cells, D = s->P.block, SS = (2 * K + 1) * (2 * K + 1);
    DevMem    cells, bbox, plane;
    SLAM_TRY(cells.alloc(sizeof(int2) * (size_t)n));
    SLAM_TRY(bbox.alloc(4 * sizeof(int)));
    const int init[4] = {INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};
    int       got[4];
    SLAM_HIP(hipMemcpyAsync(bbox.p, init, sizeof init, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(csm_model_cells_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, d_m, n, s->P.resolution, cells.as<int2>(), bbox.as<int>());
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(got, bbox.p, sizeof got, hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    if (got[0] > got[1]) return SLAM_OK; // no point with a cell
    const long long w = (long long)got[1] - got[0] + 1 + 2 * K, h = (long long)got[3] - got[2] + 1 + 2 * K;
    SLAM_REQUIRE((double)(w + D) * (double)(h + D) <= (double)kMaxTableBytes, SLAM_E_INVALID,
                 "slam_csm_create: class %d spans %lld x %lld cells, more than %zu bytes of table", c, w, h, kMaxTableBytes);
    slam_csm::Table &t = s->tab[c];
    const size_t     nT = (size_t)w * h, nW = (size_t)(w + D - 1) * (h + D - 1);
    SLAM_TRY(t.T.alloc(nT));
    SLAM_TRY(t.W.alloc(nW));
    SLAM_TRY(plane.alloc(sizeof(unsigned) * nT));
    t.ox = got[0] - K, t.oy = got[2] - K, t.w = (int)w, t.h = (int)h;
    SLAM_HIP(hipMemsetAsync(plane.p, 0, sizeof(unsigned) * nT, st));
    hipLaunchKernelGGL(csm_scatter_kernel, dim3(blocks_for((size_t)n * SS, 256)), dim3(256), 0, st, cells.as<int2>(), n, d_stamp, K, t.ox, t.oy, t.w, t.h,
                       plane.as<unsigned>());
    SLAM_HIP(hipGetLastError());
    hipLaunchKernelGGL(csm_pack_kernel, dim3(blocks_for(nT, 256)), dim3(256), 0, st, plane.as<unsigned>(), nT, t.T.as<uint8_t>());
    SLAM_HIP(hipGetLastError());
    hipLaunchKernelGGL(csm_slide_kernel, dim3(blocks_for(nW, 256)), dim3(256), 0, st, t.T.as<uint8_t>(), t.w, t.h, D, t.W.as<uint8_t>());
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipStreamSynchronize(st)); // the temporaries go back below
    return SLAM_OK;
}

int reserve_scans(slam_csm *s, int max_scans)
{
    const size_t per = (size_t)s->nth() * s->nbx() * s->nby();
    SLAM_REQUIRE((double)per * max_scans * sizeof(int32_t) < 4e9, SLAM_E_INVALID, "slam_csm_reserve: %d scans of %zu blocks are too many", max_scans, per);
    SLAM_TRY(s->U.reserve(sizeof(int32_t) * per * max_scans));
    SLAM_TRY(s->list.reserve(sizeof(int32_t) * per * max_scans));
    SLAM_TRY(s->keys.reserve(slam_csm::key_bytes(max_scans)));
    if (s->post_set) SLAM_TRY(s->post.reserve(sizeof(PostAcc) * (size_t)max_scans));
    s->max_scans = max_scans;
    return SLAM_OK;
}

// what both create calls check before they touch the device; p: the parameters in force
int create_arguments(const double *m_ga, int n_ga, const double *m_nga, int n_nga, const slam_csm_params *params, slam_csm_t **out,
                     slam_csm_params &p)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_csm_create: null out pointer");
    *out = nullptr;
    SLAM_REQUIRE(n_ga >= 0 && n_nga >= 0 && (n_ga == 0 || m_ga) && (n_nga == 0 || m_nga), SLAM_E_INVALID, "slam_csm_create: bad model arrays");
    slam_csm_default_params(&p);
    if (params) p = *params;
    SLAM_TRY(check_params(p));
    return require_device();
}

int create_common(const double *d_ga, int n_ga, const double *d_nga, int n_nga, const slam_csm_params &p, slam_csm_t **out)
{
    slam_csm *s = new (std::nothrow) slam_csm();
    SLAM_REQUIRE(s, SLAM_E_NOMEM, "slam_csm_create: out of host memory");
    s->P = p;
    const int K = p.kernel_cells, S = 2 * K + 1;
    uint8_t   stamp[(2 * kMaxK + 1) * (2 * kMaxK + 1)];
    for (int j = 0; j < S; ++j)
        for (int i = 0; i < S; ++i) {
            const double d2 = (double)((i - K) * (i - K) + (j - K) * (j - K));
            stamp[j * S + i] = (uint8_t)std::rint(255.0 * std::exp(-(d2 * (p.resolution * p.resolution)) / (2.0 * (p.sigma * p.sigma))));
        }
    DevMem d_stamp;
    int    rc = d_stamp.alloc((size_t)S * S);
    if (rc == SLAM_OK && hipMemcpy(d_stamp.p, stamp, (size_t)S * S, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("slam_csm_create: the stamp's upload failed");
        rc = SLAM_E_HIP;
    }
    if (rc == SLAM_OK) rc = build_table(s, 0, d_ga, n_ga, d_stamp.as<uint8_t>(), nullptr);
    if (rc == SLAM_OK) rc = build_table(s, 1, d_nga, n_nga, d_stamp.as<uint8_t>(), nullptr);
    if (rc == SLAM_OK) rc = reserve_scans(s, 1);
    if (rc != SLAM_OK) {
        delete s;
        return rc;
    }
    *out = s;
    return SLAM_OK;
}

// the lattice holds every cell of a w x h plane at (ox, oy) and of its W, which reaches D - 1 cells further down
bool plane_origin_ok(int ox, int oy, int w, int h, int D)
{
    const long long lim = (long long)kCellLimit;
    return (long long)ox - (D - 1) >= -lim && (long long)oy - (D - 1) >= -lim && (long long)ox + w - 1 <= lim && (long long)oy + h - 1 <= lim;
}

// what both plane create calls check before they touch the device; p: the parameters in force (sigma and kernel_cells 0:
// the plane carries the kernel)
int plane_arguments(const char *who, const uint8_t *plane, int w, int h, int ox, int oy, const slam_csm_params *params, slam_csm_t **out,
                    slam_csm_params &p)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "%s: null out pointer", who);
    *out = nullptr;
    SLAM_REQUIRE(plane, SLAM_E_INVALID, "%s: null plane", who);
    SLAM_REQUIRE(w >= 1 && h >= 1, SLAM_E_INVALID, "%s: a plane of %d x %d cells", who, w, h);
    slam_csm_default_params(&p);
    if (params) p = *params;
    p.sigma = 0.0, p.kernel_cells = 0;
    SLAM_REQUIRE(p.resolution > 0 && std::isfinite(p.resolution), SLAM_E_INVALID, "%s: resolution must be positive", who);
    SLAM_REQUIRE(p.block >= 1 && p.block <= kMaxD, SLAM_E_INVALID, "%s: block lies in 1 .. %d", who, kMaxD);
    if (check_window(p.half_x, p.half_y, p.half_theta, p.theta_step, p.block) != SLAM_OK) {
        set_error("%s: half_x, half_y and half_theta lie in 0 .. 16383, theta_step is finite, and the candidates fit a 31-bit index", who);
        return SLAM_E_INVALID;
    }
    SLAM_REQUIRE(((double)w + p.block) * ((double)h + p.block) <= (double)kMaxTableBytes, SLAM_E_INVALID,
                 "%s: a plane of %d x %d cells is more than %zu bytes of table", who, w, h, kMaxTableBytes);
    SLAM_REQUIRE(plane_origin_ok(ox, oy, w, h, p.block), SLAM_E_INVALID, "%s: origin (%d, %d) puts cells of the table beyond +-2^30", who, ox, oy);
    return require_device();
}

// T = the plane (a copy on `st`), W = its slide; enqueues only
int plane_tables(slam_csm *s, const uint8_t *plane, hipMemcpyKind kind, int ox, int oy, hipStream_t st)
{
    slam_csm::Table &t = s->tab[0];
    const size_t     nT = (size_t)t.w * t.h, nW = (size_t)(t.w + s->P.block - 1) * (t.h + s->P.block - 1);
    SLAM_HIP(hipMemcpyAsync(t.T.p, plane, nT, kind, st));
    t.ox = ox, t.oy = oy;
    hipLaunchKernelGGL(csm_slide_kernel, dim3(blocks_for(nW, 256)), dim3(256), 0, st, t.T.as<uint8_t>(), t.w, t.h, s->P.block, t.W.as<uint8_t>());
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int create_plane_common(const uint8_t *plane, hipMemcpyKind kind, int w, int h, int ox, int oy, const slam_csm_params &p, slam_csm_t **out)
{
    slam_csm *s = new (std::nothrow) slam_csm();
    SLAM_REQUIRE(s, SLAM_E_NOMEM, "slam_csm_create_from_plane: out of host memory");
    s->P = p, s->plane = true;
    s->tab[0].w = w, s->tab[0].h = h;
    int rc = s->tab[0].T.alloc((size_t)w * h);
    if (rc == SLAM_OK) rc = s->tab[0].W.alloc((size_t)(w + p.block - 1) * (h + p.block - 1));
    if (rc == SLAM_OK) rc = plane_tables(s, plane, kind, ox, oy, nullptr);
    if (rc == SLAM_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
        set_error("slam_csm_create_from_plane: the tables' construction failed");
        rc = SLAM_E_HIP;
    }
    if (rc == SLAM_OK) rc = reserve_scans(s, 1);
    if (rc != SLAM_OK) {
        delete s;
        return rc;
    }
    *out = s;
    return SLAM_OK;
}

} // namespace

extern "C" {

void slam_csm_default_params(slam_csm_params *p)
{
    if (!p) return;
    p->resolution = 0.1, p->sigma = 0.2, p->kernel_cells = 0, p->block = 8;
    p->half_x = p->half_y = 40, p->half_theta = 120, p->theta_step = 0.01, p->exhaustive = 0;
}

int slam_csm_create_dev(const double *d_m_ga, int n_ga, const double *d_m_nga, int n_nga, const slam_csm_params *params, slam_csm_t **out)
{
    slam_csm_params p;
    SLAM_TRY(create_arguments(d_m_ga, n_ga, d_m_nga, n_nga, params, out, p));
    return create_common(d_m_ga, n_ga, d_m_nga, n_nga, p, out);
}

int slam_csm_create(const double *m_ga, int n_ga, const double *m_nga, int n_nga, const slam_csm_params *params, slam_csm_t **out)
{
    slam_csm_params p;
    SLAM_TRY(create_arguments(m_ga, n_ga, m_nga, n_nga, params, out, p));
    DevMem       model;
    const size_t b_ga = sizeof(double) * 2 * (size_t)n_ga, b_nga = sizeof(double) * 2 * (size_t)n_nga;
    SLAM_TRY(model.alloc(b_ga + b_nga));
    if (b_ga) SLAM_HIP(hipMemcpy(model.p, m_ga, b_ga, hipMemcpyHostToDevice));
    if (b_nga) SLAM_HIP(hipMemcpy(model.as<char>() + b_ga, m_nga, b_nga, hipMemcpyHostToDevice));
    return create_common(model.as<double>(), n_ga, model.as<double>() + 2 * (size_t)n_ga, n_nga, p, out);
}

int slam_csm_create_from_plane_dev(const uint8_t *d_plane, int w, int h, int origin_x, int origin_y, const slam_csm_params *params,
                                   slam_csm_t **out)
{
    slam_csm_params p;
    SLAM_TRY(plane_arguments("slam_csm_create_from_plane_dev", d_plane, w, h, origin_x, origin_y, params, out, p));
    return create_plane_common(d_plane, hipMemcpyDeviceToDevice, w, h, origin_x, origin_y, p, out);
}

int slam_csm_create_from_plane(const uint8_t *plane, int w, int h, int origin_x, int origin_y, const slam_csm_params *params, slam_csm_t **out)
{
    slam_csm_params p;
    SLAM_TRY(plane_arguments("slam_csm_create_from_plane", plane, w, h, origin_x, origin_y, params, out, p));
    return create_plane_common(plane, hipMemcpyHostToDevice, w, h, origin_x, origin_y, p, out);
}

int slam_csm_set_plane_dev(slam_csm_t *csm, const uint8_t *d_plane, int origin_x, int origin_y, slam_stream_t stream)
{
    SLAM_REQUIRE(csm && d_plane, SLAM_E_INVALID, "slam_csm_set_plane_dev: null argument");
    SLAM_REQUIRE(csm->plane, SLAM_E_INVALID, "slam_csm_set_plane_dev: the handle was made from a model, not from a plane");
    SLAM_REQUIRE(plane_origin_ok(origin_x, origin_y, csm->tab[0].w, csm->tab[0].h, csm->P.block), SLAM_E_INVALID,
                 "slam_csm_set_plane_dev: origin (%d, %d) puts cells of the table beyond +-2^30", origin_x, origin_y);
    return plane_tables(csm, d_plane, hipMemcpyDeviceToDevice, origin_x, origin_y, as_stream(stream));
}

int slam_csm_score_poses_dev(slam_csm_t *csm, const double *d_pts, int n, int n_ga, const double *d_poses, int n_poses, int32_t *d_score,
                             int32_t *d_counted, slam_stream_t stream)
{
    SLAM_REQUIRE(csm && n >= 0 && n <= (1 << 23) && n_poses >= 0, SLAM_E_INVALID,
                 "slam_csm_score_poses_dev: bad arguments (at most 2^23 points, so that the sum fits)");
    if (n_poses == 0) return SLAM_OK;
    SLAM_REQUIRE((n == 0 || d_pts) && d_poses && d_score && d_counted, SLAM_E_INVALID, "slam_csm_score_poses_dev: null array");
    n_ga = n_ga < 0 ? 0 : (n_ga > n ? n : n_ga);
    hipLaunchKernelGGL(csm_score_poses_kernel, dim3(blocks_for((size_t)n_poses, 64)), dim3(64), 0, as_stream(stream), csm->geom(), d_pts, n, n_ga,
                       d_poses, n_poses, d_score, d_counted);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_csm_score_poses(slam_csm_t *csm, const double *pts, int n, int n_ga, const double *poses, int n_poses, int32_t *score, int32_t *counted)
{
    SLAM_REQUIRE(csm && n >= 0 && n <= (1 << 23) && n_poses >= 0, SLAM_E_INVALID,
                 "slam_csm_score_poses: bad arguments (at most 2^23 points, so that the sum fits)");
    if (n_poses == 0) return SLAM_OK;
    SLAM_REQUIRE((n == 0 || pts) && poses && score && counted, SLAM_E_INVALID, "slam_csm_score_poses: null array");
    const size_t pts_b = sizeof(double) * 2 * (size_t)n, pose_b = sizeof(double) * 4 * (size_t)n_poses, out_b = sizeof(int32_t) * (size_t)n_poses;
    SLAM_TRY(reserve_quarter(csm->pts, pts_b));
    SLAM_TRY(reserve_quarter(csm->poses, pose_b + 2 * out_b));
    double  *d_poses = csm->poses.as<double>();
    int32_t *d_score = reinterpret_cast<int32_t *>(csm->poses.as<char>() + pose_b), *d_counted = d_score + n_poses;
    if (n) SLAM_HIP(hipMemcpyAsync(csm->pts.p, pts, pts_b, hipMemcpyHostToDevice, nullptr));
    SLAM_HIP(hipMemcpyAsync(d_poses, poses, pose_b, hipMemcpyHostToDevice, nullptr));
    SLAM_TRY(slam_csm_score_poses_dev(csm, csm->pts.as<double>(), n, n_ga, d_poses, n_poses, d_score, d_counted, nullptr));
    SLAM_HIP(hipMemcpyAsync(score, d_score, out_b, hipMemcpyDeviceToHost, nullptr));
    SLAM_HIP(hipMemcpyAsync(counted, d_counted, out_b, hipMemcpyDeviceToHost, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

void slam_csm_destroy(slam_csm_t *csm)
{
    delete csm; // (hipFree waits for what is still enqueued)
}

int slam_csm_reserve(slam_csm_t *csm, int max_scans)
{
    SLAM_REQUIRE(csm && max_scans >= 1, SLAM_E_INVALID, "slam_csm_reserve: bad arguments");
    return reserve_scans(csm, max_scans > csm->max_scans ? max_scans : csm->max_scans);
}

int slam_csm_set_window(slam_csm_t *csm, int half_x, int half_y, int half_theta, double theta_step)
{
    SLAM_REQUIRE(csm, SLAM_E_INVALID, "slam_csm_set_window: null handle");
    SLAM_TRY(check_window(half_x, half_y, half_theta, theta_step, csm->P.block));
    const slam_csm_params old = csm->P;
    csm->P.half_x = half_x, csm->P.half_y = half_y, csm->P.half_theta = half_theta, csm->P.theta_step = theta_step;
    const int rc = reserve_scans(csm, csm->max_scans);
    if (rc != SLAM_OK) csm->P = old;
    return rc;
}

int slam_csm_set_exhaustive(slam_csm_t *csm, int exhaustive)
{
    SLAM_REQUIRE(csm, SLAM_E_INVALID, "slam_csm_set_exhaustive: null handle");
    csm->P.exhaustive = exhaustive ? 1 : 0;
    return SLAM_OK;
}

int slam_csm_angles(slam_csm_t *csm, const double R0[4], double *cs)
{
    SLAM_REQUIRE(csm && R0 && cs, SLAM_E_INVALID, "slam_csm_angles: null argument");
    const double th0 = std::atan2(R0[2], R0[0]);
    for (int k = 0; k < csm->nth(); ++k) {
        const double th = th0 + (double)(k - csm->P.half_theta) * csm->P.theta_step;
        cs[2 * k] = std::cos(th), cs[2 * k + 1] = std::sin(th);
    }
    return SLAM_OK;
}

int slam_csm_match_batch_dev(slam_csm_t *csm, const double *d_pts, const int32_t *d_scan_off, const int32_t *d_scan_nga, int n_scans,
                             const double *d_R0, const double *d_t0, const double *d_cs, double *d_R, double *d_t, slam_csm_result *d_result,
                             slam_stream_t stream)
{
    SLAM_REQUIRE(csm && n_scans >= 0, SLAM_E_INVALID, "slam_csm_match_batch_dev: bad arguments");
    if (n_scans == 0) return SLAM_OK;
    SLAM_REQUIRE(d_pts && d_scan_off && d_scan_nga && d_R0 && d_t0 && d_cs && d_R && d_t, SLAM_E_INVALID, "slam_csm_match_batch_dev: null array");
    SLAM_REQUIRE(n_scans <= csm->max_scans && n_scans <= 65535, SLAM_E_INVALID,
                 "slam_csm_match_batch_dev: %d scans, scratch is reserved for %d (slam_csm_reserve; at most 65535)", n_scans, csm->max_scans);
    hipStream_t  st = as_stream(stream);
    const Geom   G = csm->geom();
    const Scans  S{d_pts, d_scan_off, d_scan_nga, 0, 0, d_t0, d_cs};
    const int    nb = G.nbx * G.nby, per = G.nth * nb;
    auto        *top = csm->top(), *best = csm->best();
    int32_t     *count = csm->count();
    SLAM_HIP(hipMemsetAsync(csm->keys.p, 0, slam_csm::key_bytes(csm->max_scans), st));
    if (csm->P.exhaustive) {
        hipLaunchKernelGGL(csm_tiles_kernel, dim3(tile_count(G), G.nth, n_scans), dim3(256), 0, st, G, S, (int32_t *)nullptr, best);
        SLAM_HIP(hipGetLastError());
    } else {
        const int groups = (nb + 64 * kCoarsePer - 1) / (64 * kCoarsePer);
        hipLaunchKernelGGL(csm_coarse_kernel, dim3(G.nth * groups, n_scans), dim3(64), 0, st, G, S, csm->U.as<int32_t>(), top);
        SLAM_HIP(hipGetLastError());
        hipLaunchKernelGGL(csm_blocks_kernel, dim3(1, n_scans), dim3(64), 0, st, G, S, top, (const int32_t *)nullptr, (const int32_t *)nullptr, best);
        SLAM_HIP(hipGetLastError());
        hipLaunchKernelGGL(csm_select_kernel, dim3(blocks_for(per, 256), n_scans), dim3(256), 0, st, G, S, kKeepMatch, csm->U.as<int32_t>(), top,
                           best, (const PostAcc *)nullptr, csm->list.as<int32_t>(), count);
        SLAM_HIP(hipGetLastError());
        hipLaunchKernelGGL(csm_blocks_kernel, dim3(list_stride(n_scans), n_scans), dim3(64), 0, st, G, S, top, csm->list.as<int32_t>(), count, best);
        SLAM_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(csm_finish_kernel, dim3(n_scans), dim3(256), 0, st, G, S, best, count, csm->P.exhaustive ? per : 0, d_R0, d_R, d_t, d_result);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

// slam_csm_match and slam_csm_match_post: one scan from host pointers through the batch call, one wait
static int match_host(slam_csm_t *csm, const char *who, const double *t_ga, int n_tga, const double *t_nga, int n_tnga, double R[4], double t[2],
                      slam_csm_result *result, slam_csm_posterior *post)
{
    SLAM_REQUIRE(csm && R && t && n_tga >= 0 && n_tnga >= 0 && (n_tga == 0 || t_ga) && (n_tnga == 0 || t_nga), SLAM_E_INVALID, "%s: bad arguments", who);
    const int n = n_tga + n_tnga;
    SLAM_REQUIRE(n >= 5, SLAM_E_TOO_FEW_SCENE_POINTS, "%s: %d scene points, at least 5 are needed", who, n);
    // one block behind the points: offsets, class count, R0, t0, the angles, R, t, the result (and the posterior)
    const size_t cs_b = sizeof(double) * 2 * (size_t)csm->nth();
    const size_t res_at = 16 + sizeof(double) * 12 + cs_b, post_at = res_at + 32; // (the result is 28 bytes; the posterior holds int64)
    const size_t small_b = post ? post_at + sizeof(slam_csm_posterior) : res_at + sizeof(slam_csm_result);
    SLAM_TRY(reserve_quarter(csm->pts, sizeof(double) * 2 * (size_t)n));
    SLAM_TRY(csm->small.reserve(small_b));
    char *host = static_cast<char *>(pinned_scratch(small_b));
    SLAM_REQUIRE(host, SLAM_E_NOMEM, "%s: no pinned staging memory", who);
    int32_t *h_off = reinterpret_cast<int32_t *>(host);
    double  *h_pose = reinterpret_cast<double *>(host + 16), *h_cs = h_pose + 12;
    h_off[0] = 0, h_off[1] = n, h_off[2] = n_tga, h_off[3] = 0;
    std::memcpy(h_pose, R, 4 * sizeof(double));
    std::memcpy(h_pose + 4, t, 2 * sizeof(double));
    SLAM_TRY(slam_csm_angles(csm, R, h_cs));
    char    *dev = csm->small.as<char>();
    double  *d_pose = reinterpret_cast<double *>(dev + 16);
    auto    *d_res = reinterpret_cast<slam_csm_result *>(dev + res_at);
    double  *d_pts = csm->pts.as<double>();
    if (n_tga) SLAM_HIP(hipMemcpyAsync(d_pts, t_ga, sizeof(double) * 2 * (size_t)n_tga, hipMemcpyHostToDevice, nullptr));
    if (n_tnga) SLAM_HIP(hipMemcpyAsync(d_pts + 2 * (size_t)n_tga, t_nga, sizeof(double) * 2 * (size_t)n_tnga, hipMemcpyHostToDevice, nullptr));
    SLAM_HIP(hipMemcpyAsync(dev, host, res_at, hipMemcpyHostToDevice, nullptr));
    if (post)
        SLAM_TRY(slam_csm_match_post_batch_dev(csm, d_pts, reinterpret_cast<int32_t *>(dev), reinterpret_cast<int32_t *>(dev) + 2, 1, d_pose, d_pose + 4,
                                               d_pose + 12, d_pose + 6, d_pose + 10, d_res, reinterpret_cast<slam_csm_posterior *>(dev + post_at), nullptr));
    else
        SLAM_TRY(slam_csm_match_batch_dev(csm, d_pts, reinterpret_cast<int32_t *>(dev), reinterpret_cast<int32_t *>(dev) + 2, 1, d_pose, d_pose + 4,
                                          d_pose + 12, d_pose + 6, d_pose + 10, d_res, nullptr));
    SLAM_HIP(hipMemcpyAsync(host, dev, small_b, hipMemcpyDeviceToHost, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    std::memcpy(R, h_pose + 6, 4 * sizeof(double));
    std::memcpy(t, h_pose + 10, 2 * sizeof(double));
    if (result) std::memcpy(result, host + res_at, sizeof *result);
    if (post) std::memcpy(post, host + post_at, sizeof *post);
    return SLAM_OK;
}

int slam_csm_match(slam_csm_t *csm, const double *t_ga, int n_tga, const double *t_nga, int n_tnga, double R[4], double t[2],
                   slam_csm_result *result)
{
    return match_host(csm, "slam_csm_match", t_ga, n_tga, t_nga, n_tnga, R, t, result, nullptr);
}

void slam_csm_default_post_params(slam_csm_post_params *p)
{
    if (!p) return;
    p->margin_per_point = 16, p->beta = 8.0, p->excl_xy = 2, p->excl_theta = 2;
}

int slam_csm_set_post_params(slam_csm_t *csm, const slam_csm_post_params *p)
{
    SLAM_REQUIRE(csm && p, SLAM_E_INVALID, "slam_csm_set_post_params: null argument");
    SLAM_REQUIRE(p->margin_per_point >= 0 && p->margin_per_point <= 255 && std::isfinite(p->beta) && p->beta >= 0.0 && p->beta <= 64.0 &&
                     p->excl_xy >= 0 && p->excl_theta >= 0,
                 SLAM_E_INVALID, "slam_csm_set_post_params: margin_per_point lies in 0 .. 255, beta in 0 .. 64, the exclusion is not negative");
    uint32_t wtab[kPostTable];
    for (int j = 0; j < kPostTable; ++j) wtab[j] = (uint32_t)std::rint(65536.0 * std::exp(-(p->beta * (double)j) / 256.0));
    SLAM_TRY(csm->wtab.reserve(sizeof wtab));
    SLAM_TRY(csm->post.reserve(sizeof(PostAcc) * (size_t)csm->max_scans));
    SLAM_HIP(hipDeviceSynchronize()); // an earlier call may still read the table
    SLAM_HIP(hipMemcpy(csm->wtab.p, wtab, sizeof wtab, hipMemcpyHostToDevice));
    csm->PP = *p, csm->post_set = true;
    return SLAM_OK;
}

int slam_csm_read_post_table(slam_csm_t *csm, uint32_t *wtab, int cap)
{
    SLAM_REQUIRE(csm && wtab && cap >= kPostTable, SLAM_E_INVALID, "slam_csm_read_post_table: bad arguments (the table has %d entries)", kPostTable);
    SLAM_REQUIRE(csm->post_set, SLAM_E_INVALID, "slam_csm_read_post_table: slam_csm_set_post_params comes first");
    SLAM_HIP(hipMemcpy(wtab, csm->wtab.p, sizeof(uint32_t) * kPostTable, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_csm_match_post_batch_dev(slam_csm_t *csm, const double *d_pts, const int32_t *d_scan_off, const int32_t *d_scan_nga, int n_scans,
                                  const double *d_R0, const double *d_t0, const double *d_cs, double *d_R, double *d_t, slam_csm_result *d_result,
                                  slam_csm_posterior *d_post, slam_stream_t stream)
{
    SLAM_REQUIRE(csm && n_scans >= 0, SLAM_E_INVALID, "slam_csm_match_post_batch_dev: bad arguments");
    SLAM_REQUIRE(csm->post_set, SLAM_E_INVALID, "slam_csm_match_post_batch_dev: slam_csm_set_post_params comes first");
    const Geom G = csm->geom();
    {
        // the int64 sums: 65536 Dmax^2 per candidate at the most
        const unsigned __int128 dmax = (unsigned)(std::max(G.nx, std::max(G.ny, G.nth)) - 1);
        const unsigned __int128 worst = (unsigned __int128)65536 * dmax * dmax * ((unsigned __int128)G.nx * G.ny * G.nth);
        SLAM_REQUIRE(worst < ((unsigned __int128)1 << 63), SLAM_E_INVALID,
                     "slam_csm_match_post_batch_dev: a window of %d x %d x %d candidates could overflow the posterior's 64-bit sums", G.nx, G.ny, G.nth);
    }
    if (n_scans == 0) return SLAM_OK;
    // the posterior pass reads the start translations again after the match has written its answer (the angles come from d_cs)
    SLAM_REQUIRE(d_post && d_t0 && d_t != d_t0, SLAM_E_INVALID, "slam_csm_match_post_batch_dev: null d_post, or d_t is d_t0");
    SLAM_TRY(slam_csm_match_batch_dev(csm, d_pts, d_scan_off, d_scan_nga, n_scans, d_R0, d_t0, d_cs, d_R, d_t, d_result, stream));
    hipStream_t   st = as_stream(stream);
    const Scans   S{d_pts, d_scan_off, d_scan_nga, 0, 0, d_t0, d_cs};
    const PostCfg C{csm->PP.margin_per_point, csm->PP.excl_xy, csm->PP.excl_theta, csm->P.theta_step};
    const int     per = G.nth * G.nbx * G.nby;
    auto         *best = csm->best();
    int32_t      *count = csm->count();
    PostAcc      *acc = csm->post.as<PostAcc>();
    hipLaunchKernelGGL(csm_post_prepare_kernel, dim3(n_scans), dim3(256), 0, st, G, S, C, best, acc, count);
    SLAM_HIP(hipGetLastError());
    hipLaunchKernelGGL(csm_select_kernel, dim3(blocks_for(per, 256), n_scans), dim3(256), 0, st, G, S, csm->P.exhaustive ? kKeepAll : kKeepWithin,
                       csm->U.as<int32_t>(), csm->top(), best, acc, csm->list.as<int32_t>(), count);
    SLAM_HIP(hipGetLastError());
    hipLaunchKernelGGL(csm_post_accumulate_kernel, dim3(list_stride(n_scans), n_scans), dim3(64), 0, st, G, S, C, best, csm->list.as<int32_t>(), count,
                       csm->wtab.as<uint32_t>(), acc);
    SLAM_HIP(hipGetLastError());
    hipLaunchKernelGGL(csm_post_finish_kernel, dim3(blocks_for(n_scans, 64)), dim3(64), 0, st, G, S, C, n_scans, best, acc, count, d_post);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_csm_match_post(slam_csm_t *csm, const double *t_ga, int n_tga, const double *t_nga, int n_tnga, double R[4], double t[2],
                        slam_csm_result *result, slam_csm_posterior *post)
{
    SLAM_REQUIRE(post, SLAM_E_INVALID, "slam_csm_match_post: null posterior");
    return match_host(csm, "slam_csm_match_post", t_ga, n_tga, t_nga, n_tnga, R, t, result, post);
}

int slam_csm_score_volume_dev(slam_csm_t *csm, const double *d_pts, int n, int n_ga, const double *d_t0, const double *d_cs, int32_t *d_volume,
                              slam_stream_t stream)
{
    SLAM_REQUIRE(csm && d_pts && n >= 5 && n_ga >= 0 && d_t0 && d_cs && d_volume, SLAM_E_INVALID,
                 "slam_csm_score_volume_dev: bad arguments (a scan has at least 5 points)");
    const Geom  G = csm->geom();
    const Scans S{d_pts, nullptr, nullptr, n, n_ga, d_t0, d_cs};
    hipLaunchKernelGGL(csm_tiles_kernel, dim3(tile_count(G), G.nth, 1), dim3(256), 0, as_stream(stream), G, S, d_volume, (unsigned long long *)nullptr);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_csm_read_table(slam_csm_t *csm, int cls, int level, int *origin_x, int *origin_y, int *w, int *h, uint8_t *buf, size_t cap)
{
    SLAM_REQUIRE(csm && (cls == 0 || cls == 1) && (level == 0 || level == 1), SLAM_E_INVALID, "slam_csm_read_table: bad arguments");
    const Geom G = csm->geom();
    const Tab &t = level ? G.W[cls] : G.T[cls];
    if (origin_x) *origin_x = t.ox;
    if (origin_y) *origin_y = t.oy;
    if (w) *w = t.w;
    if (h) *h = t.h;
    if (buf && t.w) {
        SLAM_REQUIRE(cap >= (size_t)t.w * t.h, SLAM_E_INVALID, "slam_csm_read_table: room for %zu bytes, the table has %zu", cap, (size_t)t.w * t.h);
        SLAM_HIP(hipMemcpy(buf, t.v, (size_t)t.w * t.h, hipMemcpyDeviceToHost));
    }
    return SLAM_OK;
}

int slam_csm_info(slam_csm_t *csm, slam_csm_params *params, int dims[5], size_t *table_bytes, size_t *scratch_bytes, int *max_scans)
{
    SLAM_REQUIRE(csm, SLAM_E_INVALID, "slam_csm_info: null handle");
    if (params) *params = csm->P;
    if (dims) dims[0] = csm->nth(), dims[1] = csm->nx(), dims[2] = csm->ny(), dims[3] = csm->nbx(), dims[4] = csm->nby();
    if (table_bytes) *table_bytes = csm->tab[0].T.cap + csm->tab[0].W.cap + csm->tab[1].T.cap + csm->tab[1].W.cap;
    if (scratch_bytes) *scratch_bytes = csm->U.cap + csm->list.cap + csm->keys.cap + csm->wtab.cap + csm->post.cap;
    if (max_scans) *max_scans = csm->max_scans;
    return SLAM_OK;
}

} // extern "C"
