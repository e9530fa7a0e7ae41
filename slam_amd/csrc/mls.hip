// mls.hip -- the height-cluster MLS map (class MLS, non-rolling) on gfx950 behind the C-ABI.
//
// Reference path (under the reference checkout, mls/):
//   MLS::MLS              include/mls/mls.h:154-205  start pad
//   MLS::clearMap         src/mls.cpp:18-31
//   MLS::addToMap         src/mls.cpp:345-402        binning, window loop
//   MLS::updateCell       src/mls.cpp:152-342        clusters, ground, clearance, neighbours
//   MLS::offsetMap        src/mls.cpp:481-505
//   MLS::getSegmentedClouds src/mls.cpp:520-556
// The contract (and why a parallel schedule gives the serial answer) is docs/MLS_MAP.md; the scalar
// restatement the tests hold this against is tests/cpp/mls_map_oracle.cpp.
//
// One addToMap is a chain of launches on the caller's stream, with no host wait:
//   bin       every point -> (cell key, arrival index) behind the points still pending from earlier calls
//   sort      rocprim radix sort of the keys: each cell's points contiguous, carried first, then arrival order
//   segments  per cell [pstart, pend) into the sorted order
//   core      one lane per updated cell inside the window: updateCell's steps 1-5 (the serial point chain)
//   walk      one lane per processed cell: step 6's neighbour loop, steps 7-8; a walk that meets an updated
//             neighbour outside the window is handed to ...
//   closure   ONE workgroup with a worklist: claims such neighbours, runs their steps 1-5, resumes the walks
//   keep      the points of cells that kept them (no ground cluster, or not reached) compacted, still sorted,
//             into the pending store of the next call.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "device_mem.hpp"
#include "grid_cell.hpp"

using namespace slam;

namespace {

struct Slot { // Cluster (mls.h:20-33): mean, cov(2,2), num_pts, and sqrt(cov) kept in step with cov
    double mx, my, mz, cov, n, sq;
};

struct Prm { // the parameters the kernels read
    double max_range, normal_threshold, height_threshold, sigma, dist_threshold, combine_dist, drive_dist, robot_height;
    double min_pts, max_pts;
    int    max_clusters;
};

struct View {
    int             sx, sy, cap;
    Slot           *slots; // [cells * cap]
    int32_t        *cnt;   // clusters per cell
    int8_t         *drv, *byte;
    int32_t        *upd;   // 0, 1 = updated, 2 = claimed by the closure
    int32_t        *pstart, *pend;
    const float4   *pts;   // this call's input order
    const uint32_t *vals;  // sorted position -> input index
    Prm             p;
};

constexpr int kOutNone = 0, kOutWalk = 1;

__device__ inline void erase_slot(Slot *cl, int at, int &k)
{
    for (int r = at; r + 1 < k; ++r) cl[r] = cl[r + 1];
    --k;
}

// updateCell steps 1-5 (mls.cpp:152-304) of cell c; the caller has cleared its flag.  kOutWalk: step 6 is due.
__device__ int cell_core(const View &v, int c)
{
    Slot     *cl = v.slots + (size_t)c * v.cap;
    int       k = v.cnt[c];
    const int s0 = v.pstart[c], s1 = v.pend[c];
    const Prm &p = v.p;
    for (int s = s0; s < s1; ++s) {
        const float4 pt = v.pts[v.vals[s]];
        const double pz = (double)pt.z;
        int          ci = -1, ui = -1;
        double       ud = 100000.0;
        for (int q = 0; q < k; ++q) { // :162-180
            const double d = fabs(__dsub_rn(cl[q].mz, pz));
            if (cl[q].n < p.min_pts) {
                if (d < ud) {
                    ud = d;
                    ui = q;
                }
            } else if (d < __dadd_rn(__dmul_rn(cl[q].sq, p.sigma), p.dist_threshold)) {
                ci = q;
                break;
            }
        }
        if (ci == -1) { // :182-198
            if (ui == -1 || ud > p.robot_height) {
                if (k < p.max_clusters) {
                    cl[k] = Slot{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    ci = k++;
                } else {
                    continue; // :194 the point is dropped
                }
            } else {
                ci = ui;
            }
        }
        if (cl[ci].n == p.max_pts) { // :202-213 cap: the others lose a point, the emptied ones go (the next is skipped)
            for (int q = 1; q < k; ++q)
                if (q != ci) {
                    cl[q].n = __dsub_rn(cl[q].n, 1.0);
                    if (cl[q].n <= 0.0) erase_slot(cl, q, k);
                }
        } else {
            cl[ci].n = __dadd_rn(cl[ci].n, 1.0);
        }
        if (ci >= k) continue; // the reference's Cluster* points past the end: the update is lost
        Slot        &u = cl[ci]; // whatever cluster occupies the slot now
        const double n = u.n, a = __ddiv_rn(__dsub_rn(n, 1.0), n), b = __ddiv_rn(1.0, n); // :218-223
        u.mx = __dadd_rn(__dmul_rn(a, u.mx), __dmul_rn(b, (double)pt.x));
        u.my = __dadd_rn(__dmul_rn(a, u.my), __dmul_rn(b, (double)pt.y));
        u.mz = __dadd_rn(__dmul_rn(a, u.mz), __dmul_rn(b, pz));
        if (n > 1.0) { // :232-234
            const double dz = __dsub_rn(pz, u.mz);
            double cv = __dadd_rn(__dmul_rn(a, u.cov), __dmul_rn(__dmul_rn(__ddiv_rn(1.0, __dsub_rn(n, 1.0)), dz), dz));
            cv = cv < 0.001 ? 0.001 : cv; // std::max(cov, 0.001)
            u.cov = cv;
            u.sq = __dsqrt_rn(cv);
        } else { // :236 std::sort by mean z: insertion sort (libstdc++ below 17 elements; docs/MLS_MAP.md)
            for (int i = 1; i < k; ++i) {
                const Slot t = cl[i];
                int        j = i;
                while (j > 0 && t.mz < cl[j - 1].mz) {
                    cl[j] = cl[j - 1];
                    --j;
                }
                cl[j] = t;
            }
        }
    }
    v.cnt[c] = k;
    int g = -1; // :240-250
    for (int q = 0; q < k; ++q)
        if (cl[q].n > p.min_pts) {
            g = q;
            break;
        }
    if (g < 0) return kOutNone; // the points stay pending
    v.pend[c] = s0;             // :252 consumed
    if (g + 1 < k && cl[g + 1].n > p.min_pts) { // :282-304
        const double clearance = __dsub_rn(__dsub_rn(cl[g + 1].mz, __dmul_rn(cl[g + 1].sq, 2.0)), cl[g].mz);
        if (clearance < p.combine_dist) {
            const double n0 = cl[g].n, n1 = cl[g + 1].n, r0 = __ddiv_rn(n0, __dadd_rn(n0, n1)), r1 = __ddiv_rn(n1, __dadd_rn(n0, n1));
            cl[g].mx = __dadd_rn(__dmul_rn(r0, cl[g].mx), __dmul_rn(r1, cl[g + 1].mx));
            cl[g].my = __dadd_rn(__dmul_rn(r0, cl[g].my), __dmul_rn(r1, cl[g + 1].my));
            cl[g].mz = __dadd_rn(__dmul_rn(r0, cl[g].mz), __dmul_rn(r1, cl[g + 1].mz));
            cl[g].cov = __dadd_rn(__dmul_rn(r0, cl[g].cov), __dmul_rn(r1, cl[g + 1].cov));
            cl[g].sq = __dsqrt_rn(cl[g].cov);
            erase_slot(cl, g + 1, k);
            v.cnt[c] = k;
        } else if (clearance < p.drive_dist) {
            v.drv[c] = 0;
            v.byte[c] = 100;
            return kOutNone;
        }
    }
    return kOutWalk;
}

// updateCell steps 6-8 (mls.cpp:308-341) of cell c from neighbour w0 (w = 3*(i+1) + (j+1)).  Returns -1 when done, or the
// neighbour position w at which it met a neighbour still to be updated (*nb = its cell).
__device__ int cell_walk(const View &v, int c, int w0, int *nb)
{
    const int   x = c % v.sx, y = c / v.sx;
    const Slot *cl = v.slots + (size_t)c * v.cap;
    for (int w = w0; w < 9; ++w) {
        const int i = w / 3 - 1, j = w % 3 - 1;
        if ((i == 0 && j == 0) || i + x < 0 || i + x >= v.sx || j + y < 0 || j + y >= v.sy) continue;
        const int o = c + i + v.sx * j;
        if (__hip_atomic_load(&v.upd[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
            *nb = o;
            return w;
        }
        if (v.cnt[o] > 0 && v.slots[(size_t)o * v.cap].n > v.p.min_pts) {
            const double ndiff = __dsub_rn(cl[0].mz, v.slots[(size_t)o * v.cap].mz);
            if (ndiff > v.p.height_threshold) {
                v.drv[c] = 0;
                v.byte[c] = 100;
                return -1;
            }
        }
    }
    int       g = 0;
    const int k = v.cnt[c];
    while (g + 1 < k && !(cl[g].n > v.p.min_pts)) ++g; // step 3 found one
    if (fabs(cl[g].cov) > v.p.normal_threshold) { // :333-337
        v.drv[c] = 0;
        v.byte[c] = 100;
    } else {
        v.drv[c] = 1;
        v.byte[c] = 0;
    }
    return -1;
}

__global__ __launch_bounds__(256) void pad_keys_kernel(uint32_t *keys, uint32_t *vals, int B, const uint32_t *m, uint32_t inv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    if ((uint32_t)i >= *m) keys[i] = inv;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void bin_kernel(const float *xyz, int n, int stride, int B, int sx, int sy, double res,
                                                  double max_range, double pose_x, double pose_y, float4 *pts, uint32_t *keys,
                                                  uint32_t *vals, int32_t *upd, uint32_t inv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float px = xyz[(size_t)i * stride], py = xyz[(size_t)i * stride + 1], pz = xyz[(size_t)i * stride + 2];
    pts[B + i] = make_float4(px, py, pz, 0.f);
    vals[B + i] = (uint32_t)(B + i);
    int cx, cy;
    if (point_cell_of(sx, sy, res, max_range, pose_x, pose_y, 0, px, py, &cx, &cy)) { // mls.cpp:371-388
        const int c = cx + sx * cy;
        keys[B + i] = (uint32_t)c;
        upd[c] = 1;
    } else {
        keys[B + i] = inv;
    }
}

__global__ __launch_bounds__(256) void segments_kernel(const uint32_t *keys, int N, uint32_t inv, int32_t *pstart, int32_t *pend)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const uint32_t k = keys[s];
    if (k == inv) return;
    if (s == 0 || keys[s - 1] != k) pstart[k] = s;
    if (s == N - 1 || keys[s + 1] != k) pend[k] = s + 1;
}

struct Window {
    int x0, x1, y0, y1; // [x0, x1) x [y0, y1), clipped to the grid
};

// mls.cpp:390-399: every updated cell of the window, one lane each (lanes at segment starts; every updated cell has one)
__global__ __launch_bounds__(64) void core_kernel(View v, const uint32_t *keys, int N, uint32_t inv, Window win, uint8_t *stage)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= N) return;
    const uint32_t k = keys[s];
    uint8_t        out = kOutNone;
    if (k != inv && (s == 0 || keys[s - 1] != k) && v.upd[k] != 0) {
        const int x = (int)k % v.sx, y = (int)k / v.sx;
        if (x >= win.x0 && x < win.x1 && y >= win.y0 && y < win.y1) {
            v.upd[k] = 0; // :155
            out = (uint8_t)cell_core(v, (int)k);
        }
    }
    stage[s] = out;
}

struct Walk {
    int32_t cell, pos;
};

__global__ __launch_bounds__(256) void walk_kernel(View v, const uint32_t *keys, int N, const uint8_t *stage, Walk *blocked, int32_t *n_blocked)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N || stage[s] != kOutWalk) return;
    int       nb;
    const int w = cell_walk(v, (int)keys[s], 0, &nb);
    if (w >= 0) blocked[atomicAdd(n_blocked, 1)] = Walk{(int32_t)keys[s], w};
}

// The out-of-window part of the recursion (mls.cpp:312): rounds of (advance every open walk; claim the updated neighbours
// they stopped at) and (steps 1-5 of the claimed cells; their walks join the open ones).  One workgroup, so that no
// workgroup waits on the progress of another.
constexpr int kClosureThreads = 1024;
__global__ __launch_bounds__(kClosureThreads) void closure_kernel(View v, Walk *wa, Walk *wb, int32_t *claimed, const int32_t *n_blocked)
{
    __shared__ int n_next, n_claimed;
    int            n_open = *n_blocked;
    Walk          *in = wa, *out = wb;
    while (n_open > 0) {
        if (threadIdx.x == 0) n_next = n_claimed = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n_open; i += kClosureThreads) {
            const Walk w = in[i];
            int        nb;
            const int  at = cell_walk(v, w.cell, w.pos, &nb);
            if (at < 0) continue;
            if (atomicCAS(&v.upd[nb], 1, 2) == 1) claimed[atomicAdd(&n_claimed, 1)] = nb;
            out[atomicAdd(&n_next, 1)] = Walk{w.cell, at};
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n_claimed; i += kClosureThreads) {
            const int c = claimed[i];
            if (cell_core(v, c) == kOutWalk) out[atomicAdd(&n_next, 1)] = Walk{c, 0};
            __hip_atomic_store(&v.upd[c], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        n_open = n_next;
        Walk *t = in;
        in = out;
        out = t;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void keep_kernel(const uint32_t *keys, int N, uint32_t inv, const int32_t *pstart, const int32_t *pend,
                                                   uint8_t *keep)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const uint32_t k = keys[s];
    keep[s] = k != inv && pend[k] > pstart[k];
}

__global__ __launch_bounds__(256) void gather_kernel(int N, const uint32_t *m, const uint32_t *sel, const uint32_t *keys_s, const uint32_t *vals_s,
                                                     const float4 *pts_in, float4 *pts_out, uint32_t *keys_out)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N || (uint32_t)j >= *m) return;
    const uint32_t s = sel[j];
    pts_out[j] = pts_in[vals_s[s]];
    keys_out[j] = keys_s[s];
}

// mls.h:185-204: one lane per cell of the pad; create has checked that the pad fits in the grid, so no two lanes meet
__global__ __launch_bounds__(256) void start_pad_kernel(View v, int set_size, double res, double z, double n)
{
    const int side = 2 * set_size + 1, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= side * side) return;
    const int i = t / side - set_size, j = t % side - set_size;
    const int c = (i + v.sx / 2) + v.sx * (j + v.sy / 2);
    v.slots[(size_t)c * v.cap] = Slot{__dmul_rn((double)i, res), __dmul_rn((double)j, res), z, 0.01, n, __dsqrt_rn(0.01)};
    v.cnt[c] = 1;
}

__global__ __launch_bounds__(256) void offset_kernel(View v, double dz)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= v.sx * v.sy) return;
    Slot *cl = v.slots + (size_t)c * v.cap;
    for (int q = 0, k = v.cnt[c]; q < k; ++q) cl[q].mz = __dadd_rn(cl[q].mz, dz);
}

// getSegmentedClouds: per window cell (x outer, y inner) the obstacle and ground counts, packed (obstacle << 32 | ground)
__global__ __launch_bounds__(256) void seg_count_kernel(View v, Window win, unsigned long long *counts)
{
    const int h = win.y1 - win.y0, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (win.x1 - win.x0) * h) return;
    const int   c = (win.x0 + t / h) + v.sx * (win.y0 + t % h);
    const Slot *cl = v.slots + (size_t)c * v.cap;
    unsigned    no = 0, ng = 0;
    for (int q = 0, k = v.cnt[c]; q < k; ++q)
        if (cl[q].n >= v.p.min_pts) {
            if (v.drv[c] == 0 || q > 0) ++no;
            else ++ng;
        }
    counts[t] = ((unsigned long long)no << 32) | ng;
}

__global__ __launch_bounds__(256) void seg_total_kernel(const unsigned long long *counts, const unsigned long long *offs, int n, int32_t *tot)
{
    const unsigned long long s = offs[n - 1] + counts[n - 1];
    tot[0] = (int32_t)(s >> 32);
    tot[1] = (int32_t)(s & 0xffffffffull);
}

__global__ __launch_bounds__(256) void seg_scatter_kernel(View v, Window win, const unsigned long long *offs, float *obs, float *gnd)
{
    const int h = win.y1 - win.y0, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (win.x1 - win.x0) * h) return;
    const int   c = (win.x0 + t / h) + v.sx * (win.y0 + t % h);
    const Slot *cl = v.slots + (size_t)c * v.cap;
    unsigned    io = (unsigned)(offs[t] >> 32), ig = (unsigned)(offs[t] & 0xffffffffull);
    for (int q = 0, k = v.cnt[c]; q < k; ++q)
        if (cl[q].n >= v.p.min_pts) {
            float *o = (v.drv[c] == 0 || q > 0) ? obs + 3 * (size_t)io++ : gnd + 3 * (size_t)ig++;
            o[0] = (float)cl[q].mx, o[1] = (float)cl[q].my, o[2] = (float)cl[q].mz;
        }
}

__global__ __launch_bounds__(256) void read_cells_kernel(View v, const int32_t *cells, int n, const uint32_t *keys, const uint32_t *m,
                                                        int32_t *o_cnt, double *o_cl, int8_t *o_drv, int8_t *o_byte, uint8_t *o_upd, int32_t *o_pend)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cells[i];
    const int k = v.cnt[c];
    o_cnt[i] = k;
    for (int q = 0; o_cl && q < v.cap; ++q) {
        const Slot s = q < k ? v.slots[(size_t)c * v.cap + q] : Slot{0, 0, 0, 0, 0, 0};
        double    *o = o_cl + ((size_t)i * v.cap + q) * 5;
        o[0] = s.mx, o[1] = s.my, o[2] = s.mz, o[3] = s.cov, o[4] = s.n;
    }
    o_drv[i] = v.drv[c];
    o_byte[i] = v.byte[c];
    o_upd[i] = v.upd[c] != 0;
    // pending points: the carried keys are sorted, so the cell's run is found by two binary searches
    uint32_t lo = 0, hi = *m;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (keys[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
    }
    uint32_t e = lo, hi2 = *m;
    while (e < hi2) {
        const uint32_t mid = (e + hi2) / 2;
        if (keys[mid] <= (uint32_t)c) e = mid + 1; else hi2 = mid;
    }
    o_pend[i] = (int32_t)(e - lo);
}

inline int blocks(long n, int t) { return (int)((n + t - 1) / t); }

} // namespace

// calls whose carried count the host has not read yet, at most: a call waits for the one kInFlight calls before it, so
// the host stays a call ahead of the device and the bound below stays within m + kInFlight clouds
constexpr int kInFlight = 2;

namespace {
// The pending store: [0, m) carried points, sorted by cell (two buffers, swapped by every call), and the scratch of a call
struct Store {
    size_t               cap = 0; // points
    OwnedArray<float4>   pts[2];
    OwnedArray<uint32_t> keys[2];
    OwnedArray<uint32_t> vals_in, keys_s, vals_s, sel;
    OwnedArray<uint8_t>  stage;
    OwnedArray<Walk>     walk[2];
    OwnedArray<int32_t>  claimed;
    DevMem               tmp; // rocprim's scratch (sort and select)
};
// Last declared of a call's locals, so first destroyed: the scoped pool blocks declared before it go back to the pool
// (which does not wait) only after the device has finished with them, on every way out.
struct DeviceWait {
    ~DeviceWait() { (void)hipDeviceSynchronize(); }
};
} // namespace

struct slam_mls {
    int             sx = 0, sy = 0, cap = 0;
    double          res = 0;
    slam_mls_params p{};
    double          pose_x = 0, pose_y = 0;
    uint32_t        inv = 0;
    int             key_bits = 0;
    OwnedArray<Slot>    slots;
    OwnedArray<int32_t> cnt, upd, pstart, pend;
    OwnedArray<int8_t>  drv, byte;
    Store     store;
    int       cur = 0; // which of the store's two buffers holds the carried points
    OwnedArray<uint32_t> d_ctr; // [0] m, [1] blocked walks
    // what the host knows of m without waiting: every call (add, clear) copies m into a pinned slot and records an event;
    // calls [seen, seq) are still in flight, `known` is m after call seen - 1, and each call in flight adds at most its n
    OwnedArray<uint32_t, Mem::Pinned> h_m; // [kInFlight]
    hipEvent_t ev[kInFlight] = {};
    long       n_of[kInFlight] = {};
    long       seq = 0, seen = 0, known = 0;
    OwnedArray<float> d_in; // the host form's upload
};

namespace {

View view_of(slam_mls *m)
{
    View v;
    v.sx = m->sx, v.sy = m->sy, v.cap = m->cap;
    v.slots = m->slots, v.cnt = m->cnt, v.drv = m->drv, v.byte = m->byte, v.upd = m->upd, v.pstart = m->pstart, v.pend = m->pend;
    v.pts = m->store.pts[m->cur];
    v.vals = m->store.vals_s;
    const slam_mls_params &q = m->p;
    v.p = Prm{q.max_range, q.normal_threshold, q.height_threshold, q.cluster_sigma_factor, q.cluster_dist_threshold,
              q.cluster_combine_dist, q.drive_dist_threshold, q.robot_height, (double)q.min_cluster_points,
              (double)q.max_cluster_points, q.max_clusters};
    return v;
}

// (int)(pose/res + size/2) (mls.cpp:391-392, :524-525) and the window [cur - u, cur + u) clipped to the grid
Window window_of(const slam_mls *m)
{
    Window       w{0, 0, 0, 0};
    const double fx = m->pose_x / m->res + m->sx / 2, fy = m->pose_y / m->res + m->sy / 2;
    if (!(fx > -2147483648.0 && fx < 2147483648.0 && fy > -2147483648.0 && fy < 2147483648.0)) return w;
    const long cx = (int)fx, cy = (int)fy, u = m->p.update_dist;
    w.x0 = (int)std::max(0L, cx - u), w.x1 = (int)std::min((long)m->sx, cx + u);
    w.y0 = (int)std::max(0L, cy - u), w.y1 = (int)std::min((long)m->sy, cy + u);
    if (w.x1 < w.x0) w.x1 = w.x0;
    if (w.y1 < w.y0) w.y1 = w.y0;
    return w;
}

// A pending store of `want` items, keeping the m carried points of the current one (the stream has been waited for).
int grow_store(slam_mls *m, size_t want, uint32_t carried)
{
    Store nw; // (gives back what it got so far if the rest cannot be had)
    bool  ok = true;
    for (int b = 0; b < 2 && ok; ++b)
        ok = nw.pts[b].alloc(want * sizeof(float4)) == SLAM_OK && nw.keys[b].alloc(want * sizeof(uint32_t)) == SLAM_OK &&
             nw.walk[b].alloc(want * sizeof(Walk)) == SLAM_OK;
    ok = ok && nw.vals_in.alloc(want * 4) == SLAM_OK && nw.keys_s.alloc(want * 4) == SLAM_OK && nw.vals_s.alloc(want * 4) == SLAM_OK &&
         nw.sel.alloc(want * 4) == SLAM_OK && nw.stage.alloc(want) == SLAM_OK && nw.claimed.alloc(want * 4) == SLAM_OK;
    size_t sort_b = 0, sel_b = 0;
    if (ok) {
        ok = rocprim::radix_sort_pairs(nullptr, sort_b, nw.keys[0].get(), nw.keys_s.get(), nw.vals_in.get(), nw.vals_s.get(), want, 0,
                                       m->key_bits) == hipSuccess &&
             rocprim::select(nullptr, sel_b, rocprim::counting_iterator<uint32_t>(0), nw.stage.get(), nw.sel.get(), m->d_ctr.get(), want) ==
                 hipSuccess;
        ok = ok && nw.tmp.alloc(std::max(sort_b, sel_b)) == SLAM_OK;
    }
    if (ok && carried) {
        ok = hipMemcpy(nw.pts[0], m->store.pts[m->cur], carried * sizeof(float4), hipMemcpyDeviceToDevice) == hipSuccess &&
             hipMemcpy(nw.keys[0], m->store.keys[m->cur], carried * sizeof(uint32_t), hipMemcpyDeviceToDevice) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        set_error("slam_mls: the pending store cannot grow to %zu points", want);
        return SLAM_E_NOMEM;
    }
    nw.cap = want;
    m->store = std::move(nw); // the old store's buffers are freed here
    m->cur = 0;
    return SLAM_OK;
}

int record_count(slam_mls *m, hipStream_t st, long n_added)
{
    const int slot = (int)(m->seq % kInFlight);
    SLAM_HIP(hipMemcpyAsync(m->h_m + slot, m->d_ctr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipEventRecord(m->ev[slot], st));
    m->n_of[slot] = n_added;
    ++m->seq;
    return SLAM_OK;
}

// the calls that have finished, oldest first; with wait, the oldest in flight is waited for first
int see_counts(slam_mls *m, bool wait)
{
    if (wait && m->seen < m->seq) {
        SLAM_HIP(hipEventSynchronize(m->ev[m->seen % kInFlight]));
        m->known = m->h_m[m->seen % kInFlight];
        ++m->seen;
    }
    while (m->seen < m->seq) {
        const hipError_t e = hipEventQuery(m->ev[m->seen % kInFlight]);
        if (e == hipErrorNotReady) {
            (void)hipGetLastError();
            break;
        }
        SLAM_HIP(e);
        m->known = m->h_m[m->seen % kInFlight];
        ++m->seen;
    }
    return SLAM_OK;
}

long carried_bound(const slam_mls *m)
{
    long b = m->known;
    for (long s = m->seen; s < m->seq; ++s) b += m->n_of[s % kInFlight];
    return b;
}

bool params_ok(const slam_mls_params *p)
{
    return p && p->max_range == p->max_range && p->max_clusters >= 0;
}

} // namespace

extern "C" {

void slam_mls_default_params(slam_mls_params *p)
{
    if (!p) return;
    p->max_range = 75;
    p->update_dist = -1;
    p->max_clusters = 50;
    p->max_cluster_points = 200;
    p->min_cluster_points = 10;
    p->normal_threshold = 0.15;
    p->height_threshold = 0.4;
    p->cluster_sigma_factor = 3;
    p->cluster_dist_threshold = 0.5;
    p->cluster_combine_dist = 0.2;
    p->drive_dist_threshold = 1.0;
    p->robot_height = 1.45;
}

int slam_mls_create(int size_x, int size_y, double resolution, const slam_mls_params *params, slam_mls_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_mls_create: null out pointer");
    *out = nullptr;
    SLAM_REQUIRE(size_x > 0 && size_y > 0 && size_x <= 32767 && size_y <= 32767 && resolution > 0 && std::isfinite(resolution),
                 SLAM_E_INVALID, "slam_mls_create: size must be 1..32767 cells and resolution > 0");
    slam_mls_params p;
    if (params) p = *params; else slam_mls_default_params(&p);
    SLAM_REQUIRE(params_ok(&p) && p.max_clusters >= 1 && p.max_clusters <= 4096, SLAM_E_INVALID,
                 "slam_mls_create: max_clusters must be 1..4096 (it fixes the cluster capacity)");
    // the start pad, (int)(1/res) cells around the centre (mls.h:193), must fit in the grid (docs/MLS_MAP.md: the reference
    // would wrap it round and stack clusters; this also keeps (int)(1/res) in range)
    const double pad = std::floor(1.0 / resolution);
    SLAM_REQUIRE(2.0 * pad + 1.0 <= (double)std::min(size_x, size_y), SLAM_E_INVALID,
                 "slam_mls_create: the start pad of %.0f cells a side does not fit in a %d x %d grid", 2.0 * pad + 1.0, size_x, size_y);
    SLAM_TRY(require_device());
    slam_mls *m = new (std::nothrow) slam_mls();
    SLAM_REQUIRE(m, SLAM_E_NOMEM, "slam_mls_create: out of host memory");
    m->sx = size_x, m->sy = size_y, m->res = resolution, m->cap = p.max_clusters;
    if (p.update_dist < 0) p.update_dist = (int)fmin((int)p.max_range / resolution, size_x / 2); // mls.h:162
    m->p = p;
    const size_t cells = (size_t)size_x * size_y;
    m->key_bits = 1;
    while (((size_t)1 << m->key_bits) - 1 < cells) ++m->key_bits;
    m->inv = (uint32_t)(((size_t)1 << m->key_bits) - 1);
    std::unique_ptr<slam_mls, void (*)(slam_mls *)> guard(m, slam_mls_destroy); // an early return gives everything back
    SLAM_TRY(m->slots.alloc(cells * m->cap * sizeof(Slot)));
    SLAM_TRY(m->cnt.alloc(cells * 4));
    SLAM_TRY(m->upd.alloc(cells * 4));
    SLAM_TRY(m->pstart.alloc(cells * 4));
    SLAM_TRY(m->pend.alloc(cells * 4));
    SLAM_TRY(m->drv.alloc(cells));
    SLAM_TRY(m->byte.alloc(cells));
    SLAM_TRY(m->d_ctr.alloc(16));
    SLAM_TRY(m->h_m.alloc(sizeof(uint32_t) * kInFlight));
    for (int k = 0; k < kInFlight; ++k) {
        SLAM_HIP(hipEventCreateWithFlags(&m->ev[k], hipEventDisableTiming));
        m->h_m[k] = 0;
    }
    SLAM_HIP(hipMemset(m->cnt, 0, cells * 4));
    SLAM_HIP(hipMemset(m->upd, 0, cells * 4));
    SLAM_HIP(hipMemset(m->drv, 0xff, cells));  // drivable -1
    SLAM_HIP(hipMemset(m->byte, 0, cells));    // mls.h:175: data.resize zero-fills
    SLAM_HIP(hipMemset(m->d_ctr, 0, 16));
    const int set_size = (int)pad; // mls.h:193
    hipLaunchKernelGGL(start_pad_kernel, dim3(blocks((long)(2 * set_size + 1) * (2 * set_size + 1), 256)), dim3(256), 0, nullptr, view_of(m),
                       set_size, resolution, -p.robot_height, (double)p.min_cluster_points);
    SLAM_HIP(hipGetLastError());
    SLAM_TRY(grow_store(m, (size_t)1 << 20, 0));
    SLAM_HIP(hipDeviceSynchronize());
    *out = guard.release();
    return SLAM_OK;
}

void slam_mls_destroy(slam_mls_t *m)
{
    if (!m) return;
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : m->ev)
        if (e) (void)hipEventDestroy(e);
    delete m;
}

int slam_mls_clear(slam_mls_t *m, slam_stream_t stream) // mls.cpp:18-31 (the start pad is not put back)
{
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_mls_clear: null handle");
    SLAM_TRY(require_device());
    hipStream_t  st = as_stream(stream);
    const size_t cells = (size_t)m->sx * m->sy;
    SLAM_HIP(hipMemsetAsync(m->cnt, 0, cells * 4, st));
    SLAM_HIP(hipMemsetAsync(m->upd, 0, cells * 4, st));
    SLAM_HIP(hipMemsetAsync(m->drv, 0xff, cells, st));
    SLAM_HIP(hipMemsetAsync(m->byte, 0xff, cells, st));
    SLAM_HIP(hipMemsetAsync(m->d_ctr, 0, 16, st));
    SLAM_TRY(see_counts(m, m->seq - m->seen >= kInFlight));
    return record_count(m, st, 0);
}

int slam_mls_set_pose(slam_mls_t *m, double x, double y)
{
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_mls_set_pose: null handle");
    m->pose_x = x, m->pose_y = y;
    return SLAM_OK;
}

int slam_mls_set_params(slam_mls_t *m, const slam_mls_params *p)
{
    SLAM_REQUIRE(m && params_ok(p), SLAM_E_INVALID, "slam_mls_set_params: bad arguments");
    SLAM_REQUIRE(p->max_clusters <= m->cap, SLAM_E_INVALID, "slam_mls_set_params: max_clusters %d above the capacity %d fixed at create",
                 p->max_clusters, m->cap);
    const int u = m->p.update_dist;
    m->p = *p;
    if (p->update_dist < 0) m->p.update_dist = u;
    return SLAM_OK;
}

int slam_mls_add_cloud_dev(slam_mls_t *m, const float *d_xyz, int n, int stride, slam_stream_t stream)
{
    SLAM_REQUIRE(m && n >= 0 && stride >= 3 && (d_xyz || n == 0), SLAM_E_INVALID, "slam_mls_add_cloud_dev: bad arguments");
    SLAM_TRY(require_device());
    hipStream_t st = as_stream(stream);
    // the bound on the carried count (the padding the sort below runs over): at most kInFlight calls in flight
    SLAM_TRY(see_counts(m, m->seq - m->seen >= kInFlight));
    long bound = carried_bound(m);
    if ((size_t)bound + n > m->store.cap) {
        while (m->seen < m->seq) SLAM_TRY(see_counts(m, true));
        bound = m->known;
        if ((size_t)bound + n > m->store.cap) {
            SLAM_HIP(hipStreamSynchronize(st));
            const size_t want = std::max((size_t)bound + n + ((size_t)bound + n) / 2, 2 * m->store.cap);
            SLAM_REQUIRE(want < ((size_t)1 << 31), SLAM_E_NOMEM, "slam_mls_add_cloud_dev: %ld points pending plus %d new exceed the store",
                         bound, n);
            SLAM_TRY(grow_store(m, want, (uint32_t)bound));
        }
    }
    const int B = (int)bound, N = B + n;
    const int    c = m->cur;
    const Store &s = m->store;
    if (N == 0) return SLAM_OK;
    if (B > 0)
        hipLaunchKernelGGL(pad_keys_kernel, dim3(blocks(B, 256)), dim3(256), 0, st, s.keys[c], s.vals_in, B, m->d_ctr, m->inv);
    if (n > 0)
        hipLaunchKernelGGL(bin_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d_xyz, n, stride, B, m->sx, m->sy, m->res, m->p.max_range,
                           m->pose_x, m->pose_y, s.pts[c], s.keys[c], s.vals_in, m->upd, m->inv);
    SLAM_HIP(hipGetLastError());
    size_t tb = s.tmp.cap;
    SLAM_HIP(rocprim::radix_sort_pairs(s.tmp.p, tb, s.keys[c].get(), s.keys_s.get(), s.vals_in.get(), s.vals_s.get(),
                                       (size_t)N, 0, m->key_bits, st));
    hipLaunchKernelGGL(segments_kernel, dim3(blocks(N, 256)), dim3(256), 0, st, s.keys_s, N, m->inv, m->pstart, m->pend);
    const View   v = view_of(m);
    const Window win = window_of(m);
    hipLaunchKernelGGL(core_kernel, dim3(blocks(N, 64)), dim3(64), 0, st, v, s.keys_s, N, m->inv, win, s.stage);
    SLAM_HIP(hipMemsetAsync(m->d_ctr + 1, 0, 4, st));
    hipLaunchKernelGGL(walk_kernel, dim3(blocks(N, 256)), dim3(256), 0, st, v, s.keys_s, N, s.stage, s.walk[0], (int32_t *)(m->d_ctr + 1));
    hipLaunchKernelGGL(closure_kernel, dim3(1), dim3(kClosureThreads), 0, st, v, s.walk[0], s.walk[1], s.claimed,
                       (const int32_t *)(m->d_ctr + 1));
    hipLaunchKernelGGL(keep_kernel, dim3(blocks(N, 256)), dim3(256), 0, st, s.keys_s, N, m->inv, m->pstart, m->pend, s.stage);
    SLAM_HIP(hipGetLastError());
    tb = s.tmp.cap;
    SLAM_HIP(rocprim::select(s.tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), s.stage.get(), s.sel.get(), m->d_ctr.get(),
                             (size_t)N, st));
    hipLaunchKernelGGL(gather_kernel, dim3(blocks(N, 256)), dim3(256), 0, st, N, m->d_ctr, s.sel, s.keys_s, s.vals_s, s.pts[c],
                       s.pts[c ^ 1], s.keys[c ^ 1]);
    SLAM_HIP(hipGetLastError());
    m->cur = c ^ 1;
    return record_count(m, st, n);
}

int slam_mls_add_cloud(slam_mls_t *m, const float *xyz, int n, int stride)
{
    SLAM_REQUIRE(m && n >= 0 && stride >= 3 && (xyz || n == 0), SLAM_E_INVALID, "slam_mls_add_cloud: bad arguments");
    SLAM_TRY(require_device());
    const size_t bytes = sizeof(float) * (size_t)n * stride;
    SLAM_TRY(m->d_in.reserve(bytes));
    if (n) SLAM_HIP(hipMemcpy(m->d_in, xyz, bytes, hipMemcpyHostToDevice));
    SLAM_TRY(slam_mls_add_cloud_dev(m, m->d_in, n, stride, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_mls_offset_z(slam_mls_t *m, double dz, slam_stream_t stream) // mls.cpp:481-491
{
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_mls_offset_z: null handle");
    SLAM_TRY(require_device());
    hipLaunchKernelGGL(offset_kernel, dim3(blocks((long)m->sx * m->sy, 256)), dim3(256), 0, as_stream(stream), view_of(m), dz);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_mls_read_drivability(slam_mls_t *m, int8_t *data)
{
    SLAM_REQUIRE(m && data, SLAM_E_INVALID, "slam_mls_read_drivability: bad arguments");
    SLAM_TRY(require_device());
    SLAM_HIP(hipDeviceSynchronize());
    SLAM_HIP(hipMemcpy(data, m->byte, (size_t)m->sx * m->sy, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_mls_segmented_clouds(slam_mls_t *m, float *obstacle, int obstacle_cap, int *n_obstacle, float *ground, int ground_cap, int *n_ground)
{
    SLAM_REQUIRE(m && n_obstacle && n_ground && obstacle_cap >= 0 && ground_cap >= 0 && (obstacle || !obstacle_cap) && (ground || !ground_cap),
                 SLAM_E_INVALID, "slam_mls_segmented_clouds: bad arguments");
    SLAM_TRY(require_device());
    *n_obstacle = *n_ground = 0;
    SLAM_HIP(hipDeviceSynchronize());
    const Window win = window_of(m);
    const long   nw = (long)(win.x1 - win.x0) * (win.y1 - win.y0);
    if (nw <= 0) return SLAM_OK;
    const View          v = view_of(m);
    PoolMem    count_mem, tmp, out;
    DeviceWait wait_first;
    SLAM_TRY(count_mem.alloc(2 * nw * sizeof(unsigned long long) + 16));
    unsigned long long *counts = count_mem.as<unsigned long long>(), *offs = counts + nw;
    int32_t            *tot = (int32_t *)(offs + nw);
    size_t              tb = 0;
    hipLaunchKernelGGL(seg_count_kernel, dim3(blocks(nw, 256)), dim3(256), 0, nullptr, v, win, counts);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(rocprim::exclusive_scan(nullptr, tb, counts, offs, 0ull, (size_t)nw, rocprim::plus<unsigned long long>()));
    SLAM_TRY(tmp.alloc(tb + 16));
    SLAM_HIP(rocprim::exclusive_scan(tmp.p, tb, counts, offs, 0ull, (size_t)nw, rocprim::plus<unsigned long long>(), nullptr));
    hipLaunchKernelGGL(seg_total_kernel, dim3(1), dim3(1), 0, nullptr, counts, offs, (int)nw, tot);
    int32_t t[2];
    SLAM_HIP(hipMemcpy(t, tot, 8, hipMemcpyDeviceToHost));
    *n_obstacle = t[0], *n_ground = t[1];
    SLAM_REQUIRE(t[0] <= obstacle_cap && t[1] <= ground_cap, SLAM_E_NOMEM,
                 "slam_mls_segmented_clouds: %d obstacle / %d ground points, capacities %d / %d", t[0], t[1], obstacle_cap, ground_cap);
    const size_t bo = 12 * (size_t)t[0], bg = 12 * (size_t)t[1];
    SLAM_TRY(out.alloc(bo + bg + 16));
    float *d_o = out.as<float>(), *d_g = (float *)(out.as<char>() + bo);
    hipLaunchKernelGGL(seg_scatter_kernel, dim3(blocks(nw, 256)), dim3(256), 0, nullptr, v, win, offs, d_o, d_g);
    SLAM_HIP(hipGetLastError());
    if (bo) SLAM_HIP(hipMemcpy(obstacle, d_o, bo, hipMemcpyDeviceToHost));
    if (bg) SLAM_HIP(hipMemcpy(ground, d_g, bg, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_mls_read_cells(slam_mls_t *m, const int32_t *cells, int n, int32_t *n_clusters, double *clusters, int8_t *drivable, int8_t *bytes,
                        uint8_t *updated, int32_t *pending)
{
    SLAM_REQUIRE(m && n >= 0 && (cells || !n), SLAM_E_INVALID, "slam_mls_read_cells: bad arguments");
    for (int i = 0; i < n; ++i)
        SLAM_REQUIRE(cells[i] >= 0 && (long)cells[i] < (long)m->sx * m->sy, SLAM_E_INVALID, "slam_mls_read_cells: cell %d out of the grid",
                     cells[i]);
    SLAM_TRY(require_device());
    if (!n) return SLAM_OK;
    const size_t ncl = clusters ? (size_t)n * m->cap * 5 : 0;
    const size_t off_cl = 0, off_cnt = off_cl + 8 * ncl, off_pend = off_cnt + 4 * (size_t)n, off_cells = off_pend + 4 * (size_t)n,
                 off_drv = off_cells + 4 * (size_t)n, off_byte = off_drv + n, off_upd = off_byte + n, total = off_upd + n;
    PoolMem    block;
    DeviceWait wait_first;
    SLAM_TRY(block.alloc(total + 16));
    char             *d = block.as<char>();
    std::vector<char> h(total);
    SLAM_HIP(hipDeviceSynchronize());
    SLAM_HIP(hipMemcpy(d + off_cells, cells, 4 * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(read_cells_kernel, dim3(blocks(n, 256)), dim3(256), 0, nullptr, view_of(m), (const int32_t *)(d + off_cells), n,
                       m->store.keys[m->cur], m->d_ctr, (int32_t *)(d + off_cnt), clusters ? (double *)(d + off_cl) : nullptr, (int8_t *)(d + off_drv),
                       (int8_t *)(d + off_byte), (uint8_t *)(d + off_upd), (int32_t *)(d + off_pend));
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpy(h.data(), d, total, hipMemcpyDeviceToHost));
    if (n_clusters) std::memcpy(n_clusters, h.data() + off_cnt, 4 * (size_t)n);
    if (clusters) std::memcpy(clusters, h.data() + off_cl, 8 * ncl);
    if (drivable) std::memcpy(drivable, h.data() + off_drv, n);
    if (bytes) std::memcpy(bytes, h.data() + off_byte, n);
    if (updated) std::memcpy(updated, h.data() + off_upd, n);
    if (pending) std::memcpy(pending, h.data() + off_pend, 4 * (size_t)n);
    return SLAM_OK;
}

int slam_mls_info(slam_mls_t *m, int *size_x, int *size_y, double *resolution, int *capacity, slam_mls_params *p, int *pending_points)
{
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_mls_info: null handle");
    if (size_x) *size_x = m->sx;
    if (size_y) *size_y = m->sy;
    if (resolution) *resolution = m->res;
    if (capacity) *capacity = m->cap;
    if (p) *p = m->p;
    if (pending_points) {
        SLAM_TRY(require_device());
        SLAM_HIP(hipDeviceSynchronize());
        uint32_t v = 0;
        SLAM_HIP(hipMemcpy(&v, m->d_ctr, 4, hipMemcpyDeviceToHost));
        *pending_points = (int)v;
    }
    return SLAM_OK;
}

} // extern "C"
