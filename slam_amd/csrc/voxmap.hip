// voxmap.hip -- the exact sparse voxel map (slam_vmap_*): the growing prior map of the reference's
//   global_generate.cpp:122-232 (voxel-filter scan and map, GICP, append the moved scan)
// kept as integer sums per voxel instead of a cloud that is filtered again every round.  The contract is
// docs/VOXEL_MAP.md section 1 (restated above the declarations in slam_mi355x.h); the scalar restatement the tests hold
// this against bit for bit is tests/cpp/vmap_oracle.cpp.
//
// The table is open addressing with linear probing over a power-of-two number of slots in HBM, as five arrays in one block:
// key (u64, all ones = empty), the three sums (i64, units of 2^-20 m) and the count (u32).
//   integrate  one lane per point: transform, cell, key; the lane finds its key or claims an empty slot with a 64-bit
//              atomicCAS, then adds with three 64-bit integer atomicAdds and one 32-bit.  Nothing waits for another lane: a
//              slot's sums are zero from the moment the table is cleared, so an add may land before or after any other.
//              Integer adds commute, so no order of lanes shows in the sums; where a key sits does not show in any result
//              because extraction sorts by key.
//   rehash     one lane per old slot: claims the key's slot in the larger table and stores sums and count (keys are
//              distinct, so plain stores).  Only ever launched by the host between integrate launches.
//   extract    flag (count, box) per slot -> rocprim select of the slot indices -> gather their keys -> rocprim radix sort
//              of (key, slot) -> one lane per voxel writes centroid, count and key.
//   carve      free-space evidence for voxels that exist (docs/VOXEL_MAP.md section 8; the restatement is
//              tests/cpp/vmap_carve_oracle.cpp): two u32 planes `seen` and `miss` in units of scans and a u32 `stamp` plane
//              that makes a voxel count once per call, all three allocated at the first carve.  One lane per ray finds the
//              endpoint's voxel (phase 1: seen) and the ray's visited length; a rocprim scan over chunks of 64 steps per ray;
//              one wavefront per chunk, one lane per step, walks the closed form of the driving-axis Bresenham and charges
//              `miss` (phase 2).  No key is written: the lookup only finds.
//   moments    opt-in (docs/VOXEL_MAP.md section 9; the restatement is tests/cpp/vmap_gicp_oracle.cpp): nine i64 planes, the
//              first and second moments of a voxel's points about the cell's corner in units of 2^-16 m.  A second
//              integrate kernel adds them with nine more 64-bit integer atomicAdds; after a rehash one more launch moves the
//              planes by looking every old key up in the new table.  One lane per slot turns them into a centroid, a normal,
//              a regularised plane covariance and a flag (the distribution planes), which vmap_gicp.hip registers against.
//   absorb     (docs/VOXEL_MAP.md section 10) one lane per voxel record (key, count, sums, optionally seen and miss, optionally
//              the nine moments): validate, find or claim as integrate does, integer atomicAdds.  The records are packed
//              arrays (a file, a caller) or another table's planes (merge: one lane per source slot, empty slots leave at
//              once); one body serves both.  Load is this fed from vmap_file.hpp's parser, merge from another handle.
//   coarsen    (docs/VOXEL_MAP.md section 11) one lane per slot of a finer map: the parent cell is the cell shifted right, count
//              and sums add unchanged, the moments are re-centred on the parent's corner in integers; find or claim and
//              integer atomicAdds as absorb.  The result is the bits of a map integrated at the coarser leaf.
// The hash is the 64-bit finaliser of MurmurHash3 (fmix64: two multiply-xorshift rounds), masked to the table: neighbouring
// cells differ in the low bits of one 21-bit field, and fmix64 spreads any one-bit difference over the whole word.
// The probe loop ends after `capacity` slots and then raises the handle's error word; the host keeps the load at one half
// or below (n_voxels + n <= capacity / 2 before a launch of n points), so that never happens.
#include <cmath>
#include <cstring>
#include <new>

#include <rocprim/rocprim.hpp>

#include "device_mem.hpp"
#include "kf_gicp_math.hpp"
#include "vmap_dist.hpp"
#include "vmap_file.hpp"

using namespace slam;

namespace {

constexpr uint64_t kEmpty = ~0ull;
constexpr int64_t  kMaxSlots = 1ll << 31; // slot indices travel as u32 through select and sort
constexpr double   kFix = 1048576.0;      // 2^20: sums are in units of 2^-20 m
constexpr int      kCellLimit = 1 << 20;
constexpr float    kCoordLimit = 4194304.0f; // 2^22

struct Table {
    uint64_t           *key;
    unsigned long long *sum[3];
    uint32_t           *count;
    uint64_t            mask; // slots - 1
};
struct Transform {
    double r[9], t[3];
    int    on;
};
struct Box {
    float lo[2], hi[2];
    int   on;
};
// the handle's counters on the device
enum { kClaimed = 0, kDropped = 1, kError = 2, kSelected = 3, kCounters = 4 };
// absorb's block of its own, allocated at the first absorb as carve's is (the handle's block stays four words): the first
// three as above (kDropped counts the rejected records), then the points accepted as one u64
enum { kPoints = 4, kAbsorbCounters = 6 };

__device__ __forceinline__ uint64_t fmix64(uint64_t k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// The slot that holds `key`, claimed if nobody had; -1 when `capacity` probes found neither (the error word's case).
__device__ __forceinline__ long long find_or_claim(const Table &T, uint64_t key, uint32_t *claimed)
{
    uint64_t h = fmix64(key) & T.mask;
    for (uint64_t probe = 0; probe <= T.mask; ++probe, h = (h + 1) & T.mask) {
        uint64_t cur = __hip_atomic_load(&T.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) {
            cur = atomicCAS((unsigned long long *)&T.key[h], (unsigned long long)kEmpty, (unsigned long long)key);
            if (cur == kEmpty) {
                atomicAdd(claimed, 1u);
                return (long long)h;
            }
        }
        if (cur == key) return (long long)h;
    }
    return -1;
}

__global__ __launch_bounds__(256) void vmap_integrate_kernel(const float *xyz, int n, int stride, Transform X, double leaf, Table T,
                                                             uint32_t *ctr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; // n may be close to 2^31
    if (i >= (size_t)n) return;
    const float *p = xyz + i * stride;
    float        q[3] = {p[0], p[1], p[2]};
    if (X.on) {
        const double px = q[0], py = q[1], pz = q[2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(X.r[3 * k], px), __dmul_rn(X.r[3 * k + 1], py)), __dmul_rn(X.r[3 * k + 2], pz)),
                                    X.t[k]);
    }
    uint64_t  key = 0;
    long long f[3];
    bool      keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = q[k];
        const double c = floor((double)v / leaf);
        if (!(fabsf(v) < kCoordLimit) || !(fabs(c) < (double)kCellLimit)) { // written so that a NaN fails both tests
            keep = false;
            continue;
        }
        key |= (uint64_t)((int)c + kCellLimit) << (21 * k);
        f[k] = (long long)rint((double)v * kFix);
    }
    if (!keep) {
        atomicAdd(&ctr[kDropped], 1u);
        return;
    }
    const long long h = find_or_claim(T, key, &ctr[kClaimed]);
    if (h < 0) {
        atomicExch(&ctr[kError], 1u);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&T.sum[k][h], (unsigned long long)f[k]);
    atomicAdd(&T.count[h], 1u);
}

__global__ __launch_bounds__(256) void vmap_rehash_kernel(Table from, Table to, uint32_t *ctr)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > from.mask) return;
    const uint64_t key = from.key[i];
    if (key == kEmpty) return;
    const long long h = find_or_claim(to, key, ctr + kClaimed);
    if (h < 0) {
        atomicExch(&ctr[kError], 1u);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) to.sum[k][h] = from.sum[k][i];
    to.count[h] = from.count[i];
}

__device__ __forceinline__ float centroid(unsigned long long s, uint32_t count)
{
    return (float)(((double)(long long)s / (double)count) * (1.0 / kFix));
}

__global__ __launch_bounds__(256) void vmap_flag_kernel(Table T, Box box, uint32_t min_count, uint8_t *flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > T.mask) return;
    bool           keep = false;
    const uint32_t c = T.count[i];
    if (T.key[i] != kEmpty && c >= min_count && c > 0) {
        keep = true;
        if (box.on) {
            const float x = centroid(T.sum[0][i], c), y = centroid(T.sum[1][i], c);
            keep = box.lo[0] <= x && x <= box.hi[0] && box.lo[1] <= y && y <= box.hi[1];
        }
    }
    flag[i] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void vmap_gather_keys_kernel(Table T, const uint32_t *slot, int n, uint64_t *key)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) key[i] = T.key[slot[i]];
}

__global__ __launch_bounds__(256) void vmap_write_kernel(Table T, const uint32_t *slot, const uint64_t *key, int n, float *xyz4, uint32_t *count,
                                                         uint64_t *key_out, int64_t *sums)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint32_t s = slot[i], c = T.count[s];
    if (sums)
        for (int k = 0; k < 3; ++k) sums[3 * i + k] = (int64_t)T.sum[k][s];
    if (xyz4) {
        float4 o;
        o.x = centroid(T.sum[0][s], c), o.y = centroid(T.sum[1][s], c), o.z = centroid(T.sum[2][s], c), o.w = 0.0f;
        reinterpret_cast<float4 *>(xyz4)[i] = o;
    }
    if (count) count[i] = c;
    if (key_out) key_out[i] = key[i];
}

// ---------------------------------------------------------------- carve (docs/VOXEL_MAP.md section 8)
struct Planes {
    uint32_t *seen, *miss, *stamp;
};
struct Carve {
    int      c0[3]; // the origin's cell
    int      end_margin, tail_num, tail_den, max_ray_cells;
    uint32_t tag; // 2 s of the call's serial s: phase 1 stamps 2 s + 1, phase 2 stamps 2 s
};
// the carve counters on the device, u64 each
enum { kcDropped = 0, kcSkipped = 1, kcSteps = 2, kcSeen = 3, kcMissed = 4, kCarveCounters = 5 };
constexpr int kChunk = 64; // steps per chunk: one wavefront

// The slot that holds `key`, or -1 at the first empty slot (or after `capacity` probes): nothing is written.
__device__ __forceinline__ long long find_slot(const Table &T, uint64_t key)
{
    uint64_t h = fmix64(key) & T.mask;
    for (uint64_t probe = 0; probe <= T.mask; ++probe, h = (h + 1) & T.mask) {
        const uint64_t cur = T.key[h];
        if (cur == key) return (long long)h;
        if (cur == kEmpty) return -1;
    }
    return -1;
}

// One lane per ray: the endpoint as integrate moves it, its cell, phase 1 (seen, once per voxel and call), the visited
// length L = max(0, n - T) and the ray's number of chunks.  Lane n writes the scan's closing zero.
__global__ __launch_bounds__(256) void vmap_carve_rays_kernel(const float *xyz, int n, int stride, Transform X, double leaf, Table T, Planes P,
                                                              Carve A, int4 *ray, uint32_t *chunks, unsigned long long *ctr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t     L = 0;
    if (i < (size_t)n) {
        const float *p = xyz + i * stride;
        float        q[3] = {p[0], p[1], p[2]};
        if (X.on) {
            const double px = q[0], py = q[1], pz = q[2];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                q[k] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(X.r[3 * k], px), __dmul_rn(X.r[3 * k + 1], py)), __dmul_rn(X.r[3 * k + 2], pz)),
                                        X.t[k]);
        }
        uint64_t key = 0;
        int      c1[3] = {0, 0, 0};
        bool     keep = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float  v = q[k];
            const double c = floor((double)v / leaf);
            if (!(fabsf(v) < kCoordLimit) || !(fabs(c) < (double)kCellLimit)) { // written so that a NaN fails both tests
                keep = false;
                continue;
            }
            c1[k] = (int)c;
            key |= (uint64_t)((int)c + kCellLimit) << (21 * k);
        }
        if (!keep) {
            atomicAdd(&ctr[kcDropped], 1ull);
        } else {
            const long long h = find_slot(T, key);
            if (h >= 0 && atomicMax(&P.stamp[h], A.tag + 1u) < A.tag + 1u) {
                atomicAdd(&P.seen[h], 1u);
                atomicAdd(&ctr[kcSeen], 1ull);
            }
            int nn = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) nn = max(nn, abs(c1[k] - A.c0[k])); // both cells lie inside +-2^20
            if (nn > A.max_ray_cells) {
                atomicAdd(&ctr[kcSkipped], 1ull);
            } else {
                const long long tail = ((long long)nn * A.tail_num + A.tail_den - 1) / A.tail_den;
                const long long t = tail > A.end_margin ? tail : (long long)A.end_margin;
                L = t < nn ? (uint32_t)(nn - t) : 0u;
            }
        }
        ray[i] = make_int4(c1[0], c1[1], c1[2], (int)L);
        chunks[i] = (L + kChunk - 1) / kChunk;
    } else if (i == (size_t)n) {
        chunks[i] = 0;
    }
    uint32_t steps = L; // at most 2^21 a lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
    if ((threadIdx.x & 63) == 0 && steps) atomicAdd(&ctr[kcSteps], (unsigned long long)steps);
}

// The cell of step i on one axis: c0 + s floor((2 a i + n - 1) / (2 n)), the closed form of the driving-axis Bresenham
// (error term 2 a - n, test `> 0` before the step); on the driving axis (a = n) it is c0 + s i.
__device__ __forceinline__ int carve_cell(int c0, int c1, uint32_t i, uint32_t nn, bool small)
{
    const int      d = c1 - c0;
    const uint32_t a = (uint32_t)abs(d);
    const uint32_t k = small ? (2u * a * i + nn - 1u) / (2u * nn) : (uint32_t)((2ull * a * i + nn - 1ull) / (2ull * nn));
    return d < 0 ? c0 - (int)k : c0 + (int)k;
}

// One wavefront per chunk of 64 steps, one lane per step (phase 2).  offs is the exclusive scan of the rays' chunk counts
// (offs[n] their number); a wave finds its ray by bisection.  The key plane alone is probed; stamp and miss are touched on a
// found key only.
__global__ __launch_bounds__(256) void vmap_carve_walk_kernel(const int4 *ray, const uint32_t *offs, int n, uint32_t max_chunks, Table T, Planes P,
                                                              Carve A, unsigned long long *ctr)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4;
    const uint32_t total = min(offs[n], max_chunks);
    for (uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < total; c += n_waves) {
        int lo = 0, hi = n; // offs[lo] <= c < offs[hi]
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (offs[mid] <= c) lo = mid;
            else hi = mid;
        }
        const int4     r = ray[lo];
        const uint32_t i = ((uint32_t)c - offs[lo]) * kChunk + lane;
        if (i >= (uint32_t)r.w) continue;
        const int c1[3] = {r.x, r.y, r.z};
        uint32_t  nn = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) nn = max(nn, (uint32_t)abs(c1[k] - A.c0[k]));
        const bool small = nn < 32768u; // 2 a i + n - 1 < 2^31: the 32-bit division
        uint64_t   key = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) key |= (uint64_t)(carve_cell(A.c0[k], c1[k], i, nn, small) + kCellLimit) << (21 * k);
        const long long h = find_slot(T, key);
        if (h < 0) continue;
        if (__hip_atomic_load(&P.stamp[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.tag + 1u) continue; // an endpoint of this cloud
        if (atomicMax(&P.stamp[h], A.tag) < A.tag) {
            atomicAdd(&P.miss[h], 1u);
            atomicAdd(&ctr[kcMissed], 1ull);
        }
    }
}

// vmap_rehash_kernel for a map that has been carved: seen and miss travel with the voxel (the new stamp plane is zero).
__global__ __launch_bounds__(256) void vmap_rehash_carved_kernel(Table from, Planes pf, Table to, Planes pt, uint32_t *ctr)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > from.mask) return;
    const uint64_t key = from.key[i];
    if (key == kEmpty) return;
    const long long h = find_or_claim(to, key, ctr + kClaimed);
    if (h < 0) {
        atomicExch(&ctr[kError], 1u);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) to.sum[k][h] = from.sum[k][i];
    to.count[h] = from.count[i];
    pt.seen[h] = pf.seen[i];
    pt.miss[h] = pf.miss[i];
}

// vmap_flag_kernel with the carved rule on top: keep iff miss den <= max(seen, 1) num in u64, equality kept.
__global__ __launch_bounds__(256) void vmap_flag_carved_kernel(Table T, Planes P, Box box, uint32_t min_count, uint32_t num, uint32_t den,
                                                               uint8_t *flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > T.mask) return;
    bool           keep = false;
    const uint32_t c = T.count[i];
    if (T.key[i] != kEmpty && c >= min_count && c > 0) {
        const uint32_t seen = P.seen[i];
        keep = (uint64_t)P.miss[i] * den <= (uint64_t)(seen > 1u ? seen : 1u) * num;
        if (keep && box.on) {
            const float x = centroid(T.sum[0][i], c), y = centroid(T.sum[1][i], c);
            keep = box.lo[0] <= x && x <= box.hi[0] && box.lo[1] <= y && y <= box.hi[1];
        }
    }
    flag[i] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void vmap_write_carve_kernel(Planes P, const uint32_t *slot, const uint64_t *key, int n, uint32_t *seen,
                                                               uint32_t *miss, uint64_t *key_out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint32_t s = slot[i];
    if (seen) seen[i] = P.seen[s];
    if (miss) miss[i] = P.miss[s];
    if (key_out) key_out[i] = key[i];
}

// ---------------------------------------------------------------- moments and distributions (docs/VOXEL_MAP.md section 9)
struct Moments {
    unsigned long long *E[3], *M[6]; // first moments, then xx xy xz yy yz zz
};
struct Dist {
    float4 *cen; // centroid; w = 1.0f for a plane voxel
    double *nrm, *cov, *eig;
};
struct DistRule {
    uint32_t min_points, miss_num, miss_den; // miss_den = 0: the carve planes are not asked
    double   flat_ratio, line_ratio, eps;
};

// vmap_integrate_kernel with the moments: e = (fx - cell L) >> 4 per axis, |e| <= 2^20 (section 9 has the bound).
__global__ __launch_bounds__(256) void vmap_integrate_moments_kernel(const float *xyz, int n, int stride, Transform X, double leaf, long long L,
                                                                     Table T, Moments Q, uint32_t *ctr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; // n may be close to 2^31
    if (i >= (size_t)n) return;
    const float *p = xyz + i * stride;
    float        q[3] = {p[0], p[1], p[2]};
    if (X.on) {
        const double px = q[0], py = q[1], pz = q[2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(X.r[3 * k], px), __dmul_rn(X.r[3 * k + 1], py)), __dmul_rn(X.r[3 * k + 2], pz)),
                                    X.t[k]);
    }
    uint64_t  key = 0;
    long long f[3], e[3];
    bool      keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = q[k];
        const double c = floor((double)v / leaf);
        if (!(fabsf(v) < kCoordLimit) || !(fabs(c) < (double)kCellLimit)) { // written so that a NaN fails both tests
            keep = false;
            continue;
        }
        key |= (uint64_t)((int)c + kCellLimit) << (21 * k);
        f[k] = (long long)rint((double)v * kFix);
        e[k] = (f[k] - (long long)(int)c * L) >> 4; // arithmetic: floor
    }
    if (!keep) {
        atomicAdd(&ctr[kDropped], 1u);
        return;
    }
    const long long h = find_or_claim(T, key, &ctr[kClaimed]);
    if (h < 0) {
        atomicExch(&ctr[kError], 1u);
        return;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&T.sum[k][h], (unsigned long long)f[k]);
    atomicAdd(&T.count[h], 1u);
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&Q.E[k][h], (unsigned long long)e[k]);
    atomicAdd(&Q.M[0][h], (unsigned long long)(e[0] * e[0]));
    atomicAdd(&Q.M[1][h], (unsigned long long)(e[0] * e[1]));
    atomicAdd(&Q.M[2][h], (unsigned long long)(e[0] * e[2]));
    atomicAdd(&Q.M[3][h], (unsigned long long)(e[1] * e[1]));
    atomicAdd(&Q.M[4][h], (unsigned long long)(e[1] * e[2]));
    atomicAdd(&Q.M[5][h], (unsigned long long)(e[2] * e[2]));
}

// After either rehash kernel: every old voxel's extra planes of 8-byte words go to the slot its key has in the new table.
// The lookup only finds; keys are distinct, so plain stores.
constexpr int kMaxMoved = 9;
struct MovedPlanes {
    const unsigned long long *from[kMaxMoved];
    unsigned long long       *to[kMaxMoved];
    int                       n;
};
__global__ __launch_bounds__(256) void vmap_move_planes_kernel(Table from, Table to, MovedPlanes P, uint32_t *ctr)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > from.mask) return;
    const uint64_t key = from.key[i];
    if (key == kEmpty) return;
    const long long h = find_slot(to, key);
    if (h < 0) {
        atomicExch(&ctr[kError], 1u);
        return;
    }
#pragma unroll
    for (int k = 0; k < kMaxMoved; ++k)
        if (k < P.n) P.to[k][h] = P.from[k][i];
}

// One lane per slot, sequential f64, every operation rounded on its own (the file is compiled without contraction).
// `C` is the carve planes of a carved map when the rule asks for them, null pointers otherwise.
__global__ __launch_bounds__(256) void vmap_distributions_kernel(Table T, Moments Q, Planes C, DistRule R, Dist D)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > T.mask) return;
    const uint32_t count = T.count[i];
    float4         cen = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double         nrm[3] = {0.0, 0.0, 0.0}, cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, lam[3] = {0.0, 0.0, 0.0};
    if (T.key[i] != kEmpty && count > 0) {
        cen.x = centroid(T.sum[0][i], count), cen.y = centroid(T.sum[1][i], count), cen.z = centroid(T.sum[2][i], count);
        const double n = (double)count;
        double       m[3], s[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = (double)(long long)Q.E[k][i] / n;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = (double)(long long)Q.M[k][i] / n;
        const double scale = 1.0 / 4294967296.0; // 2^-32: e is in units of 2^-16 m
        const double c6[6] = {(s[0] - m[0] * m[0]) * scale, (s[1] - m[0] * m[1]) * scale, (s[2] - m[0] * m[2]) * scale,
                              (s[3] - m[1] * m[1]) * scale, (s[4] - m[1] * m[2]) * scale, (s[5] - m[2] * m[2]) * scale};
        double       nn[3];
        plane_eigen(c6, lam, nn);
        bool plane = count >= R.min_points && lam[1] >= R.flat_ratio * lam[2] && lam[1] >= R.line_ratio * lam[0];
        if (plane && R.miss_den > 0 && C.seen) {
            const uint32_t seen = C.seen[i];
            plane = (uint64_t)C.miss[i] * R.miss_den <= (uint64_t)(seen > 1u ? seen : 1u) * R.miss_num;
        }
        if (plane) {
            cen.w = 1.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) nrm[k] = nn[k];
            plane_from_normal(nn, R.eps, cov);
        }
    }
    D.cen[i] = cen;
#pragma unroll
    for (int k = 0; k < 3; ++k) D.nrm[3 * i + k] = nrm[k], D.eig[3 * i + k] = lam[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) D.cov[6 * i + k] = cov[k];
}

__global__ __launch_bounds__(256) void vmap_write_moments_kernel(Moments Q, const uint32_t *slot, const uint64_t *key, int n, int64_t *E3, int64_t *M6,
                                                                 uint64_t *key_out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint32_t s = slot[i];
    for (int k = 0; k < 3; ++k) E3[3 * i + k] = (int64_t)Q.E[k][s];
    for (int k = 0; k < 6; ++k) M6[6 * i + k] = (int64_t)Q.M[k][s];
    key_out[i] = key[i];
}

__global__ __launch_bounds__(256) void vmap_write_dist_kernel(Dist D, const uint32_t *slot, const uint64_t *key, int n, double *nrm3, double *cov6,
                                                              double *eig3, uint64_t *key_out, float *cen3, uint8_t *flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint32_t s = slot[i];
    const float4   c = D.cen[s];
    for (int k = 0; k < 3; ++k) nrm3[3 * i + k] = D.nrm[3 * (size_t)s + k], eig3[3 * i + k] = D.eig[3 * (size_t)s + k];
    for (int k = 0; k < 6; ++k) cov6[6 * i + k] = D.cov[6 * (size_t)s + k];
    key_out[i] = key[i];
    cen3[3 * i] = c.x, cen3[3 * i + 1] = c.y, cen3[3 * i + 2] = c.z;
    flag[i] = c.w != 0.0f ? 1 : 0;
}

// ---------------------------------------------------------------- absorb (docs/VOXEL_MAP.md section 10)
// Where a call's voxel records lie.  Packed arrays: sum[k] = sums + k with w3 = 3, E[k] = E3 + k with w3 = 3, M[k] = M6 + k
// with w6 = 6.  Another table's planes: its own pointers with w3 = w6 = 1 and `slots` set, which makes an empty key a slot
// to pass over instead of a record to reject.  seen / miss and E / M are null where the records have none.
struct Records {
    const uint64_t           *key;
    const uint32_t           *count, *seen, *miss;
    const unsigned long long *sum[3], *E[3], *M[6];
    uint32_t                  w3, w6;
    int                       slots;
};

// One lane per record.  No floating point; nothing waits for another lane; the probe is find_or_claim's, bounded by the
// capacity.  P.seen is null on a map without carve planes; the host launches records with moments only onto a map that has
// the planes Q (and never records without onto such a map).  A wave sums its accepted counts before the one atomic.
__global__ __launch_bounds__(256) void vmap_absorb_kernel(Records S, uint64_t n, Table T, Planes P, Moments Q, uint32_t *ctr)
{
    const uint64_t     i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long points = 0;
    if (i < n) {
        const uint64_t key = S.key[i];
        if (!(S.slots && key == kEmpty)) {
            const uint32_t c = S.count[i];
            bool           ok = c != 0u && !(key >> 63); // all ones has bit 63 set
#pragma unroll
            for (int k = 0; k < 3; ++k) ok = ok && ((key >> (21 * k)) & 0x1fffffull) != 0x1fffffull;
            if (!ok) {
                atomicAdd(&ctr[kDropped], 1u);
            } else {
                const long long h = find_or_claim(T, key, &ctr[kClaimed]);
                if (h < 0) {
                    atomicExch(&ctr[kError], 1u);
                } else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) atomicAdd(&T.sum[k][h], S.sum[k][i * S.w3]);
                    atomicAdd(&T.count[h], c);
                    if (S.seen && P.seen) {
                        atomicAdd(&P.seen[h], S.seen[i]);
                        atomicAdd(&P.miss[h], S.miss[i]);
                    }
                    if (S.E[0]) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) atomicAdd(&Q.E[k][h], S.E[k][i * S.w3]);
#pragma unroll
                        for (int k = 0; k < 6; ++k) atomicAdd(&Q.M[k][h], S.M[k][i * S.w6]);
                    }
                    points = c;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) points += __shfl_xor(points, o);
    if ((threadIdx.x & 63) == 0 && points) atomicAdd(reinterpret_cast<unsigned long long *>(ctr + kPoints), points);
}

// ---------------------------------------------------------------- coarsen (docs/VOXEL_MAP.md section 11)
// One lane per slot of the finer table S; an empty slot leaves at once.  The parent cell is cell >> shift per axis (arithmetic:
// it floors), its key section 1's packing, always valid.  count and the sums add unchanged.  With moments (SQ.E[0] set; the
// host launches those only onto a map that has the planes Q) they are re-centred on the parent's corner in int64:
// s_k = o_k unit with o_k = cell_k - (parent_k << shift) and unit = L / 16 of the finer map, E'_k = E_k + n s_k and
// M'_kl = M_kl + s_k E_l + s_l E_k + n s_k s_l.  No floating point; nothing waits for another lane; the probe is
// find_or_claim's, bounded by the capacity; ctr is absorb's block, used as absorb uses it.
__global__ __launch_bounds__(256) void vmap_coarsen_kernel(Table S, Moments SQ, int shift, long long unit, Table T, Moments Q, uint32_t *ctr)
{
    const uint64_t     i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long points = 0;
    if (i <= S.mask) {
        const uint64_t key = S.key[i];
        if (key != kEmpty) {
            uint64_t  parent = 0;
            long long s[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int cell = (int)((key >> (21 * k)) & 0x1fffffull) - kCellLimit;
                const int up = cell >> shift; // arithmetic: floor
                parent |= (uint64_t)(up + kCellLimit) << (21 * k);
                s[k] = (long long)(cell - up * (1 << shift)) * unit;
            }
            const long long h = find_or_claim(T, parent, &ctr[kClaimed]);
            if (h < 0) {
                atomicExch(&ctr[kError], 1u);
            } else {
                const uint32_t c = S.count[i];
#pragma unroll
                for (int k = 0; k < 3; ++k) atomicAdd(&T.sum[k][h], S.sum[k][i]);
                atomicAdd(&T.count[h], c);
                if (SQ.E[0]) {
                    const long long n = (long long)c;
                    long long       E[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        E[k] = (long long)SQ.E[k][i];
                        atomicAdd(&Q.E[k][h], (unsigned long long)(E[k] + n * s[k]));
                    }
                    int m = 0;
#pragma unroll
                    for (int k = 0; k < 3; ++k)
#pragma unroll
                        for (int l = k; l < 3; ++l, ++m)
                            atomicAdd(&Q.M[m][h], (unsigned long long)((long long)SQ.M[m][i] + s[k] * E[l] + s[l] * E[k] + n * s[k] * s[l]));
                }
                points = c;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) points += __shfl_xor(points, o);
    if ((threadIdx.x & 63) == 0 && points) atomicAdd(reinterpret_cast<unsigned long long *>(ctr + kPoints), points);
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256); }
constexpr size_t kSlotBytes = sizeof(uint64_t) + 3 * sizeof(long long) + sizeof(uint32_t);
constexpr size_t kMomentBytes = 9 * sizeof(long long);                  // per slot, the moments' block
constexpr size_t kDistBytes = sizeof(float4) + 12 * sizeof(double);     // per slot, the distributions' block

} // namespace

struct slam_vmap {
    slam_vmap_params P;
    int64_t          capacity = 0, n_voxels = 0, n_points = 0;
    DevMem           table, ctr;
    // extraction: flags and selected slots (capacity each), then keys and slots before and after the sort, rocprim's scratch
    DevMem flag, sel, keys_in, keys_out, sel_sorted, tmp;
    // staging of the host forms
    DevMem stage_in, stage_out;
    // carve: the three planes (capacity u32 each) and the counters exist from the first carve on; per call the rays' end
    // cells and visited lengths, their chunk counts and the scan of those
    DevMem   seen, miss, stamp, cctr, rays, chunks, offs;
    DevMem   actr; // absorb's counters, from the first absorb on
    uint32_t serial = 1; // of the next carve call: 1 .. 2^31 - 2
    // distributions (section 9), from slam_vmap_enable_distributions on: the nine moment planes (capacity i64 each) in one
    // block, the distribution planes (centroid and flag, normal, covariance, eigenvalues) in another, and whether the
    // latter are behind the former; a registration's tasks, results and trace
    slam_vmap_dist_params DP{};
    DevMem                mom, dist, reg_work;
    bool                  dist_on = false, dist_stale = true;

    static Moments moments(const DevMem &b, int64_t cap)
    {
        Moments             Q;
        unsigned long long *p = b.as<unsigned long long>();
        for (int k = 0; k < 3; ++k) Q.E[k] = p + (size_t)cap * k;
        for (int k = 0; k < 6; ++k) Q.M[k] = p + (size_t)cap * (3 + k);
        return Q;
    }
    Moments moments() const { return moments(mom, capacity); }
    Dist    dists() const
    {
        Dist     D;
        uint8_t *p = dist.as<uint8_t>();
        D.cen = reinterpret_cast<float4 *>(p);
        D.nrm = reinterpret_cast<double *>(p + (size_t)capacity * 16);
        D.cov = D.nrm + (size_t)capacity * 3;
        D.eig = D.cov + (size_t)capacity * 6;
        return D;
    }

    bool   carved() const { return stamp.p != nullptr; }
    Planes planes() const { return Planes{seen.as<uint32_t>(), miss.as<uint32_t>(), stamp.as<uint32_t>()}; }

    static Table view(const DevMem &b, int64_t cap)
    {
        Table    T;
        uint8_t *p = b.as<uint8_t>();
        T.key = reinterpret_cast<uint64_t *>(p);
        for (int k = 0; k < 3; ++k) T.sum[k] = reinterpret_cast<unsigned long long *>(p + (size_t)cap * 8 * (k + 1));
        T.count = reinterpret_cast<uint32_t *>(p + (size_t)cap * 32);
        T.mask = (uint64_t)cap - 1;
        return T;
    }
    Table view() const { return view(table, capacity); }
};

namespace {

// an empty table of `cap` slots in `b`, enqueued on st
int new_table(DevMem &b, int64_t cap, hipStream_t st)
{
    SLAM_REQUIRE(cap <= kMaxSlots, SLAM_E_NOMEM, "slam_vmap: a table of %lld slots is more than the %lld a map may have", (long long)cap,
                 (long long)kMaxSlots);
    SLAM_TRY(b.alloc((size_t)cap * kSlotBytes));
    SLAM_HIP(hipMemsetAsync(b.p, 0xff, (size_t)cap * 8, st));
    SLAM_HIP(hipMemsetAsync(b.as<uint8_t>() + (size_t)cap * 8, 0, (size_t)cap * (kSlotBytes - 8), st));
    return SLAM_OK;
}

int64_t pow2_at_least(int64_t v)
{
    int64_t c = 64;
    while (c < v) c <<= 1;
    return c;
}

// Room for n more points under the load rule; waits for st when it grows (the old table is freed afterwards).
int make_room(slam_vmap *m, int64_t n, hipStream_t st)
{
    if (m->n_voxels + n <= m->capacity / 2) return SLAM_OK;
    const int64_t cap = pow2_at_least(2 * (m->n_voxels + n));
    DevMem        nt;
    SLAM_TRY(new_table(nt, cap, st));
    SLAM_HIP(hipMemsetAsync(m->ctr.p, 0, kCounters * sizeof(uint32_t), st));
    DevMem np[3]; // seen, miss, stamp of the new table, when the map has been carved
    if (m->carved()) {
        for (DevMem &b : np) {
            SLAM_TRY(b.alloc((size_t)cap * sizeof(uint32_t)));
            SLAM_HIP(hipMemsetAsync(b.p, 0, (size_t)cap * sizeof(uint32_t), st));
        }
        hipLaunchKernelGGL(vmap_rehash_carved_kernel, dim3(blocks_for((uint64_t)m->capacity)), dim3(256), 0, st, m->view(), m->planes(),
                           slam_vmap::view(nt, cap), Planes{np[0].as<uint32_t>(), np[1].as<uint32_t>(), np[2].as<uint32_t>()}, m->ctr.as<uint32_t>());
    } else {
        hipLaunchKernelGGL(vmap_rehash_kernel, dim3(blocks_for((uint64_t)m->capacity)), dim3(256), 0, st, m->view(), slam_vmap::view(nt, cap),
                           m->ctr.as<uint32_t>());
    }
    SLAM_HIP(hipGetLastError());
    uint32_t *h = static_cast<uint32_t *>(pinned_scratch(kCounters * sizeof(uint32_t)));
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_vmap: no pinned memory for the counters");
    SLAM_HIP(hipMemcpyAsync(h, m->ctr.p, kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    SLAM_REQUIRE(!h[kError] && (int64_t)h[kClaimed] == m->n_voxels, SLAM_E_HIP, "slam_vmap: the rehash moved %u of %lld voxels (error word %u)",
                 h[kClaimed], (long long)m->n_voxels, h[kError]);
    DevMem nm, nd; // the moments and distributions of the new table, when the map has them
    if (m->dist_on) {
        SLAM_TRY(nm.alloc((size_t)cap * kMomentBytes));
        SLAM_TRY(nd.alloc((size_t)cap * kDistBytes));
        SLAM_HIP(hipMemsetAsync(nm.p, 0, (size_t)cap * kMomentBytes, st));
        SLAM_HIP(hipMemsetAsync(m->ctr.p, 0, kCounters * sizeof(uint32_t), st));
        MovedPlanes   P{};
        const Moments qf = m->moments(), qt = slam_vmap::moments(nm, cap);
        for (int k = 0; k < 3; ++k) P.from[k] = qf.E[k], P.to[k] = qt.E[k];
        for (int k = 0; k < 6; ++k) P.from[3 + k] = qf.M[k], P.to[3 + k] = qt.M[k];
        P.n = 9;
        hipLaunchKernelGGL(vmap_move_planes_kernel, dim3(blocks_for((uint64_t)m->capacity)), dim3(256), 0, st, m->view(), slam_vmap::view(nt, cap), P,
                           m->ctr.as<uint32_t>());
        SLAM_HIP(hipGetLastError());
        SLAM_HIP(hipMemcpyAsync(h, m->ctr.p, kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipStreamSynchronize(st));
        SLAM_REQUIRE(!h[kError], SLAM_E_HIP, "slam_vmap: the rehash lost a voxel's moments");
    }
    m->table = std::move(nt);
    if (m->carved()) m->seen = std::move(np[0]), m->miss = std::move(np[1]), m->stamp = std::move(np[2]);
    if (m->dist_on) m->mom = std::move(nm), m->dist = std::move(nd), m->dist_stale = true;
    m->capacity = cap;
    return SLAM_OK;
}

// The three carve planes and the carve counters, zeroed on st, when the map has none yet: what a first carve allocates.
int ensure_carve_planes(slam_vmap *m, hipStream_t st)
{
    if (m->carved()) return SLAM_OK;
    const size_t plane = (size_t)m->capacity * sizeof(uint32_t);
    SLAM_TRY(m->cctr.alloc(kCarveCounters * sizeof(unsigned long long)));
    SLAM_TRY(m->seen.alloc(plane));
    SLAM_TRY(m->miss.alloc(plane));
    SLAM_HIP(hipMemsetAsync(m->seen.p, 0, plane, st));
    SLAM_HIP(hipMemsetAsync(m->miss.p, 0, plane, st));
    SLAM_TRY(m->stamp.alloc(plane)); // last: carved() is true only when all three stand
    SLAM_HIP(hipMemsetAsync(m->stamp.p, 0, plane, st));
    return SLAM_OK;
}

// The qualifying slots into m->sel and their number into *n: waits for st once.
// `ratio` = {num, den} adds the carved rule; a map never carved has miss = 0 everywhere, which every ratio keeps.
int select_slots(slam_vmap *m, const float lo[2], const float hi[2], int min_count, hipStream_t st, int64_t *n, const uint32_t *ratio = nullptr)
{
    const uint64_t cap = (uint64_t)m->capacity;
    SLAM_TRY(m->flag.reserve(cap));
    SLAM_TRY(m->sel.reserve(cap * sizeof(uint32_t)));
    Box box{};
    box.on = lo != nullptr;
    if (lo) box.lo[0] = lo[0], box.lo[1] = lo[1], box.hi[0] = hi[0], box.hi[1] = hi[1];
    uint32_t *d_n = m->ctr.as<uint32_t>() + kSelected;
    if (ratio && m->carved())
        hipLaunchKernelGGL(vmap_flag_carved_kernel, dim3(blocks_for(cap)), dim3(256), 0, st, m->view(), m->planes(), box, (uint32_t)min_count, ratio[0],
                           ratio[1], m->flag.as<uint8_t>());
    else
        hipLaunchKernelGGL(vmap_flag_kernel, dim3(blocks_for(cap)), dim3(256), 0, st, m->view(), box, (uint32_t)min_count, m->flag.as<uint8_t>());
    SLAM_HIP(hipGetLastError());
    size_t tb = 0;
    SLAM_HIP(rocprim::select(nullptr, tb, rocprim::counting_iterator<uint32_t>(0), m->flag.as<uint8_t>(), m->sel.as<uint32_t>(), d_n, (size_t)cap, st));
    SLAM_TRY(m->tmp.reserve(tb + 16));
    tb = m->tmp.cap;
    SLAM_HIP(rocprim::select(m->tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), m->flag.as<uint8_t>(), m->sel.as<uint32_t>(), d_n, (size_t)cap, st));
    uint32_t *h = static_cast<uint32_t *>(pinned_scratch(sizeof(uint32_t)));
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_vmap: no pinned memory for the counters");
    SLAM_HIP(hipMemcpyAsync(h, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    *n = (int64_t)*h;
    return SLAM_OK;
}

// The n selected slots in key order into m->sel_sorted, their keys into m->keys_out: asynchronous.
int sort_slots(slam_vmap *m, int n, hipStream_t st)
{
    SLAM_TRY(reserve_quarter(m->keys_in, (size_t)n * sizeof(uint64_t)));
    SLAM_TRY(reserve_quarter(m->keys_out, (size_t)n * sizeof(uint64_t)));
    SLAM_TRY(reserve_quarter(m->sel_sorted, (size_t)n * sizeof(uint32_t)));
    hipLaunchKernelGGL(vmap_gather_keys_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, st, m->view(), m->sel.as<uint32_t>(), n,
                       m->keys_in.as<uint64_t>());
    SLAM_HIP(hipGetLastError());
    size_t tb = 0;
    SLAM_HIP(rocprim::radix_sort_pairs(nullptr, tb, m->keys_in.as<uint64_t>(), m->keys_out.as<uint64_t>(), m->sel.as<uint32_t>(),
                                       m->sel_sorted.as<uint32_t>(), (size_t)n, 0, 63, st));
    if (tb + 16 > m->tmp.cap) {
        SLAM_HIP(hipStreamSynchronize(st)); // hipFree waits anyway; the error, if any, is this stream's
        SLAM_TRY(m->tmp.reserve(tb + 16));
    }
    tb = m->tmp.cap;
    SLAM_HIP(rocprim::radix_sort_pairs(m->tmp.p, tb, m->keys_in.as<uint64_t>(), m->keys_out.as<uint64_t>(), m->sel.as<uint32_t>(),
                                       m->sel_sorted.as<uint32_t>(), (size_t)n, 0, 63, st));
    return SLAM_OK;
}

// The n selected slots in key order into the caller's device arrays: asynchronous.
int sort_and_write(slam_vmap *m, int n, float *d_xyz4, uint32_t *d_count, uint64_t *d_key, hipStream_t st, int64_t *d_sums = nullptr)
{
    if (n == 0) return SLAM_OK;
    SLAM_TRY(sort_slots(m, n, st));
    hipLaunchKernelGGL(vmap_write_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, st, m->view(), m->sel_sorted.as<uint32_t>(),
                       m->keys_out.as<uint64_t>(), n, d_xyz4, d_count, d_key, d_sums);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int check_extract(const char *who, slam_vmap *m, const float *lo, const float *hi, int min_count, int cap, int *n_out)
{
    SLAM_REQUIRE(m && n_out && cap >= 0 && min_count >= 0 && (lo == nullptr) == (hi == nullptr), SLAM_E_INVALID,
                 "%s: a map, n_out, cap >= 0, min_count >= 0, and lo_xy and hi_xy both or neither", who);
    return SLAM_OK;
}

} // namespace

extern "C" {

void slam_vmap_default_params(slam_vmap_params *p)
{
    if (!p) return;
    p->leaf = 0.30; // global_generate.cpp:26
    p->initial_capacity = 65536;
}

int slam_vmap_create(const slam_vmap_params *params, slam_vmap_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_vmap_create: out is NULL");
    slam_vmap_params p;
    slam_vmap_default_params(&p);
    if (params) p = *params;
    SLAM_REQUIRE(p.leaf > 0 && std::isfinite(p.leaf) && p.initial_capacity >= 0 && p.initial_capacity <= (1 << 30), SLAM_E_INVALID,
                 "slam_vmap_create: leaf must be positive and finite, initial_capacity lie in 0 .. 2^30");
    SLAM_TRY(require_device());
    slam_vmap *m = new (std::nothrow) slam_vmap();
    SLAM_REQUIRE(m, SLAM_E_NOMEM, "slam_vmap_create: out of host memory");
    m->P = p;
    m->capacity = pow2_at_least(p.initial_capacity);
    m->P.initial_capacity = (int)m->capacity;
    int rc = m->ctr.alloc(kCounters * sizeof(uint32_t));
    if (rc == SLAM_OK) rc = new_table(m->table, m->capacity, nullptr);
    if (rc == SLAM_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
        set_error("slam_vmap_create: clearing the table failed");
        rc = SLAM_E_HIP;
    }
    if (rc != SLAM_OK) {
        delete m;
        return rc;
    }
    *out = m;
    return SLAM_OK;
}

void slam_vmap_destroy(slam_vmap_t *m)
{
    if (!m) return;
    (void)hipDeviceSynchronize();
    delete m;
}

int slam_vmap_clear(slam_vmap_t *m, slam_stream_t stream)
{
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_vmap_clear: map is NULL");
    hipStream_t st = as_stream(stream);
    SLAM_HIP(hipMemsetAsync(m->table.p, 0xff, (size_t)m->capacity * 8, st));
    SLAM_HIP(hipMemsetAsync(m->table.as<uint8_t>() + (size_t)m->capacity * 8, 0, (size_t)m->capacity * (kSlotBytes - 8), st));
    if (m->carved())
        for (DevMem *b : {&m->seen, &m->miss, &m->stamp}) SLAM_HIP(hipMemsetAsync(b->p, 0, (size_t)m->capacity * sizeof(uint32_t), st));
    if (m->dist_on) {
        SLAM_HIP(hipMemsetAsync(m->mom.p, 0, (size_t)m->capacity * kMomentBytes, st));
        m->dist_stale = true;
    }
    m->n_voxels = m->n_points = 0;
    return SLAM_OK;
}

int slam_vmap_integrate_dev(slam_vmap_t *m, const float *d_xyz, int n, int stride, const double R[9], const double t[3], int *n_dropped,
                            slam_stream_t stream)
{
    SLAM_REQUIRE(m && n >= 0 && stride >= 3 && (d_xyz || n == 0) && (R == nullptr) == (t == nullptr), SLAM_E_INVALID,
                 "slam_vmap_integrate_dev: a map, n >= 0, stride >= 3, points, and R and t both or neither");
    if (n_dropped) *n_dropped = 0;
    if (n == 0) return SLAM_OK;
    hipStream_t st = as_stream(stream);
    SLAM_TRY(make_room(m, n, st));
    Transform X{};
    X.on = R != nullptr;
    if (R) {
        for (int k = 0; k < 9; ++k) X.r[k] = R[k];
        for (int k = 0; k < 3; ++k) X.t[k] = t[k];
    }
    uint32_t *h = static_cast<uint32_t *>(pinned_scratch(kCounters * sizeof(uint32_t)));
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_vmap: no pinned memory for the counters");
    SLAM_HIP(hipMemsetAsync(m->ctr.p, 0, kCounters * sizeof(uint32_t), st));
    if (m->dist_on) {
        hipLaunchKernelGGL(vmap_integrate_moments_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, st, d_xyz, n, stride, X, m->P.leaf,
                           (long long)std::rint(m->P.leaf * kFix), m->view(), m->moments(), m->ctr.as<uint32_t>());
        m->dist_stale = true;
    } else {
        hipLaunchKernelGGL(vmap_integrate_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, st, d_xyz, n, stride, X, m->P.leaf, m->view(),
                           m->ctr.as<uint32_t>());
    }
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(h, m->ctr.p, kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    m->n_voxels += h[kClaimed];
    m->n_points += (int64_t)n - h[kDropped];
    if (n_dropped) *n_dropped = (int)h[kDropped];
    SLAM_REQUIRE(!h[kError], SLAM_E_HIP, "slam_vmap_integrate: a probe ran through all %lld slots (%lld voxels): points were lost",
                 (long long)m->capacity, (long long)m->n_voxels);
    return SLAM_OK;
}

int slam_vmap_integrate(slam_vmap_t *m, const float *xyz, int n, int stride, const double R[9], const double t[3], int *n_dropped)
{
    SLAM_REQUIRE(m && n >= 0 && stride >= 3 && (xyz || n == 0) && (R == nullptr) == (t == nullptr), SLAM_E_INVALID,
                 "slam_vmap_integrate: a map, n >= 0, stride >= 3, points, and R and t both or neither");
    if (n_dropped) *n_dropped = 0;
    if (n == 0) return SLAM_OK;
    const size_t bytes = (size_t)n * stride * sizeof(float);
    SLAM_TRY(reserve_quarter(m->stage_in, bytes));
    SLAM_HIP(hipMemcpy(m->stage_in.p, xyz, bytes, hipMemcpyHostToDevice));
    return slam_vmap_integrate_dev(m, m->stage_in.as<float>(), n, stride, R, t, n_dropped, nullptr);
}

int slam_vmap_extract_dev(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, float *d_xyz4, uint32_t *d_count,
                          uint64_t *d_key, int cap, int *n_out, slam_stream_t stream)
{
    SLAM_TRY(check_extract("slam_vmap_extract_dev", m, lo_xy, hi_xy, min_count, cap, n_out));
    hipStream_t st = as_stream(stream);
    int64_t     n = 0;
    SLAM_TRY(select_slots(m, lo_xy, hi_xy, min_count, st, &n));
    *n_out = (int)n;
    SLAM_REQUIRE(n <= cap, SLAM_E_NOMEM, "slam_vmap_extract_dev: %lld voxels, room for %d", (long long)n, cap);
    return sort_and_write(m, (int)n, d_xyz4, d_count, d_key, st);
}

static int read_host(const char *who, slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, float *xyz4, uint32_t *count,
                     uint64_t *key, int64_t *sums, int cap, int *n_out, const uint32_t *ratio = nullptr)
{
    SLAM_TRY(check_extract(who, m, lo_xy, hi_xy, min_count, cap, n_out));
    int64_t n = 0;
    SLAM_TRY(select_slots(m, lo_xy, hi_xy, min_count, nullptr, &n, ratio));
    *n_out = (int)n;
    SLAM_REQUIRE(n <= cap, SLAM_E_NOMEM, "%s: %lld voxels, room for %d", who, (long long)n, cap);
    if (n == 0) return SLAM_OK;
    const size_t N = (size_t)n;
    SLAM_TRY(reserve_quarter(m->stage_out, N * 52)); // keys, sums, then centroids, then counts: each aligned to its type
    uint64_t *d_key = m->stage_out.as<uint64_t>();
    int64_t  *d_sums = reinterpret_cast<int64_t *>(d_key + N);
    float    *d_xyz4 = reinterpret_cast<float *>(d_sums + 3 * N);
    uint32_t *d_count = reinterpret_cast<uint32_t *>(d_xyz4 + 4 * N);
    SLAM_TRY(sort_and_write(m, (int)n, xyz4 ? d_xyz4 : nullptr, count ? d_count : nullptr, key ? d_key : nullptr, nullptr, sums ? d_sums : nullptr));
    if (xyz4) SLAM_HIP(hipMemcpy(xyz4, d_xyz4, N * 16, hipMemcpyDeviceToHost));
    if (count) SLAM_HIP(hipMemcpy(count, d_count, N * 4, hipMemcpyDeviceToHost));
    if (key) SLAM_HIP(hipMemcpy(key, d_key, N * 8, hipMemcpyDeviceToHost));
    if (sums) SLAM_HIP(hipMemcpy(sums, d_sums, N * 24, hipMemcpyDeviceToHost));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_vmap_read(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, float *xyz4, uint32_t *count, uint64_t *key,
                   int cap, int *n_out)
{
    return read_host("slam_vmap_read", m, lo_xy, hi_xy, min_count, xyz4, count, key, nullptr, cap, n_out);
}

int slam_vmap_read_sums(slam_vmap_t *m, int64_t *sums, uint32_t *count, uint64_t *key, int cap, int *n_out)
{
    return read_host("slam_vmap_read_sums", m, nullptr, nullptr, 0, nullptr, count, key, sums, cap, n_out);
}

int slam_vmap_info(slam_vmap_t *m, int64_t *n_voxels, int64_t *capacity, int64_t *n_points, size_t *device_bytes)
{
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_vmap_info: map is NULL");
    if (n_voxels) *n_voxels = m->n_voxels;
    if (capacity) *capacity = m->capacity;
    if (n_points) *n_points = m->n_points;
    if (device_bytes)
        *device_bytes = m->table.cap + m->ctr.cap + m->flag.cap + m->sel.cap + m->keys_in.cap + m->keys_out.cap + m->sel_sorted.cap + m->tmp.cap +
                        m->stage_in.cap + m->stage_out.cap + m->seen.cap + m->miss.cap + m->stamp.cap + m->cctr.cap + m->rays.cap + m->chunks.cap +
                        m->offs.cap + m->mom.cap + m->dist.cap + m->reg_work.cap + m->actr.cap;
    return SLAM_OK;
}

// ---------------------------------------------------------------- carve (docs/VOXEL_MAP.md section 8)
void slam_vmap_default_carve_params(slam_vmap_carve_params *p)
{
    if (!p) return;
    p->end_margin = 1;
    p->tail_num = 1, p->tail_den = 8;
    p->max_ray_cells = 512;
}

// Everything that can be refused without a handle, then the device, then the handle: a machine without a device answers
// SLAM_E_NO_DEVICE to well-formed arguments (no handle can exist there).
static int check_carve(const char *who, slam_vmap *m, const void *xyz, int n, int stride, const double *R, const double *t,
                       const slam_vmap_carve_params &p)
{
    SLAM_REQUIRE(n >= 0 && stride >= 3 && (xyz || n == 0) && (R == nullptr) == (t == nullptr), SLAM_E_INVALID,
                 "%s: n >= 0, stride >= 3, points, and R and t both or neither", who);
    SLAM_REQUIRE(p.end_margin >= 0 && p.tail_num >= 0 && p.tail_den > 0 && p.max_ray_cells >= 1, SLAM_E_INVALID,
                 "%s: end_margin >= 0, tail_num >= 0, tail_den > 0 and max_ray_cells >= 1", who);
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "%s: map is NULL", who);
    return SLAM_OK;
}

int slam_vmap_carve_dev(slam_vmap_t *m, const float *d_xyz, int n, int stride, const double R[9], const double t[3], const double origin[3],
                        const slam_vmap_carve_params *params, slam_vmap_carve_result *result, slam_stream_t stream)
{
    slam_vmap_carve_params p;
    slam_vmap_default_carve_params(&p);
    if (params) p = *params;
    SLAM_TRY(check_carve("slam_vmap_carve_dev", m, d_xyz, n, stride, R, t, p));
    if (result) *result = slam_vmap_carve_result{};
    Transform X{};
    X.on = R != nullptr;
    if (R) {
        for (int k = 0; k < 9; ++k) X.r[k] = R[k];
        for (int k = 0; k < 3; ++k) X.t[k] = t[k];
    }
    // the origin and its cell, with a point's arithmetic (this file is compiled without contraction): decided before any launch
    Carve A{};
    const double o[3] = {origin ? origin[0] : 0.0, origin ? origin[1] : 0.0, origin ? origin[2] : 0.0};
    for (int k = 0; k < 3; ++k) {
        float v = (float)o[k];
        if (R) {
            const double a = R[3 * k] * o[0], b = R[3 * k + 1] * o[1], c = R[3 * k + 2] * o[2];
            v = (float)(((a + b) + c) + t[k]);
        }
        const double c = std::floor((double)v / m->P.leaf);
        SLAM_REQUIRE(std::fabs(v) < kCoordLimit && std::fabs(c) < (double)kCellLimit, SLAM_E_INVALID,
                     "slam_vmap_carve: the origin has no cell (axis %d: %g)", k, (double)v);
        A.c0[k] = (int)c;
    }
    A.end_margin = p.end_margin, A.tail_num = p.tail_num, A.tail_den = p.tail_den, A.max_ray_cells = p.max_ray_cells;
    if (n == 0) return SLAM_OK;
    // chunks travel as u32 through the scan: a ray has at most 2^21 cells
    const int64_t longest = p.max_ray_cells < 2 * kCellLimit ? p.max_ray_cells : 2 * kCellLimit;
    const int64_t max_chunks = (int64_t)n * ((longest + kChunk - 1) / kChunk);
    SLAM_REQUIRE(max_chunks < (1ll << 32), SLAM_E_NOMEM, "slam_vmap_carve: %d rays of up to %lld cells are more than 2^32 chunks of %d steps", n,
                 (long long)longest, kChunk);

    hipStream_t  st = as_stream(stream);
    const size_t plane = (size_t)m->capacity * sizeof(uint32_t);
    SLAM_TRY(ensure_carve_planes(m, st));
    if (m->serial >= 0x7fffffffu) { // 2 s + 1 would no longer fit: forget every stamp and start again
        SLAM_HIP(hipMemsetAsync(m->stamp.p, 0, plane, st));
        m->serial = 1;
    }
    A.tag = 2u * m->serial++;
    m->dist_stale = true; // the carved rule may be part of the plane rule
    SLAM_TRY(reserve_quarter(m->rays, (size_t)n * sizeof(int4)));
    SLAM_TRY(reserve_quarter(m->chunks, ((size_t)n + 1) * sizeof(uint32_t)));
    SLAM_TRY(reserve_quarter(m->offs, ((size_t)n + 1) * sizeof(uint32_t)));
    size_t tb = 0;
    SLAM_HIP(rocprim::exclusive_scan(nullptr, tb, m->chunks.as<uint32_t>(), m->offs.as<uint32_t>(), 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
    SLAM_TRY(m->tmp.reserve(tb + 16));
    tb = m->tmp.cap;
    unsigned long long *h = static_cast<unsigned long long *>(pinned_scratch(kCarveCounters * sizeof(unsigned long long)));
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_vmap: no pinned memory for the counters");

    unsigned long long *d_ctr = m->cctr.as<unsigned long long>();
    SLAM_HIP(hipMemsetAsync(d_ctr, 0, kCarveCounters * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(vmap_carve_rays_kernel, dim3(blocks_for((uint64_t)n + 1)), dim3(256), 0, st, d_xyz, n, stride, X, m->P.leaf, m->view(),
                       m->planes(), A, m->rays.as<int4>(), m->chunks.as<uint32_t>(), d_ctr);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(rocprim::exclusive_scan(m->tmp.p, tb, m->chunks.as<uint32_t>(), m->offs.as<uint32_t>(), 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
    // one wave per chunk, four to a block; beyond 2048 blocks the waves stride over the chunks
    const int64_t blocks = (max_chunks + 3) / 4;
    hipLaunchKernelGGL(vmap_carve_walk_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, m->rays.as<int4>(),
                       m->offs.as<uint32_t>(), n, (uint32_t)max_chunks, m->view(), m->planes(), A, d_ctr);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(h, d_ctr, kCarveCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    if (result) {
        result->n_dropped = (int64_t)h[kcDropped];
        result->n_rays = (int64_t)n - result->n_dropped;
        result->n_skipped = (int64_t)h[kcSkipped];
        result->n_steps = (int64_t)h[kcSteps];
        result->n_seen = (int64_t)h[kcSeen];
        result->n_missed = (int64_t)h[kcMissed];
    }
    return SLAM_OK;
}

int slam_vmap_carve(slam_vmap_t *m, const float *xyz, int n, int stride, const double R[9], const double t[3], const double origin[3],
                    const slam_vmap_carve_params *params, slam_vmap_carve_result *result)
{
    slam_vmap_carve_params p;
    slam_vmap_default_carve_params(&p);
    if (params) p = *params;
    SLAM_TRY(check_carve("slam_vmap_carve", m, xyz, n, stride, R, t, p));
    const size_t bytes = (size_t)n * stride * sizeof(float);
    if (n > 0) {
        SLAM_TRY(reserve_quarter(m->stage_in, bytes));
        SLAM_HIP(hipMemcpy(m->stage_in.p, xyz, bytes, hipMemcpyHostToDevice));
    }
    return slam_vmap_carve_dev(m, m->stage_in.as<float>(), n, stride, R, t, origin, params, result, nullptr);
}

static int check_carved(const char *who, slam_vmap *m, const float *lo, const float *hi, int min_count, int num, int den, int cap, int *n_out)
{
    SLAM_REQUIRE(n_out && cap >= 0 && min_count >= 0 && (lo == nullptr) == (hi == nullptr) && num >= 0 && den > 0, SLAM_E_INVALID,
                 "%s: n_out, cap >= 0, min_count >= 0, lo_xy and hi_xy both or neither, max_miss_num >= 0 and max_miss_den > 0", who);
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "%s: map is NULL", who);
    return SLAM_OK;
}

int slam_vmap_extract_carved_dev(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, int max_miss_num, int max_miss_den,
                                 float *d_xyz4, uint32_t *d_count, uint64_t *d_key, int cap, int *n_out, slam_stream_t stream)
{
    SLAM_TRY(check_carved("slam_vmap_extract_carved_dev", m, lo_xy, hi_xy, min_count, max_miss_num, max_miss_den, cap, n_out));
    hipStream_t    st = as_stream(stream);
    int64_t        n = 0;
    const uint32_t ratio[2] = {(uint32_t)max_miss_num, (uint32_t)max_miss_den};
    SLAM_TRY(select_slots(m, lo_xy, hi_xy, min_count, st, &n, ratio));
    *n_out = (int)n;
    SLAM_REQUIRE(n <= cap, SLAM_E_NOMEM, "slam_vmap_extract_carved_dev: %lld voxels, room for %d", (long long)n, cap);
    return sort_and_write(m, (int)n, d_xyz4, d_count, d_key, st);
}

int slam_vmap_read_carved(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, int max_miss_num, int max_miss_den,
                          float *xyz4, uint32_t *count, uint64_t *key, int cap, int *n_out)
{
    SLAM_TRY(check_carved("slam_vmap_read_carved", m, lo_xy, hi_xy, min_count, max_miss_num, max_miss_den, cap, n_out));
    const uint32_t ratio[2] = {(uint32_t)max_miss_num, (uint32_t)max_miss_den};
    return read_host("slam_vmap_read_carved", m, lo_xy, hi_xy, min_count, xyz4, count, key, nullptr, cap, n_out, ratio);
}

int slam_vmap_read_carve(slam_vmap_t *m, uint32_t *seen, uint32_t *miss, uint64_t *key, int cap, int *n_out)
{
    SLAM_REQUIRE(n_out && cap >= 0, SLAM_E_INVALID, "slam_vmap_read_carve: n_out and cap >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_vmap_read_carve: map is NULL");
    int64_t n = 0;
    SLAM_TRY(select_slots(m, nullptr, nullptr, 0, nullptr, &n));
    *n_out = (int)n;
    SLAM_REQUIRE(n <= cap, SLAM_E_NOMEM, "slam_vmap_read_carve: %lld voxels, room for %d", (long long)n, cap);
    if (n == 0) return SLAM_OK;
    const size_t N = (size_t)n;
    SLAM_TRY(reserve_quarter(m->stage_out, N * 16)); // keys, then seen, then miss
    uint64_t *d_key = m->stage_out.as<uint64_t>();
    uint32_t *d_seen = reinterpret_cast<uint32_t *>(d_key + N), *d_miss = d_seen + N;
    SLAM_TRY(sort_slots(m, (int)n, nullptr));
    if (m->carved()) {
        hipLaunchKernelGGL(vmap_write_carve_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, nullptr, m->planes(), m->sel_sorted.as<uint32_t>(),
                           m->keys_out.as<uint64_t>(), (int)n, d_seen, d_miss, d_key);
        SLAM_HIP(hipGetLastError());
        if (seen) SLAM_HIP(hipMemcpy(seen, d_seen, N * 4, hipMemcpyDeviceToHost));
        if (miss) SLAM_HIP(hipMemcpy(miss, d_miss, N * 4, hipMemcpyDeviceToHost));
        if (key) SLAM_HIP(hipMemcpy(key, d_key, N * 8, hipMemcpyDeviceToHost));
    } else { // never carved: zeros, and the keys as the sort left them
        if (seen) std::memset(seen, 0, N * 4);
        if (miss) std::memset(miss, 0, N * 4);
        if (key) SLAM_HIP(hipMemcpy(key, m->keys_out.p, N * 8, hipMemcpyDeviceToHost));
    }
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

// ---------------------------------------------------------------- moments and distributions (docs/VOXEL_MAP.md section 9)
void slam_vmap_default_dist_params(slam_vmap_dist_params *p)
{
    if (!p) return;
    p->min_points = 6;
    p->flat_ratio = 4.0, p->line_ratio = 0.01;
    p->epsilon = 1e-3; // slam_kf_gicp_params.gicp_epsilon's
    p->max_miss_num = 0, p->max_miss_den = 0;
}

int slam_vmap_enable_distributions(slam_vmap_t *m, const slam_vmap_dist_params *params)
{
    slam_vmap_dist_params p;
    slam_vmap_default_dist_params(&p);
    if (params) p = *params;
    SLAM_REQUIRE(p.min_points >= 1 && p.flat_ratio >= 0 && p.line_ratio >= 0 && p.epsilon > 0 && p.max_miss_num >= 0 && p.max_miss_den >= 0,
                 SLAM_E_INVALID, "slam_vmap_enable_distributions: min_points >= 1, ratios >= 0, epsilon > 0, max_miss_num and max_miss_den >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_vmap_enable_distributions: map is NULL");
    SLAM_REQUIRE(m->n_voxels == 0, SLAM_E_INVALID, "slam_vmap_enable_distributions: the map holds %lld voxels: legal only after create or clear",
                 (long long)m->n_voxels);
    SLAM_REQUIRE(m->P.leaf <= 8.0, SLAM_E_INVALID, "slam_vmap_enable_distributions: leaf %g is more than the 8 m the moments' bound allows", m->P.leaf);
    if (!m->dist_on) {
        SLAM_TRY(m->mom.alloc((size_t)m->capacity * kMomentBytes));
        SLAM_TRY(m->dist.alloc((size_t)m->capacity * kDistBytes));
    }
    SLAM_HIP(hipMemsetAsync(m->mom.p, 0, (size_t)m->capacity * kMomentBytes, nullptr));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    m->DP = p;
    m->dist_on = true, m->dist_stale = true;
    return SLAM_OK;
}

int slam_vmap_compute_distributions(slam_vmap_t *m, slam_stream_t stream)
{
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m && m->dist_on, SLAM_E_INVALID, "slam_vmap_compute_distributions: a map with distributions enabled");
    if (!m->dist_stale) return SLAM_OK;
    DistRule R;
    R.min_points = (uint32_t)m->DP.min_points, R.miss_num = (uint32_t)m->DP.max_miss_num, R.miss_den = (uint32_t)m->DP.max_miss_den;
    R.flat_ratio = m->DP.flat_ratio, R.line_ratio = m->DP.line_ratio, R.eps = m->DP.epsilon;
    const Planes C = m->carved() ? m->planes() : Planes{nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(vmap_distributions_kernel, dim3(blocks_for((uint64_t)m->capacity)), dim3(256), 0, as_stream(stream), m->view(), m->moments(), C, R,
                       m->dists());
    SLAM_HIP(hipGetLastError());
    m->dist_stale = false;
    return SLAM_OK;
}

// every occupied voxel's slot in key order into m->sel_sorted (keys into m->keys_out) on the null stream; *n their number
static int all_slots_sorted(const char *who, slam_vmap *m, int cap, int *n_out, int64_t *n)
{
    SLAM_TRY(select_slots(m, nullptr, nullptr, 0, nullptr, n));
    *n_out = (int)*n;
    SLAM_REQUIRE(*n <= cap, SLAM_E_NOMEM, "%s: %lld voxels, room for %d", who, (long long)*n, cap);
    if (*n) SLAM_TRY(sort_slots(m, (int)*n, nullptr));
    return SLAM_OK;
}

int slam_vmap_read_moments(slam_vmap_t *m, int64_t *E3, int64_t *M6, uint64_t *key, int cap, int *n_out)
{
    SLAM_REQUIRE(n_out && cap >= 0, SLAM_E_INVALID, "slam_vmap_read_moments: n_out and cap >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m && m->dist_on, SLAM_E_INVALID, "slam_vmap_read_moments: a map with distributions enabled");
    int64_t n = 0;
    SLAM_TRY(all_slots_sorted("slam_vmap_read_moments", m, cap, n_out, &n));
    if (n == 0) return SLAM_OK;
    const size_t N = (size_t)n;
    SLAM_TRY(reserve_quarter(m->stage_out, N * 80)); // keys, E, M
    uint64_t *d_key = m->stage_out.as<uint64_t>();
    int64_t  *d_E = reinterpret_cast<int64_t *>(d_key + N), *d_M = d_E + 3 * N;
    hipLaunchKernelGGL(vmap_write_moments_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, nullptr, m->moments(), m->sel_sorted.as<uint32_t>(),
                       m->keys_out.as<uint64_t>(), (int)n, d_E, d_M, d_key);
    SLAM_HIP(hipGetLastError());
    if (E3) SLAM_HIP(hipMemcpy(E3, d_E, N * 24, hipMemcpyDeviceToHost));
    if (M6) SLAM_HIP(hipMemcpy(M6, d_M, N * 48, hipMemcpyDeviceToHost));
    if (key) SLAM_HIP(hipMemcpy(key, d_key, N * 8, hipMemcpyDeviceToHost));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

int slam_vmap_read_distributions(slam_vmap_t *m, float *centroid3, double *normal3, double *cov6, double *eig3, uint8_t *flag, uint64_t *key, int cap,
                                 int *n_out)
{
    SLAM_REQUIRE(n_out && cap >= 0, SLAM_E_INVALID, "slam_vmap_read_distributions: n_out and cap >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m && m->dist_on, SLAM_E_INVALID, "slam_vmap_read_distributions: a map with distributions enabled");
    SLAM_TRY(slam_vmap_compute_distributions(m, nullptr));
    int64_t n = 0;
    SLAM_TRY(all_slots_sorted("slam_vmap_read_distributions", m, cap, n_out, &n));
    if (n == 0) return SLAM_OK;
    const size_t N = (size_t)n;
    SLAM_TRY(reserve_quarter(m->stage_out, N * 120)); // normals, covariances, eigenvalues, keys, then centroids, then flags
    double   *d_nrm = m->stage_out.as<double>(), *d_cov = d_nrm + 3 * N, *d_eig = d_cov + 6 * N;
    uint64_t *d_key = reinterpret_cast<uint64_t *>(d_eig + 3 * N);
    float    *d_cen = reinterpret_cast<float *>(d_key + N);
    uint8_t  *d_flag = reinterpret_cast<uint8_t *>(d_cen + 3 * N);
    hipLaunchKernelGGL(vmap_write_dist_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, nullptr, m->dists(), m->sel_sorted.as<uint32_t>(),
                       m->keys_out.as<uint64_t>(), (int)n, d_nrm, d_cov, d_eig, d_key, d_cen, d_flag);
    SLAM_HIP(hipGetLastError());
    if (centroid3) SLAM_HIP(hipMemcpy(centroid3, d_cen, N * 12, hipMemcpyDeviceToHost));
    if (normal3) SLAM_HIP(hipMemcpy(normal3, d_nrm, N * 24, hipMemcpyDeviceToHost));
    if (cov6) SLAM_HIP(hipMemcpy(cov6, d_cov, N * 48, hipMemcpyDeviceToHost));
    if (eig3) SLAM_HIP(hipMemcpy(eig3, d_eig, N * 24, hipMemcpyDeviceToHost));
    if (flag) SLAM_HIP(hipMemcpy(flag, d_flag, N, hipMemcpyDeviceToHost));
    if (key) SLAM_HIP(hipMemcpy(key, d_key, N * 8, hipMemcpyDeviceToHost));
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

// ---------------------------------------------------------------- absorb, merge, save, load (docs/VOXEL_MAP.md section 10)
// `lanes` records (or source slots) of S into m, with room made for `n_new` more voxels first: waits once for st.
static int absorb_records(slam_vmap *m, Records S, uint64_t lanes, int64_t n_new, int64_t *n_rejected, hipStream_t st)
{
    SLAM_TRY(make_room(m, n_new, st));
    if (S.seen) SLAM_TRY(ensure_carve_planes(m, st)); // after the growth: at the table's size
    if (!m->actr.p) SLAM_TRY(m->actr.alloc(kAbsorbCounters * sizeof(uint32_t)));
    uint32_t *h = static_cast<uint32_t *>(pinned_scratch(kAbsorbCounters * sizeof(uint32_t)));
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_vmap: no pinned memory for the counters");
    SLAM_HIP(hipMemsetAsync(m->actr.p, 0, kAbsorbCounters * sizeof(uint32_t), st));
    const Planes  P = m->carved() ? m->planes() : Planes{nullptr, nullptr, nullptr};
    const Moments Q = m->dist_on ? m->moments() : Moments{};
    hipLaunchKernelGGL(vmap_absorb_kernel, dim3(blocks_for(lanes)), dim3(256), 0, st, S, lanes, m->view(), P, Q, m->actr.as<uint32_t>());
    SLAM_HIP(hipGetLastError());
    m->dist_stale = true;
    SLAM_HIP(hipMemcpyAsync(h, m->actr.p, kAbsorbCounters * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    m->n_voxels += h[kClaimed];
    m->n_points += (int64_t)((uint64_t)h[kPoints] | (uint64_t)h[kPoints + 1] << 32);
    if (n_rejected) *n_rejected = (int64_t)h[kDropped];
    SLAM_REQUIRE(!h[kError], SLAM_E_HIP, "slam_vmap_absorb: a probe ran through all %lld slots (%lld voxels): records were lost",
                 (long long)m->capacity, (long long)m->n_voxels);
    return SLAM_OK;
}

static Records packed_records(const uint64_t *key, const uint32_t *count, const int64_t *sums, const uint32_t *seen, const uint32_t *miss,
                              const int64_t *E3, const int64_t *M6)
{
    Records S{};
    S.key = key, S.count = count, S.seen = seen, S.miss = miss;
    for (int k = 0; k < 3; ++k) S.sum[k] = reinterpret_cast<const unsigned long long *>(sums) + k;
    if (E3) {
        for (int k = 0; k < 3; ++k) S.E[k] = reinterpret_cast<const unsigned long long *>(E3) + k;
        for (int k = 0; k < 6; ++k) S.M[k] = reinterpret_cast<const unsigned long long *>(M6) + k;
    }
    S.w3 = 3, S.w6 = 6, S.slots = 0;
    return S;
}

// What can be refused without a handle, then the device, then the handle (the rule of check_carve).
static int check_absorb(const char *who, slam_vmap *m, const void *key, const void *count, const void *sums, const void *seen, const void *miss,
                        const void *E3, const void *M6, int n)
{
    SLAM_REQUIRE(n >= 0 && (n == 0 || (key && count && sums)) && (seen == nullptr) == (miss == nullptr) && (E3 == nullptr) == (M6 == nullptr),
                 SLAM_E_INVALID, "%s: n >= 0, key, count and sums, seen and miss both or neither, E3 and M6 both or neither", who);
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "%s: map is NULL", who);
    return SLAM_OK;
}

int slam_vmap_layout(slam_vmap_t *m, double *leaf, int *carved, int *distributions, slam_vmap_dist_params *dp)
{
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_vmap_layout: map is NULL");
    if (leaf) *leaf = m->P.leaf;
    if (carved) *carved = m->carved() ? 1 : 0;
    if (distributions) *distributions = m->dist_on ? 1 : 0;
    if (dp) *dp = m->dist_on ? m->DP : slam_vmap_dist_params{};
    return SLAM_OK;
}

int slam_vmap_absorb_dev(slam_vmap_t *m, const uint64_t *d_key, const uint32_t *d_count, const int64_t *d_sums, const uint32_t *d_seen,
                         const uint32_t *d_miss, const int64_t *d_E3, const int64_t *d_M6, int n, int64_t *n_rejected, slam_stream_t stream)
{
    SLAM_TRY(check_absorb("slam_vmap_absorb_dev", m, d_key, d_count, d_sums, d_seen, d_miss, d_E3, d_M6, n));
    if (n_rejected) *n_rejected = 0;
    if (n == 0) return SLAM_OK;
    SLAM_REQUIRE((d_E3 != nullptr) == m->dist_on, SLAM_E_INVALID,
                 "slam_vmap_absorb_dev: records %s moments into a map %s distributions: a half-filled moment plane would give wrong planes",
                 d_E3 ? "with" : "without", m->dist_on ? "with" : "without");
    return absorb_records(m, packed_records(d_key, d_count, d_sums, d_seen, d_miss, d_E3, d_M6), (uint64_t)n, n, n_rejected, as_stream(stream));
}

int slam_vmap_absorb(slam_vmap_t *m, const uint64_t *key, const uint32_t *count, const int64_t *sums, const uint32_t *seen, const uint32_t *miss,
                     const int64_t *E3, const int64_t *M6, int n, int64_t *n_rejected)
{
    SLAM_TRY(check_absorb("slam_vmap_absorb", m, key, count, sums, seen, miss, E3, M6, n));
    if (n_rejected) *n_rejected = 0;
    if (n == 0) return SLAM_OK;
    SLAM_REQUIRE((E3 != nullptr) == m->dist_on, SLAM_E_INVALID,
                 "slam_vmap_absorb: records %s moments into a map %s distributions: a half-filled moment plane would give wrong planes",
                 E3 ? "with" : "without", m->dist_on ? "with" : "without");
    // staged as keys, sums, E, M (8-byte words), then count, seen, miss
    const size_t N = (size_t)n;
    SLAM_TRY(reserve_quarter(m->stage_in, N * (8 + 24 + (E3 ? 72 : 0) + 4 + (seen ? 8 : 0))));
    uint64_t *d_key = m->stage_in.as<uint64_t>();
    int64_t  *d_sums = reinterpret_cast<int64_t *>(d_key + N), *d_E = d_sums + 3 * N, *d_M = d_E + 3 * N;
    uint32_t *d_count = reinterpret_cast<uint32_t *>(E3 ? d_M + 6 * N : d_E), *d_seen = d_count + N, *d_miss = d_seen + N;
    SLAM_HIP(hipMemcpy(d_key, key, N * 8, hipMemcpyHostToDevice));
    SLAM_HIP(hipMemcpy(d_sums, sums, N * 24, hipMemcpyHostToDevice));
    SLAM_HIP(hipMemcpy(d_count, count, N * 4, hipMemcpyHostToDevice));
    if (E3) {
        SLAM_HIP(hipMemcpy(d_E, E3, N * 24, hipMemcpyHostToDevice));
        SLAM_HIP(hipMemcpy(d_M, M6, N * 48, hipMemcpyHostToDevice));
    }
    if (seen) {
        SLAM_HIP(hipMemcpy(d_seen, seen, N * 4, hipMemcpyHostToDevice));
        SLAM_HIP(hipMemcpy(d_miss, miss, N * 4, hipMemcpyHostToDevice));
    }
    return absorb_records(m, packed_records(d_key, d_count, d_sums, seen ? d_seen : nullptr, seen ? d_miss : nullptr, E3 ? d_E : nullptr, E3 ? d_M : nullptr),
                          (uint64_t)n, n, n_rejected, nullptr);
}

int slam_vmap_merge(slam_vmap_t *dst, slam_vmap_t *src, int64_t *n_rejected, slam_stream_t stream)
{
    SLAM_REQUIRE(dst != src || !dst, SLAM_E_INVALID, "slam_vmap_merge: a map cannot be merged into itself");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(dst && src, SLAM_E_INVALID, "slam_vmap_merge: a map is NULL");
    SLAM_REQUIRE(std::memcmp(&dst->P.leaf, &src->P.leaf, sizeof(double)) == 0, SLAM_E_INVALID,
                 "slam_vmap_merge: leaves %.17g and %.17g differ: the integer sums of one cannot be moved into the other's voxels", dst->P.leaf,
                 src->P.leaf);
    SLAM_REQUIRE(dst->dist_on == src->dist_on, SLAM_E_INVALID, "slam_vmap_merge: distributions on one side only");
    if (n_rejected) *n_rejected = 0;
    if (src->n_voxels == 0) return SLAM_OK;
    Records     S{};
    const Table T = src->view();
    S.key = T.key, S.count = T.count;
    for (int k = 0; k < 3; ++k) S.sum[k] = T.sum[k];
    if (src->carved()) S.seen = src->seen.as<uint32_t>(), S.miss = src->miss.as<uint32_t>();
    if (src->dist_on) {
        const Moments Q = src->moments();
        for (int k = 0; k < 3; ++k) S.E[k] = Q.E[k];
        for (int k = 0; k < 6; ++k) S.M[k] = Q.M[k];
    }
    S.w3 = S.w6 = 1, S.slots = 1;
    return absorb_records(dst, S, (uint64_t)src->capacity, src->n_voxels, n_rejected, as_stream(stream));
}

// ---------------------------------------------------------------- coarsen (docs/VOXEL_MAP.md section 11)
int slam_vmap_coarsen(slam_vmap_t *dst, slam_vmap_t *src, slam_stream_t stream)
{
    SLAM_REQUIRE(dst != src || !dst, SLAM_E_INVALID, "slam_vmap_coarsen: a map cannot be coarsened into itself");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(dst && src, SLAM_E_INVALID, "slam_vmap_coarsen: a map is NULL");
    int shift = 0;
    for (int j = 1; j <= 8 && !shift; ++j) {
        const double up = std::ldexp(src->P.leaf, j);
        if (std::memcmp(&dst->P.leaf, &up, sizeof(double)) == 0) shift = j;
    }
    SLAM_REQUIRE(shift, SLAM_E_INVALID, "slam_vmap_coarsen: leaf %.17g is not leaf %.17g times 2, 4 .. 256: the finer cells do not nest in the coarser",
                 dst->P.leaf, src->P.leaf);
    SLAM_REQUIRE(dst->dist_on == src->dist_on, SLAM_E_INVALID, "slam_vmap_coarsen: distributions on one side only");
    const double fine = std::ldexp(src->P.leaf, 16); // the leaf in units of 2^-16 m
    SLAM_REQUIRE(!src->dist_on || fine == std::floor(fine), SLAM_E_INVALID,
                 "slam_vmap_coarsen: leaf %.17g is no multiple of 2^-16 m: the moments' floor(d / 16) does not split over the finer cells", src->P.leaf);
    if (src->n_voxels == 0) return SLAM_OK;
    hipStream_t st = as_stream(stream);
    SLAM_TRY(make_room(dst, src->n_voxels, st));
    if (!dst->actr.p) SLAM_TRY(dst->actr.alloc(kAbsorbCounters * sizeof(uint32_t)));
    uint32_t *h = static_cast<uint32_t *>(pinned_scratch(kAbsorbCounters * sizeof(uint32_t)));
    SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_vmap: no pinned memory for the counters");
    SLAM_HIP(hipMemsetAsync(dst->actr.p, 0, kAbsorbCounters * sizeof(uint32_t), st));
    const Moments SQ = src->dist_on ? src->moments() : Moments{};
    const Moments Q = dst->dist_on ? dst->moments() : Moments{};
    const long long unit = src->dist_on ? (long long)fine : 0; // L / 16: L = leaf 2^20 exactly here
    hipLaunchKernelGGL(vmap_coarsen_kernel, dim3(blocks_for((uint64_t)src->capacity)), dim3(256), 0, st, src->view(), SQ, shift, unit, dst->view(), Q,
                       dst->actr.as<uint32_t>());
    SLAM_HIP(hipGetLastError());
    dst->dist_stale = true;
    SLAM_HIP(hipMemcpyAsync(h, dst->actr.p, kAbsorbCounters * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    dst->n_voxels += h[kClaimed];
    dst->n_points += (int64_t)((uint64_t)h[kPoints] | (uint64_t)h[kPoints + 1] << 32);
    SLAM_REQUIRE(!h[kError], SLAM_E_HIP, "slam_vmap_coarsen: a probe ran through all %lld slots (%lld voxels): voxels were lost",
                 (long long)dst->capacity, (long long)dst->n_voxels);
    return SLAM_OK;
}

int slam_vmap_save(slam_vmap_t *m, const char *path)
{
    SLAM_REQUIRE(path && path[0], SLAM_E_INVALID, "slam_vmap_save: path is NULL or empty");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_vmap_save: map is NULL");
    SLAM_REQUIRE(m->n_voxels <= vmap_file::kMaxVoxels, SLAM_E_INVALID, "slam_vmap_save: %lld voxels are more than the 2^30 a file holds",
                 (long long)m->n_voxels);
    try {
        const size_t          N = (size_t)m->n_voxels;
        const int             cap = (int)m->n_voxels;
        int                   got = 0;
        std::vector<uint64_t> key(N);
        std::vector<uint32_t> count(N), seen, miss;
        std::vector<int64_t>  sums(3 * N), E, M;
        vmap_file::Meta       meta;
        meta.leaf = m->P.leaf, meta.n = m->n_voxels, meta.n_points = m->n_points;
        SLAM_TRY(slam_vmap_read_sums(m, sums.data(), count.data(), key.data(), cap, &got));
        SLAM_REQUIRE(got == cap, SLAM_E_HIP, "slam_vmap_save: the table holds %d voxels, the handle counts %d", got, cap);
        if (m->carved()) {
            meta.flags |= vmap_file::kCarve;
            seen.resize(N), miss.resize(N);
            SLAM_TRY(slam_vmap_read_carve(m, seen.data(), miss.data(), nullptr, cap, &got));
        }
        if (m->dist_on) {
            meta.flags |= vmap_file::kMoments;
            meta.min_points = m->DP.min_points, meta.max_miss_num = m->DP.max_miss_num, meta.max_miss_den = m->DP.max_miss_den;
            meta.flat_ratio = m->DP.flat_ratio, meta.line_ratio = m->DP.line_ratio, meta.epsilon = m->DP.epsilon;
            E.resize(3 * N), M.resize(6 * N);
            SLAM_TRY(slam_vmap_read_moments(m, E.data(), M.data(), nullptr, cap, &got));
        }
        const std::vector<uint8_t> bytes = vmap_file::build(meta, key.data(), count.data(), sums.data(), seen.data(), miss.data(), E.data(), M.data());
        std::string                why;
        // the writer is held to the reader: a map that slam_vmap_load would refuse (a cell of 2^20 - 1, a wrapped count) is not written
        SLAM_REQUIRE(vmap_file::parse(bytes.data(), bytes.size(), nullptr, &why), SLAM_E_INVALID, "slam_vmap_save: the file format cannot hold this map: %s",
                     why.c_str());
        SLAM_REQUIRE(vmap_file::write_all(path, bytes, &why) == 0, SLAM_E_IO, "slam_vmap_save: %s", why.c_str());
    } catch (const std::bad_alloc &) {
        set_error("slam_vmap_save: out of host memory");
        return SLAM_E_NOMEM;
    }
    return SLAM_OK;
}

int slam_vmap_load(const char *path, slam_vmap_t **out)
{
    SLAM_REQUIRE(path && path[0] && out, SLAM_E_INVALID, "slam_vmap_load: path is NULL or empty, or out is NULL");
    try {
        std::vector<uint8_t> bytes;
        std::string          why;
        vmap_file::View      v;
        SLAM_REQUIRE(vmap_file::read_all(path, &bytes, &why) == 0, SLAM_E_IO, "slam_vmap_load: %s", why.c_str());
        SLAM_REQUIRE(vmap_file::parse(bytes.data(), bytes.size(), &v, &why), SLAM_E_INVALID, "slam_vmap_load: %s: %s", path, why.c_str());
        SLAM_TRY(require_device());
        const vmap_file::Meta &f = v.meta;
        slam_vmap_params       p;
        p.leaf = f.leaf;
        p.initial_capacity = (int)std::min<int64_t>(pow2_at_least(2 * f.n), 1ll << 30); // the absorb does not grow (beyond 2^29 voxels it does, once)
        slam_vmap_t *m = nullptr;
        SLAM_TRY(slam_vmap_create(&p, &m));
        int rc = SLAM_OK;
        if (f.flags & vmap_file::kMoments) {
            slam_vmap_dist_params dp;
            dp.min_points = f.min_points, dp.flat_ratio = f.flat_ratio, dp.line_ratio = f.line_ratio, dp.epsilon = f.epsilon;
            dp.max_miss_num = f.max_miss_num, dp.max_miss_den = f.max_miss_den;
            rc = slam_vmap_enable_distributions(m, &dp);
        }
        if (rc == SLAM_OK && (f.flags & vmap_file::kCarve)) { // also for a file without voxels: a carved map stays one
            rc = ensure_carve_planes(m, nullptr);
            if (rc == SLAM_OK && hipStreamSynchronize(nullptr) != hipSuccess) set_error("slam_vmap_load: clearing the carve planes failed"), rc = SLAM_E_HIP;
        }
        int64_t rejected = 0;
        if (rc == SLAM_OK)
            rc = slam_vmap_absorb(m, reinterpret_cast<const uint64_t *>(v.key), reinterpret_cast<const uint32_t *>(v.count),
                                  reinterpret_cast<const int64_t *>(v.sums), reinterpret_cast<const uint32_t *>(v.seen),
                                  reinterpret_cast<const uint32_t *>(v.miss), reinterpret_cast<const int64_t *>(v.E),
                                  reinterpret_cast<const int64_t *>(v.M), (int)f.n, &rejected);
        if (rc == SLAM_OK && (rejected != 0 || m->n_voxels != f.n || m->n_points != f.n_points)) {
            set_error("slam_vmap_load: %lld records rejected, %lld voxels of %lld, %lld points of %lld", (long long)rejected, (long long)m->n_voxels,
                      (long long)f.n, (long long)m->n_points, (long long)f.n_points);
            rc = SLAM_E_HIP;
        }
        if (rc != SLAM_OK) {
            slam_vmap_destroy(m);
            return rc;
        }
        *out = m;
    } catch (const std::bad_alloc &) {
        set_error("slam_vmap_load: out of host memory");
        return SLAM_E_NOMEM;
    }
    return SLAM_OK;
}

} // extern "C"

// ---------------------------------------------------------------- what vmap_gicp.hip sees of the handle (vmap_dist.hpp)
namespace slam {

int vmap_dist_view(slam_vmap *m, hipStream_t st, VmapDistView *out)
{
    SLAM_REQUIRE(m && m->dist_on, SLAM_E_INVALID, "slam_vmap_register_gicp: distributions were never enabled on this map");
    SLAM_TRY(slam_vmap_compute_distributions(m, reinterpret_cast<slam_stream_t>(st)));
    const Dist D = m->dists();
    out->key = m->view().key, out->mask = (uint64_t)m->capacity - 1;
    out->cen = D.cen, out->nrm = D.nrm, out->cov = D.cov;
    out->leaf = m->P.leaf;
    return SLAM_OK;
}

DevMem &vmap_register_work(slam_vmap *m) { return m->reg_work; }

} // namespace slam
