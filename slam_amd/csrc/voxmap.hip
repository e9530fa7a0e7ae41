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
//              One kernel, a template on "with moments" (below), instantiated twice: the host picks.
//   rehash     one lane per old slot: claims the key's slot in the larger table and stores everything the map has -- sums
//              and count, seen and miss of a carved map, the nine moment planes -- in one launch (keys are distinct, so plain
//              stores; planes the map has not are null pointers).  Only ever launched by the host between integrate launches.
//   extract    flag (count, box, and the carved rule where a ratio is given) per slot -> rocprim select of the slot indices
//              -> gather their keys -> rocprim radix sort of (key, slot) -> one lane per voxel writes centroid, count and key.
//              Every host reader is read_columns: one select, one sort, the wanted columns laid out in stage_out by a bump
//              allocator, the families' write kernels, the copies back.
//   carve      free-space evidence for voxels that exist (docs/VOXEL_MAP.md section 8; the restatement is
//              tests/cpp/vmap_carve_oracle.cpp): two u32 planes `seen` and `miss` in units of scans and a u32 `stamp` plane
//              that makes a voxel count once per call, all three allocated at the first carve.  One lane per ray finds the
//              endpoint's voxel (phase 1: seen) and the ray's visited length; a rocprim scan over chunks of 64 steps per ray;
//              one wavefront per chunk, one lane per step, walks the closed form of the driving-axis Bresenham and charges
//              `miss` (phase 2).  No key is written: the lookup only finds.
//   moments    opt-in (docs/VOXEL_MAP.md section 9; the restatement is tests/cpp/vmap_gicp_oracle.cpp): nine i64 planes, the
//              first and second moments of a voxel's points about the cell's corner in units of 2^-16 m.  The integrate
//              instantiation with moments adds them with nine more 64-bit integer atomicAdds; they travel with the voxel
//              through a rehash.  One lane per slot turns them into a centroid, a normal, a regularised plane covariance
//              and a flag (the distribution planes), which vmap_gicp.hip registers against.
//   absorb     (docs/VOXEL_MAP.md section 10) one lane per voxel record (key, count, sums, optionally seen and miss, optionally
//              the nine moments): validate, find or claim as integrate does, integer atomicAdds.  The records are packed
//              arrays (a file, a caller) or another table's planes (merge: one lane per source slot, empty slots leave at
//              once); one body serves both.  Load is this fed from vmap_file.hpp's parser, merge from another handle.
//   coarsen    (docs/VOXEL_MAP.md section 11) one lane per slot of a finer map: the parent cell is the cell shifted right, count
//              and sums add unchanged, the moments are re-centred on the parent's corner in integers; find or claim and
//              integer atomicAdds as absorb.  The result is the bits of a map integrated at the coarser leaf.
// Each rule stands once.  The cell rule (point -> cell -> key -> cell) and the hash are vmap_dist.hpp's, shared with
// vmap_gicp.hip; the f64 move of a point is moved_point, for the kernels and for the host's carve origin alike; the carved
// rule is carve_keeps; "zero the counters, launch, fetch them, wait" is Counters; the host half of absorb, merge and coarsen is
// absorb_with.
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

struct Table {
    uint64_t           *key;
    unsigned long long *sum[3];
    uint32_t           *count;
    uint64_t            mask; // slots - 1
};
// the carve planes (section 8) and the moment planes (section 9): null pointers on a map that has none
struct Planes {
    uint32_t *seen, *miss, *stamp;
};
struct Moments {
    unsigned long long *E[3], *M[6]; // first moments, then xx xy xz yy yz zz
};
using Transform = VmapTransform; // the f64 move of a point and moved_point are vmap_dist.hpp's, shared with vmap_search.hip
struct Box {
    float lo[2], hi[2];
    int   on;
};
// the handle's counters on the device
enum { kClaimed = 0, kDropped = 1, kError = 2, kSelected = 3, kCounters = 4 };
// absorb's block of its own, allocated at the first absorb as carve's is (the handle's block stays four words): the first
// three as above (kDropped counts the rejected records), then the points accepted as one u64
enum { kPoints = 4, kAbsorbCounters = 6 };

// The slot that holds `key`, claimed if nobody had; -1 when `capacity` probes found neither (the error word's case).
__device__ __forceinline__ long long find_or_claim(const Table &T, uint64_t key, uint32_t *claimed)
{
    uint64_t h = vmap_fmix64(key) & T.mask;
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

// kMoments adds the moments about the cell's corner: e = (fx - cell L) >> 4 per axis, |e| <= 2^20 (section 9 has the bound).
// L and Q are read by that instantiation alone.
template <bool kMoments>
__global__ __launch_bounds__(256) void vmap_integrate_kernel(const float *xyz, int n, int stride, Transform X, double leaf, long long L, Table T,
                                                             Moments Q, uint32_t *ctr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; // n may be close to 2^31
    if (i >= (size_t)n) return;
    float q[3];
    int   cell[3];
    moved_point(xyz + i * stride, X, q);
    long long f[3], e[3];
    uint64_t  key = 0;
    bool      keep = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) { // axis by axis, the fixed-point value beside the cell: the order the kernel was measured in
        if (!vmap_axis_cell(q[k], leaf, &cell[k])) {
            keep = false;
            continue;
        }
        key |= vmap_key_field(cell[k], k);
        f[k] = (long long)rint((double)q[k] * kFix);
        e[k] = (f[k] - (long long)cell[k] * L) >> 4; // arithmetic: floor
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
    if (kMoments) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(&Q.E[k][h], (unsigned long long)e[k]);
        atomicAdd(&Q.M[0][h], (unsigned long long)(e[0] * e[0]));
        atomicAdd(&Q.M[1][h], (unsigned long long)(e[0] * e[1]));
        atomicAdd(&Q.M[2][h], (unsigned long long)(e[0] * e[2]));
        atomicAdd(&Q.M[3][h], (unsigned long long)(e[1] * e[1]));
        atomicAdd(&Q.M[4][h], (unsigned long long)(e[1] * e[2]));
        atomicAdd(&Q.M[5][h], (unsigned long long)(e[2] * e[2]));
    }
}

// One lane per old slot: the voxel's slot in the new table, then everything the map has (keys are distinct, so plain
// stores).  Pf and Qf are null pointers on a map without carve planes or moments; the new stamp plane stays zero.
__global__ __launch_bounds__(256) void vmap_rehash_kernel(Table from, Planes Pf, Moments Qf, Table to, Planes Pt, Moments Qt, uint32_t *ctr)
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
    if (Pf.seen) Pt.seen[h] = Pf.seen[i], Pt.miss[h] = Pf.miss[i];
    if (Qf.E[0]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) Qt.E[k][h] = Qf.E[k][i];
#pragma unroll
        for (int k = 0; k < 6; ++k) Qt.M[k][h] = Qf.M[k][i];
    }
}

__device__ __forceinline__ float centroid(unsigned long long s, uint32_t count)
{
    return (float)(((double)(long long)s / (double)count) * (1.0 / kFix));
}

// The carved rule (section 8) for slot i: keep iff miss den <= max(seen, 1) num in u64, equality kept.
__device__ __forceinline__ bool carve_keeps(const Planes &P, uint64_t i, uint32_t num, uint32_t den)
{
    const uint32_t seen = P.seen[i];
    return (uint64_t)P.miss[i] * den <= (uint64_t)(seen > 1u ? seen : 1u) * num;
}

// P is null pointers when no ratio is given or the map was never carved: no carved rule then (a map never carved has
// miss = 0 everywhere, which every ratio keeps).
__global__ __launch_bounds__(256) void vmap_flag_kernel(Table T, Planes P, Box box, uint32_t min_count, uint32_t num, uint32_t den, uint8_t *flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > T.mask) return;
    bool           keep = false;
    const uint32_t c = T.count[i];
    if (T.key[i] != kEmpty && c >= min_count && c > 0) {
        keep = !P.seen || carve_keeps(P, i, num, den);
        if (keep && box.on) {
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
    uint64_t h = vmap_fmix64(key) & T.mask;
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
        float q[3];
        int   c1[3] = {0, 0, 0};
        moved_point(xyz + i * stride, X, q);
        if (!vmap_point_cell(q, leaf, c1)) {
            atomicAdd(&ctr[kcDropped], 1ull);
        } else {
            const long long h = find_slot(T, vmap_cell_key(c1));
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
        int        cell[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cell[k] = carve_cell(A.c0[k], c1[k], i, nn, small);
        const long long h = find_slot(T, vmap_cell_key(cell));
        if (h < 0) continue;
        if (__hip_atomic_load(&P.stamp[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == A.tag + 1u) continue; // an endpoint of this cloud
        if (atomicMax(&P.stamp[h], A.tag) < A.tag) {
            atomicAdd(&P.miss[h], 1u);
            atomicAdd(&ctr[kcMissed], 1ull);
        }
    }
}

// The three write kernels below serve the host readers alone, which take the keys from the sort's output: a null column
// is one the caller did not ask for.
__global__ __launch_bounds__(256) void vmap_write_carve_kernel(Planes P, const uint32_t *slot, int n, uint32_t *seen, uint32_t *miss)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint32_t s = slot[i];
    if (seen) seen[i] = P.seen[s];
    if (miss) miss[i] = P.miss[s];
}

// ---------------------------------------------------------------- moments and distributions (docs/VOXEL_MAP.md section 9)
struct Dist {
    float4 *cen; // centroid; w = 1.0f for a plane voxel
    double *nrm, *cov, *eig;
};
struct DistRule {
    uint32_t min_points, miss_num, miss_den; // miss_den = 0: the carve planes are not asked
    double   flat_ratio, line_ratio, eps;
};

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
        if (plane && R.miss_den > 0 && C.seen) plane = carve_keeps(C, i, R.miss_num, R.miss_den);
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

__global__ __launch_bounds__(256) void vmap_write_moments_kernel(Moments Q, const uint32_t *slot, int n, int64_t *E3, int64_t *M6)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint32_t s = slot[i];
    if (E3)
        for (int k = 0; k < 3; ++k) E3[3 * i + k] = (int64_t)Q.E[k][s];
    if (M6)
        for (int k = 0; k < 6; ++k) M6[6 * i + k] = (int64_t)Q.M[k][s];
}

__global__ __launch_bounds__(256) void vmap_write_dist_kernel(Dist D, const uint32_t *slot, int n, double *nrm3, double *cov6, double *eig3,
                                                              float *cen3, uint8_t *flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint32_t s = slot[i];
    const float4   c = D.cen[s];
    for (int k = 0; k < 3; ++k) {
        if (nrm3) nrm3[3 * i + k] = D.nrm[3 * (size_t)s + k];
        if (eig3) eig3[3 * i + k] = D.eig[3 * (size_t)s + k];
    }
    if (cov6)
        for (int k = 0; k < 6; ++k) cov6[6 * i + k] = D.cov[6 * (size_t)s + k];
    if (cen3) cen3[3 * i] = c.x, cen3[3 * i + 1] = c.y, cen3[3 * i + 2] = c.z;
    if (flag) flag[i] = c.w != 0.0f ? 1 : 0;
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

// The points a lane of absorb or coarsen took in, summed over its wave before the one atomic: every lane of the block calls it.
__device__ __forceinline__ void add_points(uint32_t *ctr, unsigned long long points)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) points += __shfl_xor(points, o);
    if ((threadIdx.x & 63) == 0 && points) atomicAdd(reinterpret_cast<unsigned long long *>(ctr + kPoints), points);
}

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
            int            cell[3];
            if (c == 0u || !vmap_key_cell(key, cell)) {
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
    add_points(ctr, points);
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
            int       cell[3], up[3];
            long long s[3];
            vmap_key_cell(key, cell);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                up[k] = cell[k] >> shift; // arithmetic: floor
                s[k] = (long long)(cell[k] - up[k] * (1 << shift)) * unit;
            }
            const long long h = find_or_claim(T, vmap_cell_key(up), &ctr[kClaimed]);
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
    add_points(ctr, points);
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
    VmapSearchWork        search; // a pose search's blocks (section 13)
    bool                  dist_on = false, dist_stale = true;

    static Moments moments(const DevMem &b, int64_t cap)
    {
        Moments             Q;
        unsigned long long *p = b.as<unsigned long long>();
        for (int k = 0; k < 3; ++k) Q.E[k] = p + (size_t)cap * k;
        for (int k = 0; k < 6; ++k) Q.M[k] = p + (size_t)cap * (3 + k);
        return Q;
    }
    Moments moments() const { return dist_on ? moments(mom, capacity) : Moments{}; } // null pointers without distributions
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
    Planes planes() const // null pointers on a map never carved
    {
        return carved() ? Planes{seen.as<uint32_t>(), miss.as<uint32_t>(), stamp.as<uint32_t>()} : Planes{nullptr, nullptr, nullptr};
    }

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

// One call's use of a block of device counters (words W).  open() names the pinned words they will be fetched into and zeroes
// the block on st; fetch() copies the whole block there and waits for st.  The calls that change the map open before their
// launches, so that nothing runs whose outcome could not be read; select_slots, which changes nothing and whose rocprim call
// writes its word itself, opens without zeroing just before it fetches.  The pinned words are the thread's scratch: they hold
// until the next call that asks for it.
template <class W>
struct Counters {
    const DevMem &dev;
    hipStream_t   st;
    W            *h = nullptr;

    int open(bool zero = true)
    {
        h = static_cast<W *>(pinned_scratch(dev.cap));
        SLAM_REQUIRE(h, SLAM_E_NOMEM, "slam_vmap: no pinned memory for the counters");
        if (zero) SLAM_HIP(hipMemsetAsync(dev.p, 0, dev.cap, st));
        return SLAM_OK;
    }
    int fetch()
    {
        SLAM_HIP(hipMemcpyAsync(h, dev.p, dev.cap, hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipStreamSynchronize(st));
        return SLAM_OK;
    }
    W operator[](int k) const { return h[k]; }
};

// every slot of the table in `b` empty, its sums and counts zero: enqueued on st
int clear_table(const DevMem &b, int64_t cap, hipStream_t st)
{
    SLAM_HIP(hipMemsetAsync(b.p, 0xff, (size_t)cap * 8, st));
    SLAM_HIP(hipMemsetAsync(b.as<uint8_t>() + (size_t)cap * 8, 0, (size_t)cap * (kSlotBytes - 8), st));
    return SLAM_OK;
}

// an empty table of `cap` slots in `b`, enqueued on st
int new_table(DevMem &b, int64_t cap, hipStream_t st)
{
    SLAM_REQUIRE(cap <= kMaxSlots, SLAM_E_NOMEM, "slam_vmap: a table of %lld slots is more than the %lld a map may have", (long long)cap,
                 (long long)kMaxSlots);
    SLAM_TRY(b.alloc((size_t)cap * kSlotBytes));
    return clear_table(b, cap, st);
}

int64_t pow2_at_least(int64_t v)
{
    int64_t c = 64;
    while (c < v) c <<= 1;
    return c;
}

// `bytes` of zeros in `b`, enqueued on st
int new_zeroed(DevMem &b, size_t bytes, hipStream_t st)
{
    SLAM_TRY(b.alloc(bytes));
    SLAM_HIP(hipMemsetAsync(b.p, 0, bytes, st));
    return SLAM_OK;
}

// Room for n more points under the load rule; waits for st when it grows (the old blocks are freed afterwards).  Every new
// block is allocated and cleared first, one launch moves whatever the map has, and only a rehash that placed every voxel
// puts the new blocks into the handle: a failure leaves the old map as it was.
int make_room(slam_vmap *m, int64_t n, hipStream_t st)
{
    if (m->n_voxels + n <= m->capacity / 2) return SLAM_OK;
    const int64_t cap = pow2_at_least(2 * (m->n_voxels + n));
    DevMem        nt, np[3], nm, nd; // the table; seen, miss, stamp; the moments and the distributions
    SLAM_TRY(new_table(nt, cap, st));
    if (m->carved())
        for (DevMem &b : np) SLAM_TRY(new_zeroed(b, (size_t)cap * sizeof(uint32_t), st));
    if (m->dist_on) {
        SLAM_TRY(new_zeroed(nm, (size_t)cap * kMomentBytes, st));
        SLAM_TRY(nd.alloc((size_t)cap * kDistBytes));
    }
    Counters<uint32_t> c{m->ctr, st};
    SLAM_TRY(c.open());
    const Planes  pt = m->carved() ? Planes{np[0].as<uint32_t>(), np[1].as<uint32_t>(), np[2].as<uint32_t>()} : Planes{nullptr, nullptr, nullptr};
    const Moments qt = m->dist_on ? slam_vmap::moments(nm, cap) : Moments{};
    hipLaunchKernelGGL(vmap_rehash_kernel, dim3(blocks_for((uint64_t)m->capacity)), dim3(256), 0, st, m->view(), m->planes(), m->moments(),
                       slam_vmap::view(nt, cap), pt, qt, m->ctr.as<uint32_t>());
    SLAM_HIP(hipGetLastError());
    SLAM_TRY(c.fetch());
    SLAM_REQUIRE(!c[kError] && (int64_t)c[kClaimed] == m->n_voxels, SLAM_E_HIP, "slam_vmap: the rehash moved %u of %lld voxels (error word %u)",
                 c[kClaimed], (long long)m->n_voxels, c[kError]);
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
    SLAM_TRY(new_zeroed(m->seen, plane, st));
    SLAM_TRY(new_zeroed(m->miss, plane, st));
    return new_zeroed(m->stamp, plane, st); // last: carved() is true only when all three stand
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
    uint32_t    *d_n = m->ctr.as<uint32_t>() + kSelected;
    const Planes P = ratio ? m->planes() : Planes{nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(vmap_flag_kernel, dim3(blocks_for(cap)), dim3(256), 0, st, m->view(), P, box, (uint32_t)min_count, ratio ? ratio[0] : 0u,
                       ratio ? ratio[1] : 0u, m->flag.as<uint8_t>());
    SLAM_HIP(hipGetLastError());
    size_t tb = 0;
    SLAM_HIP(rocprim::select(nullptr, tb, rocprim::counting_iterator<uint32_t>(0), m->flag.as<uint8_t>(), m->sel.as<uint32_t>(), d_n, (size_t)cap, st));
    SLAM_TRY(m->tmp.reserve(tb + 16));
    tb = m->tmp.cap;
    SLAM_HIP(rocprim::select(m->tmp.p, tb, rocprim::counting_iterator<uint32_t>(0), m->flag.as<uint8_t>(), m->sel.as<uint32_t>(), d_n, (size_t)cap, st));
    Counters<uint32_t> c{m->ctr, st};
    SLAM_TRY(c.open(false)); // the select wrote its word
    SLAM_TRY(c.fetch());
    *n = (int64_t)c[kSelected];
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
int sort_and_write(slam_vmap *m, int n, float *d_xyz4, uint32_t *d_count, uint64_t *d_key, hipStream_t st)
{
    if (n == 0) return SLAM_OK;
    SLAM_TRY(sort_slots(m, n, st));
    hipLaunchKernelGGL(vmap_write_kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, st, m->view(), m->sel_sorted.as<uint32_t>(),
                       m->keys_out.as<uint64_t>(), n, d_xyz4, d_count, d_key, (int64_t *)nullptr);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int check_extract(const char *who, slam_vmap *m, const float *lo, const float *hi, int min_count, int cap, int *n_out)
{
    SLAM_REQUIRE(m && n_out && cap >= 0 && min_count >= 0 && (lo == nullptr) == (hi == nullptr), SLAM_E_INVALID,
                 "%s: a map, n_out, cap >= 0, min_count >= 0, and lo_xy and hi_xy both or neither", who);
    return SLAM_OK;
}

// What a host reader asks for, one array per column in key order: a null pointer is a column not wanted.
struct Wanted {
    float    *xyz4;
    uint32_t *count;
    uint64_t *key;
    int64_t  *sums;
    uint32_t *seen, *miss; // zeros from a map never carved
    int64_t  *E3, *M6;     // the caller has made sure of the moments,
    float    *cen3;        // and has brought the distributions up to date
    double   *nrm3, *cov6, *eig3;
    uint8_t  *flag;
};
struct Column {
    void    *host;
    size_t   width, align; // bytes a voxel; what the write kernel's stores need
    uint8_t *dev;
    template <class T>
    T *as() const
    {
        return reinterpret_cast<T *>(dev);
    }
};

// Every host reader: check, select, sort, then the wanted columns laid out in stage_out one behind the other, each aligned
// to its type, written by their families' kernels and copied back.  All on the null stream; waits for it.
int read_columns(const char *who, slam_vmap *m, const float *lo, const float *hi, int min_count, const uint32_t *ratio, Wanted w, int cap, int *n_out)
{
    SLAM_TRY(check_extract(who, m, lo, hi, min_count, cap, n_out));
    int64_t n = 0;
    SLAM_TRY(select_slots(m, lo, hi, min_count, nullptr, &n, ratio));
    *n_out = (int)n;
    SLAM_REQUIRE(n <= cap, SLAM_E_NOMEM, "%s: %lld voxels, room for %d", who, (long long)n, cap);
    if (n == 0) return SLAM_OK;
    const size_t N = (size_t)n;
    SLAM_TRY(sort_slots(m, (int)n, nullptr));
    if (!m->carved()) {
        if (w.seen) std::memset(w.seen, 0, N * sizeof(uint32_t));
        if (w.miss) std::memset(w.miss, 0, N * sizeof(uint32_t));
        w.seen = w.miss = nullptr;
    }
    enum { cSums, cE, cM, cNrm, cCov, cEig, cXyz4, cCen, cCount, cSeen, cMiss, cFlag, kColumns };
    Column col[kColumns] = {{w.sums, 24, 8, nullptr}, {w.E3, 24, 8, nullptr},   {w.M6, 48, 8, nullptr},  {w.nrm3, 24, 8, nullptr},
                            {w.cov6, 48, 8, nullptr}, {w.eig3, 24, 8, nullptr}, {w.xyz4, 16, 16, nullptr}, {w.cen3, 12, 4, nullptr},
                            {w.count, 4, 4, nullptr}, {w.seen, 4, 4, nullptr},  {w.miss, 4, 4, nullptr}, {w.flag, 1, 1, nullptr}};
    size_t end = 0, at[kColumns];
    for (int k = 0; k < kColumns; ++k)
        if (col[k].host) {
            at[k] = (end + col[k].align - 1) / col[k].align * col[k].align;
            end = at[k] + N * col[k].width;
        }
    SLAM_TRY(reserve_quarter(m->stage_out, end));
    for (int k = 0; k < kColumns; ++k)
        if (col[k].host) col[k].dev = m->stage_out.as<uint8_t>() + at[k];
    const uint32_t *slot = m->sel_sorted.as<uint32_t>();
    const dim3      grid(blocks_for((uint64_t)n)), block(256);
    if (w.sums || w.xyz4 || w.count)
        hipLaunchKernelGGL(vmap_write_kernel, grid, block, 0, nullptr, m->view(), slot, m->keys_out.as<uint64_t>(), (int)n, col[cXyz4].as<float>(),
                           col[cCount].as<uint32_t>(), (uint64_t *)nullptr, col[cSums].as<int64_t>());
    if (w.seen || w.miss)
        hipLaunchKernelGGL(vmap_write_carve_kernel, grid, block, 0, nullptr, m->planes(), slot, (int)n, col[cSeen].as<uint32_t>(), col[cMiss].as<uint32_t>());
    if (w.E3 || w.M6)
        hipLaunchKernelGGL(vmap_write_moments_kernel, grid, block, 0, nullptr, m->moments(), slot, (int)n, col[cE].as<int64_t>(), col[cM].as<int64_t>());
    if (w.cen3 || w.nrm3 || w.cov6 || w.eig3 || w.flag)
        hipLaunchKernelGGL(vmap_write_dist_kernel, grid, block, 0, nullptr, m->dists(), slot, (int)n, col[cNrm].as<double>(), col[cCov].as<double>(),
                           col[cEig].as<double>(), col[cCen].as<float>(), col[cFlag].as<uint8_t>());
    SLAM_HIP(hipGetLastError());
    for (const Column &c : col)
        if (c.host) SLAM_HIP(hipMemcpy(c.host, c.dev, N * c.width, hipMemcpyDeviceToHost));
    if (w.key) SLAM_HIP(hipMemcpy(w.key, m->keys_out.p, N * sizeof(uint64_t), hipMemcpyDeviceToHost)); // as the sort left them
    SLAM_HIP(hipStreamSynchronize(nullptr));
    return SLAM_OK;
}

Transform make_transform(const double *R, const double *t)
{
    Transform X{};
    X.on = R != nullptr;
    if (R) {
        for (int k = 0; k < 9; ++k) X.r[k] = R[k];
        for (int k = 0; k < 3; ++k) X.t[k] = t[k];
    }
    return X;
}

// a host cloud into stage_in (nothing for n = 0): synchronous
int stage_cloud(slam_vmap *m, const float *xyz, int n, int stride)
{
    const size_t bytes = (size_t)n * stride * sizeof(float);
    if (!bytes) return SLAM_OK;
    SLAM_TRY(reserve_quarter(m->stage_in, bytes));
    SLAM_HIP(hipMemcpy(m->stage_in.p, xyz, bytes, hipMemcpyHostToDevice));
    return SLAM_OK;
}

// The host half of absorb, merge and coarsen: room in m for `n_new` more voxels, the carve planes when the records bring seen
// and miss (after the growth: at the table's size), absorb's counter block, the launch -- the one thing that differs, so
// `launch(ctr)` is the caller's -- and the handle's counts.  Waits once for st.  `lost` names what a full table would lose.
template <class Launch>
int absorb_with(const char *who, const char *lost, slam_vmap *m, bool with_carve, int64_t n_new, int64_t *n_rejected, hipStream_t st,
                Launch launch)
{
    SLAM_TRY(make_room(m, n_new, st));
    if (with_carve) SLAM_TRY(ensure_carve_planes(m, st));
    if (!m->actr.p) SLAM_TRY(m->actr.alloc(kAbsorbCounters * sizeof(uint32_t)));
    Counters<uint32_t> c{m->actr, st};
    SLAM_TRY(c.open());
    launch(m->actr.as<uint32_t>());
    SLAM_HIP(hipGetLastError());
    m->dist_stale = true;
    SLAM_TRY(c.fetch());
    m->n_voxels += c[kClaimed];
    m->n_points += (int64_t)((uint64_t)c[kPoints] | (uint64_t)c[kPoints + 1] << 32);
    if (n_rejected) *n_rejected = (int64_t)c[kDropped];
    SLAM_REQUIRE(!c[kError], SLAM_E_HIP, "%s: a probe ran through all %lld slots (%lld voxels): %s were lost", who, (long long)m->capacity,
                 (long long)m->n_voxels, lost);
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
    SLAM_TRY(clear_table(m->table, m->capacity, st));
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
    Counters<uint32_t> c{m->ctr, st};
    SLAM_TRY(c.open());
    const auto kernel = m->dist_on ? vmap_integrate_kernel<true> : vmap_integrate_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks_for((uint64_t)n)), dim3(256), 0, st, d_xyz, n, stride, make_transform(R, t), m->P.leaf,
                       (long long)std::rint(m->P.leaf * kFix), m->view(), m->moments(), m->ctr.as<uint32_t>());
    if (m->dist_on) m->dist_stale = true;
    SLAM_HIP(hipGetLastError());
    SLAM_TRY(c.fetch());
    m->n_voxels += c[kClaimed];
    m->n_points += (int64_t)n - c[kDropped];
    if (n_dropped) *n_dropped = (int)c[kDropped];
    SLAM_REQUIRE(!c[kError], SLAM_E_HIP, "slam_vmap_integrate: a probe ran through all %lld slots (%lld voxels): points were lost",
                 (long long)m->capacity, (long long)m->n_voxels);
    return SLAM_OK;
}

int slam_vmap_integrate(slam_vmap_t *m, const float *xyz, int n, int stride, const double R[9], const double t[3], int *n_dropped)
{
    SLAM_REQUIRE(m && n >= 0 && stride >= 3 && (xyz || n == 0) && (R == nullptr) == (t == nullptr), SLAM_E_INVALID,
                 "slam_vmap_integrate: a map, n >= 0, stride >= 3, points, and R and t both or neither");
    if (n_dropped) *n_dropped = 0;
    if (n == 0) return SLAM_OK;
    SLAM_TRY(stage_cloud(m, xyz, n, stride));
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

int slam_vmap_read(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, float *xyz4, uint32_t *count, uint64_t *key,
                   int cap, int *n_out)
{
    Wanted w{};
    w.xyz4 = xyz4, w.count = count, w.key = key;
    return read_columns("slam_vmap_read", m, lo_xy, hi_xy, min_count, nullptr, w, cap, n_out);
}

int slam_vmap_read_sums(slam_vmap_t *m, int64_t *sums, uint32_t *count, uint64_t *key, int cap, int *n_out)
{
    Wanted w{};
    w.sums = sums, w.count = count, w.key = key;
    return read_columns("slam_vmap_read_sums", m, nullptr, nullptr, 0, nullptr, w, cap, n_out);
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
                        m->offs.cap + m->mom.cap + m->dist.cap + m->reg_work.cap + m->actr.cap + m->search.stage.cap + m->search.rot.cap +
                        m->search.cells.cap + m->search.brick.cap + m->search.volume.cap + m->search.small.cap;
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
    const Transform X = make_transform(R, t);
    // the origin (f64, not rounded before it is moved) and its cell, with a point's arithmetic: decided before any launch
    Carve        A{};
    const double o[3] = {origin ? origin[0] : 0.0, origin ? origin[1] : 0.0, origin ? origin[2] : 0.0};
    float        O[3];
    moved_point(o, X, O);
    for (int k = 0; k < 3; ++k)
        SLAM_REQUIRE(vmap_axis_cell(O[k], m->P.leaf, &A.c0[k]), SLAM_E_INVALID, "slam_vmap_carve: the origin has no cell (axis %d: %g)", k, (double)O[k]);
    A.end_margin = p.end_margin, A.tail_num = p.tail_num, A.tail_den = p.tail_den, A.max_ray_cells = p.max_ray_cells;
    if (n == 0) return SLAM_OK;
    // chunks travel as u32 through the scan: a ray has at most 2^21 cells
    const int64_t longest = p.max_ray_cells < 2 * kVmapCellLimit ? p.max_ray_cells : 2 * kVmapCellLimit;
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

    unsigned long long          *d_ctr = m->cctr.as<unsigned long long>();
    Counters<unsigned long long> c{m->cctr, st};
    SLAM_TRY(c.open());
    hipLaunchKernelGGL(vmap_carve_rays_kernel, dim3(blocks_for((uint64_t)n + 1)), dim3(256), 0, st, d_xyz, n, stride, X, m->P.leaf, m->view(),
                       m->planes(), A, m->rays.as<int4>(), m->chunks.as<uint32_t>(), d_ctr);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(rocprim::exclusive_scan(m->tmp.p, tb, m->chunks.as<uint32_t>(), m->offs.as<uint32_t>(), 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), st));
    // one wave per chunk, four to a block; beyond 2048 blocks the waves stride over the chunks
    const int64_t blocks = (max_chunks + 3) / 4;
    hipLaunchKernelGGL(vmap_carve_walk_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, m->rays.as<int4>(),
                       m->offs.as<uint32_t>(), n, (uint32_t)max_chunks, m->view(), m->planes(), A, d_ctr);
    SLAM_HIP(hipGetLastError());
    SLAM_TRY(c.fetch());
    if (result) {
        result->n_dropped = (int64_t)c[kcDropped];
        result->n_rays = (int64_t)n - result->n_dropped;
        result->n_skipped = (int64_t)c[kcSkipped];
        result->n_steps = (int64_t)c[kcSteps];
        result->n_seen = (int64_t)c[kcSeen];
        result->n_missed = (int64_t)c[kcMissed];
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
    SLAM_TRY(stage_cloud(m, xyz, n, stride));
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
    Wanted         w{};
    w.xyz4 = xyz4, w.count = count, w.key = key;
    return read_columns("slam_vmap_read_carved", m, lo_xy, hi_xy, min_count, ratio, w, cap, n_out);
}

int slam_vmap_read_carve(slam_vmap_t *m, uint32_t *seen, uint32_t *miss, uint64_t *key, int cap, int *n_out)
{
    SLAM_REQUIRE(n_out && cap >= 0, SLAM_E_INVALID, "slam_vmap_read_carve: n_out and cap >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m, SLAM_E_INVALID, "slam_vmap_read_carve: map is NULL");
    Wanted w{};
    w.seen = seen, w.miss = miss, w.key = key;
    return read_columns("slam_vmap_read_carve", m, nullptr, nullptr, 0, nullptr, w, cap, n_out);
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
    hipLaunchKernelGGL(vmap_distributions_kernel, dim3(blocks_for((uint64_t)m->capacity)), dim3(256), 0, as_stream(stream), m->view(), m->moments(),
                       m->planes(), R, m->dists());
    SLAM_HIP(hipGetLastError());
    m->dist_stale = false;
    return SLAM_OK;
}

int slam_vmap_read_moments(slam_vmap_t *m, int64_t *E3, int64_t *M6, uint64_t *key, int cap, int *n_out)
{
    SLAM_REQUIRE(n_out && cap >= 0, SLAM_E_INVALID, "slam_vmap_read_moments: n_out and cap >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m && m->dist_on, SLAM_E_INVALID, "slam_vmap_read_moments: a map with distributions enabled");
    Wanted w{};
    w.E3 = E3, w.M6 = M6, w.key = key;
    return read_columns("slam_vmap_read_moments", m, nullptr, nullptr, 0, nullptr, w, cap, n_out);
}

int slam_vmap_read_distributions(slam_vmap_t *m, float *centroid3, double *normal3, double *cov6, double *eig3, uint8_t *flag, uint64_t *key, int cap,
                                 int *n_out)
{
    SLAM_REQUIRE(n_out && cap >= 0, SLAM_E_INVALID, "slam_vmap_read_distributions: n_out and cap >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m && m->dist_on, SLAM_E_INVALID, "slam_vmap_read_distributions: a map with distributions enabled");
    SLAM_TRY(slam_vmap_compute_distributions(m, nullptr));
    Wanted w{};
    w.cen3 = centroid3, w.nrm3 = normal3, w.cov6 = cov6, w.eig3 = eig3, w.flag = flag, w.key = key;
    return read_columns("slam_vmap_read_distributions", m, nullptr, nullptr, 0, nullptr, w, cap, n_out);
}


// ---------------------------------------------------------------- absorb, merge, save, load (docs/VOXEL_MAP.md section 10)
// `lanes` records (or source slots) of S into m, with room made for `n_new` more voxels first
static int absorb_records(slam_vmap *m, Records S, uint64_t lanes, int64_t n_new, int64_t *n_rejected, hipStream_t st)
{
    return absorb_with("slam_vmap_absorb", "records", m, S.seen != nullptr, n_new, n_rejected, st, [&](uint32_t *ctr) {
        hipLaunchKernelGGL(vmap_absorb_kernel, dim3(blocks_for(lanes)), dim3(256), 0, st, S, lanes, m->view(), m->planes(), m->moments(), ctr);
    });
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
    const long long unit = src->dist_on ? (long long)fine : 0; // L / 16: L = leaf 2^20 exactly here
    return absorb_with("slam_vmap_coarsen", "voxels", dst, false, src->n_voxels, nullptr, st, [&](uint32_t *ctr) {
        hipLaunchKernelGGL(vmap_coarsen_kernel, dim3(blocks_for((uint64_t)src->capacity)), dim3(256), 0, st, src->view(), src->moments(), shift, unit,
                           dst->view(), dst->moments(), ctr);
    });
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
        Wanted w{};
        w.sums = sums.data(), w.count = count.data(), w.key = key.data();
        if (m->carved()) {
            meta.flags |= vmap_file::kCarve;
            seen.resize(N), miss.resize(N);
            w.seen = seen.data(), w.miss = miss.data();
        }
        if (m->dist_on) {
            meta.flags |= vmap_file::kMoments;
            meta.min_points = m->DP.min_points, meta.max_miss_num = m->DP.max_miss_num, meta.max_miss_den = m->DP.max_miss_den;
            meta.flat_ratio = m->DP.flat_ratio, meta.line_ratio = m->DP.line_ratio, meta.epsilon = m->DP.epsilon;
            E.resize(3 * N), M.resize(6 * N);
            w.E3 = E.data(), w.M6 = M.data();
        }
        // every column with one select and one sort; a refusal reads as it did when the first of three reads was read_sums
        SLAM_TRY(read_columns("slam_vmap_read_sums", m, nullptr, nullptr, 0, nullptr, w, cap, &got));
        SLAM_REQUIRE(got == cap, SLAM_E_HIP, "slam_vmap_save: the table holds %d voxels, the handle counts %d", got, cap);
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

int vmap_search_view(slam_vmap *m, bool planes, hipStream_t st, VmapSearchView *out)
{
    SLAM_REQUIRE(!planes || m->dist_on, SLAM_E_INVALID, "slam_vmap_search: planes_only on a map on which distributions were never enabled");
    if (planes) SLAM_TRY(slam_vmap_compute_distributions(m, reinterpret_cast<slam_stream_t>(st)));
    const Table T = m->view();
    out->key = T.key, out->count = T.count, out->mask = T.mask;
    out->cen = planes ? m->dists().cen : nullptr;
    out->leaf = m->P.leaf, out->n_voxels = m->n_voxels;
    return SLAM_OK;
}

VmapSearchWork &vmap_search_work(slam_vmap *m) { return m->search; }

} // namespace slam
