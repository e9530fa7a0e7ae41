// vmap_dist.hpp -- what the voxel map (voxmap.hip) shows of itself to the registration against it (vmap_gicp.hip) and to the
// pose search over it (vmap_search.hip): the key plane of the table, the distribution planes, and the rules all must follow
// alike: the f64 move of a point, the cell rule and the hash.  The handle itself stays voxmap.hip's.
#pragma once
#include <cmath>
#include <cstdint>

#include "device_mem.hpp"

namespace slam {

// Read-only view of a map with distributions, valid until the next call that changes the map.
struct VmapDistView {
    const uint64_t *key;  // all ones = empty
    uint64_t        mask; // slots - 1
    const float4   *cen;  // centroid x y z; w = 1.0f for a plane voxel, 0.0f otherwise
    const double   *nrm;  // three doubles per slot
    const double   *cov;  // six doubles per slot: xx xy xz yy yz zz
    double          leaf;
};

// The view of `m` with its distributions brought up to date on `st` (enqueued, not waited for); SLAM_E_INVALID (error text
// set) for a map on which distributions were never enabled.
int vmap_dist_view(slam_vmap *m, hipStream_t st, VmapDistView *out);
// the map's block for a registration's tasks, results and trace
DevMem &vmap_register_work(slam_vmap *m);

constexpr int   kVmapCellLimit = 1 << 20;
constexpr float kVmapCoordLimit = 4194304.0f; // 2^22

// the 64-bit finaliser of MurmurHash3
__host__ __device__ __forceinline__ uint64_t vmap_fmix64(uint64_t k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// The cell rule (docs/VOXEL_MAP.md section 1), the only statement of it in the library.  A point is f32; its cell on an axis
// is floor(v / leaf) in f64, and it has one when |v| < 2^22 and |cell| < 2^20.  The rule has one division and no
// product-and-sum, so contraction cannot change it, on the host or on the device.
__host__ __device__ __forceinline__ bool vmap_axis_cell(float v, double leaf, int *cell)
{
    const double c = floor((double)v / leaf);
    const bool   has = !(!(fabsf(v) < kVmapCoordLimit) || !(fabs(c) < (double)kVmapCellLimit)); // written so that a NaN fails both tests
    // One exit, and the cell written either way.  With an early `return false` the compiler moves the f64 division behind a
    // branch on the first test, and the three divisions of a lane then run one after the other instead of interleaved (the
    // plain integrate measured 4 to 8 % slower so).  That is a compiler's choice, not the language's: what holds it is the
    // comparison of the integrate kernels' instruction streams with their predecessors' (docs/VOXEL_MAP.md section 12.2).
    *cell = has ? (int)c : 0;
    return has;
}
// the cell of q, false when it has none (an axis without a cell reads 0)
__host__ __device__ __forceinline__ bool vmap_point_cell(const float q[3], double leaf, int cell[3])
{
    bool has = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) has = vmap_axis_cell(q[k], leaf, &cell[k]) && has;
    return has;
}
// A cloud's transform as the kernels take it: q = R p + t in f64 (below); `on` = 0 leaves the points as they are.
struct VmapTransform {
    double r[9], t[3];
    int    on;
};

// A point as the map sees it: p (f32 from a cloud, f64 for a carve's origin) moved by X in f64, every product and sum rounded
// on its own, then rounded to f32 (docs/VOXEL_MAP.md section 1).  It stands here, once, for integrate, carve and the pose
// search (vmap_search.hip) alike.  The kernels spell the rounding with the intrinsics; the host's plain operators round the
// same way because the file is compiled without contraction.  X by value and the statements in this order: so the integrate
// kernels compile to their predecessors' instructions (docs/VOXEL_MAP.md section 12.2).
template <class S>
__host__ __device__ __forceinline__ void moved_point(const S *p, const VmapTransform X, float q[3])
{
    q[0] = (float)p[0], q[1] = (float)p[1], q[2] = (float)p[2];
    if (X.on) {
        const double px = p[0], py = p[1], pz = p[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#ifdef __HIP_DEVICE_COMPILE__ // the rounding spelled out: the kernels do not lean on the build's flags
            q[k] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(X.r[3 * k], px), __dmul_rn(X.r[3 * k + 1], py)), __dmul_rn(X.r[3 * k + 2], pz)),
                                    X.t[k]);
#else
            q[k] = (float)((((X.r[3 * k] * px) + (X.r[3 * k + 1] * py)) + (X.r[3 * k + 2] * pz)) + X.t[k]);
#endif
        }
    }
}

// What the pose search (vmap_search.hip, docs/VOXEL_MAP.md section 13) sees of the handle: the key and count planes, the
// distribution plane that carries the plane flag (null unless asked for), and the call's blocks, which the handle owns.
struct VmapSearchView {
    const uint64_t *key;
    const uint32_t *count;
    const float4   *cen; // w = 1.0f for a plane voxel; null when the view was taken without planes
    uint64_t        mask;
    double          leaf;
    int64_t         n_voxels;
};
struct VmapSearchWork {
    DevMem stage;  // the host form's points
    DevMem rot;    // the rotations: 12 doubles each
    DevMem cells;  // three int32 planes of n_yaw n cells
    DevMem brick;  // the occupancy bits
    DevMem volume; // the scores
    DevMem small;  // the box, the points with a cell per rotation, the arg-max partials and the hit list
};
// The view of `m`; with `planes` the distributions are brought up to date on `st` first (enqueued, not waited for), and a map on
// which they were never enabled is SLAM_E_INVALID (error text set).  Nothing of the map is written.
int             vmap_search_view(slam_vmap *m, bool planes, hipStream_t st, VmapSearchView *out);
VmapSearchWork &vmap_search_work(slam_vmap *m);

// a cell's key: 21 bits an axis, x lowest, each field the cell plus 2^20 (1 .. 2^21 - 1)
__host__ __device__ __forceinline__ uint64_t vmap_key_field(int cell, int axis) { return (uint64_t)(cell + kVmapCellLimit) << (21 * axis); }
__host__ __device__ __forceinline__ uint64_t vmap_cell_key(const int cell[3])
{
    return vmap_key_field(cell[0], 0) | vmap_key_field(cell[1], 1) | vmap_key_field(cell[2], 2);
}
// A key's cell.  False for a key that no voxel can have: bit 63 set (the empty word is all ones) or a field of all ones.
__host__ __device__ __forceinline__ bool vmap_key_cell(uint64_t key, int cell[3])
{
    bool valid = !(key >> 63);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t field = (uint32_t)(key >> (21 * k)) & 0x1fffffu;
        valid = valid && field != 0x1fffffu;
        cell[k] = (int)field - kVmapCellLimit;
    }
    return valid;
}

} // namespace slam
