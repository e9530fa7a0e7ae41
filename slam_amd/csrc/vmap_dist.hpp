// vmap_dist.hpp -- what the voxel map (voxmap.hip) shows of itself to the registration against it (vmap_gicp.hip): the key
// plane of the table, the distribution planes, and the two rules both must follow alike: the cell rule and the hash.  The
// handle itself stays voxmap.hip's.
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
