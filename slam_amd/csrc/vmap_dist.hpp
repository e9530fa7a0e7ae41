// vmap_dist.hpp -- what the voxel map (voxmap.hip) shows of itself to the registration against it (vmap_gicp.hip): the key
// plane of the table, the distribution planes, the cell rule's constants and the hash.  The handle itself stays voxmap.hip's.
#pragma once
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

} // namespace slam
