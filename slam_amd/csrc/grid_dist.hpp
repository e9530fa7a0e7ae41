// grid_dist.hpp -- what grid.hip needs of the distance field (grid_dist.hip) to run it over the grid's own occupancy plane:
// the build is -fno-gpu-rdc, so the kernels stay in grid_dist.hip and slam_grid_distance_field calls these host functions.
#pragma once
#include "common.hpp"

struct slam_gdist;

namespace slam {

void gdist_size(const slam_gdist *h, int *size_x, int *size_y);
// slam_gdist_compute_dev: d_occ is a window-order int8 plane of the handle's size on the device; only enqueues on `st`
int gdist_compute_on(slam_gdist *h, const int8_t *d_occ, hipStream_t st);

} // namespace slam
