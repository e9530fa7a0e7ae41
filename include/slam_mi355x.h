/*
 * slam_mi355x.h -- C-ABI of the MI355X (gfx950) implementation of the
 * servos/SLAM per-scan hot path: the ccicp2d class-constrained 2-D ICP scan
 * matcher and the mls/local_mapper occupancy-grid update.
 *
 * This is the drop-in boundary.  The reference has no
 * FFI layer: its hot path sits behind two C++ classes, so each entry point
 * below names the reference member it stands for (file:line under the
 * reference checkout).  INTEGRATION.md shows the adapter a maintainer adds to
 * ccicp2d/mls to call it; the headers in include/slam_amd/ are those adapters.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or framework types cross the ABI;
 *   - every function returns SLAM_OK (0) or a negative SLAM_E_* code and never
 *     throws; slam_last_error() gives the text of the calling thread's last
 *     failure;
 *   - "host" entry points take host memory and return when the result is in
 *     the caller's buffers (reference semantics: fit() is synchronous);
 *   - "_dev" entry points take DEVICE pointers, enqueue on `stream` and return
 *     without synchronising; inputs are borrowed until the stream reaches
 *     that point;
 *   - handles are opaque and not thread-safe (the reference is single-threaded:
 *     matrix.cpp:26-31 statics, node globals); use one handle per host thread.
 *   - there is no CPU fallback: without a usable HIP device every compute
 *     entry point fails with SLAM_E_NO_DEVICE.
 */
#ifndef SLAM_MI355X_H
#define SLAM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_OK                       0
#define SLAM_E_INVALID               -1 /* bad argument */
#define SLAM_E_NO_DEVICE             -2 /* no HIP device / runtime not usable */
#define SLAM_E_HIP                   -3 /* a HIP call failed, see slam_last_error() */
#define SLAM_E_TOO_FEW_MODEL_POINTS  -4 /* icp.cpp:38-43: fewer than 5 model points */
#define SLAM_E_TOO_FEW_SCENE_POINTS  -5 /* icp.cpp:100-103, icpTools.cpp:179-184 */
#define SLAM_E_NOMEM                 -6
#define SLAM_E_UNSUPPORTED           -7
#define SLAM_E_TIMEOUT               -8 /* slam_mi355x_rccl.h: a merge's united range did not arrive: another rank has stopped */
#define SLAM_E_COMM                  -9 /* slam_mi355x_rccl.h: the communicator (or the host transport) reports a failure */
#define SLAM_E_IO                    -10 /* a file could not be opened, read or written: slam_last_error() has the system's message */

typedef void *slam_stream_t; /* a hipStream_t; NULL = the default stream */
typedef void *slam_event_t;  /* a hipEvent_t */

const char *slam_last_error(void);
const char *slam_version(void);

/* ------------------------------------------------------------ device plumbing */
int slam_device_count(int *n);
int slam_set_device(int ordinal);
int slam_device_info(char *name, int name_len, int *compute_units, size_t *hbm_bytes);
int slam_malloc(void **dptr, size_t bytes);
int slam_free(void *dptr);
int slam_memset(void *dptr, int value, size_t bytes, slam_stream_t stream);
int slam_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, slam_stream_t stream);
int slam_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, slam_stream_t stream);
int slam_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, slam_stream_t stream); /* asynchronous */
/* pinned host memory and copies that only enqueue (for overlapping transfers with kernels on
 * other streams; the host buffer must stay valid until the stream reaches the copy) */
int slam_host_alloc(void **hptr, size_t bytes);
/* 1 when hptr points into pinned host memory (slam_host_alloc, hipHostMalloc, hipHostRegister) -- memory an _async copy really
 * is asynchronous from --, 0 otherwise (pageable memory: the runtime stages such a copy and the call waits) */
int slam_host_is_pinned(const void *hptr);
int slam_host_free(void *hptr);
int slam_memcpy_h2d_async(void *dst_dev, const void *src_pinned, size_t bytes, slam_stream_t stream);
int slam_memcpy_d2h_async(void *dst_pinned, const void *src_dev, size_t bytes, slam_stream_t stream);
int slam_stream_wait_event(slam_stream_t stream, slam_event_t ev);
int slam_stream_create(slam_stream_t *stream);
/* priority > 0: the device's highest stream priority, < 0: its lowest, 0: the middle.  When workgroups of several
 * streams wait for CUs, those of the higher priority are placed first. */
int slam_stream_create_with_priority(slam_stream_t *stream, int priority);
/* A stream whose kernels leave `reserve_per_xcd` CUs of every XCD alone (hipExtStreamCreateWithCUMask): for work that
 * would otherwise hold every CU for its whole duration -- the registration batches, 0.6 ms per workgroup -- while short
 * kernels of other streams (an RCCL all-reduce, the grid update) wait for a CU to come free.  A stream made here has a hardware
 * queue of its own (the runtime deals ordinary streams over a few shared queues, where one stream's launches can stand behind
 * another's: DESIGN.md 4.6).  With reserve_per_xcd = 0 the mask names every CU.  Two differences from slam_stream_create remain,
 * both measured (tools/exp/stream_flags.hip, round 5): the stream has a hardware queue of its own, and it is a BLOCKING stream
 * (hipExtStreamCreateWithCUMask makes hipStreamDefault streams: hipStreamGetFlags = 0) -- a kernel on it waits for whatever the
 * process has put on the legacy null stream (a synchronous hipMemcpy, a framework's default stream) and the null stream waits for
 * it, where every other stream of this library is hipStreamNonBlocking.  The library itself enqueues nothing on the null stream in
 * its asynchronous calls; a caller that does serialises with these streams.  reserve_per_xcd > 0 needs the CU numbering this was
 * measured on -- an unpartitioned gfx950 of 256 CUs -- and returns SLAM_E_UNSUPPORTED elsewhere. */
int slam_stream_create_reserving_cus(slam_stream_t *stream, int reserve_per_xcd);
int slam_stream_destroy(slam_stream_t stream);
int slam_stream_synchronize(slam_stream_t stream);
int slam_device_synchronize(void);
/* hipGraph capture of a sequence of this library's asynchronous calls on one (created) stream: record once
 * after a warm-up call of the same sequence, replay with one launch. */
typedef void *slam_graph_t;
int slam_graph_begin_capture(slam_stream_t stream);
int slam_graph_end_capture(slam_stream_t stream, slam_graph_t *out);
int slam_graph_launch(slam_graph_t graph, slam_stream_t stream);
int slam_graph_destroy(slam_graph_t graph);
int slam_event_create(slam_event_t *ev);
int slam_event_destroy(slam_event_t ev);
int slam_event_record(slam_event_t ev, slam_stream_t stream);
int slam_event_synchronize(slam_event_t ev);
int slam_event_query(slam_event_t ev, int *done);   /* hipEventQuery without blocking: *done = 1 when everything recorded before the event has finished (or it was never recorded) */
int slam_event_elapsed_ms(slam_event_t start, slam_event_t stop, float *ms);

/* ------------------------------------------------------------------- ICP
 * Stands for class IcpPointToPoint : Icp (icpPointToPoint.h:26-40, icp.h:33-102). */
typedef struct slam_icp slam_icp_t;

#define SLAM_ICP_P2P 0 /* IcpPointToPoint::fitStep, icpPointToPoint.cpp:33-172 (what the reference runs) */
#define SLAM_ICP_P2L 1 /* point-to-line 3x3 normal equations, icpPointToPlane.cpp:37-107 (not compiled upstream) */

typedef struct {
    int    max_iter;        /* icp.cpp:27 max_iter(20); icp.h:51 setMaxIterations */
    double min_delta;       /* icp.cpp:27 min_delta(1e-6); icp.h:54 setMinDeltaParam */
    int    mode;            /* SLAM_ICP_P2P | SLAM_ICP_P2L */
    int    normals_k;       /* P2L: neighbours per normal (icpPointToPlane.h: 10) */
    int    lanes_per_point; /* 0 = library default: the ring search (2 lanes per scan point) for
                               the first iterations of a scan, then the halo-list sweeps (one lane
                               per point), both in one launch; N = 1,2,4,8,16,32,64:
                               ring search only, N lanes per point; -1 = ring search, lanes chosen
                               per pass; -2 = list sweeps for every iteration (measurements) */
    double cell_size;       /* model lattice pitch in metres; 0 = sized to fit LDS */
    int    force_global;    /* 1 = keep the model index in HBM/L2 even if it fits LDS */
    int    build_on_host;   /* 1 = build the model index with the single-threaded host code instead of the
                               device kernels (the reference the device build is verified against: same bytes) */
    int    first_iterations;/* default schedule: ring-search iterations before a scan may change to list sweeps
                               (0 = library default: 10 point-to-point, 2 point-to-line) */
    int    far_div;         /* default schedule: hand over once at most n / far_div queries are beyond the lists'
                               certified radius (0 = library default, 32) */
    int    split_launch;    /* 1 = the two search forms as two launches instead of one (same results) */
    int    spread_scans;    /* batches of at most this many scans (one, in the reference's usage) run in the
                               spread form: every scan over many workgroups of one persistent launch, 64 lanes
                               per query (icp_single.hip); 0 = library default (CUs / 16), -1 = never */
    int    pair_scans;      /* default schedule, batches: two scans per workgroup sharing one LDS index, each on half the
                               wavefronts (icp_fit_pair_kernel): 1 = one lane per scan point in the ring search,
                               2 = two lanes, 0 = library default (two lanes, for batches of at least two scans per
                               CU), -1 = never (one scan per workgroup) */
    int    spread_wait_us;  /* spread form: how long a scan's workgroups wait at their FIRST exchange for one another to
                               become resident before the scan is handed to the one-workgroup form instead (another
                               spread launch, another process or a persistent kernel may hold the CUs they need; a fit
                               never fails for it, icp.cpp:80-114); 0 = library default (5000), < 0 = hand over at once */
    int    wave_tiles;      /* a model whose index does not fit LDS (the reference's cap is 2 x 19 999 points, icpTools.h:21):
                               1 = every wavefront stages the model TILE of its two passes -- the union of its queries' 3 x 3 cell
                               blocks, one contiguous span per lattice row -- into its own 9 KB of the otherwise empty LDS, keeps it
                               over the iterations and searches there; 0 = library default: every query through L2.  Measured in
                               round 5: the tiles halve the kernel's L2 traffic and make it 20-30 % SLOWER -- the
                               kernel is bound by instruction issue, not by its loads -- so the default is off; the tiled form is
                               kept for models sparse enough to stage once (tests/test_gpu_icp_tile.py pins its results) */
    double list_min_halo;   /* halo lists: the lattice built is the first -- finest -- candidate whose lists fit LDS;
                               with this set, the first whose HALO is at least this many metres, if one fits (any, otherwise).  A
                               list answers a query whose neighbour is nearer than its halo; the others go to the cooperative
                               round.  0 = library default, < 0 = no preference (the finest that fits) */
    int    spread_tile;     /* spread form (one cloud at a time against up to 2 x 19 999 points: scan_registration.cpp:139-159,
                               icpTools.h:21): every workgroup keeps its scene points and their search state -- last neighbour, radius
                               proved empty -- in LDS for the whole fit and searches from last iteration's neighbour in straight-line
                               code (icp_single.hip).  For a model that does not fit LDS the workgroups take scene points
                               that are neighbours in space and either (1) stage the TILE of the index they can reach into LDS -- for
                               cells of more than 64 points, a lidar cloud's walls: config 3 0.45 -> 0.22 ms per fit -- or (2) search the
                               index where it lies.  Same correspondences; the sums in another order.  0 = library default (by the
                               model), 1 / 2 = that form wherever the index is not in LDS, -1 = the round-5 form */
} slam_icp_params;

typedef struct {
    int    iters;  /* fitStep calls executed (icp.cpp:116-122) */
    int    n_corr; /* Icp::getNumberCorrespondences of the last step */
    double delta;  /* last fitStep return value; -1 = no correspondences */
} slam_icp_result;

void slam_icp_default_params(slam_icp_params *p);

/* Icp::Icp(M_GA, M_NGA, M_GA_num, M_NGA_num, dim=2), icp.cpp:26-70.  The host
 * arrays (xy, f64) are copied (stored as f32, icp.cpp:51-60) and a uniform-cell
 * index replaces the two kd-trees; the exact-1-NN-in-float contract is kept. */
int  slam_icp_create(const double *m_ga, int n_ga, const double *m_nga, int n_nga,
                     const slam_icp_params *params, slam_icp_t **out);
/* The same with the model arrays resident in HBM (a target built from registered scans: the sliding local
 * map of a streaming mapper).  Builds on a stream of the library's own and returns with the index complete; the
 * arrays must be complete when the call is made (it does not order itself behind any stream of the caller). */
int  slam_icp_create_dev(const double *d_m_ga, int n_ga, const double *d_m_nga, int n_nga,
                         const slam_icp_params *params, slam_icp_t **out);
void slam_icp_destroy(slam_icp_t *icp);
int  slam_icp_set_max_iterations(slam_icp_t *icp, int val);  /* icp.h:51 */
int  slam_icp_set_min_delta(slam_icp_t *icp, double val);    /* icp.h:54 */
int  slam_icp_set_subsampling_step(slam_icp_t *icp, int val);/* icp.h:48 (stored, unused there too) */

/* Icp::fit(T_GA, T_NGA, T_GA_num, T_NGA_num, R, t, indist, h_dist), icp.cpp:80-114.
 * R (2x2 row-major) and t are in/out; host pointers; synchronous.  Returns
 * SLAM_E_TOO_FEW_SCENE_POINTS (R,t untouched) where the reference logs and
 * returns early. */
int slam_icp_fit(slam_icp_t *icp, const double *t_ga, int n_tga, const double *t_nga,
                 int n_tnga, double R[4], double t[2], double indist,
                 slam_icp_result *result);

/* The same over a batch of independent scans, all operands resident in HBM.
 *   d_pts      xy f64 of all scans, scan s = points [d_scan_off[s], d_scan_off[s+1])
 *   d_scan_nga number of class-GA points at the front of scan s (the rest is NGA)
 *   d_R, d_t   n_scans x 4 / x 2 doubles, in/out (initial -> registered pose)
 *   d_result   n_scans slam_icp_result (nullable)
 *   d_trace    nullable; n_scans x max_iter x 8 doubles: R00 R01 R10 R11 t0 t1
 *              delta n_corr after each executed step
 * Scans with fewer than 5 points are left untouched (iters = 0).
 * Asynchronous on `stream`.  Batches in the workgroup-per-scan forms (more than CUs / 16 scans, or spread_scans = -1)
 * keep nothing in the handle: calls on ONE handle may be in flight on several streams at once, and that is how a
 * stream of batches should be run -- two registration streams with pair_scans = 2, the grid update on a third
 * (DESIGN.md 4.6).  The spread form (few scans) uses scratch of the handle: one such call at a time per handle; calls
 * on DIFFERENT handles and streams are fine -- the library runs a process's spread launches one after the other on the
 * device, and a scan whose workgroups cannot become resident together (another process's launch, a persistent kernel
 * on the CUs) is redone by the workgroup-per-scan form inside the same call: every scan comes back registered. */
int slam_icp_fit_batch_dev(slam_icp_t *icp, const double *d_pts, const int32_t *d_scan_off,
                           const int32_t *d_scan_nga, int n_scans, double *d_R, double *d_t,
                           double indist, slam_icp_result *d_result, double *d_trace,
                           slam_stream_t stream);
/* The same with the initial poses read from d_R0 / d_t0 and the registered poses written to d_R / d_t (the two may
 * be the same arrays: that is slam_icp_fit_batch_dev).  Icp::fit takes R, t in/out because its caller keeps one pose
 * (icp.cpp:80-114); a stream of batches whose initial poses come from elsewhere (an odometry buffer, the batch before)
 * saves the copy into the output arrays and the launch gap behind it.  A scan with fewer than 5 points gets its
 * initial pose. */
int slam_icp_fit_batch_from_dev(slam_icp_t *icp, const double *d_pts, const int32_t *d_scan_off,
                                const int32_t *d_scan_nga, int n_scans, const double *d_R0, const double *d_t0,
                                double *d_R, double *d_t, double indist, slam_icp_result *d_result,
                                double *d_trace, slam_stream_t stream);

/* KDTree::n_nearest(qv, 1, result), kdtree.cpp:378-391, for n float queries
 * against one class (0 = GA, 1 = NGA): squared float distance and ORIGINAL
 * model index (kdtree.h:31-35).  Device pointers. */
int slam_icp_nearest_dev(slam_icp_t *icp, int cls, const float *d_query_xy, int n,
                         float *d_dis, int32_t *d_idx, slam_stream_t stream);

/* IcpPointToPoint::getEdgeWeight(eW), icpPointToPoint.cpp:233-316, for the
 * correspondences of the last slam_icp_fit() call. */
int slam_icp_get_edge_weight(slam_icp_t *icp, double eW[9]);

/* IcpPointToPlane::computeNormals, icpPointToPlane.cpp:340-349 (SLAM_ICP_P2L only): the unit
 * normal of every model point, GA points first then NGA, 2 doubles each. */
int slam_icp_get_normals(slam_icp_t *icp, double *normals_xy);

/* what the index looks like (for DESIGN.md / bench reporting) */
int slam_icp_index_info(slam_icp_t *icp, int *nx, int *ny, double *cell, int *in_lds,
                        size_t *lds_bytes, int *lanes_per_point);
/* How the index was built: on_device = 1 for the device kernels; ms[0] = host wall time of enqueueing the
 * build (upload, extent, plan, cell index, lists: about twenty launches), ms[1] = its one wait, for the plan the
 * device worked out (lattice, blob layout, the list lattice that fits); ms[2..3] = 0. */
int slam_icp_build_info(slam_icp_t *icp, int *on_device, double ms[4]);
/* The index as it lies in HBM: which = 0 the cell index, 1 the halo lists (0 bytes when the model has
 * none).  bytes (optional) receives the size; buf (optional, cap bytes) the content.  Synchronous. */
int slam_icp_index_blob(slam_icp_t *icp, int which, void *buf, size_t cap, size_t *bytes);
/* The model as the index holds it: the points of class cls (0 GA, 1 NGA) as f32 xy in their ORIGINAL order within the
 * class -- the cell sort undone with the index's own original-index array -- into xy (room for cap points; null with
 * cap = 0 to ask for the count).  *n receives the class's count; with cap < *n nothing is written and the call returns
 * SLAM_E_NOMEM.  A point-to-line handle has one class (1: GA then NGA); its class 0 answers 0 points.  Copies the index to
 * the host and scatters there: no kernel.  Waits for the whole device.  An index entry that names no point of its class
 * (it cannot happen in a sound index) is SLAM_E_HIP. */
int slam_icp_read_model(slam_icp_t *icp, int cls, float *xy, int cap, int *n);
/* The default point-to-point schedule: two_forms = 1 when the halo lists fit LDS for this model (the ring
 * search then runs at least the first `first_iterations` iterations of a scan and the list sweeps the rest, in
 * one launch: the workgroup swaps its LDS contents); list lattice pitch, halo and certified radius in metres,
 * size of the list blob. */
int slam_icp_list_info(slam_icp_t *icp, int *two_forms, int *first_iterations, double *pitch, double *halo,
                       double *certified_radius, size_t *list_bytes);

/* ------------------------------------------------------------------ grid
 * Stands for class MLS in rolling/occupancy mode (mls.h:104-242) as
 * local_mapper uses it (local_mapper.cpp:29,86,107). */
typedef struct slam_grid slam_grid_t;

#define SLAM_RAYCAST_TILED  0 /* LDS-binned tiles, coalesced write-back */
#define SLAM_RAYCAST_GLOBAL 1 /* one global atomic per traversed cell */
#define SLAM_RAYCAST_TILED_MERGE 2 /* tiled, and the lanes of a wavefront that stand on one cell add once */

typedef struct {
    double max_range;           /* mls.h:161 (75) */
    double occupancy_increment; /* mls.h:188 (1.0) */
    double occupancy_decrement; /* mls.h:189 (0.3) */
    int    min_cluster_points;  /* mls.h:165 (10); local_mapper.cpp:86 sets 20 */
    int    rolling;             /* MLS(..., bool roll) mls.h:154 */
    int    raycast_impl;        /* SLAM_RAYCAST_* */
    int    raycast_seg_items;   /* tiled raycast: 64-beam blocks a workgroup takes from a tile's work list at a time (it goes
                                   on accumulating in the same LDS tile while the tile has blocks left and writes the tile
                                   back when it leaves it); 0 = library default (16); 8 ... 511 */
    int    raycast_wg_per_cu;   /* tiled raycast: persistent workgroups per CU; 0 = library default (two) */
    int    raycast_max_workgroups; /* tiled raycast: persistent workgroups in all; 0 = no cap (wg_per_cu x CUs) */
} slam_grid_params;

void slam_grid_default_params(slam_grid_params *p);

/* MLS::MLS(size_x, size_y, res, roll), mls.h:154-207 */
int  slam_grid_create(int size_x, int size_y, double resolution,
                      const slam_grid_params *params, slam_grid_t **out);
void slam_grid_destroy(slam_grid_t *g);
int  slam_grid_clear(slam_grid_t *g, slam_stream_t stream);            /* MLS::clearMap, mls.cpp:18-31 */
/* zeroes the hit/miss count planes only (batch / multi-GPU mode: a fresh local map per batch, so that the
 * all-reduce merges this batch's counts and not sums that were merged before) */
int  slam_grid_reset_counts(slam_grid_t *g, slam_stream_t stream);
int  slam_grid_set_min_cluster_points(slam_grid_t *g, int v);          /* mls.h:235 */
int  slam_grid_set_max_range(slam_grid_t *g, double v);                /* mls.h:237 */
/* MLS::setPose, mls.cpp:408-479.  Non-rolling: records curPose for the range
 * gate (mls.cpp:84-86).  Rolling: shifts the toroidal origin by
 * round(delta/res) cells and clears the cells that rolled in. */
int  slam_grid_set_pose(slam_grid_t *g, double x, double y, slam_stream_t stream);
int  slam_grid_get_pose(slam_grid_t *g, double *x, double *y);

/* MLS::addToOccupancy point loops, mls.cpp:73-142, on already segmented
 * clouds: obstacle points raise hits, ground points raise misses.  Points are
 * `stride` floats apart (x,y first; PCL PointXYZGD has stride 4). */
int slam_grid_add_endpoints(slam_grid_t *g, const float *obs, int n_obs, const float *gnd,
                            int n_gnd, int stride);
int slam_grid_add_endpoints_dev(slam_grid_t *g, const float *d_obs, int n_obs,
                                const float *d_gnd, int n_gnd, int stride,
                                slam_stream_t stream);

/* Bresenham free-space update (north-star extension; not in the reference):
 * for every beam the cells from the sensor cell up to (excluding) the end cell
 * get misses += 1, the end cell hits += 1.  origin/end are map-frame xy f32. */
int slam_grid_raycast(slam_grid_t *g, const float *origin_xy, const float *end_xy, int n);
int slam_grid_raycast_dev(slam_grid_t *g, const float *d_origin_xy, const float *d_end_xy,
                          int n, slam_stream_t stream);
/* The same straight from registered scans: end = (float)(R_s * p + t_s) formed
 * as icpPointToPoint.cpp:69-70 forms its query, origin = (float)t_s.
 * n_points = d_scan_off[n_scans] (the host built that array and knows it).  With a rolling
 * window the map-frame points are taken relative to the window centre (slam_grid_get_pose),
 * as mls.cpp:36-47 shifts the cloud before addToOccupancy. */
int slam_grid_raycast_scans_dev(slam_grid_t *g, const double *d_pts, const int32_t *d_scan_off,
                                int n_scans, int n_points, const double *d_R, const double *d_t,
                                slam_stream_t stream);
/* Reserves the raycast's scratch (beams, block boxes, work list) for calls of up to max_beams beams.  A raycast call
 * that finds its scratch too small grows it -- which frees the old block, and a free waits for the whole device: a
 * caller that streams batches of varying size (slam_mapper_* does this itself from max_points) reserves once instead. */
int slam_grid_reserve(slam_grid_t *g, int max_beams);

/* Folds the counts gathered since the last finalize into the per-cell evidence
 * value (Cluster::num_pts) and the occupancy byte by SURVEY 8(a) G3:
 *   c += inc*h; if (h>0 && c>min) occ=100;  c -= dec*m; if (m>0 && c<min) occ=0.
 * The count planes keep accumulating (they are the bit-exact contract). */
int slam_grid_finalize(slam_grid_t *g, slam_stream_t stream);
/* slam_grid_finalize followed by slam_grid_reset_counts, in one pass over the rows and one launch: what a batch step
 * ends with (fold this batch's counts into evidence and occupancy, leave the count planes zero for the next batch;
 * the accumulator planes, if any, are not touched).  Same evidence and occupancy as the two calls.  It alternates between two
 * row-range buffers from call to call, so it must not be recorded into a hipGraph that is replayed (slam_graph_*): a captured
 * step keeps slam_grid_finalize + slam_grid_reset_counts. */
int slam_grid_finalize_reset(slam_grid_t *g, slam_stream_t stream);

/* MLS::addToMap's cloud transform (mls.cpp:34-53, pcl::transformPointCloud with the pose's rotation and an offset): out = (float)(R p + t)
 * per point, R row-major, computed in double term by term as a host loop `r0*x + r1*y + r2*z + t` does (no contraction): the
 * same floats.  d_out_xyz: n x 3 floats; it may not overlap d_in_xyz unless stride == 3 and the two are the same array. */
int slam_grid_transform_cloud_dev(const float *d_in_xyz, int n, int stride, const double R[9], const double t[3], float *d_out_xyz,
                                  slam_stream_t stream);

/* One scan with the reference's own ordering and rounding (mls.cpp:73-142):
 * sequential += / -= on the per-cell double, thresholds after every point. */
int slam_grid_add_scan_inorder(slam_grid_t *g, const float *obs, int n_obs, const float *gnd,
                               int n_gnd, int stride);
/* the same with the two clouds resident in HBM (what slam_gseg_split_dev leaves); enqueues on `stream` */
int slam_grid_add_scan_inorder_dev(slam_grid_t *g, const float *d_obs, int n_obs, const float *d_gnd,
                                   int n_gnd, int stride, slam_stream_t stream);

/* read-back in WINDOW coordinates, row-major data[x + size_x*y] as
 * nav_msgs/OccupancyGrid (mls.h:167-175). Host pointers; synchronous. */
int slam_grid_read_counts(slam_grid_t *g, int32_t *hits, int32_t *misses);
int slam_grid_read_occupancy(slam_grid_t *g, int8_t *occ);      /* MLS::getDrivability()->data */
int slam_grid_read_num_pts(slam_grid_t *g, double *num_pts);
int slam_grid_total_updates(slam_grid_t *g, uint64_t *n);       /* counter increments so far */
int slam_grid_info(slam_grid_t *g, int *size_x, int *size_y, double *resolution,
                   int *origin_x, int *origin_y);
/* where a rolling window sits: the cells it has moved since creation (the sum of MLS::setPose's dx, dy,
 * mls.cpp:419-431; 0, 0 for a non-rolling grid).  Two grids hold the same world cells in the same storage rows
 * exactly when these agree (what a merge over the GPUs requires: slam_mi355x_rccl.h). */
int slam_grid_window_cell(slam_grid_t *g, int *cell_x, int *cell_y);

/* work list of the last tiled raycast: tiles of the window, (tile, 64-beam block) items, and how many times a
 * workgroup wrote a tile back (for reporting) */
int slam_grid_raycast_stats(slam_grid_t *g, int *n_tiles, int *n_items, int *n_segments);

/* the two int32 planes ([hits | misses], 2*size_x*size_y ints, toroidal
 * storage order) for a collective merge; see slam_mi355x_rccl.h */
int slam_grid_counts_dev(slam_grid_t *g, int32_t **d_planes, size_t *n_ints);
/* Whoever writes the planes through those pointers says which storage rows it wrote: the grid resets and finalizes
 * only the rows it knows to be touched (slam_grid_reset_counts, slam_grid_finalize).  The merges of
 * slam_mi355x_rccl.h do; asynchronous on `stream`, after the writes. */
int slam_grid_mark_rows(slam_grid_t *g, int row_lo, int row_hi, slam_stream_t stream);
/* Rows of the planes (storage order) that received counts since the planes were last reset or folded, tracked
 * on the device by the update kernels: a merge moves only these.  row_hi < row_lo = none.  The host form
 * synchronises; d_range = two ints {lowest row, -(highest row)} (0x7f7f7f7f each when none). */
int slam_grid_dirty_rows(slam_grid_t *g, int *row_lo, int *row_hi);
int slam_grid_dirty_rows_dev(slam_grid_t *g, int32_t **d_range);
/* Periodic merges of a running map (BASELINE config 5): with an accumulator, the count planes hold what THIS
 * GPU added since the last merge; after the all-reduce of those rows slam_grid_fold adds them to the
 * accumulator (the merged totals) and zeroes them, so that nothing is summed twice at the next merge.
 * Finalize and the read-backs see accumulator + planes. */
int slam_grid_enable_accumulator(slam_grid_t *g);
int slam_grid_fold(slam_grid_t *g, int row_lo, int row_hi, slam_stream_t stream);

/* ------------------------------------------------ grid distance field and costmap
 * What every consumer of the occupancy plane computes next (docs/GRID_DIST.md): the exact squared distance, in cells, from
 * every cell to the nearest obstacle cell, capped at R = max_cells, and the costmap that inflates obstacles by the robot's
 * footprint.  Not in the reference (MLS's robot_size only sets a height): a north-star extension like the raycast, defined by
 * the project's own brute-force restatement (tests/grid_dist_cases.py) and equal to it bit for bit.
 *
 * Planes are in WINDOW coordinates, data[x + size_x*y], as slam_grid_read_occupancy returns them.  Obstacles are the cells
 * with occ == 100, and those with occ == -1 when unknown_is_obstacle is set; cells outside the window are never obstacles
 * and distance does not wrap across its edges.
 *   dist2 (uint16)  min over obstacles of (x-x')^2 + (y-y')^2 where that is <= R*R, SLAM_GDIST_FAR otherwise (and when there
 *                   is no obstacle at all)
 *   cost  (uint8)   only with a table T of exactly R*R + 2 bytes: T[min(dist2, R*R + 1)] -- the last entry answers FAR; a
 *                   cell with occ == -1 (unknown_is_obstacle == 0) keeps that byte if it is >= unknown_keep_from and
 *                   becomes unknown_cost otherwise. */
typedef struct slam_gdist slam_gdist_t;
#define SLAM_GDIST_FAR 0xFFFFu
typedef struct {
    int max_cells;            /* R, 1..254; default 32 (a starting value, not tuned) */
    int unknown_is_obstacle;  /* default 0 */
    int unknown_cost;         /* 0..255, default 255 (costmap_2d NO_INFORMATION) */
    int unknown_keep_from;    /* 0..255, default 253 (costmap_2d INSCRIBED_INFLATED_OBSTACLE) */
} slam_gdist_params;
void slam_gdist_default_params(slam_gdist_params *p);
/* The inflation table of ROS costmap_2d's inflation layer, on the host (no device is touched): table[0] = 254; for
 * k = 1 .. R*R with d = sqrt(k) * resolution: 253 where d <= inscribed_radius, 0 where d > inflation_radius, else
 * (uint8_t)(252 * exp(-cost_scaling * (d - inscribed_radius))); table[R*R + 1] = 0.  SLAM_E_INVALID: n != R*R + 2, a
 * non-finite or negative argument, resolution == 0, inscribed_radius > inflation_radius, or inflation_radius >
 * max_cells * resolution (the distance cap would cut the inflation short). */
int  slam_grid_inflation_table(double resolution, double inscribed_radius, double inflation_radius,
                               double cost_scaling, int max_cells, uint8_t *table, int n);
/* The likelihood-field table of a grid matcher (docs/GRID_MATCH.md), on the host: table[k] = (uint8_t)rint(255 *
 * exp(-(k * resolution^2) / (2 * sigma^2))) for k = 0 .. R*R -- the expression of the correlative matcher's stamp, so entry
 * i*i + j*j is stamp entry (i, j) -- and table[R*R + 1] = 0.  SLAM_E_INVALID: n != R*R + 2, a non-finite or non-positive
 * resolution or sigma (or one whose square is 0 or infinite in a double), max_cells outside 1 .. 254. */
int  slam_grid_likelihood_table(double resolution, double sigma, int max_cells, uint8_t *table, int n);
/* outputs, scratch and the table's room are allocated here; nothing is allocated later */
int  slam_gdist_create(int size_x, int size_y, const slam_gdist_params *p, slam_gdist_t **out);
void slam_gdist_destroy(slam_gdist_t *h);
/* n == R*R + 2 bytes of any table (the inflation table above, a likelihood-field table for a matcher ...); NULL, 0 removes
 * it.  Synchronous.  The cost plane belongs to the table it was computed with: compute again before reading it. */
int  slam_gdist_set_table(slam_gdist_t *h, const uint8_t *table, int n);
/* d_occ: a device plane of size_x*size_y bytes, borrowed until the stream reaches this point.  Only enqueues kernels on
 * `stream`: no host wait, no allocation -- it can stand behind slam_grid_finalize on the grid's stream. */
int  slam_gdist_compute_dev(slam_gdist_t *h, const int8_t *d_occ, slam_stream_t stream);
int  slam_gdist_compute(slam_gdist_t *h, const int8_t *occ);               /* host plane; synchronous */
/* host planes of size_x*size_y elements; either may be NULL; waits for the device.  cost without a table, or with a table
 * set after the last compute: SLAM_E_INVALID */
int  slam_gdist_read(slam_gdist_t *h, uint16_t *dist2, uint8_t *cost);
int  slam_gdist_planes_dev(slam_gdist_t *h, uint16_t **d_dist2, uint8_t **d_cost); /* *d_cost = NULL without a table */
/* slam_gdist_compute_dev over the grid's own occupancy: exactly the plane slam_grid_read_occupancy would return at this
 * point of the stream (after the in-order mode, that mode's state; otherwise what the last finalize left -- this call does
 * not finalize).  Grid and handle must have the same size. */
int  slam_grid_distance_field(slam_grid_t *g, slam_gdist_t *h, slam_stream_t stream);

/* ------------------------------------------------ grid navigation field and path
 * What a planner computes from the cost plane (docs/GRID_NAV.md): the exact cost-to-go from every cell to the nearest of a
 * set of goal cells, and the path down it.  Not in the reference, and parity with navfn or any outside planner is not
 * claimed: the yardstick is the project's own restatement (tests/grid_nav_cases.py), which the device equals bit for bit.
 * All integer.  Planes are in WINDOW coordinates, data[x + size_x*y]; nothing wraps across the window's edges.
 *   step table  S[256] uint32, indexed by a cost byte: 0 closes the cell, otherwise 1 <= S[c] <= 2^20
 *   moves       8-connected; direction d = 0..7 is (dx, dy) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1).  A move
 *               between u and v costs m(u, v) = w * (S[cost[u]] + S[cost[v]]), w = orth_w for d even, diag_w for d odd, both
 *               1..255.  A diagonal move needs both cells that share an edge with u and with v traversable (no corner
 *               cutting); cells outside the plane are not traversable
 *   potential   uint32: the least sum of m over paths to any valid goal where that is < 0xFFFFFFFF, SLAM_GNAV_FAR otherwise
 *               (saturated, never wrapped); 0 on goals, FAR on closed and unreachable cells
 *   goals       int32 pairs (x, y); one outside the plane or on a closed cell is skipped and counted
 *   path        from a start: the next cell is the allowed neighbour of lowest d with pot[v] + m(u, v) == pot[u]; int32 pairs,
 *               the start first, the goal last, with one of the SLAM_GNAV_PATH_* statuses below */
typedef struct slam_gnav slam_gnav_t;
#define SLAM_GNAV_FAR 0xFFFFFFFFu
#define SLAM_GNAV_PATH_REACHED       0  /* the path's last cell is a goal */
#define SLAM_GNAV_PATH_NO_START      1  /* the start is outside the plane, closed or FAR (length 0) */
#define SLAM_GNAV_PATH_CUT           2  /* cut at max_len (max_len cells are valid) */
#define SLAM_GNAV_PATH_NOT_CONVERGED 3  /* the field is not converged (nothing walked) */
typedef struct {
    int orth_w, diag_w;     /* the move weights, 1 .. 255; default 12, 17 */
    int neutral;            /* the step table slam_gnav_create installs, as slam_grid_step_table makes it; default 50 */
    int lethal_from;        /* default 253 */
    int unknown_step;       /* default 0 */
} slam_gnav_params;
typedef struct {
    int64_t rounds;           /* rounds enqueued since the last restart */
    int64_t converged;        /* a round has flagged nothing (or no goal was valid): the field is exact */
    int64_t goals_used, goals_skipped;
    int64_t tiles_processed;  /* tiles relaxed since the last restart */
    int64_t last_path_len, last_path_status;
} slam_gnav_state;
void slam_gnav_default_params(slam_gnav_params *p);
/* The step table, on the host (slam_amd/csrc/grid_nav_table.hpp; no device is touched): table[c] = neutral + c for
 * c < lethal_from, 0 from there on, table[255] = unknown_step (0 keeps unknown cells closed).  SLAM_E_INVALID and nothing
 * written: n != 256, neutral outside 1 .. 2^19, lethal_from outside 1 .. 256, unknown_step outside 0 .. 2^20, a null table. */
int  slam_grid_step_table(int neutral, int lethal_from, int unknown_step, uint32_t *table, int n);
/* Everything is allocated here, nothing later; the step table of p's neutral, lethal_from, unknown_step is installed (under
 * slam_grid_step_table's rules).  Sizes 1 .. 32767, weights 1 .. 255. */
int  slam_gnav_create(int size_x, int size_y, const slam_gnav_params *p /* NULL: the defaults */, slam_gnav_t **out);
void slam_gnav_destroy(slam_gnav_t *h);
/* any 256 entries of 0 .. 2^20.  Synchronous.  The field belongs to the table it was computed with: restart afterwards. */
int  slam_gnav_set_table(slam_gnav_t *h, const uint32_t *table, int n);
/* d_cost: a device plane of size_x*size_y cost bytes; d_goals: n_goals >= 1 int32 pairs on the device; both borrowed until
 * the stream reaches this point.  restart != 0: the handle takes a copy of the cost plane and the field starts from the
 * goals; restart == 0 continues on the plane of the last restart (d_cost and d_goals are not read, but must still be non-null and
 * n_goals >= 1: one rule for both forms).  Then exactly `rounds`
 * rounds are enqueued.  No host wait, no allocation: a graph may capture it.  SLAM_E_INVALID: a null pointer, n_goals < 1,
 * rounds < 0. */
int  slam_gnav_compute_dev(slam_gnav_t *h, const uint8_t *d_cost, const int32_t *d_goals, int n_goals, int rounds, int restart,
                           slam_stream_t stream);
/* Host plane and host goals; synchronous.  Rounds in batches until the field has converged, one pinned word read per batch;
 * SLAM_E_TIMEOUT when max_rounds rounds did not suffice.  max_rounds == 0: size_x*size_y + 1, which always suffices. */
int  slam_gnav_compute(slam_gnav_t *h, const uint8_t *cost, const int32_t *goals, int n_goals, int max_rounds);
int  slam_gnav_read(slam_gnav_t *h, uint32_t *pot);                         /* size_x*size_y words; waits for the device */
int  slam_gnav_potential_dev(slam_gnav_t *h, uint32_t **d_pot);
/* One wave walks the path on the device: d_path has room for max_len int32 pairs, d_len_status is two int32 (length,
 * status).  Bounded by max_len whatever the field holds.  Asynchronous on `stream`. */
int  slam_gnav_path_dev(slam_gnav_t *h, int sx, int sy, int max_len, int32_t *d_path, int32_t *d_len_status, slam_stream_t stream);
int  slam_gnav_path(slam_gnav_t *h, int sx, int sy, int max_len, int32_t *path, int *len, int *status); /* host twin; synchronous */
int  slam_gnav_read_state(slam_gnav_t *h, slam_gnav_state *state);          /* synchronous */
/* slam_gnav_compute_dev with restart over the cost plane slam_gdist_planes_dev hands out, as it lies at this point of the
 * stream.  Grid, distance field and navigation field must have the same size, and the distance field a table. */
int  slam_grid_nav_field(slam_grid_t *g, slam_gdist_t *gdist, slam_gnav_t *gnav, const int32_t *d_goals, int n_goals, int rounds,
                         slam_stream_t stream);

/* ------------------------------------------------------------ height-cluster map
 * Stands for class MLS in its non-rolling, height-cluster mode (mls.h:154-237, mls.cpp:18-53, 152-402, 481-556):
 * graph_slam's global map (graph_slam.cpp:71).  Every cell holds up to `capacity` z clusters (mean x, y, z, cov_zz,
 * num_pts), a drivable state, a drivability byte, an `updated` flag and the points still pending for it
 * (docs/MLS_MAP.md).  Arithmetic is the reference's: double, float inputs widened, no contraction. */
typedef struct slam_mls slam_mls_t;

typedef struct {
    double max_range;              /* mls.h:161 (75) */
    int    update_dist;            /* cells (mls.h:162); -1 = (int)fmin((int)max_range/res, size_x/2), resolved at create */
    int    max_clusters;           /* mls.h:163 (50); at most the capacity fixed at create */
    int    max_cluster_points;     /* mls.h:164 (200) */
    int    min_cluster_points;     /* mls.h:165 (10) */
    double normal_threshold;       /* mls.h:177 (0.15) */
    double height_threshold;       /* mls.h:178 (0.4) */
    double cluster_sigma_factor;   /* mls.h:180 (3) */
    double cluster_dist_threshold; /* mls.h:181 (0.5) */
    double cluster_combine_dist;   /* mls.h:182 (0.2) */
    double drive_dist_threshold;   /* mls.h:183 (1.0) */
    double robot_height;           /* mls.h:184: robot_size (1.45); also the start pad's height at create (mls.h:195) */
} slam_mls_params;

void slam_mls_default_params(slam_mls_params *p);
/* MLS(size_x, size_y, res, false, robot_height), mls.h:154-205: the start pad of (2*(int)(1/res)+1)^2 cells, each
 * with one cluster (i*res, j*res, -robot_height), num_pts = min_cluster_points, cov_zz 0.01; drivability bytes 0.
 * Cluster capacity per cell = params->max_clusters (dense: 48 bytes per slot). */
int  slam_mls_create(int size_x, int size_y, double resolution, const slam_mls_params *params, slam_mls_t **out);
void slam_mls_destroy(slam_mls_t *m);
int  slam_mls_clear(slam_mls_t *m, slam_stream_t stream);                         /* MLS::clearMap, mls.cpp:18-31 */
int  slam_mls_set_pose(slam_mls_t *m, double x, double y);                         /* mls.cpp:408-414: stores the pose */
/* the setters of mls.h:223-237; update_dist < 0 keeps the current value; max_clusters above the capacity: E_INVALID */
int  slam_mls_set_params(slam_mls_t *m, const slam_mls_params *p);
/* MLS::addToMap(cloud) non-rolling, mls.cpp:345-402 -> updateCell :152-342, at the pose last set.  Points are `stride`
 * floats apart (x, y, z first).  Enqueues on `stream` without a host wait (the host form copies the cloud first);
 * the device points are borrowed until the stream reaches the call.  SLAM_E_NOMEM when the pending store cannot grow. */
int  slam_mls_add_cloud(slam_mls_t *m, const float *xyz, int n, int stride);
int  slam_mls_add_cloud_dev(slam_mls_t *m, const float *d_xyz, int n, int stride, slam_stream_t stream);
int  slam_mls_offset_z(slam_mls_t *m, double dz, slam_stream_t stream);           /* MLS::offsetMap's clusters, mls.cpp:481-491 */
int  slam_mls_read_drivability(slam_mls_t *m, int8_t *data);                      /* MLS::getDrivability()->data: size_x*size_y bytes */
/* MLS::getSegmentedClouds, mls.cpp:520-556: x, y, z floats per point in the reference's order.  The counts are always
 * returned; SLAM_E_NOMEM (nothing copied) when a capacity is short.  Synchronous. */
int  slam_mls_segmented_clouds(slam_mls_t *m, float *obstacle, int obstacle_cap, int *n_obstacle, float *ground,
                               int ground_cap, int *n_ground);
/* For n cells (linear x + size_x*y): cluster count, clusters[i*capacity + c] = (mean x, y, z, cov_zz, num_pts),
 * drivable, byte, updated flag and pending point count.  Host arrays (any may be NULL); synchronous. */
int  slam_mls_read_cells(slam_mls_t *m, const int32_t *cells, int n, int32_t *n_clusters, double *clusters, int8_t *drivable,
                         int8_t *bytes, uint8_t *updated, int32_t *pending);
/* sizes, cluster capacity, resolved parameters and the points pending now (synchronous); any pointer may be NULL */
int  slam_mls_info(slam_mls_t *m, int *size_x, int *size_y, double *resolution, int *capacity, slam_mls_params *p,
                   int *pending_points);

/* ------------------------------------------------------ ground segmentation
 * Stands for class groundSegmentation (ground_segmentation/include/ground_segmentation/
 * groundSegmentation.h:67-128), the GP-INSAC pre-filter both halves of the path run first
 * (icpTools.cpp:114-115, mls.cpp:66-67): setupGroundSegmentation + segmentGround, with
 * the constructor's parameters (groundSegmentation.cpp:31-55; field = reference setter). */
typedef struct slam_gseg slam_gseg_t;

typedef struct {
    double rmax;                     /* set_rmax(100.0) */
    int    num_seedpoints;           /* set_num_seedpoints(10) */
    double gp_lengthparameter;       /* set_gp_lengthparameter(10) */
    double gp_covariancescale;       /* set_gp_covariancescale(1.0) */
    double gp_modelnoise;            /* set_gp_modelnoise(0.3) */
    double gp_groundmodelconfidence; /* set_gp_groundmodelconfidence(5.0) */
    double gp_grounddataconfidence;  /* set_gp_grounddataconfidence(5.0) */
    double gp_groundthreshold;       /* set_gp_groundthreshold(0.3) */
    double robotheight;              /* set_robotheight(1.2) */
    double seeding_maxrange;         /* set_seeding_maxrange(50) */
    double seeding_maxheight;        /* set_seeding_maxheight(15) */
} slam_gseg_params;

#define SLAM_GSEG_DROPPED  0 /* in no output cloud: beyond rmax, or in a bin with <= 5 points */
#define SLAM_GSEG_GROUND   1 /* groundCloud */
#define SLAM_GSEG_OBSTACLE 2 /* obsCloud and drvCloud (below robot height) */
#define SLAM_GSEG_OVERHEAD 3 /* obsCloud only (drivable = 1) */

void slam_gseg_default_params(slam_gseg_params *p);
int  slam_gseg_create(const slam_gseg_params *params, slam_gseg_t **out);
void slam_gseg_destroy(slam_gseg_t *h);
int  slam_gseg_reserve(slam_gseg_t *h, int max_points);
/* one label (SLAM_GSEG_*) per input point; points are `stride` floats apart (x, y, z first) */
int  slam_gseg_segment(slam_gseg_t *h, const float *xyz, int n, int stride, uint8_t *labels);
int  slam_gseg_segment_dev(slam_gseg_t *h, const float *d_xyz, int n, int stride, uint8_t *d_labels,
                           slam_stream_t stream);
/* the ground cloud and the drvCloud as (x, y, z, 0) records -- what slam_grid_add_endpoints_dev
 * takes with stride 4; d_counts[0] = ground points, d_counts[1] = obstacle points written */
int  slam_gseg_split_dev(slam_gseg_t *h, const float *d_xyz, int n, int stride, const uint8_t *d_labels,
                         float *d_ground_xyz4, float *d_obstacle_xyz4, int32_t *d_counts,
                         slam_stream_t stream);
/* CCICP::classifyPoints, icpTools.cpp:36-103: for every point of the obstacle cloud 1 = ground
 * adjacent (GA), 0 = not (NGA), 255 = dropped there too (outside the 1200 x 1200 x 0.5 m lattice
 * or in its outermost cells).  GA/NGA are the two classes the ICP matches separately. */
int  slam_gseg_classify_ga_dev(slam_gseg_t *h, const float *d_obstacle_xyz, int n, int stride,
                               uint8_t *d_flags, slam_stream_t stream);
/* the same where the number of points is known on the device only (*d_n, at most n_capacity): no host round trip */
int  slam_gseg_classify_ga_counted_dev(slam_gseg_t *h, const float *d_obstacle_xyz, const int32_t *d_n, int n_capacity,
                                       int stride, uint8_t *d_flags, slam_stream_t stream);
/* ... and with the extent of the points the classification keeps (pcl::getMinMax3D over the finite points whose flag is not
 * 255: what setSceneCloud's voxel filter starts from, icpTools.cpp:620-633) accumulated in the same pass: d_mm[0..2] minima,
 * d_mm[3..5] maxima as ORDERED floats (the bits with the sign bit flipped for positive, all bits for negative values), which
 * the caller has set to 0xffffffff / 0 beforehand */
int  slam_gseg_classify_ga_extent_dev(slam_gseg_t *h, const float *d_obstacle_xyz, const int32_t *d_n, int n_capacity,
                                      int stride, uint8_t *d_flags, uint32_t *d_mm, slam_stream_t stream);
/* per polar bin (72 x 200): 1 = in the ground model (value = prototype height), 2 = candidate
 * that stayed out (value = GP mean), 0 = no signal point; INSAC iterations per sector */
int  slam_gseg_read_model(slam_gseg_t *h, uint8_t *bin_state, double *bin_value, int32_t *sector_iterations);

/* ------------------------------------------------------------------------
 * CCICP facade steps either side of the ICP call.  The reference does these
 * with PCL (not part of its checkout): the published PCL 1.7 algorithms are restated; parity unpinned.
 * All device-resident; every result is deterministic.
 * ---------------------------------------------------------------------- */
typedef struct slam_ccicp slam_ccicp_t;
int  slam_ccicp_create(slam_ccicp_t **out);
void slam_ccicp_destroy(slam_ccicp_t *h);

/* The points whose ground-segmentation label (SLAM_GSEG_*) is in label_mask (bit 1 << label), in cloud
 * order, as (x, y, z, 0) records: (1 << SLAM_GSEG_OBSTACLE) | (1 << SLAM_GSEG_OVERHEAD) is the outcloud
 * CCICP::segmentGround classifies, 1 << SLAM_GSEG_GROUND its ground cloud (icpTools.cpp:106-119). */
int slam_ccicp_select_dev(slam_ccicp_t *h, const float *d_xyz, int n, int stride, const uint8_t *d_labels,
                          unsigned label_mask, float *d_out_xyz4, int *n_out, slam_stream_t stream);

/* CCICP::setSceneCloud / setTargetCloud voxel filter, icpTools.cpp:620-633 (pcl::VoxelGrid, leaf
 * 0.5,0.5,2 for obstacles, 0.5,0.5,5 for ground): one output point per occupied voxel, x,y,z = centroid,
 * [3] = ground_adj averaged as PCL averages every field (then stored to the uint16 field), in increasing
 * voxel index (x fastest).  d_xyz: `stride` floats per point; the class comes from d_flag (1 = GA, as
 * slam_gseg_classify_ga_dev writes it) or, when d_flag is null and stride > 3, from float [3] > 0.5.
 * d_out: 4 floats per voxel, room for max_out; *n_out = voxels produced.  Synchronises the stream twice
 * (lattice extent, count). */
int slam_ccicp_voxel_downsample_dev(slam_ccicp_t *h, const float *d_xyz, const uint8_t *d_flag, int n, int stride,
                                    float leaf_x, float leaf_y, float leaf_z, float *d_out, int max_out, int *n_out,
                                    slam_stream_t stream);

/* The cloud as CCICP::classifyPoints leaves it (icpTools.cpp:64-101): points it keeps, bin by bin (x bin
 * major, y bin minor), original order inside a bin, as x,y,z,ground_adj records -- the order in which
 * doICPMatch applies the ICP_MAX_PTS cap to the target cloud (SCAN_TO_MAP: setTargetCloud classifies
 * without a voxel filter, icpTools.cpp:591-595).  d_flag: the flags slam_gseg_classify_ga_dev wrote for
 * the same points. */
int slam_ccicp_bin_order_dev(slam_ccicp_t *h, const float *d_xyz, const uint8_t *d_flag, int n, int stride,
                             float *d_out_xyzg, int *n_out, slam_stream_t stream);

/* CCICP::doICPMatch(initPose) marshalling, icpTools.cpp:225-276: optional crop of +-crop_dist around
 * (cur_x,cur_y) (pcl::PassThrough on x then y; the reference crops the target cloud only, 75 m), then the
 * split by isGA(ground_adj) in cloud order with at most cap-1 points per class (ICP_MAX_PTS = 20000,
 * icpTools.h:21) as f64 xy -- the arrays slam_icp_create / slam_icp_fit take.  d_xyzg: x,y,z,ground_adj
 * with `stride` >= 4 floats per point (the voxel filter's output).  counts[0] = GA, counts[1] = NGA. */
int slam_ccicp_split_dev(slam_ccicp_t *h, const float *d_xyzg, int n, int stride, int crop, double cur_x, double cur_y,
                         double crop_dist, int cap, double *d_ga_xy, double *d_nga_xy, int counts[2],
                         slam_stream_t stream);

/* The same with the crop given as the box itself, box = {x_lo, x_hi, y_lo, y_hi} (closed intervals of floats, as
 * pcl::PassThrough compares them; null = no crop): CCICP::doICPMatch filters seg_target IN PLACE (icpTools.cpp:226-239), so the
 * points a later match sees are those inside the intersection of every window since setTargetCloud -- a box again.
 * totals (optional) = points of each class inside the box before the cap (what the reference's seg_target keeps). */
int slam_ccicp_split_box_dev(slam_ccicp_t *h, const float *d_xyzg, int n, int stride, const float box[4], int cap, double *d_ga_xy,
                             double *d_nga_xy, int counts[2], int totals[2], slam_stream_t stream);

/* CCICP::doHeightInterpolate, icpTools.cpp:301-381: the four wheel points of the pose (x,y,z,qx,qy,qz,qw)
 * find their nearest ground point (exact, squared distance < 9); with four of them the new z is
 * n_z * 1.45 + mean z of the four (n = their plane normal, n_z >= 0); otherwise z stays.  nn_idx
 * (optional) gets the four nearest indices. */
int slam_ccicp_height_dev(slam_ccicp_t *h, const float *d_ground, int n, int stride, const double pose[7], double *z_out,
                          int *n_corr, int nn_idx[4], slam_stream_t stream);

/* The steps above as ONE device-resident chain, for a caller that matches cloud after cloud (scan_registration.cpp:
 * 109-199): CCICP::segmentGround + classifyPoints + setSceneCloud's voxel filter (voxel != 0; 0 = setTargetCloud's
 * bin order) + doICPMatch's crop / class split / cap, stage after stage on `stream` with every count left on the device
 * -- the stepwise entry points return each count to the host, seven round trips per cloud.  Same results, bit for bit.
 *   d_pts    out: xy f64, the GA points then the NGA points (room for 2 * (cap - 1) points)
 *   d_scan   out: int32[3] = {0, n_ga + n_nga, n_ga}: d_scan_off = d_scan, d_scan_nga = d_scan + 2 of a
 *            slam_icp_fit_batch_dev call with n_scans = 1 that registers the cloud without the host knowing its size
 *   d_ground out, nullable: the ground cloud as x,y,z,0 records (room for n)
 *   d_counts out: int32[4] = {obstacle points, ground points, points after the filter, error bits}.  Bit 1: the voxel lattice did
 *            not fit the chain's accumulator (2 M voxels; the stepwise entry point takes larger extents).  Bit 4: a block of a
 *            compaction gave up waiting for the blocks before it (a safeguard against a hang, seconds long): d_pts and d_scan are
 *            not valid.  The stepwise entry points return SLAM_E_HIP for the same.
 * Nothing is read back and nothing waits: the caller reads d_counts when it needs them. */
int slam_ccicp_scene_dev(slam_ccicp_t *h, slam_gseg_t *seg, const float *d_xyz, int n, int stride, int voxel, int crop,
                         double cur_x, double cur_y, double crop_dist, int cap, double *d_pts, int32_t *d_scan,
                         float *d_ground, int32_t *d_counts, slam_stream_t stream);
/* doHeightInterpolate for the pose a registration left on the device (d_R 2x2, d_t of one scan; yaw = atan2(R10, R00),
 * icpTools.cpp:195-197) against a ground cloud whose size is known on the device (*d_n_ground <= n_capacity):
 * d_out[0] = z, d_out[1] = neighbours within 3 m.  Asynchronous. */
int slam_ccicp_height_pose_dev(slam_ccicp_t *h, const float *d_ground, const int32_t *d_n_ground, int n_capacity,
                               int stride, const double *d_R, const double *d_t, double z0, double *d_out,
                               slam_stream_t stream);
/* ... with the roll and pitch of the initial pose, which doICPMatch keeps beside the matched yaw (tf::createQuaternionFromRPY,
 * icpTools.cpp:205-212) and doHeightInterpolate turns the wheel points by (:321-332) */
int slam_ccicp_height_rpy_pose_dev(slam_ccicp_t *h, const float *d_ground, const int32_t *d_n_ground, int n_capacity,
                                   int stride, const double *d_R, const double *d_t, double z0, double roll, double pitch,
                                   double *d_out, slam_stream_t stream);
/* ... and, behind the height, `mirror_bytes` (a multiple of 8, at most 4096) copied from mirror_src (device) to mirror_dst by the
 * last kernel of the call: with mirror_dst in pinned host memory (slam_host_alloc) the caller's result block -- pose, result,
 * height, scan descriptor -- is on the host when the stream has drained, without a copy of its own behind the match */
int slam_ccicp_height_rpy_pose_mirror_dev(slam_ccicp_t *h, const float *d_ground, const int32_t *d_n_ground, int n_capacity,
                                          int stride, const double *d_R, const double *d_t, double z0, double roll, double pitch,
                                          double *d_out, void *mirror_dst, const void *mirror_src, size_t mirror_bytes,
                                          slam_stream_t stream);
/* The throughput form of a sequence of matches (BASELINE config 3; scan_registration.cpp:109-173 is one cloud at a time): n <= 32
 * scenes made by slam_ccicp_scene_dev -- on as many streams as the caller likes, each with its own slam_ccicp_t / slam_gseg_t --
 * gathered into ONE batch for slam_icp_fit_batch_dev: d_out_pts = their points one scene after the other (room for the sum),
 * d_scan_off[n + 1] / d_scan_nga[n] as that call reads them.  d_pts[k] / d_scan[k]: the d_pts / d_scan of scene k (host arrays of
 * device pointers; the sizes stay on the device).  Asynchronous: the caller makes `stream` wait for the scenes' streams first. */
int slam_ccicp_pack_scans_dev(int n, const double *const *d_pts, const int32_t *const *d_scan, double *d_out_pts, int32_t *d_scan_off,
                              int32_t *d_scan_nga, slam_stream_t stream);
/* The filtered cloud of the last slam_ccicp_scene_dev call (x, y, z, ground_adj records: seg_scene / seg_target of
 * icpTools.h:77-78; d_counts[2] of that call says how many are valid) copied to d_out_xyzg, at most `capacity` records. */
int slam_ccicp_scene_cloud_dev(slam_ccicp_t *h, float *d_out_xyzg, int capacity, slam_stream_t stream);

/* ------------------------------------------------------------------------
 * Streaming mapper (BASELINE config 5).  Stands where scan_registration (scan_registration.cpp:109-199: one
 * doICPMatch per scan against the target it keeps) feeds local_mapper (local_mapper.cpp:65-130: addToMap at
 * 50 Hz): chunks of scans go from pinned host memory through registration into the occupancy grid on three
 * HIP streams (copy of chunk k+1 | ICP of chunk k | grid update of chunk k-1), the ICP target is a sliding
 * window of the scans registered so far, and every merge_every chunks the grid is merged over the GPUs
 * (slam_mapper_use_comm, slam_mi355x_rccl.h) and finalized.
 * ---------------------------------------------------------------------- */
typedef struct slam_mapper slam_mapper_t;

typedef struct {
    int    grid_size_x, grid_size_y;
    double resolution;
    slam_grid_params grid;     /* rolling = 1: the window follows slam_mapper_push's window_x/y (mls.cpp:408-479) */
    slam_icp_params  icp;
    double indist;             /* icpTools.cpp:188 (5.0) */
    int    max_scans, max_points; /* reservation per chunk */
    int    window_chunks;      /* sliding local map: the target is the registered points of the last W <= 8 chunks
                                  (thinned or decimated); 0 = the model given at create stays the target */
    int    rebuild_every;      /* chunks between rebuilds of the sliding target (>= 1) */
    int    target_points;      /* points the sliding target holds at most, both classes (2 x 19999: icpTools.h:21) */
    int    keep_prior;         /* 1 = the model given at create stays part of every rebuilt target */
    int    merge_every;        /* chunks between merges over the GPUs + finalize; 0 = only at slam_mapper_finish */
    int    pipelined;          /* 1 = copy, registration (two in turn for a fixed target) and grid update on streams of their
                                  own; 0 = one stage after the other on one stream (same results) */
    int    strict_window;      /* 1 = the push a rebuild is due at waits for it: the chunk meets the target built from every
                                  chunk before it (reproducible; the pipeline drains once per rebuild); 0 = the build is
                                  enqueued (same window) and adopted by a later push, see background_rebuild */
    int    slots;              /* chunks in flight (device + pinned buffers each): 2..8; 0 = default: 5 -- with a fixed target the
                                  host enqueues chunk k while two registrations run on the two registration streams and
                                  the chunks before them are mapped and read back (256-scan chunks: two 0.54 ms per chunk,
                                  three 0.43, four 0.38, five 0.37); with a sliding target, whose chunks register one after
                                  the other (config 5, rebuilt every 4 chunks): four 0.410 ms per chunk, five 0.396, six
                                  0.397-0.436, eight 0.408-0.414 -- four is slow only where it equals rebuild_every (every 3 /
                                  5 / 8 chunks: four and five slots within 1 % of each other) */
    double thin_res;           /* > 0: the window is thinned to one point per cell of this pitch (metres) and class over
                                  the grid's extent, the oldest measurement of a cell kept (where pcl::VoxelGrid keeps a
                                  centroid, icpTools.cpp:620-633); 0: every stride-th point of a chunk instead */
    int    background_rebuild; /* 1 (default) = the sliding target's rebuild is enqueued on a stream of its own (no host wait:
                                  the index build plans itself on the device) and adopted by the first push that finds it
                                  complete (a push waits for it only when the next rebuild is due or after
                                  min(rebuild_every, 4) pushes); 0 or strict_window = the push waits for it at once */
    int    registration_streams; /* 0 = default (two in turn, scans in pairs, for a fixed target; one for a sliding target), 1, 2 */
} slam_mapper_params;

void slam_mapper_default_params(slam_mapper_params *p);
/* m_ga / m_nga: the prior map (host, f64 xy), the first ICP target (at least 5 points, icp.cpp:38-43) */
int  slam_mapper_create(const slam_mapper_params *params, const double *m_ga, int n_ga, const double *m_nga, int n_nga,
                        slam_mapper_t **out);
void slam_mapper_destroy(slam_mapper_t *m);
/* The producer fills the PINNED buffers of slot slam_mapper_next_slot() -- points (xy f64), scan_off
 * (n_scans + 1, from 0), scan_nga, initial poses R0 (4 per scan) and t0 (2 per scan) -- and pushes. */
int  slam_mapper_next_slot(slam_mapper_t *m, int *slot);
int  slam_mapper_slots(slam_mapper_t *m, int *n_slots);
int  slam_mapper_chunk_buffers(slam_mapper_t *m, int slot, double **pts, int32_t **scan_off, int32_t **scan_nga,
                               double **R0, double **t0);
/* enqueues the chunk in the next slot and returns at once; window_x/y: where a rolling grid is centred for it */
int  slam_mapper_push(slam_mapper_t *m, int n_scans, int n_points, double window_x, double window_y, int *slot);
/* blocks until the chunk last pushed into `slot` is registered and mapped; its poses to host memory (optional).  (The poses
 * come back through the slot's pinned R0 / t0 buffers, which hold the REGISTERED poses from here until the producer fills
 * them for the slot's next chunk.) */
int  slam_mapper_wait(slam_mapper_t *m, int slot, double *R_out, double *t_out);
/* last merge (if a communicator is installed), finalize, and waits for everything */
int  slam_mapper_finish(slam_mapper_t *m);
int  slam_mapper_grid(slam_mapper_t *m, slam_grid_t **grid);      /* owned by the mapper */
int  slam_mapper_target(slam_mapper_t *m, slam_icp_t **icp);      /* the current ICP target (owned by the mapper) */
int  slam_mapper_stats(slam_mapper_t *m, long *chunks, long *merges, long *rebuilds, double *rebuild_ms,
                       int last_merge_rows[2]);
/* How a merge is carried out: begin is enqueued behind a chunk's grid update, finish when the next chunk's
 * registration has been enqueued (so the GPU is busy while the host waits for the rows to merge).  Installed
 * by slam_mapper_use_comm; with none, the periodic step is finalize alone. */
typedef int (*slam_mapper_merge_fn)(void *ctx, slam_grid_t *grid, slam_stream_t stream, int *row_lo, int *row_hi);
int  slam_mapper_set_merge(slam_mapper_t *m, slam_mapper_merge_fn begin, slam_mapper_merge_fn finish, void *ctx);

/* -------------------------------------------------------------------------
 * graph_slam's keyframe edges (graph_slam/src/graphSlamTools.cpp:108-364): a store of voxel-filtered keyframes, each
 * with a 3-D search lattice, and calcEdgeIcp's registration -- pcl::IterativeClosestPoint, point to point, then
 * computeEdgeInformationLUM -- for a batch of edges in one launch.  docs/KF_EDGE.md has the contract.
 * ---------------------------------------------------------------------- */
typedef struct slam_kf slam_kf_t;

typedef struct {
    double leaf_size;              /* pcl::VoxelGrid leaf, all three axes (graphSlamTools.cpp:281: 0.5) */
    double gate;                   /* setMaxCorrespondenceDistance, also computeEdgeInformationLUM's (:29, :302: 0.75) */
    double cell_size;              /* edge of the search lattice, >= gate; 0 = gate.  (The lattice adds 2^-16 of it, which
                                      covers the rounding of the f32 distance test.) */
    int    max_iterations;         /* setMaximumIterations (:31: 200) */
    double transformation_epsilon; /* setTransformationEpsilon (:33: 1e-6) */
    double fitness_epsilon;        /* setEuclideanFitnessEpsilon (:35: 1e-6) */
    int    target_in_lds;          /* 1 (default): an edge's workgroup stages the target's sorted points in LDS when they fit
                                      (6144 points); 0: they are read through L2.  Same results. */
} slam_kf_params;

/* why the iteration ended (pcl::registration::DefaultConvergenceCriteria's states) */
#define SLAM_KF_NOT_CONVERGED 0
#define SLAM_KF_ITERATIONS 1
#define SLAM_KF_TRANSFORM 2
#define SLAM_KF_ABS_MSE 3
#define SLAM_KF_REL_MSE 4
#define SLAM_KF_NO_CORRESPONDENCES 5

typedef struct {
    int   from, to;  /* keyframe ids: target = `from`, source = `to` (setInputSource(to_cld), setInputTarget(from_cld)) */
    float init[16];  /* 4 x 4 row-major: the Matrix4f handed to align() */
} slam_kf_edge_req;

typedef struct {
    float  transform[16];     /* getFinalTransformation(): the f64 result rounded once, row-major */
    double transform64[16];
    int    iterations, state; /* SLAM_KF_* */
    int    converged, pairs;  /* hasConverged(); pairs kept in the last iteration */
    double mse;               /* mean squared distance of those pairs */
    double information[36];   /* computeEdgeInformationLUM: M'M / s^2, or the identity (singular != 0) */
    int    num_corr, singular;
    float  ss;
    int    reserved;
} slam_kf_edge_result;

void slam_kf_default_params(slam_kf_params *p);
int  slam_kf_create(const slam_kf_params *params, slam_kf_t **out);
void slam_kf_destroy(slam_kf_t *s);
int  slam_kf_set_params(slam_kf_t *s, const slam_kf_params *params); /* leaf, gate and cell hold for later keyframes only:
                                                                         refused once the store holds one and they differ */
/* Filters the cloud (`stride` >= 3 floats per point, x y z first) and builds its search lattice; *id = 0, 1, 2, ... in order
 * of arrival.  The _dev form takes a device pointer.  Both wait for the work they enqueue on `stream`. */
int  slam_kf_add_keyframe(slam_kf_t *s, const float *xyz, int n, int stride, int *id);
int  slam_kf_add_keyframe_dev(slam_kf_t *s, const float *d_xyz, int n, int stride, int *id, slam_stream_t stream);
/* Lets go of keyframe `id`: its cloud, lattice and covariances are freed (waits for the device).  The id is never issued
 * again and slam_kf_count stays the number of ids issued; every later call that names the id returns SLAM_E_INVALID.  The
 * parameters that the store's keyframes had fixed (slam_kf_set_params, slam_kf_set_gicp_params) stay fixed. */
int  slam_kf_remove_keyframe(slam_kf_t *s, int id);
/* slam_kf_add_keyframe_dev's filter and lattice into the existing keyframe `id`; its covariances are dropped and computed
 * again on demand.  When the new cloud is refused the old keyframe stays.  Waits as slam_kf_add_keyframe_dev does. */
int  slam_kf_replace_keyframe_dev(slam_kf_t *s, int id, const float *d_xyz, int n, int stride, slam_stream_t stream);
/* n_points after the filter, occupied lattice cells, the largest cell, slots of the hash table, device bytes held */
int  slam_kf_keyframe_info(slam_kf_t *s, int id, int *n_points, int *n_cells, int *max_cell_points, int *table_slots,
                           long *device_bytes);
int  slam_kf_count(slam_kf_t *s);
/* the filtered cloud, 4 floats per point as slam_ccicp_voxel_downsample_dev writes them; room for max_points */
int  slam_kf_read_keyframe(slam_kf_t *s, int id, float *xyz4, int max_points, int *n_points);
/* The gated nearest neighbour of n device-resident queries in keyframe `id`: d_index[i] = index into the filtered cloud
 * or -1, d_dist2[i] = the f32 squared distance (kept when <= gate^2, or < gate^2 with strict != 0). */
int  slam_kf_nearest_dev(slam_kf_t *s, int id, const float *d_queries, int n, int stride, int strict, int32_t *d_index,
                         float *d_dist2, slam_stream_t stream);
/* Registers n_edges edges in one launch and waits for it; out[e] for req[e].  pairs_trace (optional, host): trace_cap ints
 * per edge, the pairs kept in each iteration (-1 behind the last). */
int  slam_kf_register_edges(slam_kf_t *s, const slam_kf_edge_req *req, int n_edges, slam_kf_edge_result *out,
                            slam_stream_t stream);
int  slam_kf_register_edges_traced(slam_kf_t *s, const slam_kf_edge_req *req, int n_edges, slam_kf_edge_result *out,
                                   int32_t *pairs_trace, int trace_cap, slam_stream_t stream);

/* Generalized ICP on the same store (pcl::GeneralizedIterativeClosestPoint, which global_matching's programs are built
 * on: global_match.cpp:52,225-235): a plane-to-plane cost from per-point covariances, one Gauss-Newton step per
 * iteration, a batch of requests in one launch.  docs/KF_GICP.md has the contract and its deviations from PCL. */
typedef struct {
    int    k_correspondences;      /* neighbours a covariance is taken over, the point included (20, PCL's); 4 .. 32 */
    double cov_radius;             /* neighbours lie within this radius; 0 = twice the edge of the search lattice */
    double gicp_epsilon;           /* the covariance along the normal, the other two being 1 (1e-3, PCL's) */
    int    max_iterations;         /* outer iterations (global_match.cpp:229: 10) */
    double transformation_epsilon; /* stop when no translation entry moved by more (1e-6) */
    double rotation_epsilon;       /* ... and no rotation entry by more than this (2e-3, PCL's) */
    int    cov_min_neighbours;     /* a point with fewer neighbours in the radius gets the identity (4) */
} slam_kf_gicp_params;

#define SLAM_KF_DEGENERATE 6 /* the Gauss-Newton step's 6 x 6 has a pivot that is not positive and finite */

typedef struct {
    slam_kf_edge_result edge;  /* transform, transform64, iterations, state (ITERATIONS, TRANSFORM, NO_CORRESPONDENCES,
                                  DEGENERATE), converged, pairs; mse = mean f32 d^2 of the last iteration's pairs; the LUM
                                  block on the f32 transform exactly as slam_kf_register_edges computes it */
    double cost;               /* sum r' M r / pairs of the last iteration */
    double hessian[36];        /* sum J' M J of the last iteration, unknowns (omega, v) */
    double fitness;            /* mean f32 d^2 of the source points, moved in f32 by the f32 transform, whose nearest
                                  target point lies strictly inside the gate (PCL's getFitnessScore is ungated) */
    int    fitness_pairs, reserved;
} slam_kf_gicp_result;

void slam_kf_gicp_default_params(slam_kf_gicp_params *p);
/* k_correspondences, cov_radius, gicp_epsilon and cov_min_neighbours are fixed once a keyframe holds covariances */
int  slam_kf_set_gicp_params(slam_kf_t *s, const slam_kf_gicp_params *params);
/* Per-point covariances of keyframe `id`; a second call does nothing.  A keyframe of fewer than k_correspondences points is
 * refused (SLAM_E_INVALID).  slam_kf_register_gicp calls it for every keyframe it touches that has none. */
int  slam_kf_compute_covariances(slam_kf_t *s, int id, slam_stream_t stream);
/* six doubles per point of the filtered cloud: xx xy xz yy yz zz; SLAM_E_INVALID before compute_covariances */
int  slam_kf_read_covariances(slam_kf_t *s, int id, double *cov6, int max_points, int *n_points);
/* the lists the covariances were summed over: per point *k indices into the filtered cloud (-1 behind the last) and f32
 * squared distances, ascending by (d^2, index), and the length of the list */
int  slam_kf_read_neighbours(slam_kf_t *s, int id, int32_t *index, float *dist2, int32_t *count, int max_points, int *k);
/* target = keyframe `from`, source = keyframe `to`, as slam_kf_register_edges; one workgroup per request, one launch, one
 * wait.  pairs_trace as there. */
int  slam_kf_register_gicp(slam_kf_t *s, const slam_kf_edge_req *req, int n, slam_kf_gicp_result *out, slam_stream_t stream);
int  slam_kf_register_gicp_traced(slam_kf_t *s, const slam_kf_edge_req *req, int n, slam_kf_gicp_result *out,
                                  int32_t *pairs_trace, int trace_cap, slam_stream_t stream);

/* Appearance-based loop-closure candidates on the same store, in the spirit of Scan Context (Kim & Kim, IROS 2018): per
 * keyframe a polar height descriptor of n_rings x n_sectors bytes (ring-major; 0 = empty cell, else 1 + the clamped height
 * bin of the cell's highest point), built from the filtered cloud, and an exhaustive exact search over all keyframes and
 * all yaw shifts.  Integer behind the binning: the device equals tests/cpp/sc_oracle.cpp bit for bit.  docs/SCAN_CONTEXT.md
 * has the contract. */
typedef struct {
    int    n_rings;   /* 20; 1 .. 32 */
    int    n_sectors; /* 64; a multiple of 4, 4 .. 128 */
    double max_range; /* 80.0; > 0.  Ring k ends at (k + 1) max_range / n_rings, the edge belonging to the ring outside */
    double z_min;     /* -2.0: the height of bin 0 */
    double z_step;    /* 0.02; > 0.  Heights clamp to bins 0 .. 254 */
} slam_kf_sc_params;

typedef struct {
    int distance; /* min over shifts of sum |a[r][c] - b[r][(c - shift) mod n_sectors]|; -1: removed keyframe, or the query */
    int shift;    /* the lowest shift that reaches it: the candidate rolled by +shift sectors lies on the query */
    int n_query, n_candidate, n_both; /* occupied cells of the query, of the candidate, of both at that shift */
} slam_kf_sc_match_t;

void slam_kf_sc_default_params(slam_kf_sc_params *p);
/* fixed once the first descriptor exists: a later call that changes a field is refused (SLAM_E_INVALID) */
int  slam_kf_set_sc_params(slam_kf_t *s, const slam_kf_sc_params *params);
/* The descriptor of keyframe `id`, or with id = -1 of every live keyframe that has none: one workgroup per keyframe, one
 * launch, one wait.  A second call does nothing; replacing a keyframe drops its descriptor. */
int  slam_kf_sc_compute(slam_kf_t *s, int id, slam_stream_t stream);
/* n_rings * n_sectors bytes into desc (room for cap); SLAM_E_INVALID before slam_kf_sc_compute */
int  slam_kf_sc_read(slam_kf_t *s, int id, uint8_t *desc, int cap, int *n_rings, int *n_sectors);
/* the tables the kernel bins by: edge2[n_rings] = squared ring edges, c[k], sn[k] = cos, sin(2 pi k / n_sectors) for
 * k < n_sectors / 4 (entry 0 is not used) */
int  slam_kf_sc_read_tables(slam_kf_t *s, double *edge2, double *c, double *sn);
/* out[q * slam_kf_count + id] = keyframe queries[q] against keyframe id, every id issued.  Missing descriptors are
 * computed first; then one upload, one launch (a workgroup per pair), one download, one wait. */
int  slam_kf_sc_match(slam_kf_t *s, const int *queries, int nq, slam_kf_sc_match_t *out, slam_stream_t stream);

/* -------------------------------------------------------------------------
 * Correlative scan matcher (Olson, ICRA 2009), class-constrained like the rest of ccicp2d: the best of N_theta x N_y x N_x
 * poses around a start pose by a score looked up in a rasterised model, found exactly by a two-level branch and bound.  The
 * reference has no such matcher; it is the wide-basin start for slam_icp_fit*.  docs/CSM.md has the
 * contract.  Everything behind the per-angle transform is integer: the device equals tests/cpp/csm_oracle.cpp bit for bit.
 * ---------------------------------------------------------------------- */
typedef struct slam_csm slam_csm_t;

typedef struct {
    double resolution;   /* pitch of the lattice in metres (0.1); cell(v) = floor(v / resolution) */
    double sigma;        /* standard deviation of the stamp in metres (0.2) */
    int    kernel_cells; /* K: the stamp is (2K+1) x (2K+1) cells; 0 = ceil(3 sigma / resolution - 1e-9) (6); at most 64 */
    int    block;        /* D: candidates per block and axis of the bound (8); 1 .. 16 */
    int    half_x;       /* N_x = 2 half_x + 1 translations of whole cells along x (40) */
    int    half_y;       /* (40) */
    int    half_theta;   /* N_theta = 2 half_theta + 1 angles (120) */
    double theta_step;   /* radians between two angles (0.01) */
    int    exhaustive;   /* 1 = no bound: every candidate is evaluated (measurements and tests; same answer) */
} slam_csm_params;

typedef struct {
    int k, a, b;          /* the winner: angle k, translation (a - half_x, b - half_y) cells; the lowest flat index
                             (k N_y + b) N_x + a among equal scores */
    int score;            /* its score; -1 = scan of fewer than 5 points, pose untouched */
    int max_score;        /* 255 n_points */
    int n_points;         /* points counted at angle k: of a class that has a table, finite, cells within +-2^30 */
    int blocks_evaluated; /* blocks evaluated at full resolution (a diagnostic; all of them with exhaustive = 1) */
} slam_csm_result;

void slam_csm_default_params(slam_csm_params *p);
/* The model arrays of slam_icp_create[_dev]: one table per class; a class of 3 points or fewer has none and scores nothing
 * (icpPointToPoint.cpp:59,93).  Both wait for the tables.  Scratch for one scan is reserved. */
int  slam_csm_create(const double *m_ga, int n_ga, const double *m_nga, int n_nga, const slam_csm_params *params, slam_csm_t **out);
int  slam_csm_create_dev(const double *d_m_ga, int n_ga, const double *d_m_nga, int n_nga, const slam_csm_params *params,
                         slam_csm_t **out);
void slam_csm_destroy(slam_csm_t *csm);
/* Scratch for batches of up to max_scans scans (bounds, survivor list, keys); the points are staged in pieces, so their
 * number needs none.  Waits for the device when it has to grow. */
int  slam_csm_reserve(slam_csm_t *csm, int max_scans);
/* Another search window (the tables stay); re-sizes the scratch as slam_csm_reserve does. */
int  slam_csm_set_window(slam_csm_t *csm, int half_x, int half_y, int half_theta, double theta_step);
int  slam_csm_set_exhaustive(slam_csm_t *csm, int exhaustive);
/* Host: cs[2 k], cs[2 k + 1] = cos, sin of theta_k = atan2(R0[2], R0[0]) + (k - half_theta) theta_step, N_theta pairs.  The
 * angles are the one floating-point input that libm decides, so the host computes them and the device reads them. */
int  slam_csm_angles(slam_csm_t *csm, const double R0[4], double *cs);
/* A batch of scans laid out as for slam_icp_fit_batch_from_dev; d_cs = n_scans x N_theta x 2 doubles from slam_csm_angles
 * for every scan's R0.  Writes the winner's pose to d_R / d_t (which may be d_R0 / d_t0) and d_result[s] (nullable).  A scan
 * of fewer than 5 points gets its initial pose and score -1.  Asynchronous on `stream`; allocates, frees and waits for
 * nothing (a graph may capture it); SLAM_E_INVALID beyond the reserved number of scans.  One call at a time per handle. */
int  slam_csm_match_batch_dev(slam_csm_t *csm, const double *d_pts, const int32_t *d_scan_off, const int32_t *d_scan_nga,
                              int n_scans, const double *d_R0, const double *d_t0, const double *d_cs, double *d_R, double *d_t,
                              slam_csm_result *d_result, slam_stream_t stream);
/* One scan on host pointers, synchronous, R and t in/out as slam_icp_fit; SLAM_E_TOO_FEW_SCENE_POINTS leaves them. */
int  slam_csm_match(slam_csm_t *csm, const double *t_ga, int n_tga, const double *t_nga, int n_tnga, double R[4], double t[2],
                    slam_csm_result *result);
/* The exhaustive form for one scan (n points, the first n_ga of class GA; d_t0: 2 doubles, d_cs: N_theta x 2): every score,
 * d_volume[(k N_y + b) N_x + a], int32.  Asynchronous. */
int  slam_csm_score_volume_dev(slam_csm_t *csm, const double *d_pts, int n, int n_ga, const double *d_t0, const double *d_cs,
                               int32_t *d_volume, slam_stream_t stream);
/* Table of class cls (0 = GA, 1 = NGA), level 0 = T, 1 = W (the bound): the lattice cell of its first byte, its size (0 x 0: the
 * class has no table) and, with buf, its w h bytes row by row (cap >= w h).  Synchronous. */
int  slam_csm_read_table(slam_csm_t *csm, int cls, int level, int *origin_x, int *origin_y, int *w, int *h, uint8_t *buf, size_t cap);
/* the parameters in force (kernel_cells resolved), N_theta N_x N_y and blocks per axis in dims[5], bytes of tables and scratch */
int  slam_csm_info(slam_csm_t *csm, slam_csm_params *params, int dims[5], size_t *table_bytes, size_t *scratch_bytes, int *max_scans);

/* A matcher whose table IS a byte plane (docs/GRID_MATCH.md): the cost plane a distance field computed with a likelihood table
 * (slam_grid_likelihood_table, slam_gdist_set_table), a saved map, any u8 image.  One table, read by both classes:
 * T[u, v] = plane[(u - origin_x) + w (v - origin_y)] inside the window and 0 outside; (origin_x, origin_y) is the lattice
 * cell of plane element (0, 0).  W is the same D x D slide.  sigma and kernel_cells are ignored (slam_csm_info reports 0:
 * the plane carries the kernel), the GA / NGA split of a scan makes no difference, and every search, posterior and volume
 * call runs as on a model-built handle.  The plane is copied; both wait for the tables.  SLAM_E_INVALID before the device is
 * touched: w or h < 1, (w + D)(h + D) beyond 2^28 bytes, a cell of T or W beyond +-2^30. */
int  slam_csm_create_from_plane(const uint8_t *plane, int w, int h, int origin_x, int origin_y, const slam_csm_params *params,
                                slam_csm_t **out);
int  slam_csm_create_from_plane_dev(const uint8_t *d_plane, int w, int h, int origin_x, int origin_y, const slam_csm_params *params,
                                    slam_csm_t **out);
/* Another plane of the SAME w x h (the call cannot see its size) at any origin: one copy and the slide, enqueued on `stream`.
 * Allocates nothing and waits for nothing, so it can stand behind slam_grid_distance_field on the grid's stream; a graph may
 * capture it (the origin is then the captured one, like every argument).  The origin takes effect for the calls made after
 * this one.  One call at a time per handle.  SLAM_E_INVALID on a handle made from a model. */
int  slam_csm_set_plane_dev(slam_csm_t *csm, const uint8_t *d_plane, int origin_x, int origin_y, slam_stream_t stream);
/* Scores of arbitrary poses (particles, hypotheses from elsewhere), on either kind of handle.  d_poses: n_poses x 4 doubles
 * (cos, sin, tx, ty), cos and sin from the host as with slam_csm_angles.  d_score[p] = sum over the scan's points of the
 * table byte of their class at cell(q), q = (c px - s py) + tx, (s px + c py) + ty, every operation rounded on its own;
 * d_counted[p] = the points that have a cell and a table (slam_csm_result's n_points): a point outside the table is counted
 * and scores 0, a non-finite pose counts 0 and scores 0.  n <= 2^23; n = 0 gives 0, 0 (no five-point rule); n_poses = 0
 * does nothing.  Asynchronous; allocates, frees and waits for nothing.  Where the poses form a lattice, the search calls
 * above are the faster tool: they share one rotation's cells between all translations. */
int  slam_csm_score_poses_dev(slam_csm_t *csm, const double *d_pts, int n, int n_ga, const double *d_poses, int n_poses,
                              int32_t *d_score, int32_t *d_counted, slam_stream_t stream);
/* the same on host pointers: stages and waits */
int  slam_csm_score_poses(slam_csm_t *csm, const double *pts, int n, int n_ga, const double *poses, int n_poses, int32_t *score,
                          int32_t *counted);

/* The match's posterior (docs/CSM.md section 6): every candidate whose score lies within a margin M of the winner's S* is
 * weighted by a table of exp(-beta d / M) in 16.16 fixed point, and the weights' integer moments about the winner give a
 * mean offset and a 3 x 3 covariance (index 0 = x, 1 = y, 2 = theta); the best candidate outside an exclusion box around
 * the winner is the second mode.  The set is enumerated exactly from the bound table (a block with U < S* - M holds no
 * member), the sums are int64, so the device equals tests/csm_post_oracle.py bit for bit in any order of evaluation. */
typedef struct {
    int    margin_per_point; /* M = margin_per_point * n_points, 0 .. 255 (16) */
    double beta;             /* the weight at deficit d is exp(-beta d / M); finite, 0 .. 64 (8.0) */
    int    excl_xy;          /* the second mode lies more than excl_xy cells off the winner along x or y ... (2) */
    int    excl_theta;       /* ... or more than excl_theta angular steps (2) */
} slam_csm_post_params;

typedef struct {
    int     valid;            /* 0 = scan of fewer than 5 points: everything else 0, second_score -1 */
    int     n_within;         /* candidates with S >= S* - M */
    int     margin;           /* M */
    int     blocks_evaluated; /* blocks evaluated at full resolution by the posterior pass (all of them with exhaustive = 1) */
    int     second_score;     /* the second mode: its score, -1 = none; the lowest flat index among equals */
    int     second_k, second_a, second_b;
    int64_t m0, m1[3], m2[6]; /* sums of w, w o_i, w o_i o_j over the set; o = (a - a*, b - b*, k - k*); m2: xx xy xt yy yt tt */
    double  mean[3];          /* the weighted mean's offset from the winner's pose: metres, metres, radians */
    double  cov[6];           /* xx xy xt yy yt tt in those units; no floor for the lattice's pitch (the adapters add it) */
} slam_csm_posterior;

void slam_csm_default_post_params(slam_csm_post_params *p);
/* Computes and uploads the 257 weights wtab[j] = rint(65536 exp(-(beta j) / 256)) (host libm, as the stamp) and sizes the
 * per-scan posterior scratch, which slam_csm_reserve sizes from then on as well.  May wait. */
int  slam_csm_set_post_params(slam_csm_t *csm, const slam_csm_post_params *p);
/* The table in force, 257 entries (cap >= 257); SLAM_E_INVALID before slam_csm_set_post_params. */
int  slam_csm_read_post_table(slam_csm_t *csm, uint32_t *wtab, int cap);
/* slam_csm_match_batch_dev (the same bits in d_R, d_t, d_result), then d_post[s] for every scan.  d_R may be d_R0, but d_t
 * may not be d_t0: the posterior pass reads the start translations again.  Asynchronous; allocates, frees and waits for
 * nothing.  SLAM_E_INVALID before slam_csm_set_post_params, beyond the reserved number of scans, and for
 * a window with 65536 (max(N_x, N_y, N_theta) - 1)^2 N_x N_y N_theta >= 2^63 (the int64 sums could overflow). */
int  slam_csm_match_post_batch_dev(slam_csm_t *csm, const double *d_pts, const int32_t *d_scan_off, const int32_t *d_scan_nga,
                                   int n_scans, const double *d_R0, const double *d_t0, const double *d_cs, double *d_R, double *d_t,
                                   slam_csm_result *d_result, slam_csm_posterior *d_post, slam_stream_t stream);
/* slam_csm_match with the posterior of its answer. */
int  slam_csm_match_post(slam_csm_t *csm, const double *t_ga, int n_tga, const double *t_nga, int n_tnga, double R[4], double t[2],
                         slam_csm_result *result, slam_csm_posterior *post);

/* -------------------------------------------------------------------------
 * Monte Carlo localisation over a grid matcher (docs/PARTICLE_FILTER.md): a particle filter whose likelihood step is
 * slam_csm_score_poses_dev as it stands.  The reference has no such filter (its ekf package fuses the scan matcher's pose), and
 * parity with AMCL or any outside filter is not claimed: the yardstick is the numpy restatement of tests/pf_cases.py, which
 * the device equals bit for bit, random numbers included.  Behind three host-made tables everything is integer or singly
 * rounded f64:
 *   state     per particle x, y (f64, world metres), k (int32 heading index in [0, A)), acc (int64 log-weight), as a
 *             structure of arrays on the device; the step counter t lives on the device too, so that a replayed graph advances it
 *   random    Philox-4x32-10, stateless: key = (low, high half of seed), counter = (p, t, purpose, 0); purpose 0 = predict,
 *             1 = init, 2 = the resampling offset (p = 0)
 *   limits    1 <= n_particles <= 2^18 and weights <= 2^16, chosen so that every integer sum below fits 64 bits:
 *             W < 2^35, S2 < 2^51, |MX|, |MY| < 2^63 (|q| < 2^29), |MC|, |MS| < 2^59, and C_i n, j W + r < 2^54
 * ---------------------------------------------------------------------- */
typedef struct slam_pf slam_pf_t;

typedef struct {
    int      n_particles;   /* 1 .. 2^18; default 1024 */
    int      n_angles;      /* A: headings per turn, a power of two from 2^6 to 2^16; default 4096 */
    int      gauss_bits;    /* b: the Gaussian table has 2^b entries, 4 .. 16; default 12 */
    int      weight_len;    /* L: entries of the weight table, 2 .. 65536; default 1024 */
    int      weight_shift;  /* a weight is looked up at (A_max - acc) >> weight_shift, 0 .. 14; default 4 */
    double   weight_scale;  /* the weight at deficit d is exp(-d / weight_scale); positive and finite; default 1024.0 */
    int      resample_num;  /* resample iff N_eff < (num / den) n; 0 never, num > den always; 0 .. 65535; default 1 */
    int      resample_den;  /* 1 .. 65535; default 2 */
    uint64_t seed;          /* the Philox key; default 1 */
} slam_pf_params;
/* A motion, on the host and as the predict kernel reads it on the device: 48 bytes */
typedef struct {
    double  dx, dy;         /* the odometry increment in the particle's own frame, metres */
    double  sx, sy;         /* standard deviations of its noise, metres; finite, >= 0 */
    double  sk;             /* standard deviation of the heading noise in heading steps; finite, 0 <= sk < 2^20 */
    int32_t dk;             /* the heading increment in heading steps, |dk| < 2^20 */
    int32_t reserved;       /* not read */
} slam_pf_motion;
typedef struct {
    int64_t t;              /* the step counter: predicts done (mod 2^32) */
    int64_t n;              /* n_particles */
    int64_t resampled;      /* the last update resampled */
    int64_t degenerate;     /* the last update found no finite particle: nothing moved, every sum is 0, best is -1 */
    int64_t best;           /* the lowest index whose acc reached A_max (before a resample zeroed it) */
    int64_t refused;        /* motions slam_pf_predict_dev found invalid on the device and skipped (the step did not advance) */
    int64_t n_resamples;    /* updates that resampled since creation */
    int64_t A_max;          /* the largest acc among the finite particles */
    int64_t W, S2;          /* sum w, sum w^2 */
    int64_t MX, MY;         /* sum w q(x), sum w q(y); q(v) = llrint(65536 v) saturated to +-(2^29 - 1) */
    int64_t MC, MS;         /* sum w llrint(2^24 cos), sum w llrint(2^24 sin) of the heading */
    double  x, y, theta;    /* the estimate, formed on the host: MX / (W 65536), MY / (W 65536), atan2(MS, MC); NaN when W = 0 */
} slam_pf_state;

void slam_pf_default_params(slam_pf_params *p);
/* The table makers (slam_amd/csrc/pf_tables.hpp; host only, no device is touched).  SLAM_E_INVALID and nothing written:
 *   angle   n_angles not a power of two in 2^6 .. 2^16, n != 2 n_angles.  cs[2 k], cs[2 k + 1] = cos, sin(2 pi k / n_angles);
 *           the four quadrant entries are exactly (+-1, 0) and (0, +-1)
 *   gauss   bits outside 4 .. 16, n != 2^bits.  G[i] = Phi^-1((i + 1/2) / 2^bits); G[i] == -G[2^bits - 1 - i] exactly.  No bit
 *           contract against any library: |Phi(G[i]) - (i + 1/2) / 2^bits| <= 1e-12
 *   weight  L outside 2 .. 65536, shift outside 0 .. 14, a scale that is not positive and finite.
 *           wtab[j] = (uint32_t)rint(65536 exp(-(double)(j << shift) / scale)); wtab[0] == 65536 and no entry above it */
int  slam_pf_angle_table(int n_angles, double *cs, int n);
int  slam_pf_gauss_table(int bits, double *G, int n);
int  slam_pf_weight_table(double scale, int shift, int L, uint32_t *wtab);
/* A filter with the three tables made from its parameters; the particles are all at (0, 0, 0) with acc 0, t = 0.  Every
 * refusal of a parameter is SLAM_E_INVALID before a device is touched. */
int  slam_pf_create(const slam_pf_params *p /* NULL: the defaults */, slam_pf_t **out);
void slam_pf_destroy(slam_pf_t *pf);
/* Other tables of the right lengths (2 n_angles, 2^gauss_bits, weight_len); a null table stays as it is.  cs and G must be
 * finite, wtab[0] == 65536 with no entry above it.  Synchronous. */
int  slam_pf_set_tables(slam_pf_t *pf, const double *cs, int n_cs, const double *G, int n_G, const uint32_t *wtab, int n_w);
/* Particles from and to the host, n == n_particles, synchronous.  set: every k in [0, A), every acc becomes 0 (x, y may be
 * non-finite: such a particle takes no part in an update).  read: each array nullable. */
int  slam_pf_set_particles(slam_pf_t *pf, const double *x, const double *y, const int32_t *k, int n);
int  slam_pf_read_particles(slam_pf_t *pf, double *x, double *y, int32_t *k);
/* acc (int64) and the weights w (uint32) of the last update, each nullable; synchronous */
int  slam_pf_read_weights(slam_pf_t *pf, int64_t *acc, uint32_t *w);
/* The step counter, the last update's sums and flags, and the estimate; synchronous */
int  slam_pf_read_state(slam_pf_t *pf, slam_pf_state *state);
/* Debug: d_words[4 i ..] = the four Philox words of counter (p0 + i, t, purpose, 0), i < n <= 2^20, under the filter's key.
 * Enqueued on the null stream. */
int  slam_pf_random_words_dev(slam_pf_t *pf, uint32_t p0, int n, uint32_t t, uint32_t purpose, uint32_t *d_words);
/* The motion model.  With (w0 .. w3) the particle's words of purpose 0, g(w) = G[w >> (32 - b)] and c, s = cs[k] of the OLD
 * heading, every product and sum rounded on its own:
 *     ex = dx + sx g(w0)          x' = x + (c ex - s ey)
 *     ey = dy + sy g(w1)          y' = y + (s ex + c ey)          k' = (k + dk + (int)rint(sk g(w2))) mod A
 * and t advances by one at the end.  The motion is read from the device, so that a graph can be fed new odometry; one that
 * breaks the motion's rules above is found on the device: nothing moves, t stays, and the state's `refused` counts it.
 * Asynchronous on `stream`; allocates, frees and waits for nothing.  One call at a time per handle. */
int  slam_pf_predict_dev(slam_pf_t *pf, const slam_pf_motion *d_motion, slam_stream_t stream);
/* the same from the host: an invalid motion is SLAM_E_INVALID before a device is touched; stages and waits */
int  slam_pf_predict(slam_pf_t *pf, const slam_pf_motion *motion);
/* Every particle becomes the pose (x, y, k) moved by the motion {0, 0, sx, sy, sk, 0} drawn with purpose 1 at the current t
 * (the noise lies in the pose's own frame); acc = 0; t stays.  Synchronous. */
int  slam_pf_init_gaussian(slam_pf_t *pf, double x, double y, int k, double sx, double sy, double sk);
/* The measurement step against a matcher's table, the scan as for slam_csm_score_poses_dev (n <= 2^23 points, the first n_ga
 * of class GA); (cx, cy), finite, is the centre of the matcher's window in the world frame.  In order:
 *   1  poses (c, s, x - cx, y - cy) per particle          2  slam_csm_score_poses_dev as it is          3  acc += score
 *   4  a particle whose x or y is not finite takes no part and has weight 0; A_max = max acc over the others, best = the
 *      lowest index that reaches it
 *   5  w_p = wtab[min((A_max - acc_p) >> shift, L - 1)]   6  the sums of the state
 *   7  resample iff W W den < num n S2 (128-bit); no finite particle: degenerate, nothing moves
 *   8  when decided: r = ((w0 << 32) | w1) mod W from purpose 2 at the current t, C_i = the inclusive prefix sum of w, output j
 *      copies x, y, k of src(j) = min { i : C_i n > j W + r }, every acc becomes 0; when not decided nothing changes.
 * Asynchronous on `stream`; allocates, frees and waits for nothing; a graph may capture predict + update.  One call at a
 * time per handle and per matcher. */
int  slam_pf_update_dev(slam_pf_t *pf, slam_csm_t *csm, const double *d_pts, int n, int n_ga, double cx, double cy, slam_stream_t stream);
/* the same on host points: stages and waits */
int  slam_pf_update(slam_pf_t *pf, slam_csm_t *csm, const double *pts, int n, int n_ga, double cx, double cy);
/* The resampling rule alone: d_src[j] = min { i : C_i n > j W + (r mod W) } for j < n, from n <= n_particles weights
 * (uint32; one above 65536 is read as 65536).  W = 0: d_src[j] = j.  Shares the filter's scratch.  Asynchronous. */
int  slam_pf_resample_indices_dev(slam_pf_t *pf, const uint32_t *d_w, int n, uint64_t r, int32_t *d_src, slam_stream_t stream);

/* -------------------------------------------------------------------------
 * Exact sparse voxel map: the growing prior map of global_generate.cpp (the reference keeps it as a point cloud that is
 * voxel-filtered again every round, global_generate.cpp:122-232).  Clouds are integrated in place into an open-addressing
 * table in HBM; a voxel holds a point count and three integer sums of the coordinates in units of 2^-20 m, so the map of a
 * set of (cloud, transform) pairs is the same bits in any order of clouds, points and threads.  docs/VOXEL_MAP.md has the
 * contract; the device equals tests/cpp/vmap_oracle.cpp bit for bit.
 *   point     q = (float)(((r0 x + r1 y) + r2 z) + t) per axis in double without contraction (slam_grid_transform_cloud_dev's
 *             arithmetic); q = p without a transform
 *   cell      (int32) floor((double) q / leaf); a point is dropped (and counted) when a coordinate is not finite or
 *             |q| >= 2^22, or |cell| >= 2^20 on any axis
 *   key       (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20); all ones = empty
 *   sums      int64 of rint((double) q * 2^20) (to nearest even) per axis: exact while a voxel holds fewer than 2^21 points
 *   centroid  (float)(((double) S / (double) count) * 2^-20)
 * ---------------------------------------------------------------------- */
typedef struct slam_vmap slam_vmap_t;

typedef struct {
    double leaf;             /* edge of a voxel in metres (0.30, LEAF_SIZE of global_generate.cpp:26) */
    int    initial_capacity; /* slots of the first table (65536), rounded up to a power of two, at least 64; at most 2^30 */
} slam_vmap_params;

void slam_vmap_default_params(slam_vmap_params *p);
int  slam_vmap_create(const slam_vmap_params *params, slam_vmap_t **out);
void slam_vmap_destroy(slam_vmap_t *m);
/* Empties the map and keeps the table's size.  Asynchronous on `stream`.  One call at a time per handle (the table). */
int  slam_vmap_clear(slam_vmap_t *m, slam_stream_t stream);
/* n points, `stride` floats apart (>= 3), moved by R (9 doubles, row-major) and t (3 doubles) when both are given, neither
 * otherwise.  A call that does not grow the table WAITS ONCE for `stream`, to read the voxel count, the dropped points
 * (*n_dropped, nullable) and the error word back.  The host keeps the table at most half full: when
 * n_voxels + n > capacity / 2 the call first rehashes the table into one at least twice the size, in a launch of its own.
 * Such a growing call waits THREE times and synchronises the whole device: for `stream` after the rehash (to check that every
 * voxel arrived), for the device when the old table is freed, and for the counters as above.  A probe that ran out of table is
 * SLAM_E_HIP (it cannot happen under the load rule).  One call at a time per handle. */
int  slam_vmap_integrate_dev(slam_vmap_t *m, const float *d_xyz, int n, int stride, const double R[9], const double t[3],
                             int *n_dropped, slam_stream_t stream);
int  slam_vmap_integrate(slam_vmap_t *m, const float *xyz, int n, int stride, const double R[9], const double t[3], int *n_dropped);
/* The voxels with count >= min_count whose centroid c has lo_xy[0] <= c.x <= hi_xy[0] and lo_xy[1] <= c.y <= hi_xy[1] in f32
 * (both ends kept, as pcl::PassThrough; lo_xy = hi_xy = NULL: everything), in ascending key order: d_xyz4[4 i ..] =
 * (x, y, z, 0) and, where given, d_count[i] (uint32) and d_key[i] (uint64).  *n_out is the number of such voxels; when it
 * exceeds `cap` nothing is written and the call returns SLAM_E_NOMEM.  WAITS ONCE for `stream`, to read that number; the
 * sort and the writes that follow are asynchronous.  The first call after the table grew, or with more voxels than any call
 * before, regrows the handle's scratch, which frees the old blocks and so waits for the whole device besides.  One call at a
 * time per handle: it shares the scratch and the table with integrate and clear. */
int  slam_vmap_extract_dev(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, float *d_xyz4,
                           uint32_t *d_count, uint64_t *d_key, int cap, int *n_out, slam_stream_t stream);
/* The same into host arrays (each nullable), synchronous. */
int  slam_vmap_read(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, float *xyz4, uint32_t *count,
                    uint64_t *key, int cap, int *n_out);
/* The accumulators themselves, for tests and for saving a map (slam_vmap_save does): every occupied voxel in ascending key order, sums[3 i ..] =
 * the three int64 sums in units of 2^-20 m.  Host arrays, each nullable; synchronous; `cap` and *n_out as above. */
int  slam_vmap_read_sums(slam_vmap_t *m, int64_t *sums, uint32_t *count, uint64_t *key, int cap, int *n_out);
/* occupied voxels, slots of the table, points integrated (dropped ones not counted), bytes of device memory held */
int  slam_vmap_info(slam_vmap_t *m, int64_t *n_voxels, int64_t *capacity, int64_t *n_points, size_t *device_bytes);

/* Free-space carving (docs/VOXEL_MAP.md section 8; the device equals tests/cpp/vmap_carve_oracle.cpp bit for bit).  Two more
 * u32 accumulators per voxel, in units of scans: `seen` counts the carve calls whose cloud had an endpoint in the voxel,
 * `miss` those in which a ray crossed it and no endpoint of that cloud lay in it.  A carve call touches only voxels that
 * exist: nothing is claimed.
 *   endpoint  q as slam_vmap_integrate moves and drops it; origin O = the same arithmetic on `origin` (NULL: 0, 0, 0)
 *   ray       c0 = cell(O), c1 = cell(q), a_k = |c1_k - c0_k|, n = max a_k; the cell of step i is
 *             c0_k + s_k floor((2 a_k i + n - 1) / (2 n)) per axis (the driving-axis 3-D Bresenham)
 *   visited   i = 0 .. n - T - 1 with T = max(end_margin, ceil(n tail_num / tail_den)); n > max_ray_cells: not walked
 *   phases    (1) every voxel holding an endpoint: seen += 1 once; (2) every other voxel visited: miss += 1 once
 * The planes are allocated at the first carve; a map never carved holds what it held before and answers with zeros. */
typedef struct {
    int end_margin;    /* steps before the end cell that are never visited, at least (1) */
    int tail_num;      /* the last ceil(n tail_num / tail_den) steps of a ray of n steps are not visited (1 / 8) */
    int tail_den;
    int max_ray_cells; /* a ray of more steps is not walked and counted in n_skipped (512) */
} slam_vmap_carve_params;

typedef struct {
    int64_t n_rays;    /* endpoints kept (n - n_dropped), skipped rays included */
    int64_t n_dropped; /* points dropped by integrate's rules */
    int64_t n_skipped; /* rays longer than max_ray_cells */
    int64_t n_steps;   /* cells visited, existing voxels or not */
    int64_t n_seen;    /* voxels charged in phase 1 */
    int64_t n_missed;  /* voxels charged in phase 2 */
} slam_vmap_carve_result;

void slam_vmap_default_carve_params(slam_vmap_carve_params *p);
/* Points, stride, R and t as slam_vmap_integrate_dev; origin: 3 doubles in the cloud's frame or NULL; params NULL: the
 * defaults; result nullable.  SLAM_E_INVALID before anything is launched for stride < 3, tail_den <= 0, a negative
 * end_margin or tail_num, max_ray_cells < 1, one of R / t without the other, and an origin that has no cell.  WAITS ONCE for
 * `stream`, to read the counters (the first carve allocates the planes; a call with more rays than any before regrows its
 * scratch, which waits for the device besides).  One call at a time per handle. */
int  slam_vmap_carve_dev(slam_vmap_t *m, const float *d_xyz, int n, int stride, const double R[9], const double t[3],
                         const double origin[3], const slam_vmap_carve_params *params, slam_vmap_carve_result *result,
                         slam_stream_t stream);
int  slam_vmap_carve(slam_vmap_t *m, const float *xyz, int n, int stride, const double R[9], const double t[3], const double origin[3],
                     const slam_vmap_carve_params *params, slam_vmap_carve_result *result);
/* slam_vmap_extract_dev and slam_vmap_read with one test more: a voxel is kept iff
 * (uint64) miss * max_miss_den <= (uint64) max(seen, 1) * max_miss_num, equality kept (num >= 0, den > 0; 1 / 1 keeps a voxel
 * hit at least as often as crossed). */
int  slam_vmap_extract_carved_dev(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, int max_miss_num,
                                  int max_miss_den, float *d_xyz4, uint32_t *d_count, uint64_t *d_key, int cap, int *n_out,
                                  slam_stream_t stream);
int  slam_vmap_read_carved(slam_vmap_t *m, const float lo_xy[2], const float hi_xy[2], int min_count, int max_miss_num, int max_miss_den,
                           float *xyz4, uint32_t *count, uint64_t *key, int cap, int *n_out);
/* seen and miss of every occupied voxel in ascending key order, as slam_vmap_read_sums; zeros on a map never carved. */
int  slam_vmap_read_carve(slam_vmap_t *m, uint32_t *seen, uint32_t *miss, uint64_t *key, int cap, int *n_out);

/* Per-voxel plane distributions and Generalized ICP straight against the map (docs/VOXEL_MAP.md section 9; the device
 * equals tests/cpp/vmap_gicp_oracle.cpp: moments and distributions bit for bit, the registration as docs/KF_GICP.md holds
 * the store's).  Opt-in: nine more int64 accumulators per voxel, in units of 2^-16 m and 2^-32 m^2 from the cell's corner.
 *   L         (int64) rint(leaf 2^20); fx = the point's term of the sums, rint((double) q 2^20)
 *   e_k       floor((fx_k - cell_k L) / 16): an arithmetic shift by 4
 *   moments   E_k += e_k (3), M_kl += e_k e_l for xx xy xz yy yz zz (6): exact while a voxel holds fewer than 2^21 points
 *   plane     m_k = (double) E_k / n, C_kl = ((double) M_kl / n - m_k m_l) 2^-32, every operation rounded on its own; the
 *             Jacobi decomposition of slam_kf_compute_covariances gives l0 >= l1 >= l2 and the normal; a voxel is a plane
 *             voxel iff count >= min_points, l1 >= flat_ratio l2, l1 >= line_ratio l0 and, when max_miss_den > 0, it
 *             passes slam_vmap_extract_carved_dev's rule; its covariance is (I - n n') + epsilon n n' */
typedef struct {
    int    min_points;   /* fewest points of a plane voxel (6) */
    double flat_ratio;   /* l1 >= flat_ratio l2 (4.0) */
    double line_ratio;   /* l1 >= line_ratio l0 (0.01) */
    double epsilon;      /* the covariance along the normal, as slam_kf_gicp_params.gicp_epsilon (1e-3) */
    int    max_miss_num; /* with max_miss_den > 0: a voxel failing the carved rule miss den <= max(seen, 1) num is no plane */
    int    max_miss_den; /* voxel either; 0 (default): the carve planes are ignored */
} slam_vmap_dist_params;

void slam_vmap_default_dist_params(slam_vmap_dist_params *p);
/* Legal only on a map with no voxels (after create or clear) and leaf <= 8 m: SLAM_E_INVALID otherwise.  params NULL: the
 * defaults.  Allocates the planes at the table's size; slam_vmap_params is not touched.  A second call on an empty map
 * replaces the parameters.  Synchronous: the planes are cleared on the null stream before it returns. */
int  slam_vmap_enable_distributions(slam_vmap_t *m, const slam_vmap_dist_params *params);
/* E[3 i ..] and M[6 i ..] of every occupied voxel in ascending key order, as slam_vmap_read_sums; SLAM_E_INVALID on a map
 * without distributions.  Host arrays, each nullable; synchronous. */
int  slam_vmap_read_moments(slam_vmap_t *m, int64_t *E3, int64_t *M6, uint64_t *key, int cap, int *n_out);
/* One lane per slot: centroid, normal, covariance, eigenvalues and flag of every voxel from its moments.  Idempotent;
 * does nothing when no integrate, clear, rehash or carve has happened since the last call.  Asynchronous on `stream`. */
int  slam_vmap_compute_distributions(slam_vmap_t *m, slam_stream_t stream);
/* Per occupied voxel in ascending key order: centroid (3 floats), normal (3 doubles), cov6 (xx xy xz yy yz zz), eigenvalues
 * (l0 l1 l2) and flag (1: plane voxel; the normal and cov6 of other voxels are zero).  Computes the distributions when
 * they are stale.  Host arrays, each nullable; synchronous. */
int  slam_vmap_read_distributions(slam_vmap_t *m, float *centroid3, double *normal3, double *cov6, double *eig3, uint8_t *flag,
                                  uint64_t *key, int cap, int *n_out);

typedef struct {
    int   src;      /* keyframe id of the store: its filtered cloud is the source */
    float init[16]; /* 4 x 4 row-major, as slam_kf_edge_req */
} slam_vmap_gicp_req;

typedef struct {
    double gate;                   /* a pair's centroid lies strictly inside this distance (2.0); the candidates are those of
                                      the 27 cells around the moved point whatever the gate */
    int    max_iterations;         /* 100 */
    double transformation_epsilon; /* 1e-6 */
    double rotation_epsilon;       /* 2e-3 */
} slam_vmap_gicp_params;

typedef struct {
    float  transform[16];     /* the f64 result rounded once, row-major */
    double transform64[16];
    int    iterations, state; /* SLAM_KF_ITERATIONS, _TRANSFORM, _NO_CORRESPONDENCES (fewer than 3 pairs), _DEGENERATE */
    int    converged, pairs;  /* pairs kept in the last iteration */
    double mse;               /* mean f32 d^2 (to the centroid) of those pairs */
    double cost;              /* sum r' M r / pairs of the last iteration */
    double hessian[36];       /* sum J' M J of the last iteration */
    double fitness;           /* one last pass with the f32 transform, points moved in f32: the mean over its pairs of
                                 (n . (q - x))^2 in f64, a point-to-plane score */
    int    fitness_pairs, reserved;
} slam_vmap_gicp_result;

void slam_vmap_default_gicp_params(slam_vmap_gicp_params *p);
/* Registers keyframe req[e].src of `store` against the plane voxels of `m` by the plane-to-plane Gauss-Newton iteration of
 * docs/KF_GICP.md section 1.2.  The pairs: x = the source point moved by T in f64, rounded to f32; candidates are the plane
 * voxels among the 27 cells around cell(x); d^2 to the stored centroid in f32; the winner is the smallest (d^2, key) and is
 * kept iff (double) d^2 < gate^2.  Source covariances are the store's, computed on demand.  One workgroup per request, one
 * launch.  SLAM_E_INVALID before any launch for a map without distributions, a dead keyframe id, gate <= 0,
 * max_iterations < 1, n < 0 or a null pointer.  WAITS ONCE for `stream`, for the results (and once per keyframe whose
 * covariances are computed first); stale distributions are computed on `stream` before the launch, without a wait.
 * pairs_trace (optional, host): trace_cap ints per request, the pairs of each iteration (-1 behind the last). */
int  slam_vmap_register_gicp(slam_vmap_t *m, slam_kf_t *store, const slam_vmap_gicp_req *req, int n,
                             const slam_vmap_gicp_params *params, slam_vmap_gicp_result *out, slam_stream_t stream);
int  slam_vmap_register_gicp_traced(slam_vmap_t *m, slam_kf_t *store, const slam_vmap_gicp_req *req, int n,
                                    const slam_vmap_gicp_params *params, slam_vmap_gicp_result *out, int32_t *pairs_trace,
                                    int trace_cap, slam_stream_t stream);

/* Snapshots and merging by the integer accumulators (docs/VOXEL_MAP.md section 10).  A voxel record is what the key-ordered
 * readers return: key (section 1's packing), count >= 1, sums[3], optionally seen and miss (slam_vmap_read_carve), optionally
 * E[3] and M[6] (slam_vmap_read_moments).  ABSORB adds records into a map by key: find or claim the key's slot as integrate
 * does, then integer atomic adds of count and sums and, where the planes exist, of seen, miss, E and M.  Keys may repeat
 * within a call and across calls: repeats add.  A record is rejected, counted in *n_rejected and nothing is written for it
 * when its key is all ones, has bit 63 set or a 21-bit field above 2^21 - 2, or its count is 0; the call still returns SLAM_OK.
 * n_voxels grows by the slots claimed, n_points by the counts accepted, the distributions become stale.  Two maps of equal leaf
 * built from disjoint sets of (cloud, transform) pairs therefore absorb, in any order, into the bits of the map one handle
 * would have built from all pairs.  seen and miss add as well; that sum is a joint carve's only for voxels every contributing
 * map held when each carve ran (section 10.1).  Section 1's limits hold for the totals and are not checked.
 * Moments travel exactly: records with E / M into a map without distributions, or without into a map with them, is
 * SLAM_E_INVALID and nothing is launched.  seen / miss offered to a map never carved allocates the carve planes as a first
 * carve does; records without them add nothing to a carved map's planes. */
/* leaf, whether the carve planes exist, whether distributions are enabled and their parameters (zeros when not): each
 * output nullable, no wait. */
int  slam_vmap_layout(slam_vmap_t *m, double *leaf, int *carved, int *distributions, slam_vmap_dist_params *dp);
/* n records on the device: d_sums[3 i + k], d_E3[3 i + k], d_M6[6 i + k]; d_seen / d_miss both or neither, d_E3 / d_M6
 * likewise.  SLAM_E_INVALID before any launch for n < 0, a null key / count / sums with n > 0, half a pair, or the moment
 * mismatch above; n == 0 is SLAM_OK and touches nothing.  Room is made by integrate's load rule with n the number of records,
 * before the launch.  WAITS ONCE for `stream`, for the counters; a growing call waits as a growing integrate does.  One call
 * at a time per handle.  The host form stages the arrays as slam_vmap_integrate does and is synchronous. */
int  slam_vmap_absorb_dev(slam_vmap_t *m, const uint64_t *d_key, const uint32_t *d_count, const int64_t *d_sums, const uint32_t *d_seen,
                          const uint32_t *d_miss, const int64_t *d_E3, const int64_t *d_M6, int n, int64_t *n_rejected, slam_stream_t stream);
int  slam_vmap_absorb(slam_vmap_t *m, const uint64_t *key, const uint32_t *count, const int64_t *sums, const uint32_t *seen,
                      const uint32_t *miss, const int64_t *E3, const int64_t *M6, int n, int64_t *n_rejected);
/* Absorbs every occupied slot of `src` straight from its table (one lane per slot, no extraction, no sort); src's carve planes
 * travel when it has them; src is unchanged.  SLAM_E_INVALID before any launch for dst == src, leaves whose doubles differ in
 * any bit, or distributions on one side only.  Waits as slam_vmap_absorb_dev with n = src's n_voxels; both handles are busy
 * for the call. */
int  slam_vmap_merge(slam_vmap_t *dst, slam_vmap_t *src, int64_t *n_rejected, slam_stream_t stream);
/* The map into the file of section 10.4 (96-byte header, then keys, counts, sums, seen and miss of a carved map, E and M of
 * a map with distributions, all in ascending key order, little-endian, no checksum) through slam_vmap_read_sums,
 * slam_vmap_read_carve and slam_vmap_read_moments.  Synchronous.  The bytes depend on the map's contents only, not on how it
 * was built.  SLAM_E_IO when the file cannot be written; SLAM_E_INVALID for a map the format cannot hold (more than 2^30
 * voxels, a cell of 2^20 - 1). */
int  slam_vmap_save(slam_vmap_t *m, const char *path);
/* Parses and validates the whole file on the host (SLAM_E_IO: unreadable; SLAM_E_INVALID: malformed, on a machine without a
 * device as well), then asks for the device, creates a map of the file's leaf with room for its voxels at half load, enables
 * distributions with the file's parameters when it has moments, and absorbs the records in one call. */
int  slam_vmap_load(const char *path, slam_vmap_t **out);
/* Exact coarser levels (docs/VOXEL_MAP.md section 11).  Adds every voxel of `src` into the voxel of `dst` that contains it:
 * dst's leaf must equal ldexp(src's leaf, j) bit for bit for some 1 <= j <= 8.  Per axis the parent cell is cell >> j (an
 * arithmetic shift: cell -1 goes to -1), the parent key section 1's packing; count and the three sums add unchanged; the
 * moments are re-centred on the parent's corner in int64: with o_k = cell_k - (parent_k << j) and s_k = o_k (L / 16),
 * E'_k += E_k + n s_k and M'_kl += M_kl + s_k E_l + s_l E_k + n s_k s_l.  Because doubling a leaf is exact, the result holds
 * the keys, counts, sums and moments of a map that integrated the same (cloud, transform) pairs at dst's leaf, provided src's
 * leaf dropped none of their points.  dst may hold voxels already (coarsen adds, as absorb does); n_voxels grows by the slots
 * claimed, n_points by the counts, the distributions become stale; src is unchanged.  Carve planes are not derived (seen and
 * miss count scans, and a scan seen in two children is one scan of the parent): dst's, if it has any, are not touched.
 * SLAM_E_INVALID before any launch for dst == src, any other pair of leaves (equal leaves are a merge), distributions on one
 * side only, and moments on a src leaf that is no multiple of 2^-16 m (floor(d / 16) does not split).  Room is made by
 * integrate's load rule with n = src's n_voxels, before the launch.  Waits as slam_vmap_merge does; both handles are busy for
 * the call. */
int  slam_vmap_coarsen(slam_vmap_t *dst, slam_vmap_t *src, slam_stream_t stream);

/* Exhaustive lattice pose search (docs/VOXEL_MAP.md section 13; the device equals tests/vmap_search_cases.py bit for bit):
 * "here is a scan, here is the map, where am I?" without a prior.  Opt-in; the map is not written.
 *   rotation  k of n_yaw is the f32 matrix planar(cx, cy, yaw_k) with cz as its z translation, yaw_k =
 *             (float)((double) yaw0 + 2 pi k / n_yaw), cos and sin in double of the float angle and rounded to float; the
 *             kernels see its entries promoted to double
 *   cell      point i under rotation k is moved by section 1's rule, q = (float)(((r0 x + r1 y) + r2 z) + t) in double, and
 *             takes section 1's cell at the map's leaf; a point without a cell counts nowhere for that rotation
 *   pose      (k, dx, dy, dz) with |dx| <= wx, |dy| <= wy, |dz| <= wz whole cells; its score is the number of points i whose
 *             cell c_ik + d holds a qualifying voxel (a cell with |c + d| >= 2^20 on an axis holds none)
 *   qualify   planes_only = 1: the voxel's distribution flag is 1 (section 9's plane rule, stale distributions are computed
 *             first on the stream); planes_only = 0: count >= min_count, legal on any map
 *   volume    int32 [n_yaw][2 wz + 1][2 wy + 1][2 wx + 1], dx fastest; it stays on the device unless the caller asks for it
 *   hits      up to top_m, greedily: the best remaining pose has the highest score, then the lowest flat index; once chosen
 *             it suppresses every pose with cyclic |dk| <= nms_yaw and |dd| <= nms_cells on all three axes; a pose of
 *             score 0 is never a hit */
typedef struct {
    float yaw0;         /* 0 */
    int   n_yaw;        /* 64 */
    float cx, cy, cz;   /* the window's centre: the translation of every rotation (0, 0, 0) */
    int   wx, wy, wz;   /* half-widths in cells (24, 24, 0) */
    int   planes_only;  /* 1 */
    int   min_count;    /* with planes_only = 0 (6) */
    int   top_m;        /* 4; at most 4096 */
    int   nms_yaw;      /* 2 */
    int   nms_cells;    /* 2 */
} slam_vmap_search_params;

typedef struct {
    int   score;        /* points whose cell holds a qualifying voxel */
    int   k, dx, dy, dz;
    int   n_with_cell;  /* points that had a cell under rotation k */
    float init[16];     /* planar((float)((double) cx + dx leaf), (float)((double) cy + dy leaf), yaw_k) with z
                           (float)((double) cz + dz leaf), row-major: the pose the offset stands for.  Moving the cloud by it
                           need not reproduce c + d for every point: the floats round */
} slam_vmap_search_hit;

void slam_vmap_default_search_params(slam_vmap_search_params *p);
/* n device points `stride` floats apart.  hits: room for top_m (nullable when top_m is 0); *n_hits: how many were found;
 * volume (optional, host): the whole score volume.  SLAM_E_INVALID before any launch for a null map, n < 0, stride < 3, null
 * points with n > 0, n_yaw < 1, a negative half-width, top_m < 0 or above 4096, negative nms_yaw or nms_cells, a null n_hits,
 * null hits with top_m > 0, n_yaw (2 wx + 1)(2 wy + 1)(2 wz + 1) > 2^26, and planes_only on a map without distributions.  The
 * occupancy brick is sized by the box of the moved cells plus the window, and by as much again behind it for the points
 * without a cell: above 2^31 bits it is SLAM_E_NOMEM and nothing has changed.  A map of no voxels or a source of no points
 * gives a zero volume and no hits.  WAITS TWICE for `stream`: for the box of the moved cells, which sizes the brick, and for
 * the hits (and the volume, when asked for).  One call at a time per handle. */
int  slam_vmap_search_dev(slam_vmap_t *m, const float *d_xyz, int n, int stride, const slam_vmap_search_params *params,
                          slam_vmap_search_hit *hits, int *n_hits, int32_t *volume, slam_stream_t stream);
/* Host points: staged as slam_vmap_integrate stages them (synchronously), then the same path on the null stream. */
int  slam_vmap_search(slam_vmap_t *m, const float *xyz, int n, int stride, const slam_vmap_search_params *params,
                      slam_vmap_search_hit *hits, int *n_hits, int32_t *volume);
/* The filtered cloud of keyframe `id` of `store` is the source; a null store or a dead id is SLAM_E_INVALID. */
int  slam_vmap_search_keyframe(slam_vmap_t *m, slam_kf_t *store, int id, const slam_vmap_search_params *params,
                               slam_vmap_search_hit *hits, int *n_hits, int32_t *volume, slam_stream_t stream);

/* -------------------------------------------------------------------------
 * Pose-graph optimiser: graph_slam's optimizeGraph (graph_slam.cpp:322-390), i.e. g2o's VertexSE3 / EdgeSE3 under
 * OptimizationAlgorithmLevenberg, restated in docs/PGO.md (parity with g2o itself is unpinned; the yardstick is
 * tests/cpp/pgo_oracle.cpp).  Everything is f64.
 *   pose      7 doubles: t (x y z) and a quaternion (x y z w); a quaternion arriving through the ABI is divided by its norm
 *             unless |q|^2 is within 8 ulp of 1 already (a pose read back and handed in again keeps its bits)
 *   edge      from -> to with measurement Z (a pose) and information (36 doubles, row-major, x y z then rotation x y z):
 *             e = toVectorMQT(Z^-1 Xfrom^-1 Xto), chi2 = e' info e
 *   update    X <- X fromVectorMQT(delta), quaternion renormalised
 *   system    H = sum J' info J, b = -sum J' info e with the closed-form Jacobians of docs/PGO.md, block rows in a reverse
 *             Cuthill-McKee order of the free vertices, a uniform block band, Cholesky in one workgroup
 * The graph is host state: create, clear, add_vertex, set_vertex, add_edge and destroy touch no device and work without
 * one.  The calls that take a stream upload the graph and WAIT for that stream; on a machine without a usable device they
 * return SLAM_E_HIP.  One call at a time per handle.
 * ---------------------------------------------------------------------- */
typedef struct slam_pgo slam_pgo_t;

#define SLAM_PGO_ORDER_RCM       0 /* reverse Cuthill-McKee, ties by degree then id */
#define SLAM_PGO_ORDER_NATURAL   1 /* free vertices by id (tests) */
#define SLAM_PGO_STOP_ITERATIONS 0
#define SLAM_PGO_STOP_MAX_TRIALS 1
#define SLAM_PGO_STOP_RHO_ZERO   2
#define SLAM_PGO_TRACE           64

typedef struct {
    int    max_trials;     /* 10: trials of one iteration (g2o's maxTrialsAfterFailure) */
    double tau;            /* 1e-5: lambda of iteration 0 = tau * max diag(H) */
    double good_lower;     /* 1/3 */
    double good_upper;     /* 2/3 */
    int    ordering;       /* SLAM_PGO_ORDER_* */
    size_t max_band_bytes; /* 1 GiB: a band of more bytes is SLAM_E_NOMEM, nothing is truncated */
} slam_pgo_params;

typedef struct {
    double lambda;   /* the damping this trial solved with */
    double rho;
    double chi2;     /* of the candidate poses; DBL_MAX where the factorisation met a pivot <= 0 */
    int    accepted;
    int    reserved;
} slam_pgo_trial;

typedef struct {
    int            iterations;     /* linearisations done */
    int            stop_reason;    /* SLAM_PGO_STOP_* */
    int            half_bandwidth; /* w, in blocks */
    int            free_vertices;
    double         chi2_initial;
    double         chi2_final;
    size_t         band_bytes;     /* free_vertices * (w + 1) * 36 * 8 */
    int            n_trials;       /* all trials of the call; the first SLAM_PGO_TRACE of them are in `trace` */
    int            reserved;
    slam_pgo_trial trace[SLAM_PGO_TRACE];
} slam_pgo_result;

void slam_pgo_default_params(slam_pgo_params *p);
int  slam_pgo_create(const slam_pgo_params *params, slam_pgo_t **out); /* params may be NULL */
void slam_pgo_destroy(slam_pgo_t *g);
int  slam_pgo_clear(slam_pgo_t *g); /* no vertices, no edges; the device buffers stay */
/* Ids are dense and in order: id must be the number of vertices so far.  SLAM_E_INVALID otherwise, or for a pose that is
 * not finite or has a zero quaternion. */
int  slam_pgo_add_vertex(slam_pgo_t *g, int id, const double pose[7], int fixed);
int  slam_pgo_set_vertex(slam_pgo_t *g, int id, const double pose[7]);
/* from != to, both existing vertices; Z^-1 is taken here, once. */
int  slam_pgo_add_edge(slam_pgo_t *g, int from, int to, const double meas[7], const double info[36]);
int  slam_pgo_size(slam_pgo_t *g, int *n_vertices, int *n_edges);
/* Up to `iterations` Levenberg-Marquardt iterations from the current poses; lambda starts anew in every call.  The
 * estimates replace the handle's poses.  SLAM_E_INVALID without a fixed vertex, SLAM_E_NOMEM beyond max_band_bytes.
 * Waits once per trial (one pinned record) and once for the poses. */
int  slam_pgo_optimize(slam_pgo_t *g, int iterations, slam_pgo_result *result, slam_stream_t stream);
/* 7 doubles per vertex, the quaternion with w >= 0.  Host state: no device. */
int  slam_pgo_read_vertices(slam_pgo_t *g, double *pose, int cap, int *n_out);
/* Stage entry points (tests, debugging); each applies nothing.
 * chi2: the sum and, where given, e (6 per edge) and chi2 per edge at the current poses. */
int  slam_pgo_chi2(slam_pgo_t *g, double *chi2, double *e, double *chi2_e, slam_stream_t stream);
/* The undamped system (lambda = 0) at the current poses: every block of the band's lower part as (rows[k], cols[k],
 * blocks[36 k ..]) with rows and cols in vertex numbering, b (6 per vertex, zeros at fixed ones), perm (block row ->
 * vertex, free_vertices of them) and w.  *n_blocks is the number of blocks; with more than `cap` nothing but the three
 * counts is written and the call returns SLAM_E_NOMEM.  Array arguments are nullable. */
int  slam_pgo_read_system(slam_pgo_t *g, int *rows, int *cols, double *blocks, int cap, int *n_blocks, double *b, int *perm,
                          int *free_vertices, int *half_bandwidth, slam_stream_t stream);
/* One trial at the given lambda: delta (6 per vertex, vertex numbering), chi2 before and at the candidate poses as computed
 * (not replaced by DBL_MAX), scale = sum delta (lambda delta + b) without the 1e-3, *pivot_flag = 1 where a pivot <= 0 ended
 * the factorisation (delta and scale are zero then). */
int  slam_pgo_step(slam_pgo_t *g, double lambda, double *delta, double *chi2_before, double *chi2_after, double *scale,
                   int *pivot_flag, slam_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_MI355X_H */
