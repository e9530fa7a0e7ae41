// kf_edge.hip -- graph_slam's keyframe edges on gfx950 (docs/KF_EDGE.md):
//   keyframe store                    graphSlamTools.cpp:278-286  pcl::VoxelGrid(0.5) once per keyframe + a 3-D search lattice
//   pcl::IterativeClosestPoint        :27-39, :294-296            3-D point to point, Umeyama step, PCL's stop rules
//   computeEdgeInformationLUM         :108-214                    on the f32 final transform, in the same launch
//
// A keyframe's filtered cloud is sorted by lattice cell (edge >= the gate, so the gated nearest neighbour is among the 27
// cells around a query); an open-addressing hash table of 2 n slots maps a cell key to its run of sorted points, so a
// keyframe holds O(points) bytes whatever its extent.  One workgroup registers one edge: all iterations, the 3 x 3 SVD,
// the stop rules and the LUM pass run inside one launch.  Sums are f64 (ss: f32, as the reference has it), reduced in a
// fixed order -- lanes by shuffle, waves in wave order through LDS -- so a result is the same bits on every run and
// whatever else is in the batch.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "kf_common.hpp"

namespace {

struct EdgeTask {
    KfView   src, tgt;
    int32_t *corr; // src.n ints: the sorted slot of each source point's partner, -1 = none
    float    init[16];
};

struct EdgeParams {
    double inv_cell, gate2, eps_t, eps_f;
    int    max_iter;
};

// ---------------------------------------------------------------- lattice build
__global__ __launch_bounds__(256) void kf_key_kernel(const float4 *pts, int n, double inv, unsigned long long *keys, uint32_t *vals)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    keys[i] = cell_key(cell_coord(p.x, inv), cell_coord(p.y, inv), cell_coord(p.z, inv));
    vals[i] = (uint32_t)i;
}

// sorted points, and one table entry per run of equal keys; stats[0] = cells, stats[1] = largest cell
__global__ __launch_bounds__(256) void kf_table_kernel(const float4 *pts, const unsigned long long *keys, const uint32_t *vals, int n,
                                                       float4 *sorted, int4 *table, unsigned mask, int *stats)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = vals[i];
    float4         p = pts[src];
    p.w = __int_as_float((int)src);
    sorted[i] = p;
    const unsigned long long key = keys[i];
    if (i > 0 && keys[i - 1] == key) return;
    int count = 1;
    while (i + count < n && keys[i + count] == key) ++count;
    unsigned h = slot_of(key, mask);
    for (;;) { // keys are distinct here: a slot is claimed once
        unsigned long long *kp = reinterpret_cast<unsigned long long *>(&table[h]);
        if (atomicCAS(kp, kEmpty, key) == kEmpty) {
            table[h].z = i;
            table[h].w = count;
            break;
        }
        h = (h + 1) & mask;
    }
    atomicAdd(&stats[0], 1);
    atomicMax(&stats[1], count);
}

__global__ __launch_bounds__(256) void kf_nearest_kernel(KfView t, double inv, double gate2, int strict, const float *q, int n, int stride,
                                                         int32_t *index, float *dist2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *p = q + (size_t)i * stride;
    float        d2;
    int          slot;
    const int    j = nearest27(t, inv, gate2, p[0], p[1], p[2], &d2, &slot);
    const bool   keep = j >= 0 && (strict ? (double)d2 < gate2 : (double)d2 <= gate2);
    index[i] = keep ? j : -1;
    dist2[i] = keep ? d2 : 0.0f;
}

__device__ inline double det3(const double m[9])
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// Umeyama without scaling from H = sum (q - qm)(p - pm)' / n: R = U diag(1, 1, +-1) V', t = qm - R pm.  Full rank: the sign
// of det H; a rank-deficient H (planar, collinear pairs): that of det U det V, so that R is always a proper rotation.
__device__ void umeyama(const double H[9], const double pm[3], const double qm[3], double R[9], double t[3])
{
    double    U[9], s[3], V[9];
    const int rank = svd3(H, U, s, V);
    double    sign;
    if (rank == 3)
        sign = det3(H) < 0.0 ? -1.0 : 1.0;
    else
        sign = det3(U) * det3(V) > 0.0 ? 1.0 : -1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + sign * U[3 * r + 2] * V[3 * c + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = qm[r] - ((R[3 * r] * pm[0] + R[3 * r + 1] * pm[1]) + R[3 * r + 2] * pm[2]);
}

// ---------------------------------------------------------------- one workgroup per edge
__global__ __launch_bounds__(kEdgeThreads) void kf_edge_kernel(const EdgeTask *tasks, EdgeParams P, slam_kf_edge_result *results, int32_t *trace,
                                                               int trace_cap, int lds_points)
{
    extern __shared__ float4 lds_sorted[]; // room for lds_points of the target's sorted points
    __shared__ double sT[12];
    __shared__ float  sTf[12];
    __shared__ double sD[6];
    __shared__ double red[kWaves][16];
    __shared__ double tot[16];
    __shared__ float  redf[kWaves][16];
    __shared__ float  totf[16];
    __shared__ int    sState;
    __shared__ double sMM[36]; // thread 0's, from the solve to the final scaling

    const EdgeTask      &task = tasks[blockIdx.x];
    const KfView         src = task.src;
    KfView               tgt = task.tgt;
    int32_t             *corr = task.corr;
    slam_kf_edge_result *out = results + blockIdx.x;
    const int            tid = threadIdx.x;

    // A target that fits is staged in LDS once per edge: every iteration's searches then read its points there and only the
    // table through L2.  One that does not fit is read through L2 as it lies.
    if (tgt.n <= lds_points) {
        for (int i = tid; i < tgt.n; i += kEdgeThreads) lds_sorted[i] = tgt.sorted[i];
        tgt.sorted = lds_sorted;
    }
    if (tid < 12) sT[tid] = (double)task.init[tid];
    if (tid == 0) sState = 0;
    if (trace)
        for (int i = tid; i < trace_cap; i += kEdgeThreads) trace[(size_t)blockIdx.x * trace_cap + i] = -1;
    int    iterations = 0, pairs = 0; // thread 0's are the ones that count
    double mse = 0.0, mse_prev = DBL_MAX;
    for (;;) {
        __syncthreads();
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = sT[k];
        // correspondences, the centroids' sums and the squared distances
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid; i < src.n; i += kEdgeThreads) {
            float m[3], d2;
            int   slot;
            move_f64(T, src.pts[i], m);
            const int  j = nearest27(tgt, P.inv_cell, P.gate2, m[0], m[1], m[2], &d2, &slot);
            const bool keep = j >= 0 && (double)d2 <= P.gate2; // PCL skips on >
            corr[i] = keep ? slot : -1;
            if (keep) {
                const float4 q = tgt.sorted[slot];
                acc[0] += 1.0;
                acc[1] += (double)m[0], acc[2] += (double)m[1], acc[3] += (double)m[2];
                acc[4] += (double)q.x, acc[5] += (double)q.y, acc[6] += (double)q.z;
                acc[7] += (double)d2;
            }
        }
        block_sum<double, 8>(acc, red, tot);
        const double n = tot[0];
        pairs = (int)n;
        mse = pairs ? tot[7] / n : 0.0;
        if (tid == 0 && trace && iterations < trace_cap) trace[(size_t)blockIdx.x * trace_cap + iterations] = pairs;
        if (pairs < 3) { // uniform: every thread reads the same total
            if (tid == 0) sState = SLAM_KF_NO_CORRESPONDENCES;
            break;
        }
        const double pm[3] = {tot[1] / n, tot[2] / n, tot[3] / n}, qm[3] = {tot[4] / n, tot[5] / n, tot[6] / n};
        double       h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid; i < src.n; i += kEdgeThreads) {
            const int slot = corr[i];
            if (slot < 0) continue;
            float m[3];
            move_f64(T, src.pts[i], m);
            const float4 q = tgt.sorted[slot];
            const double dq[3] = {(double)q.x - qm[0], (double)q.y - qm[1], (double)q.z - qm[2]};
            const double dp[3] = {(double)m[0] - pm[0], (double)m[1] - pm[1], (double)m[2] - pm[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) h[3 * r + c] += dq[r] * dp[c];
        }
        block_sum<double, 9>(h, red, tot);
        if (tid == 0) {
            double H[9], R[9], t[3], N[12];
            for (int k = 0; k < 9; ++k) H[k] = tot[k] / n;
            umeyama(H, pm, qm, R, t);
            for (int r = 0; r < 3; ++r) { // total <- step . total
                for (int c = 0; c < 3; ++c) N[4 * r + c] = (R[3 * r] * T[c] + R[3 * r + 1] * T[4 + c]) + R[3 * r + 2] * T[8 + c];
                N[4 * r + 3] = ((R[3 * r] * T[3] + R[3 * r + 1] * T[7]) + R[3 * r + 2] * T[11]) + t[r];
            }
            for (int k = 0; k < 12; ++k) sT[k] = N[k];
            ++iterations;
            // DefaultConvergenceCriteria, in the order of docs/KF_EDGE.md
            int state = 0;
            if (iterations >= P.max_iter)
                state = SLAM_KF_ITERATIONS;
            else {
                const double cosa = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
                const double tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
                const double d = fabs(mse - mse_prev);
                if (cosa >= 1.0 - P.eps_t && tt <= P.eps_t)
                    state = SLAM_KF_TRANSFORM;
                else if (d < 1e-12)
                    state = SLAM_KF_ABS_MSE;
                else if (d / mse_prev < P.eps_f)
                    state = SLAM_KF_REL_MSE;
                else
                    mse_prev = mse;
            }
            sState = state;
        }
        __syncthreads();
        if (sState) break;
    }
    __syncthreads();
    if (tid == 0) {
        write_transform(sT, sTf, out->transform64, out->transform);
        out->iterations = iterations, out->state = sState, out->converged = sState != SLAM_KF_NO_CORRESPONDENCES;
        out->pairs = pairs, out->mse = mse, out->reserved = 0;
    }
    __syncthreads();

    lum_pass(src, tgt, corr, P.inv_cell, P.gate2, sTf, red, tot, redf, totf, sD, sMM, out);
}

int check_params(const slam_kf_params *p)
{
    SLAM_REQUIRE(p->leaf_size > 0 && p->gate > 0 && p->max_iterations >= 1 && (p->cell_size == 0 || p->cell_size >= p->gate), SLAM_E_INVALID,
                 "slam_kf: leaf_size and gate must be positive, max_iterations >= 1, cell_size 0 or >= gate");
    return SLAM_OK;
}

} // namespace

extern "C" {

void slam_kf_default_params(slam_kf_params *p)
{
    if (!p) return;
    p->leaf_size = 0.5;               // graphSlamTools.cpp:281
    p->gate = 0.75;                   // :29
    p->cell_size = 0.0;
    p->max_iterations = 200;          // :31
    p->transformation_epsilon = 1e-6; // :33
    p->fitness_epsilon = 1e-6;        // :35
    p->target_in_lds = 1;
}

int slam_kf_create(const slam_kf_params *params, slam_kf_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_kf_create: null out pointer");
    *out = nullptr;
    slam_kf_params p;
    slam_kf_default_params(&p);
    if (params) p = *params;
    SLAM_TRY(check_params(&p));
    SLAM_TRY(require_device());
    slam_kf *s = new (std::nothrow) slam_kf();
    SLAM_REQUIRE(s, SLAM_E_NOMEM, "slam_kf_create: out of host memory");
    s->p = p;
    slam_kf_gicp_default_params(&s->gp);
    int rc = slam_ccicp_create(&s->cc);
    if (rc == SLAM_OK) rc = reserve_quarter(s->stats, 64);
    if (rc != SLAM_OK) {
        delete s;
        return rc;
    }
    *out = s;
    return SLAM_OK;
}

void slam_kf_destroy(slam_kf_t *s) { delete s; }

int slam_kf_set_params(slam_kf_t *s, const slam_kf_params *params)
{
    SLAM_REQUIRE(s && params, SLAM_E_INVALID, "slam_kf_set_params: null argument");
    SLAM_TRY(check_params(params));
    SLAM_REQUIRE(s->kfs.empty() || (params->leaf_size == s->p.leaf_size && params->gate == s->p.gate && params->cell_size == s->p.cell_size),
                 SLAM_E_INVALID, "slam_kf_set_params: leaf_size, gate and cell_size are fixed once the store holds a keyframe");
    s->p = *params;
    return SLAM_OK;
}

int slam_kf_count(slam_kf_t *s) { return s ? (int)s->kfs.size() : 0; }

int slam_kf_add_keyframe_dev(slam_kf_t *s, const float *d_xyz, int n, int stride, int *id, slam_stream_t stream)
{
    SLAM_REQUIRE(s && id && n > 0 && stride >= 3 && d_xyz, SLAM_E_INVALID, "slam_kf_add_keyframe_dev: bad arguments");
    *id = -1;
    hipStream_t st = as_stream(stream);
    SLAM_TRY(reserve_quarter(s->filtered, sizeof(float4) * (size_t)n));
    int         m = 0;
    const float leaf = (float)s->p.leaf_size;
    SLAM_TRY(slam_ccicp_voxel_downsample_dev(s->cc, d_xyz, nullptr, n, stride, leaf, leaf, leaf, static_cast<float *>(s->filtered.p), n, &m, stream));
    SLAM_REQUIRE(m > 0, SLAM_E_INVALID, "slam_kf_add_keyframe: the cloud has no finite point");
    unsigned slots = 64;
    while (slots < 2u * (unsigned)m) slots <<= 1;
    Keyframe kf;
    SLAM_TRY(kf.block.alloc(sizeof(float4) * 2 * (size_t)m + sizeof(int4) * (size_t)slots));
    float4 *pts = kf.block.as<float4>(), *sorted = pts + m;
    int4   *table = reinterpret_cast<int4 *>(sorted + m);
    kf.view = KfView{pts, sorted, table, slots - 1, m};
    SLAM_TRY(reserve_quarter(s->keys, (sizeof(unsigned long long) + sizeof(uint32_t)) * 2 * (size_t)m));
    unsigned long long *keys = s->keys.as<unsigned long long>(), *keys_s = keys + m;
    uint32_t           *vals = reinterpret_cast<uint32_t *>(keys_s + m), *vals_s = vals + m;
    size_t              tb = 0;
    SLAM_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys, keys_s, vals, vals_s, (size_t)m, 0, 63, st));
    SLAM_TRY(reserve_quarter(s->sort_tmp, tb + 16));
    int *stats = s->stats.as<int>();
    int  got[2] = {0, 0};
    // (a failure below frees the keyframe's block on the way out: hipFree waits for what has been enqueued on it)
    SLAM_HIP(hipMemcpyAsync(pts, s->filtered.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, st));
    SLAM_HIP(hipMemsetAsync(table, 0xff, sizeof(int4) * (size_t)slots, st));
    SLAM_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(kf_key_kernel, dim3(blocks(m, 256)), dim3(256), 0, st, pts, m, inv_cell(s->p), keys, vals);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(rocprim::radix_sort_pairs(s->sort_tmp.p, tb, keys, keys_s, vals, vals_s, (size_t)m, 0, 63, st));
    hipLaunchKernelGGL(kf_table_kernel, dim3(blocks(m, 256)), dim3(256), 0, st, pts, keys_s, vals_s, m, sorted, table, slots - 1, stats);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(got, stats, sizeof got, hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    kf.n_cells = got[0], kf.max_cell = got[1];
    s->kfs.push_back(std::move(kf));
    *id = (int)s->kfs.size() - 1;
    return SLAM_OK;
}

int slam_kf_add_keyframe(slam_kf_t *s, const float *xyz, int n, int stride, int *id)
{
    SLAM_REQUIRE(s && id && n > 0 && stride >= 3 && xyz, SLAM_E_INVALID, "slam_kf_add_keyframe: bad arguments");
    const size_t bytes = sizeof(float) * (size_t)n * stride;
    SLAM_TRY(reserve_quarter(s->in, bytes));
    SLAM_HIP(hipMemcpy(s->in.p, xyz, bytes, hipMemcpyHostToDevice));
    return slam_kf_add_keyframe_dev(s, static_cast<const float *>(s->in.p), n, stride, id, nullptr);
}

int slam_kf_keyframe_info(slam_kf_t *s, int id, int *n_points, int *n_cells, int *max_cell_points, int *table_slots, long *device_bytes)
{
    SLAM_REQUIRE(kf_live(s, id), SLAM_E_INVALID, "slam_kf_keyframe_info: no keyframe %d", id);
    const Keyframe &k = s->kfs[id];
    if (n_points) *n_points = k.view.n;
    if (n_cells) *n_cells = k.n_cells;
    if (max_cell_points) *max_cell_points = k.max_cell;
    if (table_slots) *table_slots = (int)(k.view.mask + 1);
    if (device_bytes) *device_bytes = (long)k.block.cap;
    return SLAM_OK;
}

int slam_kf_read_keyframe(slam_kf_t *s, int id, float *xyz4, int max_points, int *n_points)
{
    SLAM_REQUIRE(s && n_points && kf_live(s, id) && max_points >= 0 && (xyz4 || max_points == 0), SLAM_E_INVALID,
                 "slam_kf_read_keyframe: bad arguments");
    const Keyframe &k = s->kfs[id];
    *n_points = k.view.n < max_points ? k.view.n : max_points;
    if (*n_points) SLAM_HIP(hipMemcpy(xyz4, k.view.pts, sizeof(float4) * (size_t)*n_points, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_kf_nearest_dev(slam_kf_t *s, int id, const float *d_queries, int n, int stride, int strict, int32_t *d_index, float *d_dist2,
                        slam_stream_t stream)
{
    SLAM_REQUIRE(kf_live(s, id) && n >= 0 && stride >= 3 && (n == 0 || (d_queries && d_index && d_dist2)), SLAM_E_INVALID,
                 "slam_kf_nearest_dev: bad arguments");
    if (n == 0) return SLAM_OK;
    hipLaunchKernelGGL(kf_nearest_kernel, dim3(blocks(n, 256)), dim3(256), 0, as_stream(stream), s->kfs[id].view, inv_cell(s->p),
                       s->p.gate * s->p.gate, strict, d_queries, n, stride, d_index, d_dist2);
    SLAM_HIP(hipGetLastError());
    return SLAM_OK;
}

int slam_kf_register_edges_traced(slam_kf_t *s, const slam_kf_edge_req *req, int n_edges, slam_kf_edge_result *out, int32_t *pairs_trace,
                                  int trace_cap, slam_stream_t stream)
{
    SLAM_REQUIRE(s && n_edges >= 0 && (n_edges == 0 || (req && out)) && (!pairs_trace || trace_cap > 0), SLAM_E_INVALID,
                 "slam_kf_register_edges: bad arguments");
    EdgeParams P;
    P.inv_cell = inv_cell(s->p), P.gate2 = s->p.gate * s->p.gate;
    P.eps_t = s->p.transformation_epsilon, P.eps_f = s->p.fitness_epsilon, P.max_iter = s->p.max_iterations;
    return kf_register_batch(s, "slam_kf_register_edges", "edge", kf_edge_kernel, s->lds_enabled, P,
                             [](EdgeTask &, const slam_kf_edge_req &) -> int { return SLAM_OK; }, req, n_edges, out, pairs_trace, trace_cap, stream);
}

int slam_kf_register_edges(slam_kf_t *s, const slam_kf_edge_req *req, int n_edges, slam_kf_edge_result *out, slam_stream_t stream)
{
    return slam_kf_register_edges_traced(s, req, n_edges, out, nullptr, 0, stream);
}
}
