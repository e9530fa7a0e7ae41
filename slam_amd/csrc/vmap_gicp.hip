// vmap_gicp.hip -- Generalized ICP of a keyframe of the store straight against the voxel map's plane distributions
// (slam_vmap_register_gicp, docs/VOXEL_MAP.md section 9): no extraction, no lattice of the map, no neighbour search over it.
//   vmap_gicp_kernel  one workgroup per request: per iteration every source point is moved by T in f64 and rounded to f32,
//                     its cell found by the map's rule, and the 27 cells around it looked up in the map's own hash table --
//                     the 27 first probes are issued together, a collision (rare below half load) is followed alone.  The
//                     plane voxel with the smallest (f32 d^2 to its centroid, key) strictly inside the gate is the pair.  The
//                     pair's share of the sums, the f64 block sums in a fixed order and thread 0's step and stop rule are
//                     kf_gicp_solve.hpp's, the ones kf_gicp_kernel runs; the transform's write and the host's staging of a
//                     batch are kf_common.hpp's.  A last pass with the f32 transform gives the point-to-plane fitness.
//                     Lookups only find; nothing is written to the map; no workgroup waits for another; every loop is
//                     bounded by the source's size, max_iterations or the table's capacity.
// The map's rules come from vmap_dist.hpp: the hash, the limits and the key packing (vmap_cell_key).  The point-to-cell test in
// nearest_plane27 is still written out here and must follow vmap_point_cell: the kernel stands at 256 VGPRs, and with the
// shared function its SGPR spills came out three fewer -- no worse, but not the kernel that was measured (docs/VOXEL_MAP.md
// sections 9.3 and 14), so its body stays.
// The restatement is tests/cpp/vmap_gicp_oracle.cpp.
#include "kf_gicp_solve.hpp"
#include "vmap_dist.hpp"

namespace {

struct VgTask {
    KfView        src;
    const double *src_cov; // six doubles per point of the filtered cloud
    float         init[16];
};

struct VgParams {
    double gate2, eps_t, eps_r;
    int    max_iter;
};

// The plane voxel among the 27 cells around q with the smallest (d^2, key): its slot or -1, and d^2 (f32, nearest27's order
// of operations: dx dx + dy dy + dz dz without FMA).  A point without a cell has no candidates.
__device__ __forceinline__ long long nearest_plane27(const VmapDistView &V, const float q[3], float *d2, float4 *cen)
{
    int  c[3];
    bool has_cell = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double f = floor((double)q[k] / V.leaf);
        if (!(fabsf(q[k]) < kVmapCoordLimit) || !(fabs(f) < (double)kVmapCellLimit)) has_cell = false; // a NaN fails both tests
        c[k] = has_cell ? (int)f : 0;
    }
    if (!has_cell) return -1;
    // The 27 keys and their first probes, issued together.  A neighbour's key is the centre's plus a constant (the fields do
    // not carry: the cell is in range); slots fit 32 bits (a table has at most 2^31).  Only the 27 words read and their slots
    // stay in registers between the two passes.
    const uint64_t base = vmap_cell_key(c);
    const uint32_t mask = (uint32_t)V.mask;
    uint32_t       slot[27];
    uint64_t       cur[27];
    bool           in[3][3]; // per axis: may the offset -1, 0, +1 be taken
#pragma unroll
    for (int k = 0; k < 3; ++k) in[k][0] = c[k] - 1 > -kVmapCellLimit, in[k][1] = true, in[k][2] = c[k] + 1 < kVmapCellLimit;
#pragma unroll
    for (int j = 0; j < 27; ++j) {
        const int      ox = j % 3 - 1, oy = j / 3 % 3 - 1, oz = j / 9 - 1;
        const uint64_t key = base + (uint64_t)((long long)ox + (long long)oy * (1ll << 21) + (long long)oz * (1ll << 42));
        slot[j] = (uint32_t)vmap_fmix64(key) & mask;
        const uint64_t word = V.key[slot[j]]; // read whatever the cell: the slot is inside the table, and no branch parts the loads
        cur[j] = (in[0][ox + 1] && in[1][oy + 1] && in[2][oz + 1]) ? word : kEmpty;
    }
    long long best = -1;
    uint64_t  bkey = 0;
    float     bd = 0.0f;
    float4    bc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int j = 0; j < 27; ++j) {
        const int      ox = j % 3 - 1, oy = j / 3 % 3 - 1, oz = j / 9 - 1;
        const uint64_t key = base + (uint64_t)((long long)ox + (long long)oy * (1ll << 21) + (long long)oz * (1ll << 42));
        uint32_t       h = slot[j];
        uint64_t       k = cur[j];
        for (uint32_t probe = 0; k != key && k != kEmpty && probe < mask; ++probe) { // a collision: linear probing, at most capacity slots
            h = (h + 1) & mask;
            k = V.key[h];
        }
        if (k != key || k == kEmpty) continue;
        const float4 p = V.cen[h];
        if (p.w == 0.0f) continue; // no plane voxel
        const float dx = __fsub_rn(q[0], p.x), dy = __fsub_rn(q[1], p.y), dz = __fsub_rn(q[2], p.z);
        const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        if (best < 0 || d < bd || (d == bd && key < bkey)) best = (long long)h, bd = d, bkey = key, bc = p;
    }
    *d2 = bd;
    *cen = bc;
    return best;
}

__global__ __launch_bounds__(kEdgeThreads) void vmap_gicp_kernel(const VgTask *tasks, VmapDistView V, VgParams P, slam_vmap_gicp_result *results,
                                                                 int32_t *trace, int trace_cap)
{
    __shared__ double sT[12];
    __shared__ float  sTf[12];
    __shared__ double red[kWaves][16];
    __shared__ double tot[16];
    __shared__ int    sState;
    __shared__ double sH[36]; // thread 0's: the last iteration's J' M J

    const VgTask          &task = tasks[blockIdx.x];
    const KfView           src = task.src;
    const double          *src_cov = task.src_cov;
    slam_vmap_gicp_result *out = results + blockIdx.x;
    const int              tid = threadIdx.x;

    if (tid < 12) sT[tid] = (double)task.init[tid];
    if (tid < 36) sH[tid] = 0.0;
    if (tid == 0) sState = 0;
    if (trace)
        for (int i = tid; i < trace_cap; i += kEdgeThreads) trace[(size_t)blockIdx.x * trace_cap + i] = -1;
    int    iterations = 0, pairs = 0; // thread 0's are the ones that count
    double mse = 0.0, cost = 0.0;
    for (int round = 0; round <= P.max_iter; ++round) { // ends by the state; the bound is for the reader
        __syncthreads();
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { // the same for every lane: held in scalar registers, which leaves the probes 24 vector ones
            const long long b = __double_as_longlong(sT[k]);
            const unsigned  lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
            T[k] = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
        double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // pairs, d^2, cost, g
        double h16[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, h5[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < src.n; i += kEdgeThreads) {
            const float4 p = src.pts[i];
            float        m[3], d2;
            float4       q;
            move_f64(T, p, m);
            const long long slot = nearest_plane27(V, m, &d2, &q);
            if (!(slot >= 0 && (double)d2 < P.gate2)) continue; // strict
            gicp_accumulate(T, p, q, d2, src_cov + 6 * (size_t)i, V.cov + 6 * (size_t)slot, acc, h16, h5);
        }
        double g[6], hu[21];
        gicp_reduce(acc, h16, h5, red, tot, &pairs, &mse, &cost, g, hu);
        if (tid == 0) {
            if (trace && iterations < trace_cap) trace[(size_t)blockIdx.x * trace_cap + iterations] = pairs;
            sState = gicp_advance(hu, g, T, pairs, P.max_iter, P.eps_r, P.eps_t, sH, sT, iterations);
        }
        __syncthreads();
        if (sState) break;
    }
    __syncthreads();
    if (tid == 0) {
        write_transform(sT, sTf, out->transform64, out->transform);
        out->iterations = iterations, out->state = sState;
        out->converged = sState == SLAM_KF_ITERATIONS || sState == SLAM_KF_TRANSFORM;
        out->pairs = pairs, out->mse = mse, out->cost = cost;
        for (int k = 0; k < 36; ++k) out->hessian[k] = sH[k];
    }
    __syncthreads();

    // the fitness: the f32 transform, points moved in f32, the same pairing; (n . (q - x))^2 in f64
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = sTf[k];
    double f[2] = {0, 0};
    for (int i = tid; i < src.n; i += kEdgeThreads) {
        float  s[3], d2;
        float4 q;
        move_f32(M, src.pts[i], s);
        const long long slot = nearest_plane27(V, s, &d2, &q);
        if (!(slot >= 0 && (double)d2 < P.gate2)) continue;
        const double r0 = (double)q.x - (double)s[0], r1 = (double)q.y - (double)s[1], r2 = (double)q.z - (double)s[2];
        const double dot = (V.nrm[3 * (size_t)slot] * r0 + V.nrm[3 * (size_t)slot + 1] * r1) + V.nrm[3 * (size_t)slot + 2] * r2;
        f[0] += 1.0;
        f[1] += dot * dot;
    }
    block_sum<double, 2>(f, red, tot);
    if (tid == 0) {
        out->fitness_pairs = (int)tot[0], out->reserved = 0;
        out->fitness = tot[0] > 0.0 ? tot[1] / tot[0] : 0.0;
    }
}

} // namespace

extern "C" {

void slam_vmap_default_gicp_params(slam_vmap_gicp_params *p)
{
    if (!p) return;
    p->gate = 2.0;
    p->max_iterations = 100;
    p->transformation_epsilon = 1e-6;
    p->rotation_epsilon = 2e-3; // PCL's
}

int slam_vmap_register_gicp_traced(slam_vmap_t *m, slam_kf_t *store, const slam_vmap_gicp_req *req, int n, const slam_vmap_gicp_params *params,
                                   slam_vmap_gicp_result *out, int32_t *pairs_trace, int trace_cap, slam_stream_t stream)
{
    slam_vmap_gicp_params p;
    slam_vmap_default_gicp_params(&p);
    if (params) p = *params;
    SLAM_REQUIRE(n >= 0 && (n == 0 || (req && out)) && (!pairs_trace || trace_cap > 0), SLAM_E_INVALID,
                 "slam_vmap_register_gicp: n >= 0, requests and results, and trace_cap > 0 with a trace");
    SLAM_REQUIRE(p.gate > 0 && p.max_iterations >= 1 && p.transformation_epsilon >= 0 && p.rotation_epsilon >= 0, SLAM_E_INVALID,
                 "slam_vmap_register_gicp: gate > 0, max_iterations >= 1 and epsilons >= 0");
    SLAM_TRY(require_device());
    SLAM_REQUIRE(m && store, SLAM_E_INVALID, "slam_vmap_register_gicp: map or store is NULL");
    for (int e = 0; e < n; ++e)
        SLAM_REQUIRE(kf_live(store, req[e].src), SLAM_E_INVALID, "slam_vmap_register_gicp: request %d names keyframe %d, the store holds %d (removed ones are refused)",
                     e, req[e].src, (int)store->kfs.size());
    hipStream_t  st = as_stream(stream);
    VmapDistView V;
    SLAM_TRY(vmap_dist_view(m, st, &V)); // refuses a map without distributions; computes stale ones on st
    if (n == 0) return SLAM_OK;
    for (int e = 0; e < n; ++e) SLAM_TRY(slam_kf_compute_covariances(store, req[e].src, stream)); // a second call does nothing
    if (!pairs_trace) trace_cap = 0;
    BatchStage<VgTask, slam_vmap_gicp_result> stage; // in the map's own work buffer; nothing beyond tasks | results | trace
    SLAM_TRY(stage.lay_out(vmap_register_work(m), "slam_vmap_register_gicp", n, trace_cap, 0, st));
    VgTask *tasks = stage.tasks();
    for (int e = 0; e < n; ++e) {
        const Keyframe &kf = store->kfs[req[e].src];
        tasks[e].src = kf.view, tasks[e].src_cov = kf.cov6;
        std::memcpy(tasks[e].init, req[e].init, sizeof tasks[e].init);
    }
    VgParams P;
    P.gate2 = p.gate * p.gate, P.eps_t = p.transformation_epsilon, P.eps_r = p.rotation_epsilon, P.max_iter = p.max_iterations;
    SLAM_TRY(stage.upload());
    hipLaunchKernelGGL(vmap_gicp_kernel, dim3(n), dim3(kEdgeThreads), 0, st, stage.dev_tasks(), V, P, stage.dev_results(), stage.dev_trace(), trace_cap);
    SLAM_HIP(hipGetLastError());
    return stage.download(out, pairs_trace);
}

int slam_vmap_register_gicp(slam_vmap_t *m, slam_kf_t *store, const slam_vmap_gicp_req *req, int n, const slam_vmap_gicp_params *params,
                            slam_vmap_gicp_result *out, slam_stream_t stream)
{
    return slam_vmap_register_gicp_traced(m, store, req, n, params, out, nullptr, 0, stream);
}
}
