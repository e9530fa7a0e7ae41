// kf_gicp.hip -- Generalized ICP on the keyframe store (docs/KF_GICP.md), the solver global_matching is built on
// (global_match.cpp:52,225-235: pcl::GeneralizedIterativeClosestPoint):
//   kf_cov_kernel    per point of a filtered cloud: the k nearest points within a radius, ordered by (f32 d^2, index), found
//                    exactly in the store's lattice, and from them C' = V diag(1, 1, eps) V'.  One lane owns one point and
//                    sums in list order, so the covariances are the restatement's bit for bit.
//   kf_gicp_kernel   one workgroup per request: gated 1-NN pairs, M = (C'q + R C'p R')^-1 per pair, one Gauss-Newton step per
//                    iteration by a 6 x 6 Cholesky on thread 0, PCL GICP's stop rule, then the fitness and the LUM block of
//                    kf_edge.hip on the f32 transform.  Sums are f64, reduced by block_sum in a fixed order.  The iteration's
//                    pieces (a pair's share, the three block sums, thread 0's step and stop rule) are kf_gicp_solve.hpp's,
//                    which vmap_gicp.hip runs too; this file keeps the search in the lattice, the gate and the passes after.
#include "kf_gicp_solve.hpp"

namespace {

constexpr int kCovThreads = 256;
constexpr int kMaxK = 32;       // 256 lanes x 32 entries x 8 bytes = 64 KB of LDS
constexpr int kMaxRings = 8;    // cov_radius is at most this many lattice edges

struct CovParams {
    double inv_cell, edge, radius2, eps;
    int    k, rings, min_nbr;
};

struct GicpTask {
    KfView        src, tgt;
    const double *src_cov, *tgt_cov; // six doubles per point, by index in the filtered cloud
    int32_t      *corr;              // src.n ints, the LUM pass's
    float         init[16];
};

struct GicpParams {
    double inv_cell, gate2, eps_t, eps_r;
    int    max_iter;
};

// ---------------------------------------------------------------- neighbour lists and covariances, one lane per point
// A lane's list lives in LDS, entry e of lane l at [e][l], so that the lanes of a wave never share a bank.  An entry is
// (bits of the f32 d^2) << 32 | index: d^2 is never negative, so the order of the entries as integers is the order by
// (d^2, index).  Rings of cells around the point's own are visited outwards; the cells beyond ring r hold only points
// farther than r edges, so the search ends once the list is full and its last entry is nearer than that (with
// kPruneSlack against the roundings of the f32 sum), and it never goes past P.rings.  Nobody waits for anybody.
__global__ __launch_bounds__(kCovThreads) void kf_cov_kernel(KfView v, CovParams P, double *cov6, int32_t *nbr_index, float *nbr_dist2,
                                                             int32_t *nbr_count)
{
    extern __shared__ unsigned long long lds_list[]; // [P.k][kCovThreads]
    const int s = blockIdx.x * kCovThreads + threadIdx.x;
    if (s >= v.n) return;
    unsigned long long *list = lds_list + threadIdx.x;
    const float4        p = v.sorted[s];
    const int           i = __float_as_int(p.w);
    const int           c0 = cell_coord(p.x, P.inv_cell), c1 = cell_coord(p.y, P.inv_cell), c2 = cell_coord(p.z, P.inv_cell);
    const int           K = P.k;
    int                 m = 0;
    for (int r = 0; r <= P.rings; ++r) {
        for (int oz = -r; oz <= r; ++oz)
            for (int oy = -r; oy <= r; ++oy)
                for (int ox = -r; ox <= r; ++ox) {
                    if (abs(ox) != r && abs(oy) != r && abs(oz) != r) continue; // inside the ring: seen already
                    const int x = c0 + ox, y = c1 + oy, z = c2 + oz;
                    if ((x | y | z) < 0 || x >= 2 * kHalf || y >= 2 * kHalf || z >= 2 * kHalf) continue;
                    const unsigned long long key = cell_key(x, y, z);
                    unsigned                 h = slot_of(key, v.mask);
                    int                      start = 0, count = 0;
                    for (;;) { // at most half the slots are taken: the probe ends
                        const int4               e = v.table[h];
                        const unsigned long long k = ((unsigned long long)(unsigned)e.y << 32) | (unsigned)e.x;
                        if (k == key) {
                            start = e.z, count = e.w;
                            break;
                        }
                        if (k == kEmpty) break;
                        h = (h + 1) & v.mask;
                    }
                    for (int j = start; j < start + count; ++j) {
                        const float4 q = v.sorted[j];
                        const float  dx = __fsub_rn(p.x, q.x), dy = __fsub_rn(p.y, q.y), dz = __fsub_rn(p.z, q.z);
                        const float  d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                        if (!((double)d <= P.radius2)) continue;
                        const unsigned long long ent = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(q.w);
                        if (m == K && ent >= list[(K - 1) * kCovThreads]) continue;
                        int at = m < K ? m : K - 1;
                        while (at > 0) {
                            const unsigned long long prev = list[(at - 1) * kCovThreads];
                            if (prev <= ent) break;
                            list[at * kCovThreads] = prev;
                            --at;
                        }
                        list[at * kCovThreads] = ent;
                        if (m < K) ++m;
                    }
                }
        if (m == K) {
            const double last = (double)__uint_as_float((unsigned)(list[(K - 1) * kCovThreads] >> 32)), reach = (double)r * P.edge;
            if (last * kPruneSlack < reach * reach) break;
        }
    }
    double C[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (m >= P.min_nbr) {
        double s1x = 0, s1y = 0, s1z = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
        for (int e = 0; e < m; ++e) {
            const float4 q = v.pts[(int)(unsigned)list[e * kCovThreads]];
            const double dx = (double)q.x - (double)p.x, dy = (double)q.y - (double)p.y, dz = (double)q.z - (double)p.z;
            s1x += dx, s1y += dy, s1z += dz;
            sxx += dx * dx, sxy += dx * dy, sxz += dx * dz, syy += dy * dy, syz += dy * dz, szz += dz * dz;
        }
        const double dm = (double)m, mx = s1x / dm, my = s1y / dm, mz = s1z / dm;
        const double raw[6] = {sxx / dm - mx * mx, sxy / dm - mx * my, sxz / dm - mx * mz, syy / dm - my * my, syz / dm - my * mz, szz / dm - mz * mz};
        plane_covariance(raw, P.eps, C);
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) cov6[6 * (size_t)i + e] = C[e];
    for (int e = 0; e < K; ++e) {
        const unsigned long long ent = e < m ? list[e * kCovThreads] : 0ull;
        nbr_index[(size_t)i * K + e] = e < m ? (int)(unsigned)ent : -1;
        nbr_dist2[(size_t)i * K + e] = e < m ? __uint_as_float((unsigned)(ent >> 32)) : 0.0f;
    }
    nbr_count[i] = m;
}

// ---------------------------------------------------------------- one workgroup per request
__global__ __launch_bounds__(kEdgeThreads) void kf_gicp_kernel(const GicpTask *tasks, GicpParams P, slam_kf_gicp_result *results, int32_t *trace,
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
    __shared__ double sMM[36];
    __shared__ double sH[36]; // thread 0's: the last iteration's J' M J

    const GicpTask      &task = tasks[blockIdx.x];
    const KfView         src = task.src;
    KfView               tgt = task.tgt;
    const double        *src_cov = task.src_cov, *tgt_cov = task.tgt_cov;
    int32_t             *corr = task.corr;
    slam_kf_gicp_result *out = results + blockIdx.x;
    const int            tid = threadIdx.x;

    // The prologue of kf_edge_kernel, kept in both: shared as one function it took this kernel's SGPR spills from 7 to 9
    // (docs/VOXEL_MAP.md section 14).  The target's points in LDS when they fit, the table and the covariances through L2.
    if (tgt.n <= lds_points) {
        for (int i = tid; i < tgt.n; i += kEdgeThreads) lds_sorted[i] = tgt.sorted[i];
        tgt.sorted = lds_sorted;
    }
    if (tid < 12) sT[tid] = (double)task.init[tid];
    if (tid < 36) sH[tid] = 0.0;
    if (tid == 0) sState = 0;
    if (trace)
        for (int i = tid; i < trace_cap; i += kEdgeThreads) trace[(size_t)blockIdx.x * trace_cap + i] = -1;
    int    iterations = 0, pairs = 0; // thread 0's are the ones that count
    double mse = 0.0, cost = 0.0;
    for (;;) {
        __syncthreads();
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = sT[k];
        double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // pairs, d^2, cost, g
        double h16[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, h5[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < src.n; i += kEdgeThreads) {
            const float4 p = src.pts[i];
            float        m[3], d2;
            int          slot;
            move_f64(T, p, m);
            const int j = nearest27(tgt, P.inv_cell, P.gate2, m[0], m[1], m[2], &d2, &slot);
            if (!(j >= 0 && (double)d2 < P.gate2)) continue; // strict: GICP drops a pair at the gate
            gicp_accumulate(T, p, tgt.sorted[slot], d2, src_cov + 6 * (size_t)i, tgt_cov + 6 * (size_t)j, acc, h16, h5);
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
        slam_kf_edge_result *e = &out->edge;
        write_transform(sT, sTf, e->transform64, e->transform);
        e->iterations = iterations, e->state = sState;
        e->converged = sState == SLAM_KF_ITERATIONS || sState == SLAM_KF_TRANSFORM;
        e->pairs = pairs, e->mse = mse, e->reserved = 0;
        out->cost = cost;
        for (int k = 0; k < 36; ++k) out->hessian[k] = sH[k];
    }
    __syncthreads();

    lum_pass(src, tgt, corr, P.inv_cell, P.gate2, sTf, red, tot, redf, totf, sD, sMM, &out->edge);

    // the fitness, over the pairs the LUM pass has just kept: the same points moved the same way, strictly inside the gate
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = sTf[k];
    double f[2] = {0, 0};
    for (int i = tid; i < src.n; i += kEdgeThreads) {
        const int slot = corr[i];
        if (slot < 0) continue;
        float s[3];
        move_f32(M, src.pts[i], s);
        const float4 q = tgt.sorted[slot];
        const float  dx = __fsub_rn(s[0], q.x), dy = __fsub_rn(s[1], q.y), dz = __fsub_rn(s[2], q.z);
        f[0] += 1.0;
        f[1] += (double)__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    }
    block_sum<double, 2>(f, red, tot);
    if (tid == 0) {
        out->fitness_pairs = (int)tot[0], out->reserved = 0;
        out->fitness = tot[0] > 0.0 ? tot[1] / tot[0] : 0.0;
    }
}

int check_gicp_params(const slam_kf_gicp_params *p)
{
    SLAM_REQUIRE(p->k_correspondences >= 1 && p->k_correspondences <= kMaxK && p->cov_radius >= 0 && p->gicp_epsilon > 0 &&
                     p->max_iterations >= 1 && p->cov_min_neighbours >= 1,
                 SLAM_E_INVALID,
                 "slam_kf: k_correspondences must be 1 .. %d, cov_radius >= 0, gicp_epsilon > 0, max_iterations and cov_min_neighbours >= 1", kMaxK);
    return SLAM_OK;
}

double lattice_edge(const slam_kf_params &p) { return 1.0 / inv_cell(p); }
double cov_radius(const slam_kf *s) { return s->gp.cov_radius > 0 ? s->gp.cov_radius : 2.0 * lattice_edge(s->p); }

} // namespace

extern "C" {

void slam_kf_gicp_default_params(slam_kf_gicp_params *p)
{
    if (!p) return;
    p->k_correspondences = 20; // PCL's
    p->cov_radius = 0.0;
    p->gicp_epsilon = 1e-3;    // PCL's
    p->max_iterations = 10;    // global_match.cpp:229
    p->transformation_epsilon = 1e-6;
    p->rotation_epsilon = 2e-3; // PCL's
    p->cov_min_neighbours = 4;
}

int slam_kf_set_gicp_params(slam_kf_t *s, const slam_kf_gicp_params *params)
{
    SLAM_REQUIRE(s && params, SLAM_E_INVALID, "slam_kf_set_gicp_params: null argument");
    SLAM_TRY(check_gicp_params(params));
    SLAM_REQUIRE(s->n_cov == 0 || (params->k_correspondences == s->gp.k_correspondences && params->cov_radius == s->gp.cov_radius &&
                                   params->gicp_epsilon == s->gp.gicp_epsilon && params->cov_min_neighbours == s->gp.cov_min_neighbours),
                 SLAM_E_INVALID,
                 "slam_kf_set_gicp_params: k_correspondences, cov_radius, gicp_epsilon and cov_min_neighbours are fixed once a keyframe holds covariances");
    s->gp = *params;
    return SLAM_OK;
}

int slam_kf_compute_covariances(slam_kf_t *s, int id, slam_stream_t stream)
{
    SLAM_REQUIRE(kf_live(s, id), SLAM_E_INVALID, "slam_kf_compute_covariances: no keyframe %d", id);
    Keyframe &kf = s->kfs[id];
    if (kf.cov6) return SLAM_OK;
    const int    n = kf.view.n, K = s->gp.k_correspondences;
    const double edge = lattice_edge(s->p), radius = cov_radius(s);
    SLAM_REQUIRE(n >= K, SLAM_E_INVALID, "slam_kf_compute_covariances: keyframe %d has %d points, fewer than k_correspondences = %d", id, n, K);
    SLAM_REQUIRE(radius <= kMaxRings * edge, SLAM_E_INVALID, "slam_kf_compute_covariances: cov_radius %g is more than %d lattice edges of %g", radius,
                 kMaxRings, edge);
    CovParams P;
    P.inv_cell = inv_cell(s->p), P.edge = edge, P.radius2 = radius * radius, P.eps = s->gp.gicp_epsilon;
    P.k = K, P.rings = (int)ceil(radius / edge), P.min_nbr = s->gp.cov_min_neighbours;
    DevMem       mem;
    const size_t cov_b = sizeof(double) * 6 * (size_t)n, list_b = sizeof(int32_t) * (size_t)K * n;
    SLAM_TRY(mem.alloc(cov_b + 2 * list_b + sizeof(int32_t) * (size_t)n));
    double  *cov6 = mem.as<double>();
    int32_t *index = reinterpret_cast<int32_t *>(static_cast<char *>(mem.p) + cov_b);
    float   *dist2 = reinterpret_cast<float *>(index + (size_t)K * n);
    int32_t *count = reinterpret_cast<int32_t *>(dist2 + (size_t)K * n);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(kf_cov_kernel, dim3(blocks(n, kCovThreads)), dim3(kCovThreads), sizeof(unsigned long long) * kCovThreads * (size_t)K, st, kf.view, P,
                       cov6, index, dist2, count);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipStreamSynchronize(st));
    kf.cov = std::move(mem);
    kf.cov6 = cov6, kf.nbr_index = index, kf.nbr_dist2 = dist2, kf.nbr_count = count, kf.nbr_k = K;
    ++s->n_cov;
    return SLAM_OK;
}

int slam_kf_read_covariances(slam_kf_t *s, int id, double *cov6, int max_points, int *n_points)
{
    SLAM_REQUIRE(s && n_points && kf_live(s, id) && max_points >= 0 && (cov6 || max_points == 0), SLAM_E_INVALID,
                 "slam_kf_read_covariances: bad arguments");
    const Keyframe &k = s->kfs[id];
    SLAM_REQUIRE(k.cov6, SLAM_E_INVALID, "slam_kf_read_covariances: keyframe %d has no covariances yet", id);
    *n_points = k.view.n < max_points ? k.view.n : max_points;
    if (*n_points) SLAM_HIP(hipMemcpy(cov6, k.cov6, sizeof(double) * 6 * (size_t)*n_points, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_kf_read_neighbours(slam_kf_t *s, int id, int32_t *index, float *dist2, int32_t *count, int max_points, int *k)
{
    SLAM_REQUIRE(s && k && kf_live(s, id) && max_points >= 0, SLAM_E_INVALID, "slam_kf_read_neighbours: bad arguments");
    const Keyframe &kf = s->kfs[id];
    SLAM_REQUIRE(kf.cov6, SLAM_E_INVALID, "slam_kf_read_neighbours: keyframe %d has no covariances yet", id);
    *k = kf.nbr_k;
    const size_t n = (size_t)(kf.view.n < max_points ? kf.view.n : max_points);
    if (!n) return SLAM_OK;
    if (index) SLAM_HIP(hipMemcpy(index, kf.nbr_index, sizeof(int32_t) * n * kf.nbr_k, hipMemcpyDeviceToHost));
    if (dist2) SLAM_HIP(hipMemcpy(dist2, kf.nbr_dist2, sizeof(float) * n * kf.nbr_k, hipMemcpyDeviceToHost));
    if (count) SLAM_HIP(hipMemcpy(count, kf.nbr_count, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_kf_register_gicp_traced(slam_kf_t *s, const slam_kf_edge_req *req, int n_req, slam_kf_gicp_result *out, int32_t *pairs_trace, int trace_cap,
                                 slam_stream_t stream)
{
    SLAM_REQUIRE(s && n_req >= 0 && (n_req == 0 || (req && out)) && (!pairs_trace || trace_cap > 0), SLAM_E_INVALID,
                 "slam_kf_register_gicp: bad arguments");
    GicpParams P;
    P.inv_cell = inv_cell(s->p), P.gate2 = s->p.gate * s->p.gate;
    P.eps_t = s->gp.transformation_epsilon, P.eps_r = s->gp.rotation_epsilon, P.max_iter = s->gp.max_iterations;
    auto covariances = [&](GicpTask &t, const slam_kf_edge_req &r) -> int { // computed by the first request that names the keyframe
        SLAM_TRY(slam_kf_compute_covariances(s, r.from, stream));
        SLAM_TRY(slam_kf_compute_covariances(s, r.to, stream));
        t.src_cov = s->kfs[r.to].cov6, t.tgt_cov = s->kfs[r.from].cov6;
        return SLAM_OK;
    };
    return kf_register_batch(s, "slam_kf_register_gicp", "request", kf_gicp_kernel, s->gicp_lds_enabled, P, covariances, req, n_req, out, pairs_trace,
                             trace_cap, stream);
}

int slam_kf_register_gicp(slam_kf_t *s, const slam_kf_edge_req *req, int n, slam_kf_gicp_result *out, slam_stream_t stream)
{
    return slam_kf_register_gicp_traced(s, req, n, out, nullptr, 0, stream);
}
}
