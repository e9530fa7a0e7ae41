// kf_common.hpp -- what the keyframe store's two solvers share (kf_edge.hip: point-to-point ICP; kf_gicp.hip: covariances
// and Generalized ICP): the lattice view and its gated search, the fixed-order block reduction, the register-resident 3 x 3
// SVD and 6 x 6 inverse, the two ways a point is moved, the write of a result's transform, computeEdgeInformationLUM's pass,
// the store itself, the staging of a batch (BatchStage, which vmap_gicp.hip uses too) and the one host path of a batch of
// registrations between keyframes (kf_register_batch, at the end).
// Device code sits in an unnamed namespace on purpose: every translation unit compiles its own copy with internal linkage.
// Putting the host path here left the device code of all kernels of both files as it was (docs/KF_GICP.md section 2).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "device_mem.hpp"

using namespace slam;

namespace {

constexpr int                kHalf = 1 << 20; // 21 bits of cell coordinate per axis
constexpr unsigned long long kEmpty = ~0ull;
constexpr int                kEdgeThreads = 512;
constexpr int                kWaves = kEdgeThreads / 64;
constexpr double             kLatticeMargin = 1.0 + 1.0 / 65536.0;
constexpr int                kLdsPoints = 6144; // 96 KB of the CU's 160 KB: a make_cloud3d keyframe filtered at 0.5 m has up to 5 931

struct KfView {
    const float4 *pts;    // the filtered cloud, as the voxel filter wrote it
    const float4 *sorted; // the same points by cell key; w = the point's index in `pts` (bits)
    const int4   *table;  // x, y = cell key (low, high), z = first sorted point, w = points; key ~0 = empty
    unsigned      mask;   // slots - 1
    int           n;
};

__host__ __device__ inline int cell_coord(float v, double inv)
{
    double c = floor((double)v * inv);
    if (!(c >= -(double)kHalf)) c = -(double)kHalf; // also NaN
    if (c > (double)(kHalf - 1)) c = (double)(kHalf - 1);
    return (int)c + kHalf;
}
__host__ __device__ inline unsigned long long cell_key(int cx, int cy, int cz)
{
    return ((unsigned long long)cz << 42) | ((unsigned long long)cy << 21) | (unsigned long long)cx;
}
__device__ inline unsigned slot_of(unsigned long long key, unsigned mask)
{
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// The nearest point among the 27 cells around q: its index in the filtered cloud (lowest on an exact tie) or -1, the f32
// squared distance dx dx + dy dy + dz dz summed in that order without FMA, and the sorted slot it sits in.  The query's own
// cell goes first; a neighbouring cell is looked up only if the slab between it and the query is no wider than the best
// distance so far and than the gate (a point beyond the gate is dropped by both callers).  The slab width is a lower bound
// of the distance to every point of that cell, taken in double; the 2^-20 of slack is above the 3 ulp of the f32 sum, so no
// point that could win or tie is skipped and the result is that of the full search (tests hold it against brute force).
constexpr double kPruneSlack = 1.0 + 1.0 / 1048576.0;

__device__ inline int nearest27(const KfView &t, double inv, double gate2, float qx, float qy, float qz, float *d2, int *slot)
{
    const float  q[3] = {qx, qy, qz};
    const double cell = 1.0 / inv;
    int          c[3];
    double       lo[3], hi[3]; // distance to the lower and upper face of the query's cell
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double u = (double)q[k] * inv, f = floor(u);
        c[k] = cell_coord(q[k], inv);
        const bool inside = (double)(c[k] - kHalf) == f; // not clamped, not NaN
        lo[k] = inside ? (u - f) * cell : 0.0;
        hi[k] = inside ? ((f + 1.0) - u) * cell : 0.0;
    }
    int   best = -1, bslot = -1;
    float bd = 0.0f;
    auto  visit = [&](int x, int y, int z) {
        if ((x | y | z) < 0 || x >= 2 * kHalf || y >= 2 * kHalf || z >= 2 * kHalf) return;
        const unsigned long long key = cell_key(x, y, z);
        unsigned                 h = slot_of(key, t.mask);
        int                      start = 0, count = 0;
        for (;;) { // at most half the slots are taken: the probe ends
            const int4               s = t.table[h];
            const unsigned long long k = ((unsigned long long)(unsigned)s.y << 32) | (unsigned)s.x;
            if (k == key) {
                start = s.z, count = s.w;
                break;
            }
            if (k == kEmpty) break;
            h = (h + 1) & t.mask;
        }
        for (int j = start; j < start + count; ++j) {
            const float4 p = t.sorted[j];
            const float  dx = __fsub_rn(qx, p.x), dy = __fsub_rn(qy, p.y), dz = __fsub_rn(qz, p.z);
            const float  d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            const int    idx = __float_as_int(p.w);
            if (best < 0 || d < bd || (d == bd && idx < best)) best = idx, bd = d, bslot = j;
        }
    };
    visit(c[0], c[1], c[2]);
    const double gate_bound = gate2 * kPruneSlack;
    for (int oz = -1; oz <= 1; ++oz) {
        const double mz = oz < 0 ? lo[2] : oz > 0 ? hi[2] : 0.0;
        for (int oy = -1; oy <= 1; ++oy) {
            const double my = oy < 0 ? lo[1] : oy > 0 ? hi[1] : 0.0;
            for (int ox = -1; ox <= 1; ++ox) {
                if (!(ox | oy | oz)) continue;
                const double mx = ox < 0 ? lo[0] : ox > 0 ? hi[0] : 0.0;
                const double m2 = (mx * mx + my * my) + mz * mz;
                if (m2 > gate_bound || (best >= 0 && m2 > (double)bd * kPruneSlack)) continue;
                visit(c[0] + ox, c[1] + oy, c[2] + oz);
            }
        }
    }
    *d2 = bd;
    *slot = bslot;
    return best;
}

// ---------------------------------------------------------------- the 3 x 3 solve (one lane, f64)
// Every loop below has constant bounds and is unrolled, so that the small matrices stay in registers: indexed by a
// run-time value they would live in scratch memory, and one lane's trips there were most of an iteration.
__device__ inline void swap_columns(double a[9], double v[9], double s[3], int i, int j)
{
    double x = s[i];
    s[i] = s[j], s[j] = x;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        x = a[3 * r + i], a[3 * r + i] = a[3 * r + j], a[3 * r + j] = x;
        x = v[3 * r + i], v[3 * r + i] = v[3 * r + j], v[3 * r + j] = x;
    }
}

// One-sided Jacobi SVD: A = U diag(s) V', s descending; columns of U for vanishing singular values completed to a
// right-handed frame.  Returns the rank (singular values above 3 eps of the largest).
__device__ int svd3(const double A[9], double U[9], double s[3], double V[9])
{
    const double eps = DBL_EPSILON;
    double       a[9], v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = A[i], v[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    al += a[3 * i + p] * a[3 * i + p];
                    be += a[3 * i + q] * a[3 * i + q];
                    ga += a[3 * i + p] * a[3 * i + q];
                }
                if (ga == 0.0 || fabs(ga) <= eps * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double ap = a[3 * i + p], aq = a[3 * i + q];
                    a[3 * i + p] = c * ap - sn * aq;
                    a[3 * i + q] = sn * ap + c * aq;
                    const double vp = v[3 * i + p], vq = v[3 * i + q];
                    v[3 * i + p] = c * vp - sn * vq;
                    v[3 * i + q] = sn * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s[j] = sqrt(a[j] * a[j] + a[3 + j] * a[3 + j] + a[6 + j] * a[6 + j]);
    // descending, stable: the selection sort of the restatement as three compare-and-swaps
    if (s[1] > s[0]) swap_columns(a, v, s, 0, 1);
    if (s[2] > s[0]) swap_columns(a, v, s, 0, 2);
    if (s[2] > s[1]) swap_columns(a, v, s, 1, 2);
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (s[j] > 0.0 && s[j] > 3.0 * eps * s[0]) ++rank;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (j < rank) {
#pragma unroll
            for (int i = 0; i < 3; ++i) a[3 * i + j] /= s[j];
        }
    if (rank == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
        if (rank == 1) { // any unit vector orthogonal to u0: u0 x e_k, e_k the axis u0 leans on least
            int    k = 0;
            double m = fabs(a[0]);
            if (fabs(a[3]) < m) k = 1, m = fabs(a[3]);
            if (fabs(a[6]) < m) k = 2;
            const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
            const double w[3] = {a[3] * e[2] - a[6] * e[1], a[6] * e[0] - a[0] * e[2], a[0] * e[1] - a[3] * e[0]};
            const double nw = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            a[1] = w[0] / nw, a[4] = w[1] / nw, a[7] = w[2] / nw;
        }
        if (rank <= 2) { // u2 = u0 x u1
            a[2] = a[3] * a[7] - a[6] * a[4];
            a[5] = a[6] * a[1] - a[0] * a[7];
            a[8] = a[0] * a[4] - a[3] * a[1];
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) U[i] = a[i], V[i] = v[i];
    return rank;
}

// The inverse of a 6 x 6 by LU with partial pivoting (what Eigen's inverse() of a fixed 6 x 6 goes through).  A vanishing
// pivot divides by zero; the non-finite entries travel on to ss, where the test of :203 catches them.  Unrolled like the
// solve above: the pivot row is found by value and swapped in by a chain of conditional swaps.
__device__ void inverse6(const double A[36], double X[36])
{
    double a[36];
    int    piv[6];
#pragma unroll
    for (int i = 0; i < 36; ++i) a[i] = A[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) piv[i] = i;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int    m = k;
        double big = fabs(a[6 * k + k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
            if (fabs(a[6 * i + k]) > big) big = fabs(a[6 * i + k]), m = i;
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
            if (i == m) {
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const double x = a[6 * k + c];
                    a[6 * k + c] = a[6 * i + c], a[6 * i + c] = x;
                }
                const int x = piv[k];
                piv[k] = piv[i], piv[i] = x;
            }
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            a[6 * i + k] /= a[6 * k + k];
#pragma unroll
            for (int c = k + 1; c < 6; ++c) a[6 * i + c] -= a[6 * i + k] * a[6 * k + c];
        }
    }
#pragma unroll
    for (int col = 0; col < 6; ++col) {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            y[i] = piv[i] == col ? 1.0 : 0.0;
#pragma unroll
            for (int c = 0; c < i; ++c) y[i] -= a[6 * i + c] * y[c];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
#pragma unroll
            for (int c = i + 1; c < 6; ++c) y[i] -= a[6 * i + c] * y[c];
            y[i] /= a[6 * i + i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) X[6 * i + col] = y[i];
    }
}

// ---------------------------------------------------------------- reductions in a fixed order
template <typename T, int K>
__device__ inline void block_sum(T (&v)[K], T (*red)[16], T *tot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) red[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        T s = red[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) s += red[w][threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
}

// the source point moved by the total transform: in double, rounded to f32 once
__device__ inline void move_f64(const double T[12], const float4 p, float m[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) m[r] = (float)(((T[4 * r] * (double)p.x + T[4 * r + 1] * (double)p.y) + T[4 * r + 2] * (double)p.z) + T[4 * r + 3]);
}
// pcl::transformPointCloud with a Matrix4f: in float, left to right
__device__ inline void move_f32(const float M[12], const float4 p, float m[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
        m[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[4 * r], p.x), __fmul_rn(M[4 * r + 1], p.y)), __fmul_rn(M[4 * r + 2], p.z)), M[4 * r + 3]);
}
// Thread 0's, once a registration's loop has ended: the total transform sT as the result's f64 and f32 4 x 4, and the f32
// rows in sTf for the passes that follow
__device__ __forceinline__ void write_transform(const double *sT, float *sTf, double *transform64, float *transform)
{
    for (int k = 0; k < 12; ++k) {
        transform64[k] = sT[k];
        transform[k] = sTf[k] = (float)sT[k];
    }
    for (int k = 12; k < 16; ++k) transform64[k] = k == 15 ? 1.0 : 0.0, transform[k] = k == 15 ? 1.0f : 0.0f;
}
// computeEdgeInformationLUM on the f32 transform sTf (:108-214), by the whole workgroup; the LUM fields of `out` are thread
// 0's to write.  corr[i] is left holding the sorted slot of source point i's partner strictly inside the gate, or -1.
__device__ __forceinline__ void lum_pass(const KfView &src, const KfView &tgt, int32_t *corr, double inv_cell, double gate2, const float *sTf,
                                         double (*red)[16], double *tot, float (*redf)[16], float *totf, double *sD, double *sMM,
                                         slam_kf_edge_result *out)
{
    const int tid = threadIdx.x;
    // computeEdgeInformationLUM on the f32 transform (:108-214)
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = sTf[k];
    double a16[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < src.n; i += kEdgeThreads) {
        float s[3], d2;
        int   slot;
        move_f32(M, src.pts[i], s);
        const int  j = nearest27(tgt, inv_cell, gate2, s[0], s[1], s[2], &d2, &slot);
        const bool keep = j >= 0 && (double)d2 < gate2; // :132, strict
        corr[i] = keep ? slot : -1;
        if (!keep) continue;
        const float4 q = tgt.sorted[slot];
        const float  a0 = __fmul_rn(0.5f, __fadd_rn(s[0], q.x)), a1 = __fmul_rn(0.5f, __fadd_rn(s[1], q.y)), a2 = __fmul_rn(0.5f, __fadd_rn(s[2], q.z));
        const float  d0 = __fsub_rn(s[0], q.x), d1 = __fsub_rn(s[1], q.y), d2f = __fsub_rn(s[2], q.z);
        a16[0] += 1.0;
        a16[1] += (double)a0, a16[2] += (double)a1, a16[3] += (double)a2; // :155-160, up to sign
        a16[4] += (double)__fmul_rn(a0, a2);                              // -(3,4)
        a16[5] += (double)__fmul_rn(a0, a1);                              // -(3,5)
        a16[6] += (double)__fmul_rn(a1, a2);                              // -(4,5)
        a16[7] += (double)__fadd_rn(__fmul_rn(a1, a1), __fmul_rn(a2, a2));
        a16[8] += (double)__fadd_rn(__fmul_rn(a0, a0), __fmul_rn(a1, a1));
        a16[9] += (double)__fadd_rn(__fmul_rn(a0, a0), __fmul_rn(a2, a2));
        a16[10] += (double)d0, a16[11] += (double)d1, a16[12] += (double)d2f;
        a16[13] += (double)__fsub_rn(__fmul_rn(a1, d2f), __fmul_rn(a2, d1));
        a16[14] += (double)__fsub_rn(__fmul_rn(a0, d1), __fmul_rn(a1, d0));
        a16[15] += (double)__fsub_rn(__fmul_rn(a2, d0), __fmul_rn(a0, d2f));
    }
    block_sum<double, 16>(a16, red, tot);
    if (tid == 0) {
        double MM[36];
        for (int k = 0; k < 36; ++k) MM[k] = 0.0;
#define MMAT(r, c) MM[6 * (r) + (c)]
        MMAT(0, 4) = -tot[2], MMAT(0, 5) = tot[3], MMAT(1, 3) = -tot[3], MMAT(1, 4) = tot[1], MMAT(2, 3) = tot[2], MMAT(2, 5) = -tot[1];
        MMAT(3, 4) = -tot[4], MMAT(3, 5) = -tot[5], MMAT(4, 5) = -tot[6];
        MMAT(3, 3) = tot[7], MMAT(4, 4) = tot[8], MMAT(5, 5) = tot[9];
        MMAT(0, 0) = MMAT(1, 1) = MMAT(2, 2) = (double)(float)(int)tot[0];
        MMAT(4, 0) = MMAT(0, 4), MMAT(5, 0) = MMAT(0, 5), MMAT(3, 1) = MMAT(1, 3), MMAT(4, 1) = MMAT(1, 4), MMAT(3, 2) = MMAT(2, 3);
        MMAT(5, 2) = MMAT(2, 5), MMAT(4, 3) = MMAT(3, 4), MMAT(5, 3) = MMAT(3, 5), MMAT(5, 4) = MMAT(4, 5);
#undef MMAT
        double inv[36];
        inverse6(MM, inv);
        for (int k = 0; k < 36; ++k) sMM[k] = MM[k];
        for (int r = 0; r < 6; ++r) {
            double d = 0.0;
            for (int c = 0; c < 6; ++c) d += inv[6 * r + c] * tot[10 + c];
            sD[r] = d;
        }
    }
    __syncthreads();
    double D[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) D[k] = sD[k];
    float ssv[1] = {0.0f};
    for (int i = tid; i < src.n; i += kEdgeThreads) {
        const int slot = corr[i];
        if (slot < 0) continue;
        float s[3];
        move_f32(M, src.pts[i], s);
        const float4 q = tgt.sorted[slot];
        const float  a0 = __fmul_rn(0.5f, __fadd_rn(s[0], q.x)), a1 = __fmul_rn(0.5f, __fadd_rn(s[1], q.y)), a2 = __fmul_rn(0.5f, __fadd_rn(s[2], q.z));
        const float  d0 = __fsub_rn(s[0], q.x), d1 = __fsub_rn(s[1], q.y), d2f = __fsub_rn(s[2], q.z);
        const double e0 = (double)d0 - ((D[0] + (double)a2 * D[5]) - (double)a1 * D[4]); // :197-199 as written
        const double e1 = (double)d1 - ((D[1] + (double)a0 * D[4]) - (double)a2 * D[3]);
        const double e2 = (double)d2f - ((D[2] + (double)a1 * D[3]) - (double)a0 * D[5]);
        ssv[0] = __fadd_rn(ssv[0], (float)((e0 * e0 + e1 * e1) + e2 * e2));
    }
    block_sum<float, 1>(ssv, redf, totf);
    if (tid == 0) {
        const float ss = totf[0];
        const bool  singular = ss < 0.0000000000001 || !isfinite(ss); // :203
        const float w = 1.0f / ss;                                    // :211
        for (int k = 0; k < 36; ++k) out->information[k] = singular ? (k % 7 == 0 ? 1.0 : 0.0) : sMM[k] * (double)w;
        out->num_corr = (int)tot[0], out->singular = singular ? 1 : 0, out->ss = ss;
    }
}

struct Keyframe {
    DevMem block; // pts | sorted | table
    KfView view{};
    int    n_cells = 0, max_cell = 0;
    // Generalized ICP's (kf_gicp.hip), filled by slam_kf_compute_covariances: per point of the filtered cloud six doubles
    // of C', then the neighbour lists the covariances were summed over: k indices, k f32 squared distances, one count
    DevMem  cov;
    double *cov6 = nullptr;
    int32_t *nbr_index = nullptr, *nbr_count = nullptr;
    float   *nbr_dist2 = nullptr;
    int      nbr_k = 0;
    DevMem   sc; // the scan-context descriptor (kf_sc.hip), filled by slam_kf_sc_compute: n_rings x n_sectors bytes, ring-major
    bool     removed = false; // slam_kf_remove_keyframe: the id stays issued, the memory is gone, every call refuses it
};

} // namespace

struct slam_kf {
    slam_kf_params        p;
    slam_kf_gicp_params   gp;
    slam_ccicp_t         *cc = nullptr;
    std::vector<Keyframe> kfs;
    bool                  lds_enabled = false, gicp_lds_enabled = false;
    int                   n_cov = 0; // keyframes that hold covariances: their parameters are fixed from the first on
    // kf_sc.hip: the descriptor's parameters, fixed from the first descriptor on (n_sc counts the ones computed), and the
    // host's tables of them -- squared ring edges, cos and sin of the sector boundaries of a quadrant
    slam_kf_sc_params sp{20, 64, 80.0, -2.0, 0.02};
    int               n_sc = 0;
    bool              sc_tables_ready = false;
    double            sc_edge2[32], sc_cos[32], sc_sin[32];
    DevMem                in, filtered, keys, sort_tmp, work, stats; // add_keyframe's; `work` also holds a call's tasks, results, pairs
    ~slam_kf() { slam_ccicp_destroy(cc); }
};

namespace {

// an id that was issued and not removed
inline bool     kf_live(const slam_kf *s, int id) { return s && id >= 0 && id < (int)s->kfs.size() && !s->kfs[id].removed; }
inline double   inv_cell(const slam_kf_params &p) { return 1.0 / ((p.cell_size > 0 ? p.cell_size : p.gate) * kLatticeMargin); }
inline unsigned blocks(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------- the staging of one batch of registrations
// A work buffer holds tasks | results | trace | extra, each from a multiple of 256 bytes; all but `extra` (device only, the
// caller's) are mirrored in pinned memory.  lay_out, the caller writes the tasks into the mirror, upload, the caller's one
// launch, download: one upload, one download, one wait.  Between lay_out and download nobody else may touch the work buffer
// or call pinned_scratch.
template <typename Task, typename Result>
struct BatchStage {
    hipStream_t st;
    size_t      task_b, res_b, trace_b, res_off, trace_off, extra_off;
    char       *host, *dev;

    int lay_out(DevMem &work, const char *who, int n, int trace_cap, size_t extra_b, hipStream_t stream)
    {
        st = stream;
        task_b = sizeof(Task) * (size_t)n, res_b = sizeof(Result) * (size_t)n, trace_b = sizeof(int32_t) * (size_t)n * trace_cap;
        res_off = (task_b + 255) & ~(size_t)255, trace_off = res_off + ((res_b + 255) & ~(size_t)255);
        extra_off = trace_off + ((trace_b + 255) & ~(size_t)255);
        SLAM_TRY(reserve_quarter(work, extra_off + extra_b));
        host = static_cast<char *>(pinned_scratch(extra_off));
        SLAM_REQUIRE(host, SLAM_E_NOMEM, "%s: no pinned staging memory", who);
        dev = static_cast<char *>(work.p);
        return SLAM_OK;
    }
    Task       *tasks() const { return reinterpret_cast<Task *>(host); }
    const Task *dev_tasks() const { return reinterpret_cast<const Task *>(dev); }
    Result     *dev_results() const { return reinterpret_cast<Result *>(dev + res_off); }
    int32_t    *dev_trace() const { return trace_b ? reinterpret_cast<int32_t *>(dev + trace_off) : nullptr; } // null without a trace
    char       *dev_extra() const { return dev + extra_off; }
    int         upload() const
    {
        SLAM_HIP(hipMemcpyAsync(dev, host, task_b, hipMemcpyHostToDevice, st));
        return SLAM_OK;
    }
    int download(Result *out, int32_t *pairs_trace) const
    {
        SLAM_HIP(hipMemcpyAsync(host + res_off, dev + res_off, (trace_off - res_off) + trace_b, hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipStreamSynchronize(st));
        std::memcpy(out, host + res_off, res_b);
        if (trace_b) std::memcpy(pairs_trace, host + trace_off, trace_b);
        return SLAM_OK;
    }
};

// ---------------------------------------------------------------- one batch of registrations, from the requests to the results
// The host path of both of the store's solvers: `who` is the entry point's name and `what` its word for a request (both for
// the error texts), `kernel` runs one workgroup per request, `lds_enabled` is that kernel's flag in the store (its dynamic
// LDS limit is raised at most once per store), `fill(task, request)` adds what the task holds beyond the views, `corr` and
// `init` (which every task type has under these names) and may refuse.  It runs after the staging is laid out: it may launch
// work on the stream and wait for it (Generalized ICP computes missing covariances there), but must not touch s->work or
// call pinned_scratch.  The staging's `extra` is corr: one int per source point of every request.
template <typename Task, typename Result, typename Params, typename Fill>
int kf_register_batch(slam_kf *s, const char *who, const char *what, void (*kernel)(const Task *, Params, Result *, int32_t *, int, int),
                      bool &lds_enabled, const Params &P, Fill fill, const slam_kf_edge_req *req, int n, Result *out, int32_t *pairs_trace,
                      int trace_cap, slam_stream_t stream)
{
    const int nk = (int)s->kfs.size();
    size_t    n_corr = 0;
    for (int e = 0; e < n; ++e) {
        SLAM_REQUIRE(kf_live(s, req[e].from) && kf_live(s, req[e].to), SLAM_E_INVALID,
                     "%s: %s %d names keyframes %d -> %d, the store holds %d (removed ones are refused)", who, what, e, req[e].from, req[e].to, nk);
        n_corr += (size_t)s->kfs[req[e].to].view.n;
    }
    if (n == 0) return SLAM_OK;
    if (!pairs_trace) trace_cap = 0;
    BatchStage<Task, Result> stage;
    SLAM_TRY(stage.lay_out(s->work, who, n, trace_cap, sizeof(int32_t) * n_corr, as_stream(stream)));
    Task    *tasks = stage.tasks();
    int32_t *corr = reinterpret_cast<int32_t *>(stage.dev_extra());
    int      lds_points = 0;
    for (int e = 0; e < n; ++e) {
        const Keyframe &src = s->kfs[req[e].to], &tgt = s->kfs[req[e].from];
        tasks[e].src = src.view, tasks[e].tgt = tgt.view;
        tasks[e].corr = corr;
        corr += src.view.n;
        std::memcpy(tasks[e].init, req[e].init, sizeof tasks[e].init);
        SLAM_TRY(fill(tasks[e], req[e]));
        if (s->p.target_in_lds && tgt.view.n <= kLdsPoints && tgt.view.n > lds_points) lds_points = tgt.view.n;
    }
    if (lds_points && !lds_enabled) {
        SLAM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(sizeof(float4) * kLdsPoints)));
        lds_enabled = true;
    }
    SLAM_TRY(stage.upload());
    hipLaunchKernelGGL(kernel, dim3(n), dim3(kEdgeThreads), sizeof(float4) * (size_t)lds_points, stage.st, stage.dev_tasks(), P, stage.dev_results(),
                       stage.dev_trace(), trace_cap, lds_points);
    SLAM_HIP(hipGetLastError());
    return stage.download(out, pairs_trace);
}

} // namespace
