// pgo.hip -- the pose-graph optimiser behind slam_pgo_* (docs/PGO.md): SE3 vertices and edges as g2o's VertexSE3 / EdgeSE3,
// Levenberg-Marquardt as its OptimizationAlgorithmLevenberg.  The graph lives on the host; a call uploads it, and the device
// runs straight-line stages: linearise (one lane per edge, into per-edge slots), assemble (one block row per workgroup, the
// row's slots in ascending edge index: no floating-point atomics, the same bits every run), factor and solve (a block-banded
// Cholesky in ONE workgroup, so nothing ever waits on another workgroup), update, and a fixed-order reduction.  The LM
// control is the host's: one pinned record per trial.  Everything is f64 and compiled without contraction.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "device_mem.hpp"

namespace {

using namespace slam;

constexpr int kSlot = 164; // doubles per edge: four 6 x 6 products (ii ij ji jj), J_i' W e, J_j' W e, e, chi2, pad
constexpr int kSlotG = 144, kSlotE = 156, kSlotChi2 = 162;
constexpr int kRec = 8; // doubles of the trial record
enum { REC_CHI2 = 0, REC_CHI2_CAND = 1, REC_SCALE = 2, REC_LAMBDA = 3, REC_MAXDIAG = 4, REC_PIVOT = 5 };
constexpr int kFactorThreads = 256;

struct PgoEdge {
    int    from, to;
    double zinv[7]; // t, q of Z^-1
    double info[36];
};

struct RowEnt {
    int edge;
    int which; // 0: this row is the edge's `from`, 1: its `to`
    int other; // block row of the other end, -1 where that one is fixed
};

struct Quat {
    double x, y, z, w;
};

__host__ __device__ inline Quat qmul(const Quat &a, const Quat &b)
{
    Quat r;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    return r;
}

__host__ __device__ inline void qmat(const Quat &q, double R[9])
{
    const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z, wx = q.w * q.x,
                 wy = q.w * q.y, wz = q.w * q.z;
    R[0] = 1.0 - 2.0 * (yy + zz), R[1] = 2.0 * (xy - wz), R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz), R[4] = 1.0 - 2.0 * (xx + zz), R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy), R[7] = 2.0 * (yz + wx), R[8] = 1.0 - 2.0 * (xx + yy);
}

// What every edge computation starts from: A = Z^-1, B = Xi^-1 Xj, the error quaternion and translation.
struct EdgeGeom {
    Quat   qa, qb, qe;
    double Ra[9], tb[3], te[3], s;
};

__device__ inline void edge_geom(const PgoEdge &E, const double *pose, EdgeGeom &G)
{
    const double *pi = pose + 7 * (size_t)E.from, *pj = pose + 7 * (size_t)E.to;
    const Quat    qi_conj = {-pi[3], -pi[4], -pi[5], pi[6]}, qj = {pj[3], pj[4], pj[5], pj[6]};
    G.qa = Quat{E.zinv[3], E.zinv[4], E.zinv[5], E.zinv[6]};
    G.qb = qmul(qi_conj, qj);
    G.qe = qmul(G.qa, G.qb);
    double Rit[9];
    qmat(qi_conj, Rit);
    const double d[3] = {pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]};
    for (int r = 0; r < 3; ++r) G.tb[r] = Rit[3 * r] * d[0] + Rit[3 * r + 1] * d[1] + Rit[3 * r + 2] * d[2];
    qmat(G.qa, G.Ra);
    for (int r = 0; r < 3; ++r) G.te[r] = G.Ra[3 * r] * G.tb[0] + G.Ra[3 * r + 1] * G.tb[1] + G.Ra[3 * r + 2] * G.tb[2] + E.zinv[r];
    G.s = G.qe.w >= 0.0 ? 1.0 : -1.0;
}

__device__ inline void cross_matrix(const double v[3], double M[9])
{
    M[0] = 0.0, M[1] = -v[2], M[2] = v[1];
    M[3] = v[2], M[4] = 0.0, M[5] = -v[0];
    M[6] = -v[1], M[7] = v[0], M[8] = 0.0;
}

__device__ inline void mat3_mul(const double A[9], const double B[9], double C[9])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// One lane per edge.  FULL: the slot (products, gradients, e, chi2); otherwise e' W e alone, for candidate poses.
template <bool FULL>
__global__ __launch_bounds__(64) void pgo_linearize_kernel(const PgoEdge *__restrict__ edges, int n_edges, const double *__restrict__ pose,
                                                           double *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_edges) return;
    const PgoEdge &E = edges[k];
    EdgeGeom       G;
    edge_geom(E, pose, G);
    const double e[6] = {G.te[0], G.te[1], G.te[2], G.s * G.qe.x, G.s * G.qe.y, G.s * G.qe.z};
    double       We[6], chi2 = 0.0;
    for (int r = 0; r < 6; ++r) {
        double a = 0.0;
        for (int c = 0; c < 6; ++c) a += E.info[6 * r + c] * e[c];
        We[r] = a;
    }
    for (int r = 0; r < 6; ++r) chi2 += e[r] * We[r];
    if (!FULL) {
        out[k] = chi2;
        return;
    }
    double *slot = out + (size_t)k * kSlot;
    // the two Jacobians with respect to the right-multiplied increments (docs/PGO.md)
    double J[2][36];
    for (int a = 0; a < 2; ++a)
        for (int m = 0; m < 36; ++m) J[a][m] = 0.0;
    double Rb[9], Re[9], X[9], RaX[9];
    qmat(G.qb, Rb);
    mat3_mul(G.Ra, Rb, Re);
    cross_matrix(G.tb, X);
    mat3_mul(G.Ra, X, RaX);
    const double ve[3] = {G.qe.x, G.qe.y, G.qe.z}, va[3] = {G.qa.x, G.qa.y, G.qa.z}, vb[3] = {G.qb.x, G.qb.y, G.qb.z};
    double       Xe[9], Xa[9], Xb[9], P[9], Q[9], M[9];
    cross_matrix(ve, Xe);
    cross_matrix(va, Xa);
    cross_matrix(vb, Xb);
    for (int m = 0; m < 9; ++m) {
        const double id = (m % 4 == 0) ? 1.0 : 0.0;
        P[m] = G.qa.w * id + Xa[m];
        Q[m] = G.qb.w * id - Xb[m];
    }
    mat3_mul(P, Q, M); // [L(qa) Rm(qb)]_3 = (wa I + [va]x)(wb I - [vb]x) - va vb'
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            M[3 * r + c] -= va[r] * vb[c];
            const double id = r == c ? 1.0 : 0.0;
            J[0][6 * r + c] = -G.Ra[3 * r + c];
            J[0][6 * r + 3 + c] = 2.0 * RaX[3 * r + c];
            J[0][6 * (3 + r) + 3 + c] = -G.s * M[3 * r + c];
            J[1][6 * r + c] = Re[3 * r + c];
            J[1][6 * (3 + r) + 3 + c] = G.s * (G.qe.w * id + Xe[3 * r + c]);
        }
    for (int a = 0; a < 2; ++a)
        for (int c = 0; c < 6; ++c) {
            double g = 0.0;
            for (int r = 0; r < 6; ++r) g += J[a][6 * r + c] * We[r];
            slot[kSlotG + 6 * a + c] = g;
        }
    for (int c2 = 0; c2 < 2; ++c2) {
        double T[36]; // W J_c2
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                double s = 0.0;
                for (int m = 0; m < 6; ++m) s += E.info[6 * r + m] * J[c2][6 * m + c];
                T[6 * r + c] = s;
            }
        for (int a = 0; a < 2; ++a)
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) {
                    double s = 0.0;
                    for (int m = 0; m < 6; ++m) s += J[a][6 * m + r] * T[6 * m + c];
                    slot[(2 * a + c2) * 36 + 6 * r + c] = s;
                }
    }
    for (int r = 0; r < 6; ++r) slot[kSlotE + r] = e[r];
    slot[kSlotChi2] = chi2;
    slot[kSlotChi2 + 1] = 0.0;
}

// One block row per workgroup of 64.  Lane t < 36 owns element t of every block of the row, lanes 36..41 the row's b; each
// walks the row's incident edges in ascending edge index.  Block (r, r - d) is at ((r (w + 1) + d) 36).
__global__ __launch_bounds__(64) void pgo_assemble_kernel(const double *__restrict__ slots, const int *__restrict__ rowptr,
                                                          const RowEnt *__restrict__ ent, int n, int w, double *__restrict__ band,
                                                          double *__restrict__ b, double *__restrict__ rowmax)
{
    const int r = blockIdx.x, t = threadIdx.x;
    if (r >= n) return;
    double *row = band + (size_t)r * (w + 1) * 36;
    for (int k = t; k < (w + 1) * 36; k += 64) row[k] = 0.0;
    __syncthreads();
    const int p0 = rowptr[r], p1 = rowptr[r + 1];
    if (t < 36) {
        double diag = 0.0;
        for (int p = p0; p < p1; ++p) {
            const RowEnt  en = ent[p];
            const double *s = slots + (size_t)en.edge * kSlot;
            diag += s[(3 * en.which) * 36 + t];
            if (en.other >= 0 && en.other < r && r - en.other <= w) row[(r - en.other) * 36 + t] += s[(2 * en.which + (1 - en.which)) * 36 + t];
        }
        row[t] = diag;
    } else if (t < 42) {
        double g = 0.0;
        for (int p = p0; p < p1; ++p) {
            const RowEnt en = ent[p];
            g += slots[(size_t)en.edge * kSlot + kSlotG + 6 * en.which + (t - 36)];
        }
        b[6 * r + (t - 36)] = -g;
    }
    __syncthreads();
    if (t == 0) {
        double m = row[0];
        for (int c = 1; c < 6; ++c) m = fmax(m, row[7 * c]);
        rowmax[r] = m;
    }
}

// Sum (op 0) or maximum (op 1) of in[0], in[stride], ... in one workgroup: strided partials, then a tree in LDS.  The order is
// a function of n alone.
__global__ __launch_bounds__(256) void pgo_reduce_kernel(const double *__restrict__ in, int stride, int n, int op, double *__restrict__ out)
{
    __shared__ double red[256];
    const int         t = threadIdx.x;
    double            a = 0.0;
    bool              any = false;
    for (int k = t; k < n; k += 256) {
        const double v = in[(size_t)k * stride];
        a = !any ? v : (op ? fmax(a, v) : a + v);
        any = true;
    }
    red[t] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h && t + h < n) red[t] = op ? fmax(red[t], red[t + h]) : red[t] + red[t + h];
        __syncthreads();
    }
    if (t == 0) *out = n > 0 ? red[0] : 0.0;
}

// ONE workgroup: copies the band, adds lambda, factors it (right-looking block-banded Cholesky), substitutes forward and
// back, and writes delta in vertex numbering with sum delta (lambda delta + b).  Every loop bound is a kernel argument; a
// pivot <= 0 goes through an LDS flag that all threads read after a barrier, so they leave together.
// lambda = tau * maxdiag[0] where tau > 0 (iteration 0), lambda_abs otherwise.
__global__ __launch_bounds__(kFactorThreads) void pgo_factor_solve_kernel(const double *__restrict__ band, const double *__restrict__ b,
                                                                          const int *__restrict__ perm, int n, int n_vertices, int w,
                                                                          double lambda_abs, double tau, const double *__restrict__ maxdiag,
                                                                          double *work, double *y, double *delta, double *rec)
{
    __shared__ double Lkk[36];
    __shared__ int    bad;
    __shared__ double red[kFactorThreads];
    const int         t = threadIdx.x, T = kFactorThreads, W1 = w + 1;
    const double      lambda = tau > 0.0 ? tau * maxdiag[0] : lambda_abs;
    const size_t      total = (size_t)n * W1 * 36;
    for (size_t k = t; k < total; k += T) {
        double       v = band[k];
        const size_t blk = k / 36;
        const int    el = (int)(k % 36);
        if (blk % W1 == 0 && el % 7 == 0) v += lambda;
        work[k] = v;
    }
    for (int k = t; k < 6 * n; k += T) y[k] = b[k];
    for (int k = t; k < 6 * n_vertices; k += T) delta[k] = 0.0;
    if (t == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        double *D = work + (size_t)k * W1 * 36;
        if (t == 0) {
            for (int j = 0; j < 6 && !bad; ++j) {
                double s = D[7 * j];
                for (int m = 0; m < j; ++m) s -= Lkk[6 * j + m] * Lkk[6 * j + m];
                if (!(s > 0.0)) {
                    bad = 1;
                    break;
                }
                const double d = sqrt(s);
                Lkk[7 * j] = d;
                for (int i = j + 1; i < 6; ++i) {
                    double v = D[6 * i + j];
                    for (int m = 0; m < j; ++m) v -= Lkk[6 * i + m] * Lkk[6 * j + m];
                    Lkk[6 * i + j] = v / d;
                    Lkk[6 * j + i] = 0.0;
                }
            }
            if (!bad)
                for (int m = 0; m < 36; ++m) D[m] = Lkk[m];
        }
        __syncthreads();
        if (bad) break;
        const int m = min(w, n - 1 - k);
        // panel: block (k + 1 + a, k) <- block L_kk^-T, one row of a block per task
        for (int task = t; task < 6 * m; task += T) {
            const int a = task / 6, row = task % 6;
            double   *B = work + ((size_t)(k + 1 + a) * W1 + (a + 1)) * 36 + 6 * row;
            double    x[6];
            for (int c = 0; c < 6; ++c) {
                double v = B[c];
                for (int mm = 0; mm < c; ++mm) v -= x[mm] * Lkk[6 * c + mm];
                x[c] = v / Lkk[7 * c];
            }
            for (int c = 0; c < 6; ++c) B[c] = x[c];
        }
        __syncthreads();
        // trailing update: block (k+1+a, k+1+c) -= L_(k+1+a,k) L_(k+1+c,k)' for c <= a, one element per task
        const long long tasks = (long long)m * m * 36;
        for (long long task = t; task < tasks; task += T) {
            const int el = (int)(task % 36);
            const int pr = (int)(task / 36), a = pr / m, c = pr % m;
            if (c > a) continue;
            const int     i = el / 6, j = el % 6;
            const double *A = work + ((size_t)(k + 1 + a) * W1 + (a + 1)) * 36 + 6 * i;
            const double *Bc = work + ((size_t)(k + 1 + c) * W1 + (c + 1)) * 36 + 6 * j;
            double        s = 0.0;
            for (int mm = 0; mm < 6; ++mm) s += A[mm] * Bc[mm];
            work[((size_t)(k + 1 + a) * W1 + (a - c)) * 36 + el] -= s;
        }
        __syncthreads();
    }
    if (bad) { // the same for every thread: read after the barrier that followed its only write
        if (t == 0) rec[REC_SCALE] = 0.0, rec[REC_LAMBDA] = lambda, rec[REC_PIVOT] = 1.0;
        return;
    }
    // L y = b
    for (int k = 0; k < n; ++k) {
        const double *L = work + (size_t)k * W1 * 36;
        if (t == 0) {
            double *yk = y + 6 * k;
            for (int c = 0; c < 6; ++c) {
                double v = yk[c];
                for (int mm = 0; mm < c; ++mm) v -= L[6 * c + mm] * yk[mm];
                yk[c] = v / L[7 * c];
            }
        }
        __syncthreads();
        const int m = min(w, n - 1 - k);
        for (int task = t; task < 6 * m; task += T) {
            const int     a = task / 6, row = task % 6;
            const double *B = work + ((size_t)(k + 1 + a) * W1 + (a + 1)) * 36 + 6 * row;
            double        s = 0.0;
            for (int mm = 0; mm < 6; ++mm) s += B[mm] * y[6 * k + mm];
            y[6 * (k + 1 + a) + row] -= s;
        }
        __syncthreads();
    }
    // L' x = y
    for (int k = n - 1; k >= 0; --k) {
        const double *L = work + (size_t)k * W1 * 36;
        if (t == 0) {
            double *yk = y + 6 * k;
            for (int c = 5; c >= 0; --c) {
                double v = yk[c];
                for (int mm = c + 1; mm < 6; ++mm) v -= L[6 * mm + c] * yk[mm];
                yk[c] = v / L[7 * c];
            }
        }
        __syncthreads();
        const int m = min(w, k);
        for (int task = t; task < 6 * m; task += T) {
            const int     d = task / 6 + 1, col = task % 6;
            const double *B = work + ((size_t)k * W1 + d) * 36;
            double        s = 0.0;
            for (int mm = 0; mm < 6; ++mm) s += B[6 * mm + col] * y[6 * k + mm];
            y[6 * (k - d) + col] -= s;
        }
        __syncthreads();
    }
    double part = 0.0;
    for (int k = t; k < 6 * n; k += T) {
        const double x = y[k];
        delta[6 * (size_t)perm[k / 6] + k % 6] = x;
        part += x * (lambda * x + b[k]);
    }
    red[t] = part;
    __syncthreads();
    for (int h = T / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) rec[REC_SCALE] = red[0], rec[REC_LAMBDA] = lambda, rec[REC_PIVOT] = 0.0;
}

// candidate = current (+) delta: X fromVectorMQT(delta), quaternion renormalised.  A fixed vertex is copied.
__global__ __launch_bounds__(64) void pgo_update_kernel(const double *__restrict__ cur, const double *__restrict__ delta,
                                                        const uint8_t *__restrict__ fixed, int n_vertices, double *__restrict__ cand)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vertices) return;
    const double *p = cur + 7 * (size_t)v, *d = delta + 6 * (size_t)v;
    double       *o = cand + 7 * (size_t)v;
    if (fixed[v]) {
        for (int k = 0; k < 7; ++k) o[k] = p[k];
        return;
    }
    const double n2 = d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
    Quat         dq;
    if (n2 > 1.0) {
        const double inv = 1.0 / sqrt(n2);
        dq = Quat{d[3] * inv, d[4] * inv, d[5] * inv, 0.0};
    } else
        dq = Quat{d[3], d[4], d[5], sqrt(1.0 - n2)};
    const Quat q = {p[3], p[4], p[5], p[6]};
    double     R[9];
    qmat(q, R);
    for (int r = 0; r < 3; ++r) o[r] = R[3 * r] * d[0] + R[3 * r + 1] * d[1] + R[3 * r + 2] * d[2] + p[r];
    const Quat   qn = qmul(q, dq);
    const double nn = sqrt(qn.x * qn.x + qn.y * qn.y + qn.z * qn.z + qn.w * qn.w);
    o[3] = qn.x / nn, o[4] = qn.y / nn, o[5] = qn.z / nn, o[6] = qn.w / nn;
}

__global__ __launch_bounds__(64) void pgo_gather_e_kernel(const double *__restrict__ slots, int n_edges, double *__restrict__ e,
                                                          double *__restrict__ chi2_e)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_edges) return;
    for (int r = 0; r < 6; ++r) e[6 * (size_t)k + r] = slots[(size_t)k * kSlot + kSlotE + r];
    chi2_e[k] = slots[(size_t)k * kSlot + kSlotChi2];
}

// ------------------------------------------------------------------ host
// A quaternion through the ABI: divided by its norm unless |q|^2 is within 8 ulp of 1 (a pose read back keeps its bits).
bool take_pose(const double in[7], double out[7])
{
    for (int k = 0; k < 7; ++k)
        if (!std::isfinite(in[k])) return false;
    const double n2 = in[3] * in[3] + in[4] * in[4] + in[5] * in[5] + in[6] * in[6];
    if (!(n2 > 0.0) || !std::isfinite(n2)) return false;
    for (int k = 0; k < 3; ++k) out[k] = in[k];
    if (std::fabs(n2 - 1.0) <= 8.0 * DBL_EPSILON) {
        for (int k = 3; k < 7; ++k) out[k] = in[k];
    } else {
        const double n = std::sqrt(n2);
        for (int k = 3; k < 7; ++k) out[k] = in[k] / n;
    }
    return true;
}

} // namespace

struct slam_pgo {
    slam_pgo_params      P;
    std::vector<double>  pose; // 7 per vertex
    std::vector<uint8_t> fixed;
    std::vector<PgoEdge> edges;
    // what prepare() derives from the graph
    std::vector<int>    perm, row_of, rowptr;
    std::vector<RowEnt> ent;
    int                 n_free = 0, w = 0;
    size_t              band_bytes = 0;
    // device
    DevMem    d_pose[2], d_fixed, d_edges, d_slots, d_chi2e, d_band, d_work, d_b, d_y, d_delta, d_perm, d_rowptr, d_ent, d_rowmax, d_rec,
        d_e;
    PinnedMem h_rec;
    int       cur = 0;

    int n_vertices() const { return (int)fixed.size(); }
    int n_edges() const { return (int)edges.size(); }

    // Reverse Cuthill-McKee over the free vertices (or their ids), the half-bandwidth and every block row's incident edges.
    void order()
    {
        const int nv = n_vertices();
        perm.clear();
        row_of.assign(nv, -1);
        std::vector<std::vector<int>> adj(nv);
        for (const PgoEdge &E : edges)
            if (!fixed[E.from] && !fixed[E.to]) adj[E.from].push_back(E.to), adj[E.to].push_back(E.from);
        std::vector<int> deg(nv, 0);
        for (int v = 0; v < nv; ++v) {
            std::sort(adj[v].begin(), adj[v].end());
            adj[v].erase(std::unique(adj[v].begin(), adj[v].end()), adj[v].end());
            deg[v] = (int)adj[v].size();
        }
        auto less = [&](int a, int b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; };
        if (P.ordering == SLAM_PGO_ORDER_NATURAL) {
            for (int v = 0; v < nv; ++v)
                if (!fixed[v]) perm.push_back(v);
        } else {
            std::vector<char> seen(nv, 0);
            std::vector<int>  level(nv, 0);
            // breadth first from `root` over unseen vertices, neighbours by (degree, id); returns the visit order
            auto bfs = [&](int root, std::vector<int> &out) {
                out.clear();
                out.push_back(root);
                std::vector<char> mark(nv, 0);
                mark[root] = 1, level[root] = 0;
                for (size_t h = 0; h < out.size(); ++h) {
                    std::vector<int> nb;
                    for (int u : adj[out[h]])
                        if (!mark[u] && !seen[u]) nb.push_back(u), mark[u] = 1, level[u] = level[out[h]] + 1;
                    std::sort(nb.begin(), nb.end(), less);
                    out.insert(out.end(), nb.begin(), nb.end());
                }
            };
            std::vector<int> comp, next;
            for (;;) {
                int root = -1;
                for (int v = 0; v < nv; ++v)
                    if (!fixed[v] && !seen[v] && (root < 0 || less(v, root))) root = v;
                if (root < 0) break;
                bfs(root, comp);
                // a pseudo-peripheral start: move to the smallest vertex of the last level while the depth grows
                for (int guard = 0; guard < nv; ++guard) {
                    const int depth = level[comp.back()];
                    int       far = -1;
                    for (int v : comp)
                        if (level[v] == depth && (far < 0 || less(v, far))) far = v;
                    bfs(far, next);
                    if (level[next.back()] <= depth) break;
                    comp.swap(next);
                }
                for (int v : comp) seen[v] = 1;
                perm.insert(perm.end(), comp.begin(), comp.end());
            }
            std::reverse(perm.begin(), perm.end());
        }
        n_free = (int)perm.size();
        for (int r = 0; r < n_free; ++r) row_of[perm[r]] = r;
        w = 0;
        std::vector<int> count(n_free + 1, 0);
        for (const PgoEdge &E : edges) {
            const int a = row_of[E.from], b = row_of[E.to];
            if (a >= 0 && b >= 0) w = std::max(w, std::abs(a - b));
            if (a >= 0) ++count[a + 1];
            if (b >= 0) ++count[b + 1];
        }
        rowptr.assign(n_free + 1, 0);
        for (int r = 0; r < n_free; ++r) rowptr[r + 1] = rowptr[r] + count[r + 1];
        ent.assign(rowptr[n_free], RowEnt{0, 0, -1});
        std::vector<int> fill(rowptr.begin(), rowptr.end() - 1);
        for (int k = 0; k < n_edges(); ++k) { // ascending edge index within every row
            const int a = row_of[edges[k].from], b = row_of[edges[k].to];
            if (a >= 0) ent[fill[a]++] = RowEnt{k, 0, b};
            if (b >= 0) ent[fill[b]++] = RowEnt{k, 1, a};
        }
        band_bytes = (size_t)n_free * (size_t)(w + 1) * 36 * sizeof(double);
    }
};

namespace {

template <class T>
int room(DevMem &d, size_t count)
{
    return reserve_quarter(d, std::max<size_t>(count, 1) * sizeof(T));
}

template <class T>
int upload(DevMem &d, const T *src, size_t count, hipStream_t st)
{
    if (count) SLAM_HIP(hipMemcpyAsync(d.p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
    return SLAM_OK;
}

int require_fixed(const slam_pgo *g)
{
    for (uint8_t f : g->fixed)
        if (f) return SLAM_OK;
    slam::set_error("slam_pgo: no vertex is fixed (%d vertices): the system has a gauge freedom", g->n_vertices());
    return SLAM_E_INVALID;
}

// A usable device, the order, the cap, the buffers and the upload.  The graph's poses go to d_pose[0].
int prepare(slam_pgo *g, hipStream_t st)
{
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        slam::set_error("slam_pgo: the graph is host state, this call runs on the device and no HIP device is usable");
        return SLAM_E_HIP;
    }
    g->order();
    SLAM_REQUIRE(g->band_bytes <= g->P.max_band_bytes, SLAM_E_NOMEM,
                 "slam_pgo: the band of %d block rows at half-bandwidth %d takes %zu bytes, max_band_bytes is %zu", g->n_free, g->w,
                 g->band_bytes, g->P.max_band_bytes);
    const size_t nv = g->n_vertices(), ne = g->n_edges(), nf = g->n_free;
    // every buffer first, then the copies: a call that fails for memory leaves no copy in flight
    SLAM_TRY(room<double>(g->d_pose[0], 7 * nv));
    SLAM_TRY(room<double>(g->d_pose[1], 7 * nv));
    SLAM_TRY(room<uint8_t>(g->d_fixed, nv));
    SLAM_TRY(room<PgoEdge>(g->d_edges, ne));
    SLAM_TRY(room<int>(g->d_perm, nf));
    SLAM_TRY(room<int>(g->d_rowptr, nf + 1));
    SLAM_TRY(room<RowEnt>(g->d_ent, g->ent.size()));
    SLAM_TRY(room<double>(g->d_slots, ne * kSlot));
    SLAM_TRY(room<double>(g->d_chi2e, ne));
    SLAM_TRY(room<double>(g->d_e, 6 * ne));
    SLAM_TRY(room<double>(g->d_band, g->band_bytes / sizeof(double)));
    SLAM_TRY(room<double>(g->d_work, g->band_bytes / sizeof(double)));
    SLAM_TRY(room<double>(g->d_b, 6 * nf));
    SLAM_TRY(room<double>(g->d_y, 6 * nf));
    SLAM_TRY(room<double>(g->d_rowmax, nf));
    SLAM_TRY(room<double>(g->d_delta, 6 * nv));
    if (!g->d_rec.p) SLAM_TRY(g->d_rec.alloc(kRec * sizeof(double)));
    if (!g->h_rec.p) SLAM_TRY(g->h_rec.alloc(kRec * sizeof(double)));
    SLAM_TRY(upload(g->d_pose[0], g->pose.data(), 7 * nv, st));
    SLAM_TRY(upload(g->d_fixed, g->fixed.data(), nv, st));
    SLAM_TRY(upload(g->d_edges, g->edges.data(), ne, st));
    SLAM_TRY(upload(g->d_perm, g->perm.data(), nf, st));
    SLAM_TRY(upload(g->d_rowptr, g->rowptr.data(), nf + 1, st));
    SLAM_TRY(upload(g->d_ent, g->ent.data(), g->ent.size(), st));
    g->cur = 0;
    return SLAM_OK;
}

inline dim3 lanes(int n) { return dim3((unsigned)std::max(1, (n + 63) / 64)); }

// linearise at the current poses, assemble, chi2 and max diag(H) into the record
void enqueue_system(slam_pgo *g, hipStream_t st)
{
    double *rec = g->d_rec.as<double>(), *slots = g->d_slots.as<double>();
    if (g->n_edges())
        hipLaunchKernelGGL(pgo_linearize_kernel<true>, lanes(g->n_edges()), dim3(64), 0, st, g->d_edges.as<PgoEdge>(), g->n_edges(),
                           g->d_pose[g->cur].as<double>(), slots);
    if (g->n_free)
        hipLaunchKernelGGL(pgo_assemble_kernel, dim3(g->n_free), dim3(64), 0, st, slots, g->d_rowptr.as<int>(), g->d_ent.as<RowEnt>(),
                           g->n_free, g->w, g->d_band.as<double>(), g->d_b.as<double>(), g->d_rowmax.as<double>());
    hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, st, slots + kSlotChi2, kSlot, g->n_edges(), 0, rec + REC_CHI2);
    hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, st, g->d_rowmax.as<double>(), 1, g->n_free, 1, rec + REC_MAXDIAG);
}

// one trial: solve at lambda (tau > 0: tau * max diag), candidate poses into the other buffer, their chi2; the record comes
// back through pinned memory and the call waits for it
int run_trial(slam_pgo *g, double lambda, double tau, hipStream_t st)
{
    double *rec = g->d_rec.as<double>();
    hipLaunchKernelGGL(pgo_factor_solve_kernel, dim3(1), dim3(kFactorThreads), 0, st, g->d_band.as<double>(), g->d_b.as<double>(),
                       g->d_perm.as<int>(), g->n_free, g->n_vertices(), g->w, lambda, tau, rec + REC_MAXDIAG, g->d_work.as<double>(),
                       g->d_y.as<double>(), g->d_delta.as<double>(), rec);
    hipLaunchKernelGGL(pgo_update_kernel, lanes(g->n_vertices()), dim3(64), 0, st, g->d_pose[g->cur].as<double>(), g->d_delta.as<double>(),
                       g->d_fixed.as<uint8_t>(), g->n_vertices(), g->d_pose[1 - g->cur].as<double>());
    if (g->n_edges())
        hipLaunchKernelGGL(pgo_linearize_kernel<false>, lanes(g->n_edges()), dim3(64), 0, st, g->d_edges.as<PgoEdge>(), g->n_edges(),
                           g->d_pose[1 - g->cur].as<double>(), g->d_chi2e.as<double>());
    hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, st, g->d_chi2e.as<double>(), 1, g->n_edges(), 0, rec + REC_CHI2_CAND);
    SLAM_HIP(hipGetLastError());
    SLAM_HIP(hipMemcpyAsync(g->h_rec.p, rec, kRec * sizeof(double), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    return SLAM_OK;
}

} // namespace

extern "C" {

void slam_pgo_default_params(slam_pgo_params *p)
{
    if (!p) return;
    p->max_trials = 10;
    p->tau = 1e-5;
    p->good_lower = 1.0 / 3.0;
    p->good_upper = 2.0 / 3.0;
    p->ordering = SLAM_PGO_ORDER_RCM;
    p->max_band_bytes = (size_t)1 << 30;
}

int slam_pgo_create(const slam_pgo_params *params, slam_pgo_t **out)
{
    SLAM_REQUIRE(out, SLAM_E_INVALID, "slam_pgo_create: out is null");
    *out = nullptr;
    slam_pgo_params P;
    slam_pgo_default_params(&P);
    if (params) P = *params;
    SLAM_REQUIRE(P.max_trials >= 1 && P.tau > 0.0 && std::isfinite(P.tau) && P.good_lower > 0.0 && P.good_lower <= P.good_upper &&
                     (P.ordering == SLAM_PGO_ORDER_RCM || P.ordering == SLAM_PGO_ORDER_NATURAL),
                 SLAM_E_INVALID, "slam_pgo_create: max_trials %d, tau %g, good steps [%g, %g] or ordering %d is not valid", P.max_trials,
                 P.tau, P.good_lower, P.good_upper, P.ordering);
    slam_pgo *g = new slam_pgo;
    g->P = P;
    *out = g;
    return SLAM_OK;
}

void slam_pgo_destroy(slam_pgo_t *g)
{
    if (!g) return;
    if (g->d_rec.p) (void)hipDeviceSynchronize();
    delete g;
}

int slam_pgo_clear(slam_pgo_t *g)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "slam_pgo_clear: null handle");
    g->pose.clear(), g->fixed.clear(), g->edges.clear();
    return SLAM_OK;
}

int slam_pgo_add_vertex(slam_pgo_t *g, int id, const double pose[7], int fixed)
{
    SLAM_REQUIRE(g && pose, SLAM_E_INVALID, "slam_pgo_add_vertex: null argument");
    SLAM_REQUIRE(id == g->n_vertices(), SLAM_E_INVALID, "slam_pgo_add_vertex: id %d, the next vertex is %d (ids are dense and in order)", id,
                 g->n_vertices());
    double p[7];
    SLAM_REQUIRE(take_pose(pose, p), SLAM_E_INVALID, "slam_pgo_add_vertex: vertex %d's pose is not finite or its quaternion is zero", id);
    g->pose.insert(g->pose.end(), p, p + 7);
    g->fixed.push_back(fixed ? 1 : 0);
    return SLAM_OK;
}

int slam_pgo_set_vertex(slam_pgo_t *g, int id, const double pose[7])
{
    SLAM_REQUIRE(g && pose, SLAM_E_INVALID, "slam_pgo_set_vertex: null argument");
    SLAM_REQUIRE(id >= 0 && id < g->n_vertices(), SLAM_E_INVALID, "slam_pgo_set_vertex: no vertex %d (%d vertices)", id, g->n_vertices());
    double p[7];
    SLAM_REQUIRE(take_pose(pose, p), SLAM_E_INVALID, "slam_pgo_set_vertex: vertex %d's pose is not finite or its quaternion is zero", id);
    std::memcpy(&g->pose[7 * (size_t)id], p, sizeof p);
    return SLAM_OK;
}

int slam_pgo_add_edge(slam_pgo_t *g, int from, int to, const double meas[7], const double info[36])
{
    SLAM_REQUIRE(g && meas && info, SLAM_E_INVALID, "slam_pgo_add_edge: null argument");
    const int nv = g->n_vertices();
    SLAM_REQUIRE(from >= 0 && to >= 0 && from < nv && to < nv && from != to, SLAM_E_INVALID,
                 "slam_pgo_add_edge: %d -> %d does not join two different vertices of the %d present", from, to, nv);
    double z[7];
    SLAM_REQUIRE(take_pose(meas, z), SLAM_E_INVALID, "slam_pgo_add_edge: the measurement is not finite or its quaternion is zero");
    for (int k = 0; k < 36; ++k) SLAM_REQUIRE(std::isfinite(info[k]), SLAM_E_INVALID, "slam_pgo_add_edge: information[%d] is not finite", k);
    PgoEdge E;
    E.from = from, E.to = to;
    const Quat qa = {-z[3], -z[4], -z[5], z[6]}; // Z^-1 = (q*, -R(q*) t)
    double     Ra[9];
    qmat(qa, Ra);
    for (int r = 0; r < 3; ++r) E.zinv[r] = -(Ra[3 * r] * z[0] + Ra[3 * r + 1] * z[1] + Ra[3 * r + 2] * z[2]);
    E.zinv[3] = qa.x, E.zinv[4] = qa.y, E.zinv[5] = qa.z, E.zinv[6] = qa.w;
    std::memcpy(E.info, info, sizeof E.info);
    g->edges.push_back(E);
    return SLAM_OK;
}

int slam_pgo_size(slam_pgo_t *g, int *n_vertices, int *n_edges)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "slam_pgo_size: null handle");
    if (n_vertices) *n_vertices = g->n_vertices();
    if (n_edges) *n_edges = g->n_edges();
    return SLAM_OK;
}

int slam_pgo_read_vertices(slam_pgo_t *g, double *pose, int cap, int *n_out)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "slam_pgo_read_vertices: null handle");
    if (n_out) *n_out = g->n_vertices();
    if (!pose) return SLAM_OK;
    SLAM_REQUIRE(cap >= g->n_vertices(), SLAM_E_NOMEM, "slam_pgo_read_vertices: room for %d vertices, the graph has %d", cap, g->n_vertices());
    for (int v = 0; v < g->n_vertices(); ++v) {
        const double *p = &g->pose[7 * (size_t)v];
        const double  s = p[6] < 0.0 ? -1.0 : 1.0; // toVectorQT: w >= 0
        for (int k = 0; k < 3; ++k) pose[7 * (size_t)v + k] = p[k];
        for (int k = 3; k < 7; ++k) pose[7 * (size_t)v + k] = s * p[k];
    }
    return SLAM_OK;
}

int slam_pgo_optimize(slam_pgo_t *g, int iterations, slam_pgo_result *result, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "slam_pgo_optimize: null handle");
    SLAM_REQUIRE(iterations >= 0, SLAM_E_INVALID, "slam_pgo_optimize: %d iterations", iterations);
    SLAM_TRY(require_fixed(g));
    hipStream_t st = as_stream(stream);
    SLAM_TRY(prepare(g, st));
    slam_pgo_result R;
    std::memset(&R, 0, sizeof R);
    R.half_bandwidth = g->w, R.free_vertices = g->n_free, R.band_bytes = g->band_bytes;
    R.stop_reason = SLAM_PGO_STOP_ITERATIONS;
    const double *rec = g->h_rec.as<double>();
    double        lambda = 0.0, nu = 2.0, chi2 = 0.0;
    bool          have_chi2 = false;
    for (int it = 0; it < iterations && g->n_free > 0; ++it) {
        enqueue_system(g, st);
        double rho = 0.0;
        int    trials = 0;
        do {
            SLAM_TRY(run_trial(g, lambda, it == 0 && trials == 0 ? g->P.tau : 0.0, st));
            if (!have_chi2) R.chi2_initial = rec[REC_CHI2], have_chi2 = true;
            if (trials == 0) chi2 = rec[REC_CHI2];
            lambda = rec[REC_LAMBDA];
            const double cand = rec[REC_PIVOT] != 0.0 ? DBL_MAX : rec[REC_CHI2_CAND];
            rho = (chi2 - cand) / (rec[REC_SCALE] + 1e-3);
            const bool accept = rho > 0.0 && std::isfinite(cand);
            if (R.n_trials < SLAM_PGO_TRACE) R.trace[R.n_trials] = slam_pgo_trial{lambda, rho, cand, accept ? 1 : 0, 0};
            ++R.n_trials;
            if (accept) {
                double alpha = 1.0 - std::pow(2.0 * rho - 1.0, 3);
                alpha = std::min(alpha, g->P.good_upper);
                lambda *= std::max(g->P.good_lower, alpha);
                nu = 2.0;
                chi2 = cand;
                g->cur = 1 - g->cur;
            } else {
                lambda *= nu;
                nu *= 2.0;
            }
            ++trials;
        } while (rho < 0.0 && trials < g->P.max_trials);
        ++R.iterations;
        if (trials == g->P.max_trials || rho == 0.0) {
            R.stop_reason = trials == g->P.max_trials ? SLAM_PGO_STOP_MAX_TRIALS : SLAM_PGO_STOP_RHO_ZERO;
            break;
        }
    }
    if (!have_chi2) { // no iteration ran: the chi2 of the poses as they are
        hipLaunchKernelGGL(pgo_linearize_kernel<false>, lanes(g->n_edges()), dim3(64), 0, st, g->d_edges.as<PgoEdge>(), g->n_edges(),
                           g->d_pose[g->cur].as<double>(), g->d_chi2e.as<double>());
        hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, st, g->d_chi2e.as<double>(), 1, g->n_edges(), 0,
                           g->d_rec.as<double>() + REC_CHI2);
        SLAM_HIP(hipGetLastError());
        SLAM_HIP(hipMemcpyAsync(g->h_rec.p, g->d_rec.p, kRec * sizeof(double), hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipStreamSynchronize(st));
        R.chi2_initial = chi2 = rec[REC_CHI2];
    }
    R.chi2_final = chi2;
    if (g->n_vertices()) {
        SLAM_HIP(hipMemcpyAsync(g->pose.data(), g->d_pose[g->cur].p, g->pose.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipStreamSynchronize(st));
    }
    if (result) *result = R;
    return SLAM_OK;
}

int slam_pgo_chi2(slam_pgo_t *g, double *chi2, double *e, double *chi2_e, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "slam_pgo_chi2: null handle");
    hipStream_t st = as_stream(stream);
    SLAM_TRY(prepare(g, st));
    const int ne = g->n_edges();
    double   *rec = g->d_rec.as<double>(), *slots = g->d_slots.as<double>();
    if (ne)
        hipLaunchKernelGGL(pgo_linearize_kernel<true>, lanes(ne), dim3(64), 0, st, g->d_edges.as<PgoEdge>(), ne, g->d_pose[0].as<double>(), slots);
    hipLaunchKernelGGL(pgo_reduce_kernel, dim3(1), dim3(256), 0, st, slots + kSlotChi2, kSlot, ne, 0, rec + REC_CHI2);
    SLAM_HIP(hipGetLastError());
    if (ne && (e || chi2_e)) {
        hipLaunchKernelGGL(pgo_gather_e_kernel, lanes(ne), dim3(64), 0, st, slots, ne, g->d_e.as<double>(), g->d_chi2e.as<double>());
        SLAM_HIP(hipGetLastError());
        if (e) SLAM_HIP(hipMemcpyAsync(e, g->d_e.p, (size_t)ne * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (chi2_e) SLAM_HIP(hipMemcpyAsync(chi2_e, g->d_chi2e.p, (size_t)ne * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    SLAM_HIP(hipMemcpyAsync(g->h_rec.p, rec, kRec * sizeof(double), hipMemcpyDeviceToHost, st));
    SLAM_HIP(hipStreamSynchronize(st));
    if (chi2) *chi2 = g->h_rec.as<double>()[REC_CHI2];
    return SLAM_OK;
}

int slam_pgo_read_system(slam_pgo_t *g, int *rows, int *cols, double *blocks, int cap, int *n_blocks, double *b, int *perm, int *free_vertices,
                         int *half_bandwidth, slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "slam_pgo_read_system: null handle");
    SLAM_TRY(require_fixed(g));
    hipStream_t st = as_stream(stream);
    SLAM_TRY(prepare(g, st));
    const int n = g->n_free, w = g->w;
    long long nb = 0;
    for (int r = 0; r < n; ++r) nb += std::min(r, w) + 1;
    if (n_blocks) *n_blocks = (int)nb;
    if (free_vertices) *free_vertices = n;
    if (half_bandwidth) *half_bandwidth = w;
    SLAM_REQUIRE(!(rows || cols || blocks) || nb <= cap, SLAM_E_NOMEM, "slam_pgo_read_system: room for %d blocks, the band has %lld", cap, nb);
    enqueue_system(g, st);
    SLAM_HIP(hipGetLastError());
    std::vector<double> band((size_t)n * (w + 1) * 36), hb((size_t)n * 6);
    if (n) {
        SLAM_HIP(hipMemcpyAsync(band.data(), g->d_band.p, band.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipMemcpyAsync(hb.data(), g->d_b.p, hb.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    SLAM_HIP(hipStreamSynchronize(st));
    size_t k = 0;
    for (int r = 0; r < n; ++r)
        for (int d = 0; d <= std::min(r, w); ++d, ++k) {
            if (rows) rows[k] = g->perm[r];
            if (cols) cols[k] = g->perm[r - d];
            if (blocks) std::memcpy(blocks + 36 * k, &band[((size_t)r * (w + 1) + d) * 36], 36 * sizeof(double));
        }
    if (b) {
        std::fill(b, b + 6 * (size_t)g->n_vertices(), 0.0);
        for (int r = 0; r < n; ++r) std::memcpy(b + 6 * (size_t)g->perm[r], &hb[6 * (size_t)r], 6 * sizeof(double));
    }
    if (perm) std::copy(g->perm.begin(), g->perm.end(), perm);
    return SLAM_OK;
}

int slam_pgo_step(slam_pgo_t *g, double lambda, double *delta, double *chi2_before, double *chi2_after, double *scale, int *pivot_flag,
                  slam_stream_t stream)
{
    SLAM_REQUIRE(g, SLAM_E_INVALID, "slam_pgo_step: null handle");
    SLAM_REQUIRE(lambda >= 0.0 && std::isfinite(lambda), SLAM_E_INVALID, "slam_pgo_step: lambda %g", lambda);
    SLAM_TRY(require_fixed(g));
    hipStream_t st = as_stream(stream);
    SLAM_TRY(prepare(g, st));
    enqueue_system(g, st);
    SLAM_TRY(run_trial(g, lambda, 0.0, st));
    const double *rec = g->h_rec.as<double>();
    if (chi2_before) *chi2_before = rec[REC_CHI2];
    if (chi2_after) *chi2_after = rec[REC_CHI2_CAND];
    if (scale) *scale = rec[REC_SCALE];
    if (pivot_flag) *pivot_flag = rec[REC_PIVOT] != 0.0;
    if (delta && g->n_vertices()) {
        SLAM_HIP(hipMemcpyAsync(delta, g->d_delta.p, (size_t)g->n_vertices() * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
        SLAM_HIP(hipStreamSynchronize(st));
    }
    return SLAM_OK;
}

} // extern "C"
