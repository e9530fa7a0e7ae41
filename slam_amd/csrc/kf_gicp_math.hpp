// kf_gicp_math.hpp -- the scalar pieces of Generalized ICP that more than one file runs (kf_gicp.hip: the keyframe store's
// solver; voxmap.hip and vmap_gicp.hip: the voxel map's distributions and the registration against them): the plane
// covariance, one pair's share of the Gauss-Newton sums and the step.  Each is the same text as tests/cpp/kf_gicp_oracle.cpp.
// Device code sits in an unnamed namespace, as in kf_common.hpp: every translation unit compiles its own copy.
#pragma once
#include <cfloat>
#include <cmath>

namespace {

constexpr int kJacobiSweeps = 8;

// C' = V diag(1, 1, eps) V' of the symmetric C (xx xy xz yy yz zz): a cyclic Jacobi eigen-decomposition with a fixed number
// of sweeps on scalars (nothing is indexed at run time), then, with n the eigenvector of the smallest eigenvalue (the last of
// equal ones, as a stable descending sort leaves it), (I - n n') + eps n n', which is V diag(1, 1, eps) V' for an orthonormal V
// and is exact when n is an axis.  The same text as tests/cpp/kf_gicp_oracle.cpp.
__device__ inline void plane_covariance(const double C[6], double eps, double out[6])
{
    double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#define KF_JACOBI(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                                                  \
    if (apq != 0.0) {                                                                                                                     \
        const double th = (aqq - app) / (2.0 * apq);                                                                                      \
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));                                                     \
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                                                                              \
        app = app - t * apq, aqq = aqq + t * apq, apq = 0.0;                                                                              \
        const double rp = arp, rq = arq, x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;                                      \
        arp = c * rp - s * rq, arq = s * rp + c * rq;                                                                                     \
        v0p = c * x0 - s * y0, v0q = s * x0 + c * y0;                                                                                     \
        v1p = c * x1 - s * y1, v1q = s * x1 + c * y1;                                                                                     \
        v2p = c * x2 - s * y2, v2q = s * x2 + c * y2;                                                                                     \
    }
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        KF_JACOBI(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        KF_JACOBI(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        KF_JACOBI(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    }
#undef KF_JACOBI
    int    n = 0;
    double mn = a00;
    if (a11 <= mn) n = 1, mn = a11;
    if (a22 <= mn) n = 2;
    const double nx = n == 0 ? v00 : n == 1 ? v01 : v02, ny = n == 0 ? v10 : n == 1 ? v11 : v12, nz = n == 0 ? v20 : n == 1 ? v21 : v22;
    const double xx = nx * nx, xy = nx * ny, xz = nx * nz, yy = ny * ny, yz = ny * nz, zz = nz * nz;
    out[0] = (1.0 - xx) + eps * xx, out[1] = (0.0 - xy) + eps * xy, out[2] = (0.0 - xz) + eps * xz;
    out[3] = (1.0 - yy) + eps * yy, out[4] = (0.0 - yz) + eps * yz, out[5] = (1.0 - zz) + eps * zz;
}

// ---------------------------------------------------------------- one pair's share of the Gauss-Newton sums
// x = R p + t in f64 from the original f32 point, r = q - x, M = (C'q + R C'p R')^-1 by the closed-form symmetric inverse,
// J = [ [x]x , -I ]; h (the 21 entries of the upper triangle of J' M J, row by row), g = J' M r and r' M r are added to.
// Every loop has constant bounds and is unrolled.  The same text as tests/cpp/kf_gicp_oracle.cpp.
__device__ inline void gicp_pair(const double T[12], const float p[3], const float q[3], const double Cp[6], const double Cq[6], double h[21],
                                 double g[6], double *cost)
{
    double x[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k] = ((T[4 * k] * (double)p[0] + T[4 * k + 1] * (double)p[1]) + T[4 * k + 2] * (double)p[2]) + T[4 * k + 3];
        r[k] = (double)q[k] - x[k];
    }
    const double cp[9] = {Cp[0], Cp[1], Cp[2], Cp[1], Cp[3], Cp[4], Cp[2], Cp[4], Cp[5]};
    double       B[9], A[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) B[3 * a + b] = (T[4 * a] * cp[b] + T[4 * a + 1] * cp[3 + b]) + T[4 * a + 2] * cp[6 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) A[3 * a + b] = (B[3 * a] * T[4 * b] + B[3 * a + 1] * T[4 * b + 1]) + B[3 * a + 2] * T[4 * b + 2];
    const double s00 = Cq[0] + A[0], s01 = Cq[1] + A[1], s02 = Cq[2] + A[2], s11 = Cq[3] + A[4], s12 = Cq[4] + A[5], s22 = Cq[5] + A[8];
    const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    const double M[9] = {c00 / det, c01 / det, c02 / det, c01 / det, c11 / det, c12 / det, c02 / det, c12 / det, c22 / det};
    const double J[18] = {0.0, -x[2], x[1], -1.0, 0.0, 0.0, x[2], 0.0, -x[0], 0.0, -1.0, 0.0, -x[1], x[0], 0.0, 0.0, 0.0, -1.0};
    double       Mr[3], MJ[18];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Mr[a] = (M[3 * a] * r[0] + M[3 * a + 1] * r[1]) + M[3 * a + 2] * r[2];
#pragma unroll
        for (int b = 0; b < 6; ++b) MJ[6 * a + b] = (M[3 * a] * J[b] + M[3 * a + 1] * J[6 + b]) + M[3 * a + 2] * J[12 + b];
    }
    int at = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        g[a] += (J[a] * Mr[0] + J[6 + a] * Mr[1]) + J[12 + a] * Mr[2];
#pragma unroll
        for (int b = a; b < 6; ++b, ++at) h[at] += (J[a] * MJ[b] + J[6 + a] * MJ[6 + b]) + J[12 + a] * MJ[12 + b];
    }
    *cost += (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
}

// The step of one iteration from the full sums: H xi = -g by an unrolled Cholesky, Exp(omega) by Rodrigues (below
// theta^2 = 1e-16 the series 1 - theta^2/6 and 1/2 - theta^2/24), N = step . T.  False when a pivot is not positive and
// finite; N is then not to be used.  The same text as tests/cpp/kf_gicp_oracle.cpp.
__device__ inline bool gicp_step(const double H[36], const double g[6], const double T[12], double N[12])
{
    double L[36], y[6], xi[6];
    bool   ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double d = H[6 * k + k];
#pragma unroll
        for (int j = 0; j < k; ++j) d -= L[6 * k + j] * L[6 * k + j];
        if (!(d > 0.0) || !(d <= DBL_MAX)) ok = false;
        L[6 * k + k] = sqrt(d);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double s = H[6 * i + k];
#pragma unroll
            for (int j = 0; j < k; ++j) s -= L[6 * i + j] * L[6 * k + j];
            L[6 * i + k] = s / L[6 * k + k];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = -g[i];
#pragma unroll
        for (int j = 0; j < i; ++j) s -= L[6 * i + j] * y[j];
        y[i] = s / L[6 * i + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) s -= L[6 * j + i] * xi[j];
        xi[i] = s / L[6 * i + i];
    }
    const double wx = xi[0], wy = xi[1], wz = xi[2];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double       a, b;
    if (th2 < 1e-16) {
        a = 1.0 - th2 / 6.0, b = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        a = sin(th) / th, b = (1.0 - cos(th)) / th2;
    }
    // I + a [w]x + b [w]x^2, [w]x^2 = w w' - theta^2 I
    const double Rs[9] = {1.0 + b * (wx * wx - th2), b * (wx * wy) - a * wz,     b * (wx * wz) + a * wy,
                          b * (wx * wy) + a * wz,     1.0 + b * (wy * wy - th2), b * (wy * wz) - a * wx,
                          b * (wx * wz) - a * wy,     b * (wy * wz) + a * wx,     1.0 + b * (wz * wz - th2)};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) N[4 * r + c] = (Rs[3 * r] * T[c] + Rs[3 * r + 1] * T[4 + c]) + Rs[3 * r + 2] * T[8 + c];
        N[4 * r + 3] = ((Rs[3 * r] * T[3] + Rs[3 * r + 1] * T[7]) + Rs[3 * r + 2] * T[11]) + xi[3 + r];
    }
    return ok;
}

// plane_covariance's decomposition with its results laid open (the voxel map's distributions, docs/VOXEL_MAP.md section 9):
// the same sweeps in the same order with the same skip rule, then lam[0] >= lam[1] >= lam[2] and nrm, the eigenvector
// plane_covariance takes for the normal (of the smallest eigenvalue, the last of equal ones).  The same text as
// tests/cpp/vmap_gicp_oracle.cpp.
__host__ __device__ inline void plane_eigen(const double C[6], double lam[3], double nrm[3])
{
    double a00 = C[0], a01 = C[1], a02 = C[2], a11 = C[3], a12 = C[4], a22 = C[5];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#define KF_JACOBI(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                                                  \
    if (apq != 0.0) {                                                                                                                     \
        const double th = (aqq - app) / (2.0 * apq);                                                                                      \
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));                                                     \
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;                                                                              \
        app = app - t * apq, aqq = aqq + t * apq, apq = 0.0;                                                                              \
        const double rp = arp, rq = arq, x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;                                      \
        arp = c * rp - s * rq, arq = s * rp + c * rq;                                                                                     \
        v0p = c * x0 - s * y0, v0q = s * x0 + c * y0;                                                                                     \
        v1p = c * x1 - s * y1, v1q = s * x1 + c * y1;                                                                                     \
        v2p = c * x2 - s * y2, v2q = s * x2 + c * y2;                                                                                     \
    }
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
        KF_JACOBI(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        KF_JACOBI(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        KF_JACOBI(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    }
#undef KF_JACOBI
    int    n = 0;
    double mn = a00;
    if (a11 <= mn) n = 1, mn = a11;
    if (a22 <= mn) n = 2;
    nrm[0] = n == 0 ? v00 : n == 1 ? v01 : v02, nrm[1] = n == 0 ? v10 : n == 1 ? v11 : v12, nrm[2] = n == 0 ? v20 : n == 1 ? v21 : v22;
    const double p = n == 0 ? a11 : a00, q = n == 2 ? a11 : a22; // the other two, by index
    lam[0] = p >= q ? p : q, lam[1] = p >= q ? q : p, lam[2] = n == 0 ? a00 : n == 1 ? a11 : a22;
}

// (I - n n') + eps n n' in the text plane_covariance uses
__host__ __device__ inline void plane_from_normal(const double nrm[3], double eps, double out[6])
{
    const double nx = nrm[0], ny = nrm[1], nz = nrm[2];
    const double xx = nx * nx, xy = nx * ny, xz = nx * nz, yy = ny * ny, yz = ny * nz, zz = nz * nz;
    out[0] = (1.0 - xx) + eps * xx, out[1] = (0.0 - xy) + eps * xy, out[2] = (0.0 - xz) + eps * xz;
    out[3] = (1.0 - yy) + eps * yy, out[4] = (0.0 - yz) + eps * yz, out[5] = (1.0 - zz) + eps * zz;
}

} // namespace
