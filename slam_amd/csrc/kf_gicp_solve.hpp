// kf_gicp_solve.hpp -- one Gauss-Newton iteration of Generalized ICP by a workgroup, in the pieces that kf_gicp_kernel
// (kf_gicp.hip) and vmap_gicp_kernel (vmap_gicp.hip) both run: a pair's share added to the lane's sums, the three block
// sums in their fixed order, and thread 0's step and stop rule.  A kernel keeps its own loop, its own way of getting T
// into registers, its own search and gate test, its trace entry and its passes after the loop: the whole loop as one
// template moved the registers of both kernels (docs/VOXEL_MAP.md section 14), these pieces do not.
#pragma once
#include "kf_common.hpp"
#include "kf_gicp_math.hpp"

namespace {

// source point p (the original f32 one) paired with q at the f32 squared distance d2; Cp and Cq point at their six doubles
__device__ __forceinline__ void gicp_accumulate(const double T[12], const float4 p, const float4 q, float d2, const double *Cp6, const double *Cq6,
                                                double acc[9], double h16[16], double h5[5])
{
    const float pf[3] = {p.x, p.y, p.z}, qf[3] = {q.x, q.y, q.z};
    double      Cp[6], Cq[6], h[21] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, g[6] = {0, 0, 0, 0, 0, 0}, c = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) Cp[e] = Cp6[e], Cq[e] = Cq6[e];
    gicp_pair(T, pf, qf, Cp, Cq, h, g, &c);
    acc[0] += 1.0, acc[1] += (double)d2, acc[2] += c;
#pragma unroll
    for (int e = 0; e < 6; ++e) acc[3 + e] += g[e];
#pragma unroll
    for (int e = 0; e < 16; ++e) h16[e] += h[e];
#pragma unroll
    for (int e = 0; e < 5; ++e) h5[e] += h[16 + e];
}

// the lanes' sums (acc: pairs, d^2, cost, g) to the workgroup's, the same in every thread: 9, then 16, then 5 doubles
__device__ __forceinline__ void gicp_reduce(double (&acc)[9], double (&h16)[16], double (&h5)[5], double (*red)[16], double *tot, int *pairs, double *mse,
                                            double *cost, double g[6], double hu[21])
{
    block_sum<double, 9>(acc, red, tot);
    const double n = tot[0];
    *pairs = (int)n;
    *mse = *pairs ? tot[1] / n : 0.0;
    *cost = *pairs ? tot[2] / n : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) g[e] = tot[3 + e];
    block_sum<double, 16>(h16, red, tot);
#pragma unroll
    for (int e = 0; e < 16; ++e) hu[e] = tot[e];
    block_sum<double, 5>(h5, red, tot);
#pragma unroll
    for (int e = 0; e < 5; ++e) hu[16 + e] = tot[e];
}

// Thread 0's: H from its upper triangle into sH, the step into sT, and the state the iteration ends in (0: go on)
__device__ __forceinline__ int gicp_advance(const double (&hu)[21], const double (&g)[6], const double (&T)[12], const int pairs, const int max_iter,
                                            const double eps_r, const double eps_t, double (&sH)[36], double (&sT)[12], int &iterations)
{
    double H[36];
    int    at = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b, ++at) H[6 * a + b] = H[6 * b + a] = hu[at];
#pragma unroll
    for (int k = 0; k < 36; ++k) sH[k] = H[k];
    int state = 0;
    if (pairs < 3)
        state = SLAM_KF_NO_CORRESPONDENCES;
    else {
        double N[12];
        if (!gicp_step(H, g, T, N))
            state = SLAM_KF_DEGENERATE;
        else {
#pragma unroll
            for (int k = 0; k < 12; ++k) sT[k] = N[k];
            ++iterations;
            if (iterations >= max_iter)
                state = SLAM_KF_ITERATIONS;
            else { // PCL GICP's rule: no entry of the rotation moved by more than eps_r, none of the translation by more than eps_t
                double dr = 0.0, dt = 0.0;
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    const double d = fabs(N[k] - T[k]);
                    if (k % 4 == 3)
                        dt = d > dt ? d : dt;
                    else
                        dr = d > dr ? d : dr;
                }
                if (dr <= eps_r && dt <= eps_t) state = SLAM_KF_TRANSFORM;
            }
        }
    }
    return state;
}

} // namespace
