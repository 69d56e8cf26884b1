// The weight of one distribution-to-distribution correspondence, shared by gicp.hip (float32 target covariances) and
// vgicp.hip (float64 voxel covariances): ONE definition of the order in which R Cp R^T is evaluated -- and of the plane
// regulariser both put on a covariance.
#pragma once

#include "eigen3.h"
#include "pass_device.h"

// the plane regulariser C = I - (1 - eps) n n^T as xx xy xz yy yz zz: eigenvalues (eps, 1, 1); the sign of n cancels
__device__ __forceinline__ void plane_cov6(const double n[3], double eps, double c[6]) {
    const double s = 1.0 - eps;
    c[0] = 1.0 - s * n[0] * n[0]; c[1] = -s * n[0] * n[1]; c[2] = -s * n[0] * n[2];
    c[3] = 1.0 - s * n[1] * n[1]; c[4] = -s * n[1] * n[2]; c[5] = 1.0 - s * n[2] * n[2];
}

// M6 = (Cq + R Cp R^T)^-1 as xx xy xz yy yz zz, float64.  CQ: the type the target side's covariance is stored in (widened
// entry by entry before the sum)
template <typename CQ>
__device__ __forceinline__ void gicp_weight(const PoseK &P, const float cp[6], const CQ cq[6], double m6[6]) {
    const double Cp[3][3] = {{cp[0], cp[1], cp[2]}, {cp[1], cp[3], cp[4]}, {cp[2], cp[4], cp[5]}};
    double B[3][3];                                  // R Cp
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i][j] = (P.R[3 * i] * Cp[0][j] + P.R[3 * i + 1] * Cp[1][j]) + P.R[3 * i + 2] * Cp[2][j];
    double S[3][3];                                  // (R Cp) R^T, upper triangle mirrored: symmetric by construction
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            S[i][j] = (B[i][0] * P.R[3 * j] + B[i][1] * P.R[3 * j + 1]) + B[i][2] * P.R[3 * j + 2];
            S[j][i] = S[i][j];
        }
    const double m[9] = {(double)cq[0] + S[0][0], (double)cq[1] + S[0][1], (double)cq[2] + S[0][2],
                         (double)cq[1] + S[1][0], (double)cq[3] + S[1][1], (double)cq[4] + S[1][2],
                         (double)cq[2] + S[2][0], (double)cq[4] + S[2][1], (double)cq[5] + S[2][2]};
    double o[9];
    icov_closed_form(m, o);
    m6[0] = o[0]; m6[1] = o[1]; m6[2] = o[2]; m6[3] = o[4]; m6[4] = o[5]; m6[5] = o[8];
}
