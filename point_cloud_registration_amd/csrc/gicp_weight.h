// The weight of one distribution-to-distribution correspondence, shared by gicp.hip (float32 target covariances) and
// vgicp.hip (float64 voxel covariances): ONE definition of the order in which R Cp R^T is evaluated -- and of the plane
// regulariser both put on a covariance, of the scan side of their pass (DistSide) and of the check of mode and eps.
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

// What the two SIDEs of match_pass.h with a covariance on the scan share: the scan covariance through phase A as three
// float2, and residual -> weight -> acc_ndt (with M6).  D (GicpArgs, VgicpArgs) adds the target side:
//   Match, gather             (match_pass.h)
//   Res                       the type of the residual (float / double)
//   residual(a, m, t.., d..)  residual_f32<true> / residual_f64<true> on the gathered match: residual and gate
//   weight(P, cp, m, m6)      gicp_weight with the match's covariance
template <typename D>
struct DistSide {
    const float *scov;       // scan covariances, device order, 6 floats per point

    struct Scan { float2 c[3]; };
    __device__ __forceinline__ void load(int64_t i, Scan &s) const {
        const float2 *c = reinterpret_cast<const float2 *>(scov + 6 * i);
        s.c[0] = c[0]; s.c[1] = c[1]; s.c[2] = c[2];
    }
    template <typename MATCH>
    __device__ __forceinline__ void add(double *acc, const LinArgs &a, const PoseK &P, float x, float y, float z, float tx, float ty, float tz,
                                        const Scan &s, const MATCH &m) const {
        const D &d = static_cast<const D &>(*this);
        typename D::Res dx, dy, dz;
        if (!d.residual(a, m, tx, ty, tz, dx, dy, dz)) return;
        const float cpv[6] = {s.c[0].x, s.c[0].y, s.c[1].x, s.c[1].y, s.c[2].x, s.c[2].y};
        double m6[6];
        d.weight(P, cpv, m, m6);
        acc_ndt(acc, P, (double)x, (double)y, (double)z, m6, (double)dx, (double)dy, (double)dz);
    }
};

// ---- covariance arguments ------------------------------------------------------------------------------------------------
static inline pcr_status check_cov_mode(int mode, double eps) {
    PCR_REQUIRE(mode == PCR_COV_PLANE || mode == PCR_COV_RAW, "mode must be PCR_COV_PLANE or PCR_COV_RAW");
    PCR_REQUIRE(mode == PCR_COV_RAW || (eps > 0.0 && eps <= 1.0), "eps must be in (0, 1]");
    return PCR_OK;
}
