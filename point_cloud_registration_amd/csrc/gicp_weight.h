// The weight of one distribution-to-distribution correspondence, shared by gicp.hip (float32 target covariances) and
// vgicp.hip (float64 voxel covariances): ONE definition of the order in which R Cp R^T is evaluated -- and of the plane
// regulariser both put on a covariance, of the scan side of their pass (DistSide) and of the check of mode and eps.
#pragma once

#include "eigen3.h"
#include "match_pass.h"

// the plane regulariser C = I - (1 - eps) n n^T as xx xy xz yy yz zz: eigenvalues (eps, 1, 1); the sign of n cancels
__device__ __forceinline__ void plane_cov6(const double n[3], double eps, double c[6]) {
    const double s = 1.0 - eps;
    c[0] = 1.0 - s * n[0] * n[0]; c[1] = -s * n[0] * n[1]; c[2] = -s * n[0] * n[2];
    c[3] = 1.0 - s * n[1] * n[1]; c[4] = -s * n[1] * n[2]; c[5] = 1.0 - s * n[2] * n[2];
}

// what a per-point covariance estimate does with the raw covariance of a neighbourhood (k_gicp_cov, k_ball_moments):
// PCR_COV_PLANE replaces it by the plane regulariser of its normal, PCR_COV_RAW keeps it
__device__ __forceinline__ void cov6_finish(int mode, double eps, double c[6]) {
    if (mode == PCR_COV_PLANE) {
        double n[3];
        smallest_eigvec3(c, n);
        plane_cov6(n, eps, c);
    }
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

// s = d^T M d of include/pcr.h: Md_i = (M_i0 d_0 + M_i1 d_1) + M_i2 d_2, s = (d_0 Md_0 + d_1 Md_1) + d_2 Md_2
__device__ __forceinline__ double dist_s(const double m6[6], double d0, double d1, double d2) {
    const double c0 = (m6[0] * d0 + m6[1] * d1) + m6[2] * d2;
    const double c1 = (m6[1] * d0 + m6[3] * d1) + m6[4] * d2;
    const double c2 = (m6[2] * d0 + m6[4] * d1) + m6[5] * d2;
    return (d0 * c0 + d1 * c1) + d2 * c2;
}

// The three f of a distribution SIDE (match_pass.h): f(M6, d).  Plain: acc_ndt.  Weighted: acc_ndt with w M in the place of M,
// w = robust_weight(d^T M d), one product per entry.  Resid: d^T M d
struct DistPlain {
    double *acc;
    const PoseK &P;
    float x, y, z;
    __device__ __forceinline__ DistPlain(double *acc_, const PoseK &P_, float x_, float y_, float z_) : acc(acc_), P(P_), x(x_), y(y_), z(z_) {}
    template <typename RES>                          // (the residual is widened where acc_ndt takes it, as the coordinates are)
    __device__ __forceinline__ void operator()(const double m6[6], RES d0, RES d1, RES d2) const {
        acc_ndt(acc, P, (double)x, (double)y, (double)z, m6, (double)d0, (double)d1, (double)d2);
    }
};
struct DistWeighted {
    double *acc;
    const PoseK &P;
    float x, y, z;
    const RobustK &rb;
    __device__ __forceinline__ DistWeighted(double *acc_, const PoseK &P_, float x_, float y_, float z_, const RobustK &rb_)
        : acc(acc_), P(P_), x(x_), y(y_), z(z_), rb(rb_) {}
    template <typename RES>
    __device__ __forceinline__ void operator()(const double m6[6], RES r0, RES r1, RES r2) const {
        const double d0 = r0, d1 = r1, d2 = r2;
        const double w = robust_weight(rb, dist_s(m6, d0, d1, d2));
        double wm[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) wm[k] = w * m6[k];
        acc_ndt(acc, P, (double)x, (double)y, (double)z, wm, d0, d1, d2);
    }
};
struct DistResid {
    double *s;
    __device__ __forceinline__ DistResid(double *s_, const PoseK &, float, float, float) : s(s_) {}
    template <typename RES>
    __device__ __forceinline__ void operator()(const double m6[6], RES d0, RES d1, RES d2) const { s[0] = dist_s(m6, (double)d0, (double)d1, (double)d2); }
};

// What the two SIDEs of match_pass.h with a covariance on the scan share: the scan covariance through phase A as three
// float2, and the ONE statement of a correspondence, each: residual -> weight -> f(M6, d).  D (GicpArgs, VgicpArgs) adds the
// target side:
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
    typedef DistPlain Plain;
    typedef DistWeighted Weighted;
    typedef DistResid Resid;
    static constexpr int M = 1;
    template <typename MATCH, typename F>
    __device__ __forceinline__ void each(const LinArgs &a, const PoseK &P, float, float, float, float tx, float ty, float tz,
                                         const Scan &s, const MATCH &m, const F &f) const {
        const D &d = static_cast<const D &>(*this);
        typename D::Res dx, dy, dz;
        if (!d.residual(a, m, tx, ty, tz, dx, dy, dz)) return;
        const float cpv[6] = {s.c[0].x, s.c[0].y, s.c[1].x, s.c[1].y, s.c[2].x, s.c[2].y};
        double m6[6];
        d.weight(P, cpv, m, m6);
        f(m6, dx, dy, dz);
    }
    template <typename MATCH>
    __device__ __forceinline__ void add(double *acc, const LinArgs &a, const PoseK &P, float x, float y, float z, float tx, float ty, float tz,
                                        const Scan &s, const MATCH &m) const {
        each(a, P, x, y, z, tx, ty, tz, s, m, Plain(acc, P, x, y, z));
    }
};

// ---- covariance arguments ------------------------------------------------------------------------------------------------
static inline pcr_status check_cov_mode(int mode, double eps) {
    PCR_REQUIRE(mode == PCR_COV_PLANE || mode == PCR_COV_RAW, "mode must be PCR_COV_PLANE or PCR_COV_RAW");
    PCR_REQUIRE(mode == PCR_COV_RAW || (eps > 0.0 && eps <= 1.0), "eps must be in (0, 1]");
    return PCR_OK;
}
