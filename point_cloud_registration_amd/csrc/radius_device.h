// The float32 ball walk of the exact radius search (device functions), shared by radius.hip and fpfh.hip.
//
// Membership is decided by the distance pcr_knn_query would report for the pair: d2 = dist2_f32(q - p) (nn_device.h), member
// iff __builtin_sqrtf(d2) <= r.  The walk has the form of s64_ball_walk (seam64_device.h): slabs, rows skipped by their (y, z)
// gap, each row's x range clipped by sqrt(B - dyz2) + slack, cells clamped into the grid, records fetched KNN_BATCH at a time
// and none past the end of a range offered (knn_scan_range's rule).  A ball that misses the grid box returns before the first
// row look-up.
//
// A sink has  bound()                       an upper bound on the d2 of everything it wants (rad_bound2), read once
//             offer(d2, j, orig)            one record: its float32 d2, cell-sorted index and original index
#pragma once

#include <float.h>

#include "knn_device.h"

#define RAD_BLOCK 64
#define RAD_ROWS 4           // rows whose cell_start entries are requested together

// ---- membership -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool rad_member(float d2, float r) { return __builtin_sqrtf(d2) <= r; }
__device__ __forceinline__ bool rad_member(double d2, double r) { return __builtin_sqrt(d2) <= r; }
// an upper bound on the d2 of every member (pruning and the pre-test only; rad_member decides).  The smallest normal number
// covers radii whose square is subnormal.
__device__ __forceinline__ float rad_bound2(float r) { return r * r * 1.00001f + FLT_MIN; }
__device__ __forceinline__ double rad_bound2(double r) { const double rr = r * 1.0000001; return rr * rr + DBL_MIN; }
// all three coordinates of a query finite (false for NaN): a query that is not walks nothing
template <typename Real>
__device__ __forceinline__ bool rad_finite(Real x, Real y, Real z) {
    const Real big = RealTraits<Real>::inf();
    return x > -big && x < big && y > -big && y < big && z > -big && z < big;
}

// ---- the float32 ball walk ------------------------------------------------------------------------------------------------
template <typename SINK>
__device__ __forceinline__ void rad_scan_f32(SINK &S, const PtF *__restrict__ pts, uint32_t s, uint32_t e, float qx, float qy, float qz) {
    for (uint32_t j = s; j < e; j += KNN_BATCH) {
        PtF p[KNN_BATCH];
#pragma unroll
        for (int u = 0; u < KNN_BATCH; ++u) p[u] = pts[j + u];
#pragma unroll
        for (int u = 0; u < KNN_BATCH; ++u) {
            if (j + u < e) {
                const float dx = qx - p[u].x, dy = qy - p[u].y, dz = qz - p[u].z;
                S.offer(dist2_f32(dx, dy, dz), j + u, pt_orig(p[u]));
            }
        }
    }
}

// |q - p| >= this for every record of cell c of one axis (a record lies within `slack` of its cell)
__device__ __forceinline__ float rad_cell_gap(const Geom<float> &g, float q, float o, int c) {
    const float lo = (o + (float)c * g.h) - g.slack, hi = (o + (float)(c + 1) * g.h) + g.slack;
    return fmaxf(fmaxf(lo - q, q - hi), 0.f);
}
// the cell of a coordinate, NOT clamped into the grid (NaN: far below)
__device__ __forceinline__ int rad_cell(const Geom<float> &g, float v, float o) {
    return (int)floorf(fminf(fmaxf((v - o) * g.inv_h, -1.0e9f), 1.0e9f));
}

template <typename SINK>
__device__ __forceinline__ void rad_ball_walk(const Geom<float> &g, const PtF *__restrict__ pts, const uint32_t *__restrict__ cs,
                                              float qx, float qy, float qz, float r, SINK &S) {
    const float lim = 1.0e9f;
    // g.slack covers roundings at the magnitude of the grid's own coordinates; a query far from the grid rounds at its own
    const float pad = g.slack + 1.0e-6f * (fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)) + r);
    const float R = r + pad;
    int xl = rad_cell(g, qx - R, g.ox), xh = rad_cell(g, qx + R, g.ox);
    int yl = rad_cell(g, qy - R, g.oy), yh = rad_cell(g, qy + R, g.oy);
    int zl = rad_cell(g, qz - R, g.oz), zh = rad_cell(g, qz + R, g.oz);
    if (xl > g.nx - 1 || xh < 0 || yl > g.ny - 1 || yh < 0 || zl > g.nz - 1 || zh < 0) return;       // the ball misses the grid box
    xl = max(xl, 0); xh = min(xh, g.nx - 1);
    yl = max(yl, 0); yh = min(yh, g.ny - 1);
    zl = max(zl, 0); zh = min(zh, g.nz - 1);
    const float B = S.bound();
    for (int z = zl; z <= zh; ++z) {
        const float dzm = rad_cell_gap(g, qz, g.oz, z);
        const float dz2 = dzm * dzm;
        if (dz2 > B) continue;
        for (int y0 = yl; y0 <= yh; y0 += RAD_ROWS) {
            uint32_t s_[RAD_ROWS], e_[RAD_ROWS];
#pragma unroll
            for (int u = 0; u < RAD_ROWS; ++u) {
                const int y = min(y0 + u, yh);
                const float dym = rad_cell_gap(g, qy, g.oy, y);
                const float dyz2 = dz2 + dym * dym;
                int x0 = xl, x1 = xh;
                const float xr = __builtin_sqrtf(fmaxf(B - dyz2, 0.f)) + pad;
                const float a = (qx - xr - g.ox) * g.inv_h, b = (qx + xr - g.ox) * g.inv_h;
                if (a > (float)x0) x0 = (int)floorf(fminf(a, lim));
                if (b < (float)x1) x1 = (int)floorf(fmaxf(b, -lim));
                const bool live = y0 + u <= yh && dyz2 <= B && x0 <= x1;
                x0 = min(max(x0, 0), g.nx - 1); x1 = min(max(x1, 0), g.nx - 1);      // (a dead row is still addressed)
                const size_t row = ((size_t)z * (size_t)g.ny + (size_t)y) * (size_t)g.nx;
                const uint32_t s0 = cs[row + x0] & g.cs_mask, e0 = cs[row + x1 + 1] & g.cs_mask;
                s_[u] = s0; e_[u] = live ? e0 : s0;
            }
#pragma unroll
            for (int u = 0; u < RAD_ROWS; ++u) rad_scan_f32(S, pts, s_[u], e_[u], qx, qy, qz);
        }
    }
}

// ---- a sink: the moments of the members ------------------------------------------------------------------------------------
// Float64 sums of d = q - a and d d^T over the members, a = the FIRST member offered.  rad_ball_walk offers records in ascending
// cell-sorted index for any query -- slabs by z, rows by y, a row's cells by x, one contiguous range of records per row -- so the
// anchor and the order of the sums are functions of the member set alone.  The anchor, the 9 sums and k stay in registers.
// Shared by keypoints.hip (k_iss_saliency) and ball_moments.hip; add() alone sums a list that is not walked.
struct RadMoments {
    float r, b2;
    const PtF *pts;
    double ax, ay, az;       // the anchor: the first member offered
    double s1[3], s2[6];     // sums of d and of d d^T (xx xy xz yy yz zz)
    uint32_t k;
    __device__ __forceinline__ void init(float r_, const PtF *pts_) {
        r = r_; b2 = rad_bound2(r_); pts = pts_; k = 0u;
        ax = ay = az = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) s1[c] = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s2[c] = 0.0;
    }
    __device__ __forceinline__ float bound() const { return b2; }
    __device__ __forceinline__ void add(const PtF q) {
        if (k == 0u) { ax = (double)q.x; ay = (double)q.y; az = (double)q.z; }
        const double dx = (double)q.x - ax, dy = (double)q.y - ay, dz = (double)q.z - az;
        s1[0] = s1[0] + dx; s1[1] = s1[1] + dy; s1[2] = s1[2] + dz;
        s2[0] = s2[0] + dx * dx; s2[1] = s2[1] + dx * dy; s2[2] = s2[2] + dx * dz;
        s2[3] = s2[3] + dy * dy; s2[4] = s2[4] + dy * dz; s2[5] = s2[5] + dz * dz;
        ++k;
    }
    __device__ __forceinline__ void offer(float d2f, uint32_t j, uint32_t) {
        if (d2f <= b2 && rad_member(d2f, r)) add(pts[j]);                    // (NaN fails the pre-test)
    }
    // m = s1 / k and the raw covariance C = s2 / k - m m^T (xx xy xz yy yz zz); zeros for the empty set
    __device__ __forceinline__ void finish(double m[3], double c[6]) const {
        const double kd = (double)(k != 0u ? k : 1u);
        m[0] = s1[0] / kd; m[1] = s1[1] / kd; m[2] = s1[2] / kd;
        c[0] = s2[0] / kd - m[0] * m[0]; c[1] = s2[1] / kd - m[0] * m[1]; c[2] = s2[2] / kd - m[0] * m[2];
        c[3] = s2[3] / kd - m[1] * m[1]; c[4] = s2[4] / kd - m[1] * m[2]; c[5] = s2[5] / kd - m[2] * m[2];
    }
};
