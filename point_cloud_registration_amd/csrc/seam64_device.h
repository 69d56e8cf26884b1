// The float64 searches over a grid's cells (device functions), shared by seam64.hip (pcr_nn_query_dd, pcr_knn_query_f64) and
// radius.hip (the float64 radius search): a ball walk and a ring search that feed a pluggable sink.
//
// One lane = one query.  Distances are (dx*dx + dy*dy) + dz*dz with dx = q - p in float64, no contraction -- nn_test<double>'s
// expression.  Every pruning bound is the distance expression itself evaluated on per-axis gaps (monotone under rounding, so
// a bound never exceeds the computed distance of a record behind it, whatever the magnitudes).
#pragma once

#include "knn_device.h"
#include "pass_device.h"

#define S64_BLOCK KNN_BLOCK
// cells outside the grid box up to which a query is still handed to the searches that start from its own cell
#define S64_PLACE 8

__device__ __forceinline__ double s64_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

template <typename Real>
__device__ __forceinline__ bool s64_placeable(const Geom<Real> &g, Real qx, Real qy, Real qz) {
    const Real m = (Real)S64_PLACE;
    const Real rx = (qx - g.ox) * g.inv_h, ry = (qy - g.oy) * g.inv_h, rz = (qz - g.oz) * g.inv_h;
    // (false for NaN and +-inf)
    return rx >= -m && rx <= (Real)g.nx + m && ry >= -m && ry <= (Real)g.ny + m && rz >= -m && rz <= (Real)g.nz + m;
}

// how far rounding to float32 moved the query (metres, rounded up)
__device__ __forceinline__ double s64_displacement(double qx, double qy, double qz, float fx, float fy, float fz) {
    const double ex = qx - (double)fx, ey = qy - (double)fy, ez = qz - (double)fz;
    return __builtin_sqrt((ex * ex + ey * ey) + ez * ez) * 1.000000001;
}

// ---- what a search feeds: the best record (k = 1) or the sorted list ---------------------------------------------------
// bound(): a region is skipped when a lower bound on its records' computed distances EXCEEDS it (a record AT the bound may
// still win on the smaller index)
struct S64Best {
    double bd;
    uint32_t bj, bo;
    __device__ __forceinline__ void init(double bound2) { bd = bound2; bj = PCR_NONE; bo = PCR_NONE; }
    __device__ __forceinline__ double bound() const { return bd; }
    __device__ __forceinline__ void offer(double d, uint32_t j, uint32_t o) {
        const bool take = (d < bd) | ((d == bd) & (o < bo));               // nn_test<double>'s rule
        bd = take ? d : bd; bj = take ? j : bj; bo = take ? o : bo;
    }
};

// (float64 squared distance, cell-sorted index), ascending by (distance, original index); [slot][lane] in LDS, 12 bytes per
// slot and lane.  The original index is read from the records only when two distances are equal.
struct S64List {
    double *d;          // + lane
    uint32_t *j;        // + lane
    const PtD *pts;
    int k, cnt;
    double kth;         // the k-th best once the list is full; before that an upper bound on it (+inf: none)
    uint32_t kth_j;
    __device__ __forceinline__ void init(char *smem, int k_, const PtD *pts_) {
        k = k_; pts = pts_;
        d = (double *)smem + threadIdx.x;
        j = (uint32_t *)(smem + sizeof(double) * (size_t)k_ * S64_BLOCK) + threadIdx.x;
        reset(s64_inf());
    }
    __device__ __forceinline__ void reset(double bound2) { cnt = 0; kth = bound2; kth_j = PCR_NONE; }
    __device__ __forceinline__ double bound() const { return kth; }
    __device__ __forceinline__ double &D(int s) { return d[s * S64_BLOCK]; }
    __device__ __forceinline__ uint32_t &J(int s) { return j[s * S64_BLOCK]; }
    __device__ __forceinline__ uint32_t O(int s) { return pt_orig(pts[j[s * S64_BLOCK]]); }
    __device__ __forceinline__ void offer(double dd, uint32_t jj, uint32_t oo) {
        if (cnt == k) {
            if (!(dd < kth || (dd == kth && oo < pt_orig(pts[kth_j])))) return;
        } else if (!(dd <= kth)) return;                                    // (beyond the first radius, or NaN)
        int p = cnt < k ? cnt : k - 1;
        while (p > 0) {
            const double dp = D(p - 1);
            if (!(dp > dd || (dp == dd && O(p - 1) > oo))) break;
            D(p) = dp; J(p) = J(p - 1);
            --p;
        }
        D(p) = dd; J(p) = jj;
        if (cnt < k) ++cnt;
        if (cnt == k) { kth = D(k - 1); kth_j = J(k - 1); }
    }
};

// Records [s, e), four requested together.  A batch may read past e (the arrays carry PCR_PTS_PAD sentinels), but those
// records are not offered: they belong to a cell that is visited on its own, and a list would hold them twice.
template <typename SINK>
__device__ __forceinline__ void s64_scan(SINK &S, const PtD *__restrict__ pts, uint32_t s, uint32_t e, double qx, double qy, double qz) {
    for (uint32_t j = s; j < e; j += 4) {
        PtD p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = pts[j + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j + u < e) {
                const double dx = qx - p[u].x, dy = qy - p[u].y, dz = qz - p[u].z;
                S.offer((dx * dx + dy * dy) + dz * dz, j + u, pt_orig(p[u]));
            }
        }
    }
}

// |q - p| >= this for every coordinate p in [lo, hi], and fl(q - p) too: rounding is monotone
__device__ __forceinline__ double s64_gap(double q, double lo, double hi) { return fmax(fmax(lo - q, q - hi), 0.0); }
// the coordinates of cells c0..c1 of one axis (a record's float64 position lies within `slack` of its cell)
__device__ __forceinline__ double s64_cells_gap(const Geom<double> &g, double q, double o, int c0, int c1) {
    return s64_gap(q, (o + (double)c0 * g.h) - g.slack, (o + (double)(c1 + 1) * g.h) + g.slack);
}
// the cell of a coordinate, clamped into the grid (nn_box_f64's)
__device__ __forceinline__ int s64_cell(const Geom<double> &g, double v, double o, int n) {
    const double c = fmin(fmax((v - o) * g.inv_h, -1.0e9), 1.0e9);
    return min(max((int)floor(c), 0), n - 1);
}

// The ball of radius r (slack included) around the query: its cell box slab by slab, the entries of five rows requested
// together, as nn_box_f64 walks the ball through a nominee; a slab or row beyond the sink's bound is skipped.
template <typename SINK>
__device__ __forceinline__ void s64_ball_walk(const Geom<double> &g, const PtD *__restrict__ pts, const uint32_t *__restrict__ cs,
                                              double qx, double qy, double qz, double r, SINK &S) {
    const int xl = s64_cell(g, qx - r, g.ox, g.nx), xh = s64_cell(g, qx + r, g.ox, g.nx);
    const int yl = s64_cell(g, qy - r, g.oy, g.ny), yh = s64_cell(g, qy + r, g.oy, g.ny);
    const int zl = s64_cell(g, qz - r, g.oz, g.nz), zh = s64_cell(g, qz + r, g.oz, g.nz);
    const uint32_t unx = (uint32_t)g.nx, plane = (uint32_t)g.ny * unx;
    for (int z = zl; z <= zh; ++z) {
        const double az = s64_cells_gap(g, qz, g.oz, z, z);
        const double az2 = az * az;
        if (az2 > S.bound()) continue;
        for (int y0 = yl; y0 <= yh; y0 += 5) {
            uint32_t s_[5], e_[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int y = min(y0 + u, yh);
                const double ay = s64_cells_gap(g, qy, g.oy, y, y);
                const bool live = y0 + u <= yh && ay * ay + az2 <= S.bound();
                const uint32_t row = (uint32_t)z * plane + (uint32_t)y * unx;
                const uint32_t s0 = cs[row + (uint32_t)xl] & g.cs_mask, e0 = cs[row + (uint32_t)xh + 1u] & g.cs_mask;
                s_[u] = s0; e_[u] = live ? e0 : s0;
            }
#pragma unroll
            for (int u = 0; u < 5; ++u) s64_scan(S, pts, s_[u], e_[u], qx, qy, qz);
        }
    }
}

// Exact search from nothing: Chebyshev rings of cells around the query's cell clamped into the grid.  After rings 0..k-1 every
// record not yet seen lies beyond one of the six faces of that cube of cells; the nearest such face (faces past the grid's
// edge hold nothing) bounds them all.  At most max(nx, ny, nz) rings, wherever the query is.
template <typename SINK>
__device__ __forceinline__ void s64_ring_search(const Geom<double> &g, const PtD *__restrict__ pts, const uint32_t *__restrict__ cs,
                                                double qx, double qy, double qz, SINK &S) {
    const int cx = s64_cell(g, qx, g.ox, g.nx), cy = s64_cell(g, qy, g.oy, g.ny), cz = s64_cell(g, qz, g.oz, g.nz);
    const int kmax = max(max(max(cx, g.nx - 1 - cx), max(cy, g.ny - 1 - cy)), max(cz, g.nz - 1 - cz));
    const uint32_t unx = (uint32_t)g.nx, plane = (uint32_t)g.ny * unx;
    for (int k = 0; k <= kmax; ++k) {
        if (k >= 1) {
            double lb = s64_inf();
            if (cx - k >= 0) { const double a = s64_cells_gap(g, qx, g.ox, 0, cx - k); lb = fmin(lb, a * a); }
            if (cx + k < g.nx) { const double a = s64_cells_gap(g, qx, g.ox, cx + k, g.nx - 1); lb = fmin(lb, a * a); }
            if (cy - k >= 0) { const double a = s64_cells_gap(g, qy, g.oy, 0, cy - k); lb = fmin(lb, a * a); }
            if (cy + k < g.ny) { const double a = s64_cells_gap(g, qy, g.oy, cy + k, g.ny - 1); lb = fmin(lb, a * a); }
            if (cz - k >= 0) { const double a = s64_cells_gap(g, qz, g.oz, 0, cz - k); lb = fmin(lb, a * a); }
            if (cz + k < g.nz) { const double a = s64_cells_gap(g, qz, g.oz, cz + k, g.nz - 1); lb = fmin(lb, a * a); }
            if (lb > S.bound()) break;
        }
        const int ylo = max(cy - k, 0), yhi = min(cy + k, g.ny - 1);
        const int xlo = max(cx - k, 0), xhi = min(cx + k, g.nx - 1);
        for (int z = max(cz - k, 0); z <= min(cz + k, g.nz - 1); ++z) {
            const double az = s64_cells_gap(g, qz, g.oz, z, z);
            const double az2 = az * az;
            if (az2 > S.bound()) continue;
            const bool zshell = z - cz == k || cz - z == k;
            for (int y = ylo; y <= yhi; ++y) {
                const double ay = s64_cells_gap(g, qy, g.oy, y, y);
                const double ay2 = ay * ay;
                if (ay2 + az2 > S.bound()) continue;
                const uint32_t row = (uint32_t)z * plane + (uint32_t)y * unx;
                // a cell of this row is worth a visit while (ax*ax + ay*ay) + az*az, the distance expression on the gaps, is
                // within the bound
                auto beyond = [&](int x) {
                    const double ax = s64_cells_gap(g, qx, g.ox, x, x);
                    return (ax * ax + ay2) + az2 > S.bound();
                };
                if (zshell || y - cy == k || cy - y == k) {            // a face row of the ring: cells xlo..xhi, cut to the bound
                    int xl = xlo, xh = xhi;
                    while (xl <= xh && beyond(xl)) ++xl;
                    while (xh > xl && beyond(xh)) --xh;
                    if (xl <= xh) s64_scan(S, pts, cs[row + (uint32_t)xl] & g.cs_mask, cs[row + (uint32_t)xh + 1u] & g.cs_mask, qx, qy, qz);
                } else {                                                // an interior row: its two end cells
                    const int xa = cx - k, xb = cx + k;
                    if (xa >= 0 && !beyond(xa)) s64_scan(S, pts, cs[row + (uint32_t)xa] & g.cs_mask, cs[row + (uint32_t)xa + 1u] & g.cs_mask, qx, qy, qz);
                    if (xb < g.nx && !beyond(xb)) s64_scan(S, pts, cs[row + (uint32_t)xb] & g.cs_mask, cs[row + (uint32_t)xb + 1u] & g.cs_mask, qx, qy, qz);
                }
            }
        }
    }
}
