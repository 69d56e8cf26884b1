// Per-correspondence rows: the kernel that WRITES what k_reduce_finalize accumulates.
//
// k_rows<KIND, MODE> sits where the reduce kernel would: it streams nn_j, the scan SoA and the matched record, and takes the
// correspondence (gather_point, residual_f32 / _f64: residual and gate) and every Jacobian expression (plane_row, skew_A / skew_row,
// icp_v, acc_plane, acc_ndt) from pass_device.h, where the reduce and fused kernels take them: a point is in or out exactly as in
// pcr_linearize, and nothing below restates an expression of the sums.
//   MODE 0 (rows):  per scan point J (m x 6), r (m), w (1 in / 0 out), idx (target index, -1 out) and, for NDT, the
//                   symmetric 3 x 3 inverse covariance; rows of a gated-out point are zero.  Runs in the scan's DEVICE
//                   order (lane l of a wave = point l of 64 consecutive ones, like reduce_stream) and scatters each
//                   point's rows to its caller index through pcr_scan::order.
//   MODE 2 (flags): the gate alone, in device order: flag[caller index] = in / out, inv[caller index] = device position.
//   MODE 1 (terms): after an exclusive scan of the flags, in CALLER order: the gated-in point with caller index c writes
//                   column off[c] of the row-major P[28][stride] -- [triu(H) 21, g 6, e2], exactly what one call of
//                   accumulate<KIND, true> adds to a zeroed acc -- and col_idx[off[c]] = c.  Neighbouring lanes write
//                   neighbouring columns: each of the 28 stores of a wave is coalesced, and the columns are the gated-in
//                   points in ascending caller index whatever the grid.  The price is the gather of the point itself
//                   (index + 12 bytes) through inv, against 224 bytes written.
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "pass_device.h"

// what one correspondence is made of (zero / -1 when the point has no match inside the gate)
struct RowCorr {
    bool ok;
    double x, y, z;          // the scan point (untransformed)
    double d0, d1, d2;       // transformed point - matched point
    double n0, n1, n2;       // the matched normal (PLANE / VPLANE)
    const double *c6;        // the matched inverse covariance (NDT): xx xy xz yy yz zz
    int64_t tidx;            // caller's target index / voxel position
};

// fills RowCorr from the shared residual + gate (pass_device.h: residual_f32 / residual_f64)
template <int KIND>
__device__ __forceinline__ RowCorr row_corr(const LinArgs &a, const PoseK &P, int64_t i, uint32_t j, const float4 &q, const float4 &nr) {
    RowCorr c;
    c.ok = false; c.x = c.y = c.z = 0.0; c.d0 = c.d1 = c.d2 = 0.0; c.n0 = c.n1 = c.n2 = 0.0; c.c6 = nullptr; c.tidx = -1;
    if (j == PCR_NONE) return c;
    const float x = a.sx[i], y = a.sy[i], z = a.sz[i];
    float tx, ty, tz;
    xform(P, x, y, z, tx, ty, tz);
    if (KIND == PCR_ICP || KIND == PCR_PLANE) {
        float dx, dy, dz;
        if (!residual_f32<true>(a, q, tx, ty, tz, dx, dy, dz)) return c;
        c.d0 = (double)dx; c.d1 = (double)dy; c.d2 = (double)dz;
        if (KIND == PCR_PLANE) { c.n0 = nr.x; c.n1 = nr.y; c.n2 = nr.z; }
        c.tidx = (int64_t)__float_as_uint(q.w);
    } else {
        PtD m;
        double dx, dy, dz;
        if (!residual_f64<true>(a, j, tx, ty, tz, m, dx, dy, dz)) return c;
        c.d0 = dx; c.d1 = dy; c.d2 = dz;
        if (KIND == PCR_VPLANE) { const double *nn = vox_normal(a, j); c.n0 = nn[0]; c.n1 = nn[1]; c.n2 = nn[2]; }
        else c.c6 = vox_icov(a, j);
        c.tidx = (int64_t)__double_as_longlong(m.w);
    }
    c.ok = true; c.x = x; c.y = y; c.z = z;
    return c;
}

__device__ __forceinline__ void store2(double *p, double v0, double v1) { *reinterpret_cast<double2 *>(p) = make_double2(v0, v1); }

// MODE 0: the rows of one point, at row `dest` of the caller-order arrays
template <int KIND>
__device__ __forceinline__ void rows_store(const RowArgs &ra, const PoseK &P, const RowCorr &c, int64_t dest) {
    ra.w[dest] = c.ok ? 1.0 : 0.0;
    if (ra.idx) ra.idx[dest] = c.tidx;
    if (KIND == PCR_PLANE || KIND == PCR_VPLANE) {
        double Jr[6];
        const double r = plane_row(P, c.x, c.y, c.z, c.n0, c.n1, c.n2, c.d0, c.d1, c.d2, Jr);
        double *J = ra.J + 6 * dest;                                                        // 48 bytes: three 16-byte stores
        store2(J, Jr[0], Jr[1]);
        store2(J + 2, Jr[2], Jr[3]);
        store2(J + 4, Jr[4], Jr[5]);
        ra.r[dest] = r;
    } else {
        const double one = c.ok ? 1.0 : 0.0;
        double *J = ra.J + 18 * dest;                                                       // 144 bytes: nine 16-byte stores
#pragma unroll
        for (int i = 0; i < 3; ++i) {                                                       // (row by row: nine values never live at once)
            double Ai[3];
            skew_row(P, i, c.x, c.y, c.z, Ai);
            store2(J + 6 * i, i == 0 ? one : 0.0, i == 1 ? one : 0.0);
            store2(J + 6 * i + 2, i == 2 ? one : 0.0, Ai[0]);
            store2(J + 6 * i + 4, Ai[1], Ai[2]);
        }
        double *r = ra.r + 3 * dest;
        r[0] = c.d0; r[1] = c.d1; r[2] = c.d2;
        if (KIND == PCR_NDT && ra.W) {
            double *W = ra.W + 9 * dest;
            double v[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = c.ok ? c.c6[k] : 0.0;
            W[0] = v[0]; W[1] = v[1]; W[2] = v[2];
            W[3] = v[1]; W[4] = v[3]; W[5] = v[4];
            W[6] = v[2]; W[7] = v[4]; W[8] = v[5];
        }
    }
}

// MODE 1: the point's 28 terms under the call's flags, into column `col` of P
template <int KIND>
__device__ __forceinline__ void terms_store(const LinArgs &a, const RowArgs &ra, const PoseK &P, const RowCorr &c, int64_t col, int64_t caller) {
    double acc[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    if (KIND == PCR_PLANE || KIND == PCR_VPLANE) {
        acc_plane(acc, P, c.x, c.y, c.z, c.n0, c.n1, c.n2, c.d0, c.d1, c.d2);
    } else if (KIND == PCR_NDT) {
        acc_ndt(acc, P, c.x, c.y, c.z, c.c6, c.d0, c.d1, c.d2);
    } else {
        // ICP, written out from J = [I, A], A = -R skew(p): H = [[I, A], [., A^T A]], g = [r, p x v], e2 = r . r
        double A[3][3];
        skew_A(P, c.x, c.y, c.z, A);
        int p = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i; j < 3; ++j) { acc[p] = i == j ? 1.0 : 0.0; ++p; }
#pragma unroll
            for (int j = 0; j < 3; ++j) { acc[p] = A[i][j]; ++p; }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) { acc[p] = A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j]; ++p; }
        const double r0 = c.d0, r1 = c.d1, r2 = c.d2;
        const double3 v = icp_v(P, a.flags, r0, r1, r2);
        acc[21] = r0; acc[22] = r1; acc[23] = r2;
        acc[24] = c.y * v.z - c.z * v.y; acc[25] = c.z * v.x - c.x * v.z; acc[26] = c.x * v.y - c.y * v.x;
        acc[27] = r0 * r0 + r1 * r1 + r2 * r2;
    }
#pragma unroll
    for (int m = 0; m < 28; ++m) ra.P[(int64_t)m * ra.stride + col] = acc[m];
    ra.col_idx[col] = caller;
}

template <int KIND, int MODE>
__global__ void __launch_bounds__(256) k_rows(const LinArgs a, const RowArgs ra) {
    const PoseK &P = a.hp;                       // host-driven: the pose came by value
    constexpr bool POINT = KIND == PCR_ICP || KIND == PCR_PLANE;
    constexpr int W = POINT ? 2 : 1;             // point targets: two gathers in flight per lane (reduce_stream)
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x; t0 < a.n; t0 += W * stride) {
        int64_t i[W];
        uint32_t j[W];
        float4 q[W], nr[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const int64_t t = t0 + u * stride;
            i[u] = -1; j[u] = PCR_NONE;
            if (t < a.n) {
                if (MODE == 1) {
                    if (ra.flag[t]) i[u] = ra.inv ? (int64_t)ra.inv[t] : t;
                } else {
                    i[u] = t;
                }
                if (i[u] >= 0) j[u] = a.nn_j[i[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < W; ++u) gather_point<KIND>(a, j[u], q[u], nr[u]);
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const int64_t t = t0 + u * stride;
            if (t >= a.n || i[u] < 0) continue;
            const RowCorr c = row_corr<KIND>(a, P, i[u], j[u], q[u], nr[u]);
            if (MODE == 1) {
                if (!c.ok) continue;             // (cannot happen: the flag pass applied the same gate to the same numbers)
                terms_store<KIND>(a, ra, P, c, (int64_t)ra.off[t], t);
            } else {
                const int64_t dest = ra.order ? (int64_t)ra.order[i[u]] : i[u];
                if (MODE == 2) { ra.flag[dest] = c.ok ? 1u : 0u; if (ra.inv) ra.inv[dest] = (uint32_t)i[u]; }
                else rows_store<KIND>(ra, P, c, dest);
            }
        }
    }
}

void launch_rows(int kind, int mode, dim3 grid, hipStream_t st, const LinArgs &a, const RowArgs &ra) {
    with_const<4>(kind, [&](auto K) {
        with_const<3>(mode, [&](auto M) { hipLaunchKernelGGL((k_rows<K(), M()>), grid, dim3(256), 0, st, a, ra); });
    });
}

// off[0 .. n] = exclusive sums of flag[0 .. n] (flag[n] = 0, so off[n] is the number of gated-in points)
pcr_status pcr_rows_offsets(pcr_context *ctx, const uint32_t *flag, uint32_t *off, int64_t n_plus_1) {
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, flag, off, 0u, (size_t)n_plus_1, rocprim::plus<uint32_t>(), ctx->stream));
    DevBuf<char> tmp;
    HIP_TRY(tmp.alloc_bytes(tmp_bytes));
    HIP_TRY(rocprim::exclusive_scan(tmp.p, tmp_bytes, flag, off, 0u, (size_t)n_plus_1, rocprim::plus<uint32_t>(), ctx->stream));
    return PCR_OK;
}
