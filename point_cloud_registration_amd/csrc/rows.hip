// Per-correspondence rows: the sibling of the reduce kernel that WRITES what k_reduce_finalize accumulates.
//
// k_rows<KIND, MODE> streams what the reduce kernel streams -- nn_j, the scan SoA, the matched record -- through the same
// xform and the same gate_f32 / gate_f64, so a point is in or out exactly as in pcr_linearize.
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

template <int KIND>
__device__ __forceinline__ RowCorr row_corr(const LinArgs &a, const PoseK &P, int64_t i, uint32_t j, const float4 &q, const float4 &nr) {
    RowCorr c;
    c.ok = false; c.x = c.y = c.z = 0.0; c.d0 = c.d1 = c.d2 = 0.0; c.n0 = c.n1 = c.n2 = 0.0; c.c6 = nullptr; c.tidx = -1;
    if (j == PCR_NONE) return c;
    const float x = a.sx[i], y = a.sy[i], z = a.sz[i];
    float tx, ty, tz;
    xform(P, x, y, z, tx, ty, tz);
    if (KIND == PCR_ICP || KIND == PCR_PLANE) {
        const float dx = tx - q.x, dy = ty - q.y, dz = tz - q.z;
        if (!gate_f32(a, dx, dy, dz)) return c;
        c.d0 = (double)dx; c.d1 = (double)dy; c.d2 = (double)dz;
        if (KIND == PCR_PLANE) { c.n0 = nr.x; c.n1 = nr.y; c.n2 = nr.z; }
        c.tidx = (int64_t)__float_as_uint(q.w);
    } else {
        const PtD m = a.means[j];
        const double dx = (double)tx - m.x, dy = (double)ty - m.y, dz = (double)tz - m.z;
        if (!gate_f64(a, dx, dy, dz)) return c;
        c.d0 = dx; c.d1 = dy; c.d2 = dz;
        if (KIND == PCR_VPLANE) {
            const double *nn = a.vnorm + 3 * (size_t)j;
            c.n0 = nn[0]; c.n1 = nn[1]; c.n2 = nn[2];
        } else {
            c.c6 = a.vicov + 6 * (size_t)j;
        }
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
        const double r = (c.n0 * c.d0 + c.n1 * c.d1) + c.n2 * c.d2;                         // acc_plane's expressions
        const double ta = P.R[0] * c.n0 + P.R[3] * c.n1 + P.R[6] * c.n2;
        const double tb = P.R[1] * c.n0 + P.R[4] * c.n1 + P.R[7] * c.n2;
        const double tc = P.R[2] * c.n0 + P.R[5] * c.n1 + P.R[8] * c.n2;
        double *J = ra.J + 6 * dest;                                                        // 48 bytes: three 16-byte stores
        store2(J, c.n0, c.n1);
        store2(J + 2, c.n2, -c.z * tb + c.y * tc);
        store2(J + 4, c.z * ta - c.x * tc, -c.y * ta + c.x * tb);
        ra.r[dest] = r;
    } else {
        const double one = c.ok ? 1.0 : 0.0;
        double *J = ra.J + 18 * dest;                                                       // 144 bytes: nine 16-byte stores
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double ri0 = P.R[3 * i], ri1 = P.R[3 * i + 1], ri2 = P.R[3 * i + 2];
            const double a0 = -(ri1 * c.z - ri2 * c.y), a1 = -(-ri0 * c.z + ri2 * c.x), a2 = -(ri0 * c.y - ri1 * c.x);   // acc_ndt's A
            store2(J + 6 * i, i == 0 ? one : 0.0, i == 1 ? one : 0.0);
            store2(J + 6 * i + 2, i == 2 ? one : 0.0, a0);
            store2(J + 6 * i + 4, a1, a2);
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
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double ri0 = P.R[3 * i], ri1 = P.R[3 * i + 1], ri2 = P.R[3 * i + 2];
            A[i][0] = -(ri1 * c.z - ri2 * c.y);
            A[i][1] = -(-ri0 * c.z + ri2 * c.x);
            A[i][2] = -(ri0 * c.y - ri1 * c.x);
        }
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
        double v0, v1, v2;
        if (a.flags & PCR_FLAG_ICP_RR_QUIRK) {                                   // quirk Q1: p x (R r), as acc_icp
            v0 = P.R[0] * r0 + P.R[1] * r1 + P.R[2] * r2;
            v1 = P.R[3] * r0 + P.R[4] * r1 + P.R[5] * r2;
            v2 = P.R[6] * r0 + P.R[7] * r1 + P.R[8] * r2;
        } else {                                                                 // J^T r: p x (R^T r)
            v0 = P.R[0] * r0 + P.R[3] * r1 + P.R[6] * r2;
            v1 = P.R[1] * r0 + P.R[4] * r1 + P.R[7] * r2;
            v2 = P.R[2] * r0 + P.R[5] * r1 + P.R[8] * r2;
        }
        acc[21] = r0; acc[22] = r1; acc[23] = r2;
        acc[24] = c.y * v2 - c.z * v1; acc[25] = c.z * v0 - c.x * v2; acc[26] = c.x * v1 - c.y * v0;
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
        for (int u = 0; u < W; ++u) {
            q[u] = make_float4(0, 0, 0, 0); nr[u] = q[u];
            if (POINT && j[u] != PCR_NONE) {
                if (KIND == PCR_PLANE) { const float4 *rec = reinterpret_cast<const float4 *>(a.pn + j[u]); q[u] = rec[0]; nr[u] = rec[1]; }
                else q[u] = a.pts[j[u]];
            }
        }
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
#define ROWS_CASE(K, M) if (kind == K && mode == M) { hipLaunchKernelGGL((k_rows<K, M>), grid, dim3(256), 0, st, a, ra); return; }
#define ROWS_KIND(K) ROWS_CASE(K, 0) ROWS_CASE(K, 1) ROWS_CASE(K, 2)
    ROWS_KIND(PCR_ICP) ROWS_KIND(PCR_PLANE) ROWS_KIND(PCR_VPLANE) ROWS_KIND(PCR_NDT)
#undef ROWS_KIND
#undef ROWS_CASE
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
