// The distribution pass behind GICP and VGICP, stated once: the three-phase reduce loop, the fold, and the host driver of
// the two launches.  Included by gicp.hip and vgicp.hip only; each keeps its own __global__ one-liners (k_gicp_* / k_vgicp_*).
//
// A SIDE is the target side's kernel-argument struct (GicpArgs, VgicpArgs): scov, the target array, rows -- and
//   Match, Res                what phase B gathers per correspondence, and the type of the residual (float / double)
//   gather(a, j, Match&)      the loads of one match at cell-sorted index j; nothing else
//   residual(a, m, t.., d..)  residual_f32<true> / residual_f64<true> on the gathered match: residual and gate
//   weight(P, cp, m, m6)      gicp_weight with the match's covariance
#pragma once

#include "gicp_weight.h"
#include "host_util.h"

// W points per lane in flight, the phases of reduce_stream (pass_device.h):
//   phase A  index, coordinates and scan covariance of all W points.  A point past the end reads the lane's first point.
//   phase B  the W matches.  No match: element 0 through a select on the index -- always there -- and skipped in phase C;
//            no branch between the gathers.
//   phase C  residual, gate, weight, sums (acc_ndt with M6) -- in index order.
// Fold: wave shuffles in a fixed order, LDS across the waves in wave order, ONE row of 32 doubles per block with plain
// stores (block_store_partials).  No tickets, no atomics, no in-launch hand-off.
template <int W, typename SIDE>
__device__ __forceinline__ void dist_reduce(const LinArgs &a, const SIDE &sd) {
    const PoseK &P = a.hp;                           // host-driven: the pose came by value
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x; t0 < a.n; t0 += W * stride) {
        uint32_t j[W];
        float x[W], y[W], z[W];
        float2 cp[W][3];
        typename SIDE::Match m[W];
        bool use[W];
        // phase A
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const int64_t t = t0 + u * stride;
            use[u] = t < a.n;
            const int64_t i = use[u] ? t : t0;
            j[u] = a.nn_j[i];
            x[u] = a.sx[i]; y[u] = a.sy[i]; z[u] = a.sz[i];
            const float2 *c = reinterpret_cast<const float2 *>(sd.scov + 6 * i);
            cp[u][0] = c[0]; cp[u][1] = c[1]; cp[u][2] = c[2];
        }
        reduce_phase();
#pragma unroll
        for (int u = 0; u < W; ++u) reduce_pin(j[u]);
        // phase B
#pragma unroll
        for (int u = 0; u < W; ++u) {
            use[u] = use[u] && j[u] != PCR_NONE;
            sd.gather(a, use[u] ? j[u] : 0u, m[u]);
        }
        reduce_phase();
        // phase C
#pragma unroll
        for (int u = 0; u < W; ++u) {
            if (!use[u]) continue;
            float tx, ty, tz;
            typename SIDE::Res dx, dy, dz;
            xform(P, x[u], y[u], z[u], tx, ty, tz);
            if (!sd.residual(a, m[u], tx, ty, tz, dx, dy, dz)) continue;
            const float cpv[6] = {cp[u][0].x, cp[u][0].y, cp[u][1].x, cp[u][1].y, cp[u][2].x, cp[u][2].y};
            double m6[6];
            sd.weight(P, cpv, m[u], m6);
            acc_ndt(acc, P, (double)x[u], (double)y[u], (double)z[u], m6, (double)dx, (double)dy, (double)dz);
        }
    }
    block_store_partials<false>(acc, sd.rows);
}

// one block: thread e < 29 adds rows 0 .. nb-1 in order.  The kernel boundary is the only ordering between the two launches;
// the grid depends on n and the device only, so two calls return the same bits.
__device__ __forceinline__ void dist_fold(const double *__restrict__ rows, int nb, double *out) {
    const int e = threadIdx.x;
    if (e >= 29) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += rows[(size_t)b * 32 + e];
    out[e] = s;
}

// reduce + fold + 29 doubles back behind a search into `a`: one stream synchronisation, device blocks from the context's
// block cache.  sd comes with scov and the target array set.
template <typename SIDE>
static pcr_status dist_launch(pcr_context *ctx, const char *range_name, void (*reduce)(const LinArgs, const SIDE),
                              void (*fold)(const double *, int, double *), const LinArgs &a, SIDE sd, int64_t n, double out[29]) {
    const int nb = choose_blocks(ctx, n);            // n and the device only
    DevBuf<double> rows, sums;
    HIP_TRY(rows.alloc(32 * (size_t)nb)); HIP_TRY(sums.alloc(32));
    sd.rows = rows.p;
    {
        RoctxRange range(range_name);
        hipLaunchKernelGGL(reduce, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a, sd);
        hipLaunchKernelGGL(fold, dim3(1), dim3(64), 0, ctx->stream, (const double *)rows.p, nb, sums.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sums.p, 29 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// ---- covariance arguments ------------------------------------------------------------------------------------------------
static pcr_status check_cov_mode(int mode, double eps) {
    PCR_REQUIRE(mode == PCR_COV_PLANE || mode == PCR_COV_RAW, "mode must be PCR_COV_PLANE or PCR_COV_RAW");
    PCR_REQUIRE(mode == PCR_COV_RAW || (eps > 0.0 && eps <= 1.0), "eps must be in (0, 1]");
    return PCR_OK;
}
template <typename T>
static pcr_status check_cov_finite(const T *v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!isfinite(v[i])) { pcr_set_error("invalid argument: covariances must be finite"); return PCR_ERR_INVALID; }
    return PCR_OK;
}
