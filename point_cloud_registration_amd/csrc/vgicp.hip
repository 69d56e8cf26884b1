// Voxelized GICP (distribution to voxel; Koide, Yokozuka, Oishi, Banno: "Voxelized GICP", ICRA 2021) on the voxel targets:
// every correspondence -- found and gated exactly as NDT / VPlaneICP find and gate it -- is weighed with
// M = (Cv + R Cp R^T)^-1, Cv the float64 covariance of the matched voxel, Cp the float32 covariance of the scan point (GICP's:
// gicp.hip puts them on a scan).  Built BESIDE the hot path like gicp.hip: its own kernels and entry points, no new kind in the
// templated pass kernels (pass_device.h / gicp_weight.h are included; kernels.hip, rows.hip, gicp.hip, seam64.hip do not change).
//
//   k_vgicp_plane_cov  one thread per kept voxel, key order: C = I - (1 - eps) n n^T from the voxel's normal (st_norm), float64,
//                      six values xx xy xz yy yz zz.  Eigenvalues (eps, 1, 1); the sign of n cancels.
//   k_vgicp_cov_out    cell-sorted rows back into key order (the inverse of pcr_permute_rows_f64), for the read-back.
//   k_vgicp_reduce     sits where k_gicp_reduce sits: behind a full float64 centroid search (pass.hip: pcr_rows_search with
//                      PCR_VPLANE, which needs the voxel normals only) into a match buffer of the call.  VGICP_W points per lane
//                      in flight: index, coordinates and scan covariance of all of them (phase A), then the matched centroids
//                      (32 bytes of `means`) and voxel covariances (48 bytes of `vcov`) with no branch between the gathers
//                      (phase B), then residual_f64<true> on the loaded centroid, gicp_weight, acc_ndt in index order
//                      (phase C): nothing is restated here.  One row of 32 doubles per block with plain stores
//                      (block_store_partials<false>).  No tickets, no atomics.
//   k_vgicp_fold       one block: thread e < 29 adds rows 0 .. nb-1 in order.  The grid depends on n and the device only, so
//                      two calls return the same bits.
//
// Target side: pcr_target::vcov, [n][6] float64 in the cell-sorted order of `means`, produced from key-order rows by
// pcr_permute_rows_f64 exactly as vicov is.  Centroid and covariance stay two arrays (80 bytes per correspondence in two
// lines); a single padded 128-byte record per voxel was not built (docs/EXPERIMENTS.md).
#include <math.h>
#include <string.h>

#include "gicp_weight.h"

// ---- voxel covariances --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_vgicp_plane_cov(const double *__restrict__ norm, int64_t n, double eps, double *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double n0 = norm[3 * i], n1 = norm[3 * i + 1], n2 = norm[3 * i + 2];
    const double s = 1.0 - eps;
    double *c = out + 6 * (size_t)i;
    c[0] = 1.0 - s * n0 * n0; c[1] = -(s * n0 * n1); c[2] = -(s * n0 * n2);
    c[3] = 1.0 - s * n1 * n1; c[4] = -(s * n1 * n2); c[5] = 1.0 - s * n2 * n2;
}

__global__ void __launch_bounds__(256) k_vgicp_cov_out(const double *__restrict__ vcov, int64_t n, const PtD *__restrict__ means, double *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t i = (size_t)__double_as_longlong(means[j].w);      // key-order index of the voxel at cell-sorted position j
#pragma unroll
    for (int k = 0; k < 6; ++k) out[6 * i + k] = vcov[6 * (size_t)j + k];
}

static dim3 grid256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

extern "C" pcr_status pcr_target_voxels_set_covariances(pcr_target *t, int mode, double eps, const double *cov6_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    if (!t->is_voxel) { pcr_set_error("voxel covariances belong to voxel targets"); return PCR_ERR_NO_TARGET; }
    const int cols6[6] = {0, 1, 2, 3, 4, 5}, cols9[6] = {0, 1, 2, 4, 5, 8};
    if (!cov6_or_null) {
        PCR_REQUIRE(mode == PCR_COV_PLANE || mode == PCR_COV_RAW, "mode must be PCR_COV_PLANE or PCR_COV_RAW");
        PCR_REQUIRE(mode == PCR_COV_RAW || (eps > 0.0 && eps <= 1.0), "eps must be in (0, 1]");
        if (mode == PCR_COV_PLANE && !t->st_norm) { pcr_set_error("voxel target does not hold 'norm'"); return PCR_ERR_NO_TARGET; }
        if (mode == PCR_COV_RAW && !t->st_cov) { pcr_set_error("voxel target does not hold 'cov'"); return PCR_ERR_NO_TARGET; }
    } else {
        // (checked before anything of the target changes: a refused set leaves the old covariances)
        for (size_t i = 0; i < 6 * (size_t)t->n; ++i)
            if (!isfinite(cov6_or_null[i])) { pcr_set_error("invalid argument: covariances must be finite"); return PCR_ERR_INVALID; }
    }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t rows = (size_t)(t->n ? t->n : 1);
    if (!t->vcov) {
        HIP_TRY(pcr_persist_alloc((void **)&t->vcov, sizeof(double) * 6 * rows));
        HIP_TRY(hipMemsetAsync(t->vcov, 0, sizeof(double) * 6 * rows, ctx->stream));
    }
    if (t->n > 0) {
        if (cov6_or_null) {
            DevBuf<double> key;
            HIP_TRY(key.alloc(6 * rows));
            HIP_TRY(hipMemcpyAsync(key.p, cov6_or_null, sizeof(double) * 6 * (size_t)t->n, hipMemcpyHostToDevice, ctx->stream));
            PCR_TRY(pcr_permute_rows_f64(ctx, key.p, t->n, 6, cols6, 6, t->means, t->vcov));
            HIP_TRY(hipStreamSynchronize(ctx->stream));      // (the host array is being read until here)
            return PCR_OK;
        }
        if (mode == PCR_COV_RAW) {
            PCR_TRY(pcr_permute_rows_f64(ctx, t->st_cov, t->n, 9, cols9, 6, t->means, t->vcov));
        } else {
            DevBuf<double> key;
            HIP_TRY(key.alloc(6 * rows));
            hipLaunchKernelGGL(k_vgicp_plane_cov, grid256(t->n), dim3(256), 0, ctx->stream, (const double *)t->st_norm, t->n, eps, key.p);
            HIP_TRY(hipGetLastError());
            PCR_TRY(pcr_permute_rows_f64(ctx, key.p, t->n, 6, cols6, 6, t->means, t->vcov));
        }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_voxels_get_covariances(pcr_target *t, double *cov6) {
    PCR_REQUIRE(t && (cov6 || t->n == 0), "NULL argument");
    if (!t->is_voxel || !t->vcov) { pcr_set_error("target has no per-voxel covariances (pcr_target_voxels_set_covariances)"); return PCR_ERR_NO_TARGET; }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (t->n == 0) return PCR_OK;
    CtxScope scope(ctx);
    DevBuf<double> key;
    HIP_TRY(key.alloc(6 * (size_t)t->n));
    hipLaunchKernelGGL(k_vgicp_cov_out, grid256(t->n), dim3(256), 0, ctx->stream, (const double *)t->vcov, t->n, (const PtD *)t->means, key.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cov6, key.p, sizeof(double) * 6 * (size_t)t->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// ---- the pass ---------------------------------------------------------------------------------------------------------
struct VgicpArgs {
    const float *scov;       // scan covariances, device order, 6 floats per point
    const double *vcov;      // voxel covariances, cell-sorted, 6 doubles per voxel (16-byte aligned rows)
    double *rows;            // [gridDim.x][32]
};

// points per lane in flight.  2: a point carries a float64 centroid (8 registers) and a float64 Cv (12) through phase B where
// k_gicp_reduce carries 10 of float32; see docs/EXPERIMENTS.md for the register figures
#ifndef VGICP_W
#define VGICP_W 2
#endif

__global__ void __launch_bounds__(256) k_vgicp_reduce(const LinArgs a, const VgicpArgs va) {
    const PoseK &P = a.hp;                           // host-driven: the pose came by value
    constexpr int W = VGICP_W;
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x; t0 < a.n; t0 += W * stride) {
        uint32_t j[W];
        float x[W], y[W], z[W];
        float2 cp[W][3];
        double2 m0[W], m1[W], cv[W][3];
        bool use[W];
        // phase A: index, coordinates and covariance of all W points (a point past the end reads the lane's first point)
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const int64_t t = t0 + u * stride;
            use[u] = t < a.n;
            const int64_t i = use[u] ? t : t0;
            j[u] = a.nn_j[i];
            x[u] = a.sx[i]; y[u] = a.sy[i]; z[u] = a.sz[i];
            const float2 *c = reinterpret_cast<const float2 *>(va.scov + 6 * i);
            cp[u][0] = c[0]; cp[u][1] = c[1]; cp[u][2] = c[2];
        }
        reduce_phase();
#pragma unroll
        for (int u = 0; u < W; ++u) reduce_pin(j[u]);
        // phase B: the matched centroids and voxel covariances (no match: voxel 0 through a select on the index -- always
        // there -- and skipped in phase C; no branch between the gathers)
#pragma unroll
        for (int u = 0; u < W; ++u) {
            use[u] = use[u] && j[u] != PCR_NONE;
            const size_t jj = use[u] ? j[u] : 0u;
            const double2 *mp = reinterpret_cast<const double2 *>(a.means + jj);
            const double2 *cq = reinterpret_cast<const double2 *>(va.vcov + 6 * jj);
            m0[u] = mp[0]; m1[u] = mp[1];
            cv[u][0] = cq[0]; cv[u][1] = cq[1]; cv[u][2] = cq[2];
        }
        reduce_phase();
        // phase C: residual, gate, weight, sums -- in index order
#pragma unroll
        for (int u = 0; u < W; ++u) {
            if (!use[u]) continue;
            float tx, ty, tz;
            double dx, dy, dz;
            xform(P, x[u], y[u], z[u], tx, ty, tz);
            const PtD m = make_double4(m0[u].x, m0[u].y, m1[u].x, m1[u].y);
            if (!residual_f64<true>(a, m, tx, ty, tz, dx, dy, dz)) continue;
            const float cpv[6] = {cp[u][0].x, cp[u][0].y, cp[u][1].x, cp[u][1].y, cp[u][2].x, cp[u][2].y};
            const double cvv[6] = {cv[u][0].x, cv[u][0].y, cv[u][1].x, cv[u][1].y, cv[u][2].x, cv[u][2].y};
            double m6[6];
            gicp_weight(P, cpv, cvv, m6);
            acc_ndt(acc, P, (double)x[u], (double)y[u], (double)z[u], m6, dx, dy, dz);
        }
    }
    block_store_partials<false>(acc, va.rows);
}

__global__ void __launch_bounds__(64) k_vgicp_fold(const double *__restrict__ rows, int nb, double *out) {
    const int e = threadIdx.x;
    if (e >= 29) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += rows[(size_t)b * 32 + e];
    out[e] = s;
}

// search + reduce + fold + 29 doubles back: one stream synchronisation, device blocks from the context's block cache
pcr_status pcr_run_vgicp(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double out[29]) {
    if (!t->is_voxel) { pcr_set_error("VGICP needs a voxel target"); return PCR_ERR_NO_TARGET; }
    if (!t->vcov) { pcr_set_error("VGICP target has no covariances (pcr_target_voxels_set_covariances)"); return PCR_ERR_NO_TARGET; }
    if (!s->cov) { pcr_set_error("VGICP scan has no covariances (pcr_scan_estimate_covariances / _set_covariances)"); return PCR_ERR_NO_TARGET; }
    pcr_context *ctx = t->ctx;
    for (int i = 0; i < 29; ++i) out[i] = 0.0;
    if (t->n == 0) {                                 // no kept voxel: no match (and no voxel 0 for the select of phase B)
        PCR_REQUIRE(s->ctx == ctx, "scan and target belong to different contexts");
        PCR_REQUIRE(max_dist > 0, "max_dist must be positive");
        if (ctx->comm != nullptr) { pcr_set_error("VGICP passes are not available on a context with a communicator attached"); return PCR_ERR_UNSUPPORTED; }
        return PCR_OK;
    }
    LinArgs a;
    DevBuf<uint32_t> nn;
    PCR_TRY(pcr_rows_search(&a, &nn, t, s, PCR_VPLANE, T, max_dist, flags, false));
    if (s->n == 0) return PCR_OK;
    const int nb = choose_blocks(ctx, s->n);         // n and the device only
    DevBuf<double> rows, sums;
    HIP_TRY(rows.alloc(32 * (size_t)nb)); HIP_TRY(sums.alloc(32));
    VgicpArgs va;
    va.scov = s->cov; va.vcov = t->vcov; va.rows = rows.p;
    {
        RoctxRange range("pcr:vgicp_reduce");
        hipLaunchKernelGGL(k_vgicp_reduce, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a, va);
        hipLaunchKernelGGL(k_vgicp_fold, dim3(1), dim3(64), 0, ctx->stream, (const double *)rows.p, nb, sums.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sums.p, 29 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_vgicp_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double out[29]) {
    PCR_REQUIRE(t && s && T && out, "NULL argument");
    CtxScope scope(t->ctx);
    return pcr_run_vgicp(t, s, T, max_dist, flags, out);
}

// the host-driven Gauss-Newton loop of pcr_align (api.hip: pcr_align_host_loop) over pcr_run_vgicp: same gn_step, same trace rows
static pcr_status vgicp_pass(pcr_target *t, pcr_scan *s, int, const double T[16], double max_dist, unsigned flags, double out[29]) {
    return pcr_run_vgicp(t, s, T, max_dist, flags, out);
}
extern "C" pcr_status pcr_vgicp_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                      unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    PCR_REQUIRE(t && s && T_init && T_out, "NULL argument");
    CtxScope scope(t->ctx);
    return pcr_align_host_loop(vgicp_pass, t, s, PCR_VPLANE, T_init, max_iter, tol, max_dist, flags, T_out, iterations, trace_or_null);
}
