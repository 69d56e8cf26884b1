// Voxelized GICP (distribution to voxel; Koide, Yokozuka, Oishi, Banno: "Voxelized GICP", ICRA 2021) on the voxel targets:
// every correspondence -- found and gated exactly as NDT / VPlaneICP find and gate it -- is weighed with
// M = (Cv + R Cp R^T)^-1, Cv the float64 covariance of the matched voxel, Cp the float32 covariance of the scan point (GICP's:
// gicp.hip puts them on a scan).  Built BESIDE the hot path like gicp.hip: its own kernels and entry points, no new kind in the
// templated pass kernels (pass_device.h / match_pass.h are included; kernels.hip, rows.hip, gicp.hip, seam64.hip do not change).
//
//   k_vgicp_plane_cov  one thread per kept voxel, key order: C = I - (1 - eps) n n^T from the voxel's normal (st_norm), float64,
//                      six values xx xy xz yy yz zz.  Eigenvalues (eps, 1, 1); the sign of n cancels.
//   k_vgicp_cov_out    cell-sorted rows back into key order (the inverse of pcr_permute_rows_f64), for the read-back.
//   k_vgicp_reduce     sits where k_gicp_reduce sits: behind a full float64 centroid search (pass.hip: pcr_rows_search with
//   k_vgicp_fold       PCR_VPLANE, which needs the voxel normals only) into a match buffer of the call.  The pass over a match
//                      list of match_pass.h (match_reduce, match_fold, match_run) with VgicpArgs as its SIDE -- the scan side
//                      and the sums are DistSide's (gicp_weight.h), shared with gicp.hip -- VGICP_W points per lane in flight:
//                      residual_f64<true> on the gathered centroid, gicp_weight, acc_ndt -- nothing is restated here.
//   k_vgicp_robust     the same pass with M replaced by w M, w a robust kernel of d^T M d (RobustSide<VgicpArgs>,
//   k_vgicp_residuals  VGICP_ROBUST_W points per lane in flight), folded by k_vgicp_fold; d^T M d of every scan point in the
//                      caller's order (match_residuals)
//   k_vgicp_keys       the adaptive pass (include/pcr.h): a key per scan point in device order (match_residuals<., true>)
//   k_vgicp_adaptive   k_vgicp_robust's reduce behind the selection over the keys (select.hip), its kernel read from the
//                      selection's state (AdaptiveSide)
//   VgicpUnit          (vgicp_side.h) what the seven entry points differ in -- the target with no kept voxel among it; the
//                      rest of them is match_pass.h's (match_run, match_linearize, match_align, match_residuals_entry,
//                      match_linearize_adaptive, match_align_adaptive).  vgicp_direct.hip derives its unit from it and
//                      folds with k_vgicp_fold
//
// Target side: pcr_target::vcov, [n][6] float64 in the cell-sorted order of `means`, produced from key-order rows by
// pcr_permute_rows_f64 exactly as vicov is.  Centroid and covariance stay two arrays (80 bytes per correspondence in two
// lines); a single padded 128-byte record per voxel was not built (docs/EXPERIMENTS.md).
#include <math.h>
#include <string.h>

#include "vgicp_side.h"

// ---- voxel covariances --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_vgicp_plane_cov(const double *__restrict__ norm, int64_t n, double eps, double *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double nv[3] = {norm[3 * i], norm[3 * i + 1], norm[3 * i + 2]};
    plane_cov6(nv, eps, out + 6 * (size_t)i);
}

__global__ void __launch_bounds__(256) k_vgicp_cov_out(const double *__restrict__ vcov, int64_t n, const PtD *__restrict__ means, double *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t i = key_index(means[j]);            // of the voxel at cell-sorted position j
#pragma unroll
    for (int k = 0; k < 6; ++k) out[6 * i + k] = vcov[6 * (size_t)j + k];
}

extern "C" pcr_status pcr_target_voxels_set_covariances(pcr_target *t, int mode, double eps, const double *cov6_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    if (!t->is_voxel) { pcr_set_error("voxel covariances belong to voxel targets"); return PCR_ERR_NO_TARGET; }
    const int cols6[6] = {0, 1, 2, 3, 4, 5}, cols9[6] = {0, 1, 2, 4, 5, 8};
    if (!cov6_or_null) {
        PCR_TRY(check_cov_mode(mode, eps));
        if (mode == PCR_COV_PLANE && !t->st_norm) { pcr_set_error("voxel target does not hold 'norm'"); return PCR_ERR_NO_TARGET; }
        if (mode == PCR_COV_RAW && !t->st_cov) { pcr_set_error("voxel target does not hold 'cov'"); return PCR_ERR_NO_TARGET; }
    } else {
        // (checked before anything of the target changes: a refused set leaves the old covariances)
        PCR_TRY(check_finite(cov6_or_null, 6 * (size_t)t->n, "covariances"));
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
            hipLaunchKernelGGL(k_vgicp_plane_cov, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const double *)t->st_norm, t->n, eps, key.p);
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
    hipLaunchKernelGGL(k_vgicp_cov_out, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const double *)t->vcov, t->n, (const PtD *)t->means, key.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cov6, key.p, sizeof(double) * 6 * (size_t)t->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// ---- the pass ---------------------------------------------------------------------------------------------------------
// VgicpArgs, the SIDE: vgicp_side.h (shared with vgicp_direct.hip)

// points per lane in flight.  2: a point carries a float64 centroid (8 registers) and a float64 Cv (12) through phase B where
// k_gicp_reduce carries 10 of float32; see docs/EXPERIMENTS.md for the register figures
#ifndef VGICP_W
#define VGICP_W 2
#endif

__global__ void __launch_bounds__(256) k_vgicp_reduce(const LinArgs a, const VgicpArgs va) { match_reduce<VGICP_W>(a, va); }
__global__ void __launch_bounds__(64) k_vgicp_fold(const double *__restrict__ rows, int nb, double *out) { match_fold(rows, nb, out); }

// the pass under a robust weight (include/pcr.h: "robust kernels"): the same three phases, fold and grid; for its registers
// and VGICP_ROBUST_W see docs/EXPERIMENTS.md
#ifndef VGICP_ROBUST_W
#define VGICP_ROBUST_W VGICP_W
#endif
__global__ void __launch_bounds__(256) k_vgicp_robust(const LinArgs a, const RobustSide<VgicpArgs> va) { match_reduce<VGICP_ROBUST_W>(a, va); }
// d^T M d of every scan point in the caller's order, +inf where there is no correspondence
__global__ void __launch_bounds__(256) k_vgicp_residuals(const LinArgs a, const VgicpArgs va, const uint32_t *order, double *out) {
    match_residuals(a, va, order, out);
}
// the adaptive pass (include/pcr.h: "adaptive pass"): a key per scan point in device order, +inf where there is no
// correspondence; behind the selection over the keys (select.hip), k_vgicp_robust's reduce with its kernel read from the
// selection's state (AdaptiveSide), folded by k_vgicp_fold
__global__ void __launch_bounds__(256) k_vgicp_keys(const LinArgs a, const VgicpArgs va, double *out) {
    match_residuals<VgicpArgs, true>(a, va, nullptr, out);
}
__global__ void __launch_bounds__(256) k_vgicp_adaptive(const LinArgs a, const AdaptiveSide<VgicpArgs> va) {
    match_reduce<VGICP_ROBUST_W>(a, adaptive_side(va));
}

// ---- the entry points: VgicpUnit (vgicp_side.h), a UNIT of match_pass.h ------------------------------------------------
extern "C" pcr_status pcr_vgicp_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double out[29]) {
    return match_linearize<VgicpUnit>(t, s, T, max_dist, nullptr, flags, out);
}
extern "C" pcr_status pcr_vgicp_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                      unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    return match_align<VgicpUnit>(t, s, T_init, max_iter, tol, max_dist, nullptr, flags, T_out, iterations, trace_or_null);
}
extern "C" pcr_status pcr_vgicp_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_robust *rb,
                                                 unsigned flags, double out[29]) {
    return match_linearize<VgicpUnit>(t, s, T, max_dist, rb, flags, out);
}
extern "C" pcr_status pcr_vgicp_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             const pcr_robust *rb, unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    return match_align<VgicpUnit>(t, s, T_init, max_iter, tol, max_dist, rb, flags, T_out, iterations, trace_or_null);
}
extern "C" pcr_status pcr_vgicp_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double *s_out) {
    return match_residuals_entry<VgicpUnit>(t, s, T, max_dist, flags, s_out);
}
extern "C" pcr_status pcr_vgicp_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_adaptive *ad,
                                                 unsigned flags, double out[29], double stats[4]) {
    return match_linearize_adaptive<VgicpUnit>(t, s, T, max_dist, ad, flags, out, stats);
}
extern "C" pcr_status pcr_vgicp_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations,
                                             double *trace_or_null, double *stats_or_null) {
    return match_align_adaptive<VgicpUnit>(t, s, T_init, max_iter, tol, max_dist, ad, flags, T_out, iterations, trace_or_null, stats_or_null);
}
