// Generalized ICP (distribution to distribution; Segal, Haehnel, Thrun 2009): per-point covariances and the pass that weighs
// every correspondence with M = (Cq + R Cp R^T)^-1.  Built BESIDE the hot path: its own kernels, its own entry points, no new
// kind in the templated pass kernels (kernels.hip / pass_device.h are included, not edited).
//
//   k_gicp_cov<REG>   sibling of k_knn_normals<REG> (knn_normals.hip): the k nearest neighbours of every point of an indexed
//                     cloud within that cloud (the point itself included), two-pass float64 covariance with divisor =
//                     neighbours found, then PCR_COV_PLANE: C = I - (1 - eps) n n^T with n = smallest_eigvec3(cov) -- the
//                     usual "eigenvalues -> (eps, 1, 1)", which depends on the normal only -- or PCR_COV_RAW: cov itself.
//                     Six floats (xx xy xz yy yz zz) per point, written through pt_orig: the INPUT order of the indexed cloud.
//   k_gicp_reduce     sits where k_rows sits: behind a full search (pass.hip: pcr_rows_search) into a match buffer of the call.
//   k_gicp_fold       The pass over a match list of match_pass.h (match_reduce, match_fold, match_run) with GicpArgs as its
//                     SIDE -- the scan side and the sums are DistSide's (gicp_weight.h), shared with vgicp.hip -- GICP_W points
//                     per lane in flight.  The correspondence is ICP's (xform, the matched PtF, residual_f32<true>), the sums
//                     are acc_ndt's with M6 from icov_closed_form: nothing is restated here.
//   k_gicp_scov_perm  the scan's covariances between caller and device order: ScanPayload<6> (scan_payload.h)
//   k_gicp_robust     the same pass with M replaced by w M, w a robust kernel of d^T M d (RobustSide<GicpArgs>, GICP_ROBUST_W
//                     points per lane in flight), folded by k_gicp_fold
//   k_gicp_residuals  d^T M d of every scan point in the caller's order (match_residuals)
//   k_gicp_keys       the adaptive pass (include/pcr.h): a key per scan point in device order (match_residuals<., true>)
//   k_gicp_adaptive   k_gicp_robust's reduce behind the selection over the keys (select.hip), its kernel read from the
//                     selection's state (AdaptiveSide)
//   GicpUnit          what the seven entry points differ in; the rest of them is match_pass.h's (match_run, match_linearize,
//                     match_align, match_residuals_entry, match_linearize_adaptive, match_align_adaptive)
//
// Target side: ONE 64-byte aligned record per point in cell-sorted order -- xyz, orig, c6, padding (GicpRec) -- so a
// correspondence costs one line, the reason PtN exists.  The record is gathered whole (three 16-byte loads of one line); its
// first 16 bytes are the index's own PtF, so residual_f32<true> sees exactly what gather_point<PCR_ICP> would have handed it.
// det == 0 of Cq + R Cp R^T (e.g. two RAW covariances of single-point neighbourhoods): icov_closed_form's rule applies, the
// adjugate is divided by 1e6 instead -- such a correspondence contributes (almost) nothing instead of Inf / NaN.
#include <math.h>
#include <string.h>

#include "gicp_weight.h"
#include "knn_device.h"
#include "match_pass.h"
#include "scan_payload.h"

extern __shared__ __attribute__((aligned(16))) char gicp_smem[];

// ---- covariances ------------------------------------------------------------------------------------------------------
template <typename LIST>
__device__ __forceinline__ void gicp_cov_finish(const PtF *pts, const PtF me, int mode, double eps, float *cov, LIST &L) {
    double c[6];
    knn_cov6_f64(L, pts, c);
    cov6_finish(mode, eps, c);
    float *dst = cov + 6 * (size_t)pt_orig(me);
#pragma unroll
    for (int a = 0; a < 6; ++a) dst[a] = (float)c[a];
}

// REG = 1: the collect path (k <= 16); 0: the LDS list (knn_self, knn_device.h)
template <int REG>
__global__ void __launch_bounds__(KNN_BLOCK) k_gicp_cov(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n, int k, int mode,
                                                        double eps, float *cov) {
    const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    knn_self<REG>(g, pts, cs, me, k, gicp_smem, [&](auto &L) { gicp_cov_finish(pts, me, mode, eps, cov, L); });
}

// the covariances of the n points behind the index (g, pts, cs), into cov[6 n] in the index's INPUT order
static pcr_status gicp_estimate(pcr_context *ctx, const Geom<float> &g, const PtF *pts, const uint32_t *cs, int64_t n, int k, int mode,
                                double eps, float *cov) {
    if (n <= 0) return PCR_OK;
    knn_launch(k_gicp_cov<1>, k_gicp_cov<0>, k <= KNN_REG_K, n, k, ctx->stream, g, pts, cs, n, k, mode, eps, cov);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

// the GICP gather record of a point target, cell-sorted, one 64-byte line: the index's PtF (xyz + original index), then the
// covariance xx xy xz yy | yz zz, then padding
struct __attribute__((aligned(64))) GicpRec {
    float4 p, c0, c1, pad;
};
static_assert(sizeof(GicpRec) == 64, "one line per correspondence");

// target: caller order (6 floats) <-> cell-sorted records
__global__ void __launch_bounds__(256) k_gicp_tcov_in(const float *__restrict__ in, int64_t n, const PtF *__restrict__ pts, GicpRec *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const PtF p = pts[j];
    const float *c = in + 6 * (size_t)pt_orig(p);
    GicpRec r;
    r.p = p;
    r.c0 = make_float4(c[0], c[1], c[2], c[3]);
    r.c1 = make_float4(c[4], c[5], 0.f, 0.f);
    r.pad = make_float4(0.f, 0.f, 0.f, 0.f);
    out[j] = r;
}
__global__ void __launch_bounds__(256) k_gicp_tcov_out(const GicpRec *__restrict__ in, int64_t n, float *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float4 p = in[j].p, a = in[j].c0, b = in[j].c1;
    float *c = out + 6 * (size_t)pt_orig(p);
    c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y;
}
// scan: caller order <-> device order through pcr_scan::order (scan_payload.h)
template <bool TO_DEVICE>
__global__ void __launch_bounds__(256) k_gicp_scov_perm(const float *__restrict__ in, int64_t n, const uint32_t *__restrict__ order, float *out) {
    payload_perm<6, TO_DEVICE>(in, n, order, out);
}
static const ScanPayload<6> scan_cov{&pcr_scan::cov, k_gicp_scov_perm<true>, k_gicp_scov_perm<false>};
__global__ void __launch_bounds__(256) k_gicp_soa_to_aos(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                         int64_t n, float *xyz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    xyz[3 * i] = x[i]; xyz[3 * i + 1] = y[i]; xyz[3 * i + 2] = z[i];
}

static pcr_status check_cov_args(int k, int mode, double eps) {
    if (k < 1 || k > KNN_MAX_K) { pcr_set_error("k must be in [1, %d]", KNN_MAX_K); return PCR_ERR_INVALID; }
    return check_cov_mode(mode, eps);
}

static pcr_status target_cov_alloc(pcr_target *t) {
    if (!t->gcov) HIP_TRY(pcr_persist_alloc((void **)&t->gcov, sizeof(GicpRec) * (size_t)(t->n ? t->n : 1)));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_estimate_covariances(pcr_target *t, int k, int mode, double eps, float *cov_out_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_REQUIRE(!t->is_voxel, "covariances belong to point targets");
    PCR_TRY(check_cov_args(k, mode, eps));
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    PCR_TRY(target_cov_alloc(t));
    if (t->n == 0) return PCR_OK;
    DevBuf<float> d_cov;                             // caller order
    HIP_TRY(d_cov.alloc(6 * (size_t)t->n));
    PCR_TRY(gicp_estimate(ctx, t->gf, t->pts, t->cell_start, t->n, k, mode, eps, d_cov.p));
    hipLaunchKernelGGL(k_gicp_tcov_in, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const float *)d_cov.p, t->n, t->pts, (GicpRec *)t->gcov);
    HIP_TRY(hipGetLastError());
    if (cov_out_or_null) HIP_TRY(hipMemcpyAsync(cov_out_or_null, d_cov.p, 24 * (size_t)t->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_set_covariances(pcr_target *t, const float *cov6) {
    PCR_REQUIRE(t && (cov6 || t->n == 0), "NULL argument");
    PCR_REQUIRE(!t->is_voxel, "covariances belong to point targets");
    PCR_TRY(check_finite(cov6, 6 * (size_t)t->n, "covariances"));
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    PCR_TRY(target_cov_alloc(t));
    if (t->n == 0) return PCR_OK;
    DevBuf<float> d_cov;
    HIP_TRY(d_cov.alloc(6 * (size_t)t->n));
    HIP_TRY(hipMemcpyAsync(d_cov.p, cov6, 24 * (size_t)t->n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_gicp_tcov_in, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const float *)d_cov.p, t->n, t->pts, (GicpRec *)t->gcov);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_get_covariances(pcr_target *t, float *cov6) {
    PCR_REQUIRE(t && (cov6 || t->n == 0), "NULL argument");
    if (t->is_voxel || !t->gcov) { pcr_set_error("target has no per-point covariances"); return PCR_ERR_NO_TARGET; }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (t->n == 0) return PCR_OK;
    CtxScope scope(ctx);
    DevBuf<float> d_cov;
    HIP_TRY(d_cov.alloc(6 * (size_t)t->n));
    hipLaunchKernelGGL(k_gicp_tcov_out, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const GicpRec *)t->gcov, t->n, d_cov.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(cov6, d_cov.p, 24 * (size_t)t->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

pcr_status pcr_scan_self_index(pcr_scan *s, TmpIndex *idx) {
    pcr_context *ctx = s->ctx;
    DevBuf<float> xyz;
    HIP_TRY(xyz.alloc(3 * (size_t)s->n));
    hipLaunchKernelGGL(k_gicp_soa_to_aos, grid_for(s->n, 256), dim3(256), 0, ctx->stream, (const float *)s->x, (const float *)s->y, (const float *)s->z,
                       s->n, xyz.p);
    HIP_TRY(hipGetLastError());
    idx->t = new pcr_target();
    idx->t->ctx = ctx; idx->t->n = s->n;
    // (no extended lists: the k-NN search reads cell_start and the cell-sorted points only)
    PCR_TRY(pcr_build_point_grid(ctx, xyz.p, s->n, 0.f, idx->t, false, 0.0));
    return PCR_OK;      // (xyz goes back to the context's cache: a later user of the block queues behind the build on the one stream)
}

extern "C" pcr_status pcr_scan_estimate_covariances(pcr_scan *s, int k, int mode, double eps, float *cov_out_or_null) {
    PCR_REQUIRE(s, "NULL argument");
    PCR_TRY(check_cov_args(k, mode, eps));
    PCR_REQUIRE(!cov_out_or_null || pcr_scan_knows_order(s), PCR_NEED_ORDER);
    return scan_cov.estimate(s, cov_out_or_null, [&](const pcr_target *idx, float *dst) {
        return gicp_estimate(s->ctx, idx->gf, idx->pts, idx->cell_start, s->n, k, mode, eps, dst);
    });
}

extern "C" pcr_status pcr_scan_set_covariances(pcr_scan *s, const float *cov6) {
    PCR_REQUIRE(s && (cov6 || s->n == 0), "NULL argument");
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    PCR_TRY(check_finite(cov6, 6 * (size_t)s->n, "covariances"));
    return scan_cov.set(s, cov6);
}

extern "C" pcr_status pcr_scan_get_covariances(pcr_scan *s, float *cov6) {
    PCR_REQUIRE(s && (cov6 || s->n == 0), "NULL argument");
    if (!s->cov) { pcr_set_error("scan has no per-point covariances"); return PCR_ERR_NO_TARGET; }
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    return scan_cov.get(s, cov6);
}

// ---- the pass ---------------------------------------------------------------------------------------------------------
struct GicpArgs : DistSide<GicpArgs> {
    const GicpRec *trec;     // target records, cell-sorted: point + covariance in one line
    double *rows;            // [gridDim.x][32]

    // the match: the record, whole (one line, three 16-byte loads)
    struct Match { float4 p, c0, c1; };
    typedef float Res;
    __device__ __forceinline__ void gather(const LinArgs &, uint32_t j, Match &m) const {
        const GicpRec *r = trec + j;
        m.p = r->p; m.c0 = r->c0; m.c1 = r->c1;
    }
    __device__ __forceinline__ bool residual(const LinArgs &a, const Match &m, float tx, float ty, float tz, float &dx, float &dy, float &dz) const {
        return residual_f32<true>(a, m.p, tx, ty, tz, dx, dy, dz);
    }
    __device__ __forceinline__ void weight(const PoseK &P, const float cp[6], const Match &m, double m6[6]) const {
        const float cq[6] = {m.c0.x, m.c0.y, m.c0.z, m.c0.w, m.c1.x, m.c1.y};
        gicp_weight(P, cp, cq, m6);
    }
};

// points per lane in flight.  3: the per-correspondence arithmetic (R Cp R^T, the closed-form inverse, acc_ndt) needs its
// registers beside 32 float64 sums; see docs/EXPERIMENTS.md for the register figures
#ifndef GICP_W
#define GICP_W 3
#endif

__global__ void __launch_bounds__(256) k_gicp_reduce(const LinArgs a, const GicpArgs ga) { match_reduce<GICP_W>(a, ga); }
__global__ void __launch_bounds__(64) k_gicp_fold(const double *__restrict__ rows, int nb, double *out) { match_fold(rows, nb, out); }

// the pass under a robust weight (include/pcr.h: "robust kernels"): the same three phases, fold and grid; for its registers
// and GICP_ROBUST_W see docs/EXPERIMENTS.md
#ifndef GICP_ROBUST_W
#define GICP_ROBUST_W GICP_W
#endif
__global__ void __launch_bounds__(256) k_gicp_robust(const LinArgs a, const RobustSide<GicpArgs> ga) { match_reduce<GICP_ROBUST_W>(a, ga); }
// d^T M d of every scan point in the caller's order, +inf where there is no correspondence
__global__ void __launch_bounds__(256) k_gicp_residuals(const LinArgs a, const GicpArgs ga, const uint32_t *order, double *out) {
    match_residuals(a, ga, order, out);
}
// the adaptive pass (include/pcr.h: "adaptive pass"): a key per scan point in device order, +inf where there is no
// correspondence; behind the selection over the keys (select.hip), k_gicp_robust's reduce with its kernel read from the
// selection's state (AdaptiveSide), folded by k_gicp_fold
__global__ void __launch_bounds__(256) k_gicp_keys(const LinArgs a, const GicpArgs ga, double *out) {
    match_residuals<GicpArgs, true>(a, ga, nullptr, out);
}
__global__ void __launch_bounds__(256) k_gicp_adaptive(const LinArgs a, const AdaptiveSide<GicpArgs> ga) {
    match_reduce<GICP_ROBUST_W>(a, adaptive_side(ga));
}

// ---- the entry points: a UNIT of match_pass.h -------------------------------------------------------------------------
// The search is ICP's; a call has no parameter of the unit's own
struct GicpUnit : MatchUnit {
    typedef GicpArgs Side;
    static constexpr int kind = PCR_ICP;
    static pcr_status payloads(const pcr_target *t, const pcr_scan *s) {
        if (t->is_voxel || !t->gcov) { pcr_set_error("GICP target has no covariances (pcr_target_estimate_covariances / _set_covariances)"); return PCR_ERR_NO_TARGET; }
        if (!s->cov) { pcr_set_error("GICP scan has no covariances (pcr_scan_estimate_covariances / _set_covariances)"); return PCR_ERR_NO_TARGET; }
        return PCR_OK;
    }
    static Side side(const pcr_target *t, const pcr_scan *s, const Params &) { return {{s->cov}, (const GicpRec *)t->gcov, nullptr}; }
    static constexpr auto reduce = k_gicp_reduce;
    static constexpr auto robust = k_gicp_robust;
    static constexpr auto fold = k_gicp_fold;
    static constexpr auto residuals = k_gicp_residuals;
    static constexpr auto keys = k_gicp_keys;
    static constexpr auto adaptive = k_gicp_adaptive;
    static constexpr const char *reduce_range = "pcr:gicp_reduce", *robust_range = "pcr:gicp_robust", *residuals_range = "pcr:gicp_residuals",
                                *adaptive_range = "pcr:gicp_adaptive";
};

extern "C" pcr_status pcr_gicp_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double out[29]) {
    return match_linearize<GicpUnit>(t, s, T, max_dist, nullptr, flags, out);
}
extern "C" pcr_status pcr_gicp_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                     unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    return match_align<GicpUnit>(t, s, T_init, max_iter, tol, max_dist, nullptr, flags, T_out, iterations, trace_or_null);
}
extern "C" pcr_status pcr_gicp_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_robust *rb,
                                                unsigned flags, double out[29]) {
    return match_linearize<GicpUnit>(t, s, T, max_dist, rb, flags, out);
}
extern "C" pcr_status pcr_gicp_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                            const pcr_robust *rb, unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    return match_align<GicpUnit>(t, s, T_init, max_iter, tol, max_dist, rb, flags, T_out, iterations, trace_or_null);
}
extern "C" pcr_status pcr_gicp_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double *s_out) {
    return match_residuals_entry<GicpUnit>(t, s, T, max_dist, flags, s_out);
}
extern "C" pcr_status pcr_gicp_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_adaptive *ad,
                                                 unsigned flags, double out[29], double stats[4]) {
    return match_linearize_adaptive<GicpUnit>(t, s, T, max_dist, ad, flags, out, stats);
}
extern "C" pcr_status pcr_gicp_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations,
                                             double *trace_or_null, double *stats_or_null) {
    return match_align_adaptive<GicpUnit>(t, s, T_init, max_iter, tol, max_dist, ad, flags, T_out, iterations, trace_or_null, stats_or_null);
}
