// Symmetric point-to-plane ICP (Rusinkiewicz: "A Symmetric Objective Function for ICP", SIGGRAPH 2019; the fixed-normal-sum
// form PCL offers): PlaneICP's row with the mean of BOTH clouds' normals in the place of the target's.  Built BESIDE the hot
// path like gicp.hip: its own kernels and entry points, no new kind in the templated pass kernels (pass_device.h / match_pass.h
// are included; kernels.hip, rows.hip, gicp.hip, vgicp.hip keep their device code).  The definition is in include/pcr.h.
//
//   k_symm_normals<REG>  sibling of k_gicp_cov<REG>: the k nearest neighbours of every point of an indexed cloud within that cloud
//                        (knn_self), two-pass float64 covariance (knn_cov6_f64), smallest_eigvec3 -- what
//                        pcr_target_estimate_normals(compat = 0) computes -- three floats per point, written through pt_orig: the
//                        INPUT order of the indexed cloud, which for a scan's temporary self-index is its device order.
//   k_symm_perm<TO_DEV>  caller order <-> device order through pcr_scan::order: ScanPayload<3> (scan_payload.h)
//   k_symm_reduce        sits where k_gicp_reduce sits: behind a full search (pass.hip: pcr_rows_search, ICP's) into a match
//   k_symm_fold          buffer of the call.  The pass over a match list of match_pass.h (match_reduce, match_fold, match_run)
//                        with SymmArgs as its SIDE, SYMM_W points per lane in flight.
//   k_symm_robust        the same pass with every correspondence weighed by a robust kernel of r r (RobustSide<SymmArgs>,
//                        SYMM_ROBUST_W points per lane in flight), folded by k_symm_fold
//   k_symm_residuals     r r of every scan point in the caller's order (match_residuals)
//   k_symm_keys          the adaptive pass (include/pcr.h): a key per scan point in device order (match_residuals<., true>)
//   k_symm_adaptive      k_symm_robust's reduce behind the selection over the keys (select.hip), its kernel read from the
//                        selection's state (AdaptiveSide)
//   SymmUnit             what the seven entry points differ in; the rest of them is match_pass.h's (match_run, match_linearize,
//                        match_align, match_residuals_entry, match_linearize_adaptive, match_align_adaptive)
//
// Scan side: pcr_scan::nrm, three floats per point in device order (12 bytes beside the 16 of index and coordinates).  Target
// side: the PtN records PlaneICP gathers -- point and normal in one 32-byte sector.
#include <math.h>
#include <string.h>

#include "eigen3.h"
#include "knn_device.h"
#include "match_pass.h"
#include "scan_payload.h"

extern __shared__ __attribute__((aligned(16))) char symm_smem[];

// ---- normals on a scan ------------------------------------------------------------------------------------------------
// A neighbourhood of one point (a one-point cloud, k = 1) has the zero covariance: smallest_eigvec3 then returns (1, 0, 0),
// the first column of the identity it starts from -- a unit vector, never zero or NaN.
template <typename LIST>
__device__ __forceinline__ void symm_normal_finish(const PtF *pts, const PtF me, float *nrm, LIST &L) {
    double c[6], n[3];
    knn_cov6_f64(L, pts, c);
    smallest_eigvec3(c, n);
    float *dst = nrm + 3 * (size_t)pt_orig(me);
    dst[0] = (float)n[0]; dst[1] = (float)n[1]; dst[2] = (float)n[2];
}

// REG = 1: the collect path (k <= 16); 0: the LDS list (knn_self, knn_device.h)
template <int REG>
__global__ void __launch_bounds__(KNN_BLOCK) k_symm_normals(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n, int k, float *nrm) {
    const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    knn_self<REG>(g, pts, cs, me, k, symm_smem, [&](auto &L) { symm_normal_finish(pts, me, nrm, L); });
}

// caller order <-> device order through pcr_scan::order (scan_payload.h)
template <bool TO_DEVICE>
__global__ void __launch_bounds__(256) k_symm_perm(const float *__restrict__ in, int64_t n, const uint32_t *__restrict__ order, float *out) {
    payload_perm<3, TO_DEVICE>(in, n, order, out);
}
static const ScanPayload<3> scan_nrm{&pcr_scan::nrm, k_symm_perm<true>, k_symm_perm<false>};

extern "C" pcr_status pcr_scan_estimate_normals(pcr_scan *s, int k, float *normals_out_or_null) {
    PCR_REQUIRE(s, "NULL argument");
    if (k < 1 || k > KNN_MAX_K) { pcr_set_error("k must be in [1, %d]", KNN_MAX_K); return PCR_ERR_INVALID; }
    PCR_REQUIRE(!normals_out_or_null || pcr_scan_knows_order(s), PCR_NEED_ORDER);
    return scan_nrm.estimate(s, normals_out_or_null, [&](const pcr_target *idx, float *dst) -> pcr_status {
        knn_launch(k_symm_normals<1>, k_symm_normals<0>, k <= KNN_REG_K, s->n, k, s->ctx->stream, idx->gf, (const PtF *)idx->pts,
                   (const uint32_t *)idx->cell_start, s->n, k, dst);
        HIP_TRY(hipGetLastError());
        return PCR_OK;
    });
}

extern "C" pcr_status pcr_scan_set_normals(pcr_scan *s, const float *normals) {
    PCR_REQUIRE(s && (normals || s->n == 0), "NULL argument");
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    // (checked before anything of the scan changes: a refused set leaves the old normals)
    PCR_TRY(check_finite(normals, 3 * (size_t)s->n, "normals"));
    return scan_nrm.set(s, normals);
}

extern "C" pcr_status pcr_scan_get_normals(pcr_scan *s, float *normals) {
    PCR_REQUIRE(s && (normals || s->n == 0), "NULL argument");
    if (!s->nrm) { pcr_set_error("scan has no per-point normals"); return PCR_ERR_NO_TARGET; }
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    return scan_nrm.get(s, normals);
}

// ---- the pass ---------------------------------------------------------------------------------------------------------
// A SIDE of match_pass.h.  Phase A carries the three normal floats of a scan point, phase B the PtN record of the match (two
// 16-byte loads of one sector); each is the arithmetic of include/pcr.h up to the row (J, r), add its plain accumulation
struct SymmArgs {
    const float *snrm;       // scan normals, device order, 3 floats per point
    double min_cos;          // normal gate: kept iff |n_q . R n_p| >= min_cos
    double *rows;            // [gridDim.x][32]

    struct Scan { float nx, ny, nz; };
    struct Match { float4 q, nq; };
    __device__ __forceinline__ void load(int64_t i, Scan &s) const {
        const float *np = snrm + 3 * i;
        s.nx = np[0]; s.ny = np[1]; s.nz = np[2];
    }
    __device__ __forceinline__ void gather(const LinArgs &a, uint32_t j, Match &m) const {
        const float4 *rec = reinterpret_cast<const float4 *>(a.pn + j);
        m.q = rec[0]; m.nq = rec[1];
    }
    typedef RowsPlain Plain;
    typedef RowsWeighted Weighted;
    typedef RowsResid Resid;
    static constexpr int M = 1;
    // the ONE statement of a correspondence: both gates, then f on its row
    template <typename F>
    __device__ __forceinline__ void each(const LinArgs &a, const PoseK &P, float x, float y, float z, float tx, float ty, float tz,
                                         const Scan &s, const Match &m, const F &f) const {
        float dx, dy, dz;
        if (!residual_f32<true>(a, m.q, tx, ty, tz, dx, dy, dz)) return;
        const double px = s.nx, py = s.ny, pz = s.nz;
        const double v0 = (P.R[0] * px + P.R[1] * py) + P.R[2] * pz;
        const double v1 = (P.R[3] * px + P.R[4] * py) + P.R[5] * pz;
        const double v2 = (P.R[6] * px + P.R[7] * py) + P.R[8] * pz;
        const double q0 = m.nq.x, q1 = m.nq.y, q2 = m.nq.z;
        const double c = (q0 * v0 + q1 * v1) + q2 * v2;
        if (!(fabs(c) >= min_cos)) return;                           // (a NaN c is skipped)
        const double sg = c < 0.0 ? -1.0 : 1.0;
        const double m0 = 0.5 * (q0 + sg * v0), m1 = 0.5 * (q1 + sg * v1), m2 = 0.5 * (q2 + sg * v2);
        double J[6];
        const double r = plane_row(P, (double)x, (double)y, (double)z, m0, m1, m2, (double)dx, (double)dy, (double)dz, J);
        f(0, J, r);
    }
    __device__ __forceinline__ void add(double *acc, const LinArgs &a, const PoseK &P, float x, float y, float z, float tx, float ty, float tz,
                                        const Scan &s, const Match &m) const {
        each(a, P, x, y, z, tx, ty, tz, s, m, Plain(acc, P, x, y, z));
    }
};

// points per lane in flight.  A point carries 7 registers through phase A and 8 more through phase B.  3: 122 registers, four
// waves per SIMD; 4 needs 136 and drops to three waves for the same twelve points in flight (docs/EXPERIMENTS.md)
#ifndef SYMM_W
#define SYMM_W 3
#endif

__global__ void __launch_bounds__(256) k_symm_reduce(const LinArgs a, const SymmArgs sa) { match_reduce<SYMM_W>(a, sa); }
__global__ void __launch_bounds__(64) k_symm_fold(const double *__restrict__ rows, int nb, double *out) { match_fold(rows, nb, out); }

// the pass under a robust weight (include/pcr.h: "robust kernels"): the same three phases, fold and grid.  The weight (a
// float64 divide and square root, w J beside J) does not fit beside the 32 sums within the 128 registers of four waves per
// SIMD at any width -- forced there it spills -- so the kernel runs at three waves, where k_gicp_reduce runs: 2 points in
// flight need 162 registers, 3 need 174 and would drop to two waves (docs/EXPERIMENTS.md)
#ifndef SYMM_ROBUST_W
#define SYMM_ROBUST_W 2
#endif
__global__ void __launch_bounds__(256) k_symm_robust(const LinArgs a, const RobustSide<SymmArgs> sa) { match_reduce<SYMM_ROBUST_W>(a, sa); }
// r * r of every scan point in the caller's order, +inf where there is no correspondence
__global__ void __launch_bounds__(256) k_symm_residuals(const LinArgs a, const SymmArgs sa, const uint32_t *order, double *out) {
    match_residuals(a, sa, order, out);
}
// the adaptive pass (include/pcr.h: "adaptive pass"): a key per scan point in device order, +inf where there is no
// correspondence; behind the selection over the keys (select.hip), k_symm_robust's reduce with its kernel read from the
// selection's state (AdaptiveSide), folded by k_symm_fold
__global__ void __launch_bounds__(256) k_symm_keys(const LinArgs a, const SymmArgs sa, double *out) {
    match_residuals<SymmArgs, true>(a, sa, nullptr, out);
}
__global__ void __launch_bounds__(256) k_symm_adaptive(const LinArgs a, const AdaptiveSide<SymmArgs> sa) {
    match_reduce<SYMM_ROBUST_W>(a, adaptive_side(sa));
}

// ---- the entry points: a UNIT of match_pass.h -------------------------------------------------------------------------
// The search is ICP's (its LinArgs carries the PtN records too: pass.hip, pass_fill_lin); the parameter of a call is the normal
// gate min_cos
struct SymmUnit : MatchUnit {
    typedef SymmArgs Side;
    typedef double Params;
    static pcr_status check(Params *p, double min_cos) {
        PCR_REQUIRE(min_cos >= 0.0 && min_cos <= 1.0, "min_cos must be in [0, 1]");      // (false for NaN)
        *p = min_cos;
        return PCR_OK;
    }
    static constexpr int kind = PCR_ICP;
    static pcr_status payloads(const pcr_target *t, const pcr_scan *s) {
        if (t->is_voxel) { pcr_set_error("SymmetricICP needs a point target"); return PCR_ERR_NO_TARGET; }
        if (!t->pn) { pcr_set_error("SymmetricICP target has no normals (pcr_target_estimate_normals / _set_normals)"); return PCR_ERR_NO_TARGET; }
        if (!s->nrm) { pcr_set_error("SymmetricICP scan has no normals (pcr_scan_estimate_normals / _set_normals)"); return PCR_ERR_NO_TARGET; }
        return PCR_OK;
    }
    static Side side(const pcr_target *, const pcr_scan *s, const Params &min_cos) { return {s->nrm, min_cos, nullptr}; }
    static constexpr auto reduce = k_symm_reduce;
    static constexpr auto robust = k_symm_robust;
    static constexpr auto fold = k_symm_fold;
    static constexpr auto residuals = k_symm_residuals;
    static constexpr auto keys = k_symm_keys;
    static constexpr auto adaptive = k_symm_adaptive;
    static constexpr const char *reduce_range = "pcr:symm_reduce", *robust_range = "pcr:symm_robust", *residuals_range = "pcr:symm_residuals",
                                *adaptive_range = "pcr:symm_adaptive";
};

extern "C" pcr_status pcr_symm_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos, unsigned flags,
                                         double out[29]) {
    return match_linearize<SymmUnit>(t, s, T, max_dist, nullptr, flags, out, min_cos);
}
extern "C" pcr_status pcr_symm_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                     double min_cos, unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    return match_align<SymmUnit>(t, s, T_init, max_iter, tol, max_dist, nullptr, flags, T_out, iterations, trace_or_null, min_cos);
}
extern "C" pcr_status pcr_symm_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos,
                                                const pcr_robust *rb, unsigned flags, double out[29]) {
    return match_linearize<SymmUnit>(t, s, T, max_dist, rb, flags, out, min_cos);
}
extern "C" pcr_status pcr_symm_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                            double min_cos, const pcr_robust *rb, unsigned flags, double T_out[16], int *iterations,
                                            double *trace_or_null) {
    return match_align<SymmUnit>(t, s, T_init, max_iter, tol, max_dist, rb, flags, T_out, iterations, trace_or_null, min_cos);
}
extern "C" pcr_status pcr_symm_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos, unsigned flags,
                                         double *s_out) {
    return match_residuals_entry<SymmUnit>(t, s, T, max_dist, flags, s_out, min_cos);
}
extern "C" pcr_status pcr_symm_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos, const pcr_adaptive *ad,
                                                 unsigned flags, double out[29], double stats[4]) {
    return match_linearize_adaptive<SymmUnit>(t, s, T, max_dist, ad, flags, out, stats, min_cos);
}
extern "C" pcr_status pcr_symm_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             double min_cos, const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations,
                                             double *trace_or_null, double *stats_or_null) {
    return match_align_adaptive<SymmUnit>(t, s, T_init, max_iter, tol, max_dist, ad, flags, T_out, iterations, trace_or_null, stats_or_null, min_cos);
}
