// Colored ICP (Park, Zhou, Koltun: "Colored Point Cloud Registration Revisited", ICCV 2017; the form Open3D offers): PlaneICP's
// row plus a second row per correspondence, the difference of the two points' intensities with the target's intensity carried
// along its tangent plane by a per-point gradient.  Built BESIDE the hot path like symm.hip: its own kernels and entry points, no
// new kind in the templated pass kernels (pass_device.h / match_pass.h / knn_device.h are included; every other unit keeps its
// device code).  The definition is in include/pcr.h.
//
//   k_color_gather         caller-order intensities -> the index's cell-sorted order (pt_orig): pcr_target::cint
//   k_color_pack           cell-sorted intensities + caller-order gradients (or none: zeros) -> the records pcr_target::col
//   k_color_unpack         the records -> caller-order intensities and gradients
//   k_color_gradient<REG>  one lane per target point, a knn_self finish functor: the least-squares gradient of the intensity over
//                          the k nearest neighbours, in the tangent plane of the point's normal.  Reads the neighbours'
//                          intensities from cint and writes {I, gx, gy, gz} into col -- a different array
//   k_color_perm<TO_DEV>   one float per point, caller order <-> device order through pcr_scan::order: ScanPayload<1>
//                          (scan_payload.h)
//   k_color_reduce         sits where k_symm_reduce sits: behind a full search (pass.hip: pcr_rows_search, ICP's) into a match
//   k_color_fold           buffer of the call.  The pass over a match list of match_pass.h (match_reduce, match_fold,
//                          match_run) with ColorArgs as its SIDE, COLOR_W points per lane in flight.
//   k_color_robust         the same pass with each of the two rows weighed by a robust kernel of its own r r
//                          (RobustSide<ColorArgs>, COLOR_ROBUST_W points per lane in flight), folded by k_color_fold
//   k_color_residuals      both rows' r r of every scan point in the caller's order (match_residuals)
//   k_color_keys           the adaptive pass (include/pcr.h): a key per scan point in device order (match_residuals<., true>)
//   k_color_adaptive       k_color_robust's reduce behind the selection over the keys (select.hip), its kernel read from the
//                          selection's state (AdaptiveSide)
//   ColorUnit              what the seven entry points differ in; the rest of them is match_pass.h's (match_run, match_linearize,
//                          match_align, match_residuals_entry, match_linearize_adaptive, match_align_adaptive)
//
// Scan side: pcr_scan::inten, one float per point in device order.  Target side: the PtN records PlaneICP gathers and the
// 16-byte colour records, 48 bytes per match from two arrays.
#include <math.h>
#include <string.h>

#include "knn_device.h"
#include "match_pass.h"
#include "scan_payload.h"

extern __shared__ __attribute__((aligned(16))) char color_smem[];

// ---- the target's records ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_color_gather(const float *__restrict__ in, const PtF *__restrict__ pts, int64_t n, float *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    out[j] = in[pt_orig(pts[j])];
}

// grad: caller order, 3 floats per point; NULL: zeros
__global__ void __launch_bounds__(256) k_color_pack(const float *__restrict__ cint, const float *__restrict__ grad, const PtF *__restrict__ pts,
                                                    int64_t n, float4 *__restrict__ col) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float4 r = make_float4(cint[j], 0.f, 0.f, 0.f);
    if (grad) {
        const float *g = grad + 3 * (size_t)pt_orig(pts[j]);
        r.y = g[0]; r.z = g[1]; r.w = g[2];
    }
    col[j] = r;
}

// inten / grad: caller order; either may be NULL
__global__ void __launch_bounds__(256) k_color_unpack(const float4 *__restrict__ col, const PtF *__restrict__ pts, int64_t n, float *inten, float *grad) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const float4 r = col[j];
    const size_t i = pt_orig(pts[j]);
    if (inten) inten[i] = r.x;
    if (grad) { grad[3 * i] = r.y; grad[3 * i + 1] = r.z; grad[3 * i + 2] = r.w; }
}

// The gradient of include/pcr.h over the neighbours found (nearest first; the point itself and exact duplicates, squared
// distance 0, are left out).  Zero when fewer than three neighbours remain, when det M is not > 0, when a component is not finite.
template <typename LIST>
__device__ __forceinline__ void color_gradient_finish(const PtF *pts, const PtN *pn, const float *cint, const uint32_t j, const PtF me,
                                                      float4 *col, LIST &L) {
    const PtN rec = pn[j];
    const double n0 = rec.nx, n1 = rec.ny, n2 = rec.nz;
    const float Iq = cint[j];
    double M[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};      // xx xy xz yy yz zz
    int w = 0;
    L.for_each([&](int, float d2, uint32_t js) {
        if (!(d2 > 0.f)) return;
        const PtF p = pts[js];
        const double e0 = (double)p.x - (double)me.x, e1 = (double)p.y - (double)me.y, e2 = (double)p.z - (double)me.z;
        const double en = (e0 * n0 + e1 * n1) + e2 * n2;
        const double u0 = e0 - en * n0, u1 = e1 - en * n1, u2 = e2 - en * n2;
        const double dI = (double)cint[js] - (double)Iq;
        M[0] += u0 * u0; M[1] += u0 * u1; M[2] += u0 * u2; M[3] += u1 * u1; M[4] += u1 * u2; M[5] += u2 * u2;
        b[0] += u0 * dI; b[1] += u1 * dI; b[2] += u2 * dI;
        ++w;
    });
    const double ww = (double)(w * w);
    M[0] += ww * (n0 * n0); M[1] += ww * (n0 * n1); M[2] += ww * (n0 * n2);
    M[3] += ww * (n1 * n1); M[4] += ww * (n1 * n2); M[5] += ww * (n2 * n2);
    // the closed-form symmetric inverse, the expressions of icov_closed_form (eigen3.h) with the determinant kept
    const double a_ = M[0], b_ = M[3], c_ = M[5], d_ = M[1], e_ = M[2], f_ = M[4];
    const double f2 = f_ * f_, d2 = d_ * d_, e2 = e_ * e_;
    const double bc = b_ * c_, ac = a_ * c_, ab = a_ * b_;
    const double dc = d_ * c_, de = d_ * e_, ef = e_ * f_;
    const double af = a_ * f_, df = d_ * f_, eb = e_ * b_;
    const double det = a_ * bc + 2 * de * f_ - a_ * f2 - b_ * e2 - c_ * d2;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (w >= 3 && det > 0.0) {
        const double c0 = (bc - f2) / det, c1 = -(dc - ef) / det, c2 = (df - eb) / det;
        const double c3 = (ac - e2) / det, c4 = -(af - de) / det, c5 = (ab - d2) / det;
        const double s0 = (c0 * b[0] + c1 * b[1]) + c2 * b[2];
        const double s1 = (c1 * b[0] + c3 * b[1]) + c4 * b[2];
        const double s2 = (c2 * b[0] + c4 * b[1]) + c5 * b[2];
        const double sn = (s0 * n0 + s1 * n1) + s2 * n2;
        g0 = (float)(s0 - sn * n0); g1 = (float)(s1 - sn * n1); g2 = (float)(s2 - sn * n2);
        if (!(isfinite(g0) && isfinite(g1) && isfinite(g2))) { g0 = 0.f; g1 = 0.f; g2 = 0.f; }
    }
    col[j] = make_float4(Iq, g0, g1, g2);
}

// REG = 1: the collect path (k <= 16); 0: the LDS list (knn_self, knn_device.h)
template <int REG>
__global__ void __launch_bounds__(KNN_BLOCK) k_color_gradient(Geom<float> g, const PtF *pts, const uint32_t *cs, const PtN *pn, const float *cint,
                                                              int64_t n, int k, float4 *col) {
    const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    knn_self<REG>(g, pts, cs, me, k, color_smem, [&](auto &L) { color_gradient_finish(pts, pn, cint, (uint32_t)i, me, col, L); });
}

static pcr_status check_color_target(const pcr_target *t) {
    if (t->is_voxel || !t->pn) { pcr_set_error("intensities belong to point targets with normals (pcr_target_estimate_normals / _set_normals)"); return PCR_ERR_NO_TARGET; }
    return PCR_OK;
}

extern "C" pcr_status pcr_target_set_intensity(pcr_target *t, const float *intensity, const float *gradient_or_null) {
    PCR_REQUIRE(t && (intensity || t->n == 0), "NULL argument");
    PCR_TRY(check_color_target(t));
    // (checked before anything of the target changes: a refused set leaves the old payload)
    PCR_TRY(check_finite(intensity, (size_t)t->n, "intensities"));
    if (gradient_or_null) PCR_TRY(check_finite(gradient_or_null, 3 * (size_t)t->n, "gradients"));
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t nn = (size_t)(t->n ? t->n : 1);
    DevBuf<float> d_i, d_g;
    HIP_TRY(d_i.alloc(nn));
    if (gradient_or_null) HIP_TRY(d_g.alloc(3 * nn));
    if (!t->cint) HIP_TRY(pcr_persist_alloc((void **)&t->cint, sizeof(float) * nn));
    if (!t->col) HIP_TRY(pcr_persist_alloc((void **)&t->col, sizeof(float4) * nn));
    if (t->n == 0) return PCR_OK;
    HIP_TRY(hipMemcpyAsync(d_i.p, intensity, 4 * (size_t)t->n, hipMemcpyHostToDevice, ctx->stream));
    if (gradient_or_null) HIP_TRY(hipMemcpyAsync(d_g.p, gradient_or_null, 12 * (size_t)t->n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_color_gather, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const float *)d_i.p, (const PtF *)t->pts, t->n, t->cint);
    hipLaunchKernelGGL(k_color_pack, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const float *)t->cint, (const float *)d_g.p, (const PtF *)t->pts,
                       t->n, t->col);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_get_color(pcr_target *t, float *intensity_or_null, float *gradient_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    if (t->is_voxel || !t->col) { pcr_set_error("target has no per-point intensities"); return PCR_ERR_NO_TARGET; }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (t->n == 0 || (!intensity_or_null && !gradient_or_null)) return PCR_OK;
    CtxScope scope(ctx);
    DevBuf<float> d_i, d_g;
    if (intensity_or_null) HIP_TRY(d_i.alloc((size_t)t->n));
    if (gradient_or_null) HIP_TRY(d_g.alloc(3 * (size_t)t->n));
    hipLaunchKernelGGL(k_color_unpack, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const float4 *)t->col, (const PtF *)t->pts, t->n, d_i.p, d_g.p);
    HIP_TRY(hipGetLastError());
    if (intensity_or_null) HIP_TRY(hipMemcpyAsync(intensity_or_null, d_i.p, 4 * (size_t)t->n, hipMemcpyDeviceToHost, ctx->stream));
    if (gradient_or_null) HIP_TRY(hipMemcpyAsync(gradient_or_null, d_g.p, 12 * (size_t)t->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_estimate_color_gradients(pcr_target *t, int k, float *gradient_out_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    if (k < 1 || k > KNN_MAX_K) { pcr_set_error("k must be in [1, %d]", KNN_MAX_K); return PCR_ERR_INVALID; }
    PCR_TRY(check_color_target(t));
    if (!t->col) { pcr_set_error("target has no per-point intensities (pcr_target_set_intensity)"); return PCR_ERR_NO_TARGET; }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    if (t->n > 0) {
        knn_launch(k_color_gradient<1>, k_color_gradient<0>, k <= KNN_REG_K, t->n, k, ctx->stream, t->gf, (const PtF *)t->pts,
                   (const uint32_t *)t->cell_start, (const PtN *)t->pn, (const float *)t->cint, t->n, k, t->col);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (gradient_out_or_null) return pcr_target_get_color(t, nullptr, gradient_out_or_null);
    return PCR_OK;
}

// ---- intensities on a scan --------------------------------------------------------------------------------------------
// caller order <-> device order through pcr_scan::order (scan_payload.h)
template <bool TO_DEVICE>
__global__ void __launch_bounds__(256) k_color_perm(const float *__restrict__ in, int64_t n, const uint32_t *__restrict__ order, float *out) {
    payload_perm<1, TO_DEVICE>(in, n, order, out);
}
static const ScanPayload<1> scan_inten{&pcr_scan::inten, k_color_perm<true>, k_color_perm<false>};

extern "C" pcr_status pcr_scan_set_intensity(pcr_scan *s, const float *intensity) {
    PCR_REQUIRE(s && (intensity || s->n == 0), "NULL argument");
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    // (checked before anything of the scan changes: a refused set leaves the old intensities)
    PCR_TRY(check_finite(intensity, (size_t)s->n, "intensities"));
    return scan_inten.set(s, intensity);
}

extern "C" pcr_status pcr_scan_get_intensity(pcr_scan *s, float *intensity) {
    PCR_REQUIRE(s && (intensity || s->n == 0), "NULL argument");
    if (!s->inten) { pcr_set_error("scan has no per-point intensities"); return PCR_ERR_NO_TARGET; }
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    return scan_inten.get(s, intensity);
}

// ---- the pass ---------------------------------------------------------------------------------------------------------
// A SIDE of match_pass.h.  Phase A carries the intensity of a scan point, phase B the PtN record of the match (two 16-byte
// loads of one sector) and its colour record (one 16-byte load); each is the arithmetic of include/pcr.h up to the two rows
// (J, r) of a correspondence, add their plain accumulation: two rows, one count
struct ColorArgs {
    const float *sint;       // scan intensities, device order
    const float4 *col;       // the target's colour records, cell-sorted
    double ag, ac;           // sqrt(lambda), sqrt(1 - lambda)
    double *rows;            // [gridDim.x][32]

    typedef float Scan;
    struct Match { float4 q, nq, cq; };
    __device__ __forceinline__ void load(int64_t i, Scan &ip) const { ip = sint[i]; }
    __device__ __forceinline__ void gather(const LinArgs &a, uint32_t j, Match &m) const {
        const float4 *rec = reinterpret_cast<const float4 *>(a.pn + j);
        m.q = rec[0]; m.nq = rec[1];
        m.cq = col[j];
    }
    typedef RowsPlain Plain;
    typedef RowsWeighted Weighted;
    typedef RowsResid Resid;
    static constexpr int M = 2;
    // the ONE statement of a correspondence: the gate, then f on the geometric row and on the colour row
    template <typename F>
    __device__ __forceinline__ void each(const LinArgs &a, const PoseK &P, float x, float y, float z, float tx, float ty, float tz,
                                         const Scan &ip, const Match &m, const F &f) const {
        float dx, dy, dz;
        if (!residual_f32<true>(a, m.q, tx, ty, tz, dx, dy, dz)) return;
        const double n0 = m.nq.x, n1 = m.nq.y, n2 = m.nq.z;
        const double g0 = m.cq.y, g1 = m.cq.z, g2 = m.cq.w;
        const double d0 = dx, d1 = dy, d2 = dz;
        const double px = x, py = y, pz = z;
        double J[6];
        // the geometric row: PlaneICP's, times sqrt(lambda)
        double r = plane_row(P, px, py, pz, n0, n1, n2, d0, d1, d2, J);
#pragma unroll
        for (int i = 0; i < 6; ++i) J[i] *= ag;
        f(0, J, ag * r);
        // the colour row: the gradient's tangent part in the place of the normal, times sqrt(1 - lambda)
        const double gn = (g0 * n0 + g1 * n1) + g2 * n2;
        const double m0 = g0 - gn * n0, m1 = g1 - gn * n1, m2 = g2 - gn * n2;
        r = ((double)m.cq.x - (double)ip) + plane_row(P, px, py, pz, m0, m1, m2, d0, d1, d2, J);
#pragma unroll
        for (int i = 0; i < 6; ++i) J[i] *= ac;
        f(1, J, ac * r);                                             // (a second row does not count: out[28] counts correspondences)
    }
    __device__ __forceinline__ void add(double *acc, const LinArgs &a, const PoseK &P, float x, float y, float z, float tx, float ty, float tz,
                                        const Scan &ip, const Match &m) const {
        each(a, P, x, y, z, tx, ty, tz, ip, m, Plain(acc, P, x, y, z));
    }
};

// points per lane in flight.  A point carries 5 registers through phase A and 12 more through phase B.  2: 126 registers, four
// waves per SIMD; 3 needs 140 and drops to three waves, 4 needs 154 (docs/EXPERIMENTS.md)
#ifndef COLOR_W
#define COLOR_W 2
#endif

__global__ void __launch_bounds__(256) k_color_reduce(const LinArgs a, const ColorArgs ca) { match_reduce<COLOR_W>(a, ca); }
__global__ void __launch_bounds__(64) k_color_fold(const double *__restrict__ rows, int nb, double *out) { match_fold(rows, nb, out); }

// the pass under a robust weight per row (include/pcr.h: "robust kernels"): the same three phases, fold and grid; for its
// registers and COLOR_ROBUST_W see docs/EXPERIMENTS.md
#ifndef COLOR_ROBUST_W
#define COLOR_ROBUST_W 2
#endif
__global__ void __launch_bounds__(256) k_color_robust(const LinArgs a, const RobustSide<ColorArgs> ca) { match_reduce<COLOR_ROBUST_W>(a, ca); }
// the squared residuals of both rows of every scan point in the caller's order, +inf where there is no correspondence
__global__ void __launch_bounds__(256) k_color_residuals(const LinArgs a, const ColorArgs ca, const uint32_t *order, double *out) {
    match_residuals(a, ca, order, out);
}
// the adaptive pass (include/pcr.h: "adaptive pass"): a key per scan point in device order, +inf where there is no
// correspondence; behind the selection over the keys (select.hip), k_color_robust's reduce with its kernel read from the
// selection's state (AdaptiveSide), folded by k_color_fold
__global__ void __launch_bounds__(256) k_color_keys(const LinArgs a, const ColorArgs ca, double *out) {
    match_residuals<ColorArgs, true>(a, ca, nullptr, out);
}
__global__ void __launch_bounds__(256) k_color_adaptive(const LinArgs a, const AdaptiveSide<ColorArgs> ca) {
    match_reduce<COLOR_ROBUST_W>(a, adaptive_side(ca));
}

// ---- the entry points: a UNIT of match_pass.h -------------------------------------------------------------------------
// The search is ICP's (its LinArgs carries the PtN records too); the parameter of a call is lambda_geometric, taken through
// the pass as sqrt(lambda) and sqrt(1 - lambda): once, in double
struct ColorUnit : MatchUnit {
    typedef ColorArgs Side;
    struct Params { double ag, ac; };
    static pcr_status check(Params *p, double lambda) {
        PCR_REQUIRE(lambda >= 0.0 && lambda <= 1.0, "lambda_geometric must be in [0, 1]");      // (false for NaN)
        p->ag = sqrt(lambda);
        p->ac = sqrt(1.0 - lambda);
        return PCR_OK;
    }
    static constexpr int kind = PCR_ICP;
    static pcr_status payloads(const pcr_target *t, const pcr_scan *s) {
        if (t->is_voxel) { pcr_set_error("ColoredICP needs a point target"); return PCR_ERR_NO_TARGET; }
        if (!t->pn) { pcr_set_error("ColoredICP target has no normals (pcr_target_estimate_normals / _set_normals)"); return PCR_ERR_NO_TARGET; }
        if (!t->col) { pcr_set_error("ColoredICP target has no colour records (pcr_target_set_intensity; replacing the normals frees them)"); return PCR_ERR_NO_TARGET; }
        if (!s->inten) { pcr_set_error("ColoredICP scan has no intensities (pcr_scan_set_intensity)"); return PCR_ERR_NO_TARGET; }
        return PCR_OK;
    }
    static Side side(const pcr_target *t, const pcr_scan *s, const Params &p) { return {s->inten, t->col, p.ag, p.ac, nullptr}; }
    static constexpr auto reduce = k_color_reduce;
    static constexpr auto robust = k_color_robust;
    static constexpr auto fold = k_color_fold;
    static constexpr auto residuals = k_color_residuals;
    static constexpr auto keys = k_color_keys;
    static constexpr auto adaptive = k_color_adaptive;
    static constexpr const char *reduce_range = "pcr:color_reduce", *robust_range = "pcr:color_robust", *residuals_range = "pcr:color_residuals",
                                *adaptive_range = "pcr:color_adaptive";
};

extern "C" pcr_status pcr_color_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric,
                                          unsigned flags, double out[29]) {
    return match_linearize<ColorUnit>(t, s, T, max_dist, nullptr, flags, out, lambda_geometric);
}
extern "C" pcr_status pcr_color_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                      double lambda_geometric, unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    return match_align<ColorUnit>(t, s, T_init, max_iter, tol, max_dist, nullptr, flags, T_out, iterations, trace_or_null, lambda_geometric);
}
extern "C" pcr_status pcr_color_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric,
                                                 const pcr_robust *rb, unsigned flags, double out[29]) {
    return match_linearize<ColorUnit>(t, s, T, max_dist, rb, flags, out, lambda_geometric);
}
extern "C" pcr_status pcr_color_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             double lambda_geometric, const pcr_robust *rb, unsigned flags, double T_out[16], int *iterations,
                                             double *trace_or_null) {
    return match_align<ColorUnit>(t, s, T_init, max_iter, tol, max_dist, rb, flags, T_out, iterations, trace_or_null, lambda_geometric);
}
extern "C" pcr_status pcr_color_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric,
                                          unsigned flags, double *s_out) {
    return match_residuals_entry<ColorUnit>(t, s, T, max_dist, flags, s_out, lambda_geometric);
}
extern "C" pcr_status pcr_color_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric, const pcr_adaptive *ad,
                                                 unsigned flags, double out[29], double stats[4]) {
    return match_linearize_adaptive<ColorUnit>(t, s, T, max_dist, ad, flags, out, stats, lambda_geometric);
}
extern "C" pcr_status pcr_color_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             double lambda_geometric, const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations,
                                             double *trace_or_null, double *stats_or_null) {
    return match_align_adaptive<ColorUnit>(t, s, T_init, max_iter, tol, max_dist, ad, flags, T_out, iterations, trace_or_null, stats_or_null, lambda_geometric);
}
