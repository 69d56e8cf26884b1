// Symmetric point-to-plane ICP (Rusinkiewicz: "A Symmetric Objective Function for ICP", SIGGRAPH 2019; the fixed-normal-sum
// form PCL offers): PlaneICP's row with the mean of BOTH clouds' normals in the place of the target's.  Built BESIDE the hot
// path like gicp.hip: its own kernels and entry points, no new kind in the templated pass kernels (pass_device.h / dist_pass.h
// are included; kernels.hip, rows.hip, gicp.hip, vgicp.hip keep their device code).  The definition is in include/pcr.h.
//
//   k_symm_normals<REG>  sibling of k_gicp_cov<REG>: the k nearest neighbours of every point of an indexed cloud within that cloud
//                        (knn_self), two-pass float64 covariance (knn_cov6_f64), smallest_eigvec3 -- what
//                        pcr_target_estimate_normals(compat = 0) computes -- three floats per point, written through pt_orig: the
//                        INPUT order of the indexed cloud, which for a scan's temporary self-index is its device order.
//   k_symm_perm<TO_DEV>  caller order <-> device order through pcr_scan::order
//   k_symm_reduce        sits where k_gicp_reduce sits: behind a full search (pass.hip: pcr_rows_search, ICP's) into a match
//   k_symm_fold          buffer of the call.  symm_reduce is the three-phase loop of dist_reduce with a normal where that has a
//                        covariance; fold and the two launches are dist_fold / dist_launch as they are.
//
// Scan side: pcr_scan::nrm, three floats per point in device order (12 bytes beside the 16 of index and coordinates).  Target
// side: the PtN records PlaneICP gathers -- point and normal in one 32-byte sector.
#include <math.h>
#include <string.h>

#include "dist_pass.h"
#include "eigen3.h"
#include "knn_device.h"

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

// TO_DEVICE: dev[i] = caller[order[i]]; else caller[order[i]] = dev[i] (order NULL: the same order)
template <bool TO_DEVICE>
__global__ void __launch_bounds__(256) k_symm_perm(const float *__restrict__ in, int64_t n, const uint32_t *__restrict__ order, float *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t c = order ? (size_t)order[i] : (size_t)i;
    const float *src = in + 3 * (TO_DEVICE ? c : (size_t)i);
    float *dst = out + 3 * (TO_DEVICE ? (size_t)i : c);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

static pcr_status scan_nrm_alloc(pcr_scan *s) {
    if (!s->nrm) HIP_TRY(pcr_scan_alloc(s, (void **)&s->nrm, 12 * (size_t)(s->n ? s->n : 1)));
    return PCR_OK;
}

// device-order normals of a scan -> the caller's array
static pcr_status scan_nrm_read(pcr_scan *s, float *normals) {
    pcr_context *ctx = s->ctx;
    if (s->n == 0) return PCR_OK;
    DevBuf<float> d;
    HIP_TRY(d.alloc(3 * (size_t)s->n));
    hipLaunchKernelGGL(k_symm_perm<false>, grid_for(s->n, 256), dim3(256), 0, ctx->stream, (const float *)s->nrm, s->n, (const uint32_t *)s->order, d.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(normals, d.p, 12 * (size_t)s->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_scan_estimate_normals(pcr_scan *s, int k, float *normals_out_or_null) {
    PCR_REQUIRE(s, "NULL argument");
    if (k < 1 || k > KNN_MAX_K) { pcr_set_error("k must be in [1, %d]", KNN_MAX_K); return PCR_ERR_INVALID; }
    PCR_REQUIRE(!normals_out_or_null || pcr_scan_knows_order(s), PCR_NEED_ORDER);
    pcr_context *ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    if (s->n == 0) return scan_nrm_alloc(s);
    // into the scan's array when it has one, else into a block the scan takes over only once the estimate is complete: a
    // failure on the way must not leave a scan that "has normals" holding uninitialised ones
    float *dst = s->nrm;
    bool fresh = false;
    if (!dst) {
        HIP_TRY(pcr_scan_alloc(s, (void **)&dst, 12 * (size_t)s->n));
        fresh = true;
    }
    struct Undo {
        pcr_scan *s; float *p; bool armed;
        ~Undo() { if (armed) { pcr_scan_free(s, p); } }
    } undo{s, dst, fresh};
    if (!fresh) { s->nrm = nullptr; undo.armed = true; }      // (re-estimating: a failure leaves the scan without normals)
    {
        TmpIndex idx;
        PCR_TRY(pcr_scan_self_index(s, &idx));
        knn_launch(k_symm_normals<1>, k_symm_normals<0>, k <= KNN_REG_K, s->n, k, ctx->stream, idx.t->gf, (const PtF *)idx.t->pts,
                   (const uint32_t *)idx.t->cell_start, s->n, k, dst);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    undo.armed = false;
    s->nrm = dst;
    if (normals_out_or_null) return scan_nrm_read(s, normals_out_or_null);
    return PCR_OK;
}

extern "C" pcr_status pcr_scan_set_normals(pcr_scan *s, const float *normals) {
    PCR_REQUIRE(s && (normals || s->n == 0), "NULL argument");
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    // (checked before anything of the scan changes: a refused set leaves the old normals)
    for (size_t i = 0; i < 3 * (size_t)s->n; ++i)
        if (!isfinite(normals[i])) { pcr_set_error("invalid argument: normals must be finite"); return PCR_ERR_INVALID; }
    pcr_context *ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    PCR_TRY(scan_nrm_alloc(s));
    if (s->n == 0) return PCR_OK;
    DevBuf<float> d;
    HIP_TRY(d.alloc(3 * (size_t)s->n));
    HIP_TRY(hipMemcpyAsync(d.p, normals, 12 * (size_t)s->n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_symm_perm<true>, grid_for(s->n, 256), dim3(256), 0, ctx->stream, (const float *)d.p, s->n, (const uint32_t *)s->order, s->nrm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_scan_get_normals(pcr_scan *s, float *normals) {
    PCR_REQUIRE(s && (normals || s->n == 0), "NULL argument");
    if (!s->nrm) { pcr_set_error("scan has no per-point normals"); return PCR_ERR_NO_TARGET; }
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    HIP_TRY(hipSetDevice(s->ctx->device));
    CtxScope scope(s->ctx);
    return scan_nrm_read(s, normals);
}

// ---- the pass ---------------------------------------------------------------------------------------------------------
struct SymmArgs {
    const float *snrm;       // scan normals, device order, 3 floats per point
    double min_cos;          // normal gate: kept iff |n_q . R n_p| >= min_cos
    double *rows;            // [gridDim.x][32]
};

// points per lane in flight.  A point carries 7 registers through phase A and 8 more through phase B.  3: 122 registers, four
// waves per SIMD; 4 needs 136 and drops to three waves for the same twelve points in flight (docs/EXPERIMENTS.md)
#ifndef SYMM_W
#define SYMM_W 3
#endif

// The three-phase loop of dist_reduce (dist_pass.h) with a scan normal where that carries a covariance:
//   phase A  index, coordinates and the three normal floats of all W points.  A point past the end reads the lane's first point.
//   phase B  the W PtN records, two 16-byte loads of one sector.  No match: record 0 through a select on the index.
//   phase C  the arithmetic of include/pcr.h, in index order.
template <int W>
__device__ __forceinline__ void symm_reduce(const LinArgs &a, const SymmArgs &sa) {
    const PoseK &P = a.hp;                           // host-driven: the pose came by value
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x; t0 < a.n; t0 += W * stride) {
        uint32_t j[W];
        float x[W], y[W], z[W], nx[W], ny[W], nz[W];
        float4 q[W], nq[W];
        bool use[W];
        // phase A
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const int64_t t = t0 + u * stride;
            use[u] = t < a.n;
            const int64_t i = use[u] ? t : t0;
            j[u] = a.nn_j[i];
            x[u] = a.sx[i]; y[u] = a.sy[i]; z[u] = a.sz[i];
            const float *np = sa.snrm + 3 * i;
            nx[u] = np[0]; ny[u] = np[1]; nz[u] = np[2];
        }
        reduce_phase();
#pragma unroll
        for (int u = 0; u < W; ++u) reduce_pin(j[u]);
        // phase B
#pragma unroll
        for (int u = 0; u < W; ++u) {
            use[u] = use[u] && j[u] != PCR_NONE;
            const float4 *rec = reinterpret_cast<const float4 *>(a.pn + (use[u] ? j[u] : 0u));
            q[u] = rec[0]; nq[u] = rec[1];
        }
        reduce_phase();
        // phase C
#pragma unroll
        for (int u = 0; u < W; ++u) {
            if (!use[u]) continue;
            float tx, ty, tz, dx, dy, dz;
            xform(P, x[u], y[u], z[u], tx, ty, tz);
            if (!residual_f32<true>(a, q[u], tx, ty, tz, dx, dy, dz)) continue;
            const double px = nx[u], py = ny[u], pz = nz[u];
            const double v0 = (P.R[0] * px + P.R[1] * py) + P.R[2] * pz;
            const double v1 = (P.R[3] * px + P.R[4] * py) + P.R[5] * pz;
            const double v2 = (P.R[6] * px + P.R[7] * py) + P.R[8] * pz;
            const double q0 = nq[u].x, q1 = nq[u].y, q2 = nq[u].z;
            const double c = (q0 * v0 + q1 * v1) + q2 * v2;
            if (!(fabs(c) >= sa.min_cos)) continue;                  // (a NaN c is skipped)
            const double sg = c < 0.0 ? -1.0 : 1.0;
            const double m0 = 0.5 * (q0 + sg * v0), m1 = 0.5 * (q1 + sg * v1), m2 = 0.5 * (q2 + sg * v2);
            double J[6];
            const double r = plane_row(P, (double)x[u], (double)y[u], (double)z[u], m0, m1, m2, (double)dx, (double)dy, (double)dz, J);
            acc_rank1(acc, J, r);
        }
    }
    block_store_partials<false>(acc, sa.rows);
}

__global__ void __launch_bounds__(256) k_symm_reduce(const LinArgs a, const SymmArgs sa) { symm_reduce<SYMM_W>(a, sa); }
__global__ void __launch_bounds__(64) k_symm_fold(const double *__restrict__ rows, int nb, double *out) { dist_fold(rows, nb, out); }

static pcr_status check_min_cos(double min_cos) {
    PCR_REQUIRE(min_cos >= 0.0 && min_cos <= 1.0, "min_cos must be in [0, 1]");      // (false for NaN)
    return PCR_OK;
}

// search + the symmetric pass.  A pcr_pass_fn: `kind` is not read, the search is ICP's (its LinArgs carries the PtN records
// too: pass.hip, pass_fill_lin); the normal gate comes in pcr_scan::symm_min_cos, set by the entry points below
static pcr_status pcr_run_symm(pcr_target *t, pcr_scan *s, int, const double T[16], double max_dist, unsigned flags, double out[29]) {
    if (t->is_voxel) { pcr_set_error("SymmetricICP needs a point target"); return PCR_ERR_NO_TARGET; }
    if (!t->pn) { pcr_set_error("SymmetricICP target has no normals (pcr_target_estimate_normals / _set_normals)"); return PCR_ERR_NO_TARGET; }
    if (!s->nrm) { pcr_set_error("SymmetricICP scan has no normals (pcr_scan_estimate_normals / _set_normals)"); return PCR_ERR_NO_TARGET; }
    LinArgs a;
    DevBuf<uint32_t> nn;
    PCR_TRY(pcr_rows_search(&a, &nn, t, s, PCR_ICP, T, max_dist, flags, false));
    for (int i = 0; i < 29; ++i) out[i] = 0.0;
    if (s->n == 0) return PCR_OK;
    const SymmArgs sa{s->nrm, s->symm_min_cos, nullptr};
    return dist_launch(t->ctx, "pcr:symm_reduce", k_symm_reduce, k_symm_fold, a, sa, s->n, out);
}

extern "C" pcr_status pcr_symm_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos, unsigned flags,
                                         double out[29]) {
    PCR_REQUIRE(t && s && T && out, "NULL argument");
    PCR_TRY(check_min_cos(min_cos));
    CtxScope scope(t->ctx);
    s->symm_min_cos = min_cos;
    return pcr_run_symm(t, s, PCR_ICP, T, max_dist, flags, out);
}

// the host-driven Gauss-Newton loop of pcr_align (api.hip: pcr_align_host_loop) over the pass: same gn_step, same trace rows
extern "C" pcr_status pcr_symm_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                     double min_cos, unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    PCR_REQUIRE(t && s && T_init && T_out, "NULL argument");
    PCR_TRY(check_min_cos(min_cos));
    CtxScope scope(t->ctx);
    s->symm_min_cos = min_cos;
    return pcr_align_host_loop(pcr_run_symm, t, s, PCR_ICP, T_init, max_iter, tol, max_dist, flags, T_out, iterations, trace_or_null);
}
