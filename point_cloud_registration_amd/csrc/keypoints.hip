// ISS keypoints (Zhong: Intrinsic Shape Signatures, a shape descriptor for 3D object recognition, ICCV workshops 2009; the
// Open3D form) of a point target.  The contract is in include/pcr.h.
//
//   pcr_target_iss_saliency    k_iss_saliency<1>                eigenvalues, saliency and k in the caller's order (the seam of
//                                                               the exact test)
//   pcr_target_iss_keypoints   k_iss_saliency<0>, k_iss_nms     one byte per point in the caller's order
//
// Both kernels: one lane = one point in CELL-SORTED order, so the lanes of a wave are spatial neighbours, and one
// rad_ball_walk (radius_device.h), the walk of pcr_radius_query: the support set IS what the radius search finds, the point
// itself and its exact duplicates included.  No atomics, the grid depends on n only: two calls return the same bits.
//   k_iss_saliency   the sink sums d = q - a and d d^T in float64 over the members, a = the FIRST member offered.  rad_ball_walk
//                    offers records in ascending cell-sorted index for any query -- slabs by z, rows by y, a row's cells by x,
//                    one contiguous range of records per row -- so the anchor and the order of the sums are functions of the
//                    member set alone: two points with the same support set get the same bits, whatever their own place.
//                    9 float64 accumulators, the anchor and k stay in registers; eigenvalues by eigen3.h's cyclic Jacobi.
//   k_iss_nms        the same walk at the non-maximum radius; the sink reads the saliency at the neighbour's cell-sorted index
//                    and keeps a count and a "beaten" flag.  A lane whose own saliency is 0 skips its walk.
#include "eigen3.h"
#include "radius_device.h"

#define ISS_BLOCK RAD_BLOCK

typedef RadMoments IssSink;      // (radius_device.h: the anchor and the 9 float64 sums, shared with ball_moments.hip)

struct IssNmsSink {
    float r, b2;
    const double *sal;       // [n], cell-sorted
    double mine;
    uint32_t me, my_orig;
    uint32_t count;
    bool beaten;
    __device__ __forceinline__ float bound() const { return b2; }
    __device__ __forceinline__ void offer(float d2f, uint32_t j, uint32_t orig) {
        if (d2f <= b2 && rad_member(d2f, r)) {
            ++count;
            if (j != me) {
                const double sj = sal[j];
                // j loses iff s_j < s_i, or s_j == s_i and it came later in the caller's array
                if (!(sj < mine || (sj == mine && orig > my_orig))) beaten = true;
            }
        }
    }
};

// ORIG = 0: the outputs at the lane's cell-sorted index (what k_iss_nms gathers); 1: at the point's original index.  eig and
// kk may be NULL; sal_orig (or NULL): the saliency once more, at the original index.
template <int ORIG>
__global__ void __launch_bounds__(ISS_BLOCK) k_iss_saliency(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n, float r, double g21,
                                                            double g32, uint32_t min_nb, double *eig, double *sal, uint32_t *kk,
                                                            double *sal_orig) {
    const int64_t i = (int64_t)blockIdx.x * ISS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    IssSink S;
    S.r = r; S.b2 = rad_bound2(r); S.pts = pts; S.k = 0u;
    S.ax = S.ay = S.az = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) S.s1[c] = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) S.s2[c] = 0.0;
    if (rad_finite(me.x, me.y, me.z)) rad_ball_walk(g, pts, cs, me.x, me.y, me.z, r, S);
    double lam[3] = {0.0, 0.0, 0.0};
    if (S.k != 0u) {
        const double kd = (double)S.k;
        const double mx = S.s1[0] / kd, my = S.s1[1] / kd, mz = S.s1[2] / kd;
        const double c[6] = {S.s2[0] / kd - mx * mx, S.s2[1] / kd - mx * my, S.s2[2] / kd - mx * mz,
                             S.s2[3] / kd - my * my, S.s2[4] / kd - my * mz, S.s2[5] / kd - mz * mz};
        eigvals3_sorted(c, lam);
    }
    const bool salient = S.k >= min_nb && lam[0] > 0.0 && lam[1] < g21 * lam[0] && lam[2] < g32 * lam[1] && lam[2] > 0.0;
    const double s = salient ? lam[2] : 0.0;
    const int64_t o = ORIG ? (int64_t)pt_orig(me) : i;
    if (eig) { eig[3 * o] = lam[0]; eig[3 * o + 1] = lam[1]; eig[3 * o + 2] = lam[2]; }
    sal[o] = s;
    if (kk) kk[o] = S.k;
    if (sal_orig) sal_orig[pt_orig(me)] = s;
}

__global__ void __launch_bounds__(ISS_BLOCK) k_iss_nms(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n, float r, const double *sal,
                                                       uint32_t min_nb, uint8_t *is_keypoint) {
    const int64_t i = (int64_t)blockIdx.x * ISS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    IssNmsSink S;
    S.r = r; S.b2 = rad_bound2(r); S.sal = sal; S.mine = sal[i]; S.me = (uint32_t)i; S.my_orig = pt_orig(me); S.count = 0u; S.beaten = false;
    // (a point that is not finite has k = 0 and with it a saliency of 0)
    if (S.mine > 0.0) rad_ball_walk(g, pts, cs, me.x, me.y, me.z, r, S);
    is_keypoint[pt_orig(me)] = (S.mine > 0.0 && S.count >= min_nb && !S.beaten) ? (uint8_t)1 : (uint8_t)0;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// PCR_ISS_TIMES=1 (developer, tools/iss_time.py): the calls bracket their kernels with events (StageTimes) and report the
// milliseconds on stderr

// a point target, a finite radius >= 0, gammas finite and > 0, min_neighbors >= 1
static pcr_status iss_check(const pcr_target *t, float r, double g21, double g32, int min_neighbors, const char *who) {
    PCR_TRY(check_point_target(t, who));
    PCR_TRY(check_radius<float>(r, who));
    if (!(g21 > 0 && g21 <= DBL_MAX && g32 > 0 && g32 <= DBL_MAX)) {
        pcr_set_error("invalid argument: %s needs gamma_21 and gamma_32 finite and > 0", who);
        return PCR_ERR_INVALID;
    }
    if (min_neighbors < 1) { pcr_set_error("invalid argument: %s needs min_neighbors >= 1", who); return PCR_ERR_INVALID; }
    return PCR_OK;
}

// k_iss_saliency<ORIG> over the whole target; any of eig, kk, sal_orig may be NULL
template <int ORIG>
static void iss_saliency_launch(pcr_target *t, float r, double g21, double g32, int min_neighbors, double *eig, double *sal, uint32_t *kk,
                                double *sal_orig) {
    hipLaunchKernelGGL(k_iss_saliency<ORIG>, grid_for(t->n, ISS_BLOCK), dim3(ISS_BLOCK), 0, t->ctx->stream, t->gf, (const PtF *)t->pts,
                       (const uint32_t *)t->cell_start, t->n, r, g21, g32, (uint32_t)min_neighbors, eig, sal, kk, sal_orig);
}

extern "C" pcr_status pcr_target_iss_saliency(pcr_target *t, float r, double gamma21, double gamma32, int min_neighbors, double *eig,
                                              double *saliency, int64_t *k) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_TRY(iss_check(t, r, gamma21, gamma32, min_neighbors, "pcr_target_iss_saliency"));
    if (t->n == 0) return PCR_OK;
    PCR_REQUIRE(eig && saliency && k, "NULL argument");
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t n = (size_t)t->n;
    DevBuf<double> d_eig, d_sal;
    DevBuf<uint32_t> d_k;
    HIP_TRY(d_eig.alloc(3 * n));
    HIP_TRY(d_sal.alloc(n));
    HIP_TRY(d_k.alloc(n));
    static const bool times = env_flag("PCR_ISS_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    iss_saliency_launch<1>(t, r, gamma21, gamma32, min_neighbors, d_eig.p, d_sal.p, d_k.p, nullptr);
    HIP_TRY(hipGetLastError());
    ev.mark(1, ctx->stream);
    HIP_TRY(hipMemcpyAsync(eig, d_eig.p, 8 * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(saliency, d_sal.p, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    PCR_TRY(download_u32_as_i64(ctx, d_k.p, n, k));
    if (ev.on) fprintf(stderr, "pcr_iss_times points %lld saliency_ms %.4f\n", (long long)t->n, ev.ms(0));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_iss_keypoints(pcr_target *t, float r_salient, float r_nonmax, double gamma21, double gamma32, int min_neighbors,
                                               uint8_t *is_keypoint, double *saliency_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_TRY(iss_check(t, r_salient, gamma21, gamma32, min_neighbors, "pcr_target_iss_keypoints"));
    PCR_TRY(iss_check(t, r_nonmax, gamma21, gamma32, min_neighbors, "pcr_target_iss_keypoints"));
    if (t->n == 0) return PCR_OK;
    PCR_REQUIRE(is_keypoint, "NULL argument");
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t n = (size_t)t->n;
    DevBuf<double> d_sal, d_sal_orig;
    DevBuf<uint8_t> d_key;
    HIP_TRY(d_sal.alloc(n));
    HIP_TRY(d_key.alloc(n));
    if (saliency_or_null) HIP_TRY(d_sal_orig.alloc(n));
    static const bool times = env_flag("PCR_ISS_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    iss_saliency_launch<0>(t, r_salient, gamma21, gamma32, min_neighbors, nullptr, d_sal.p, nullptr, saliency_or_null ? d_sal_orig.p : nullptr);
    HIP_TRY(hipGetLastError());
    ev.mark(1, ctx->stream);
    hipLaunchKernelGGL(k_iss_nms, grid_for(t->n, ISS_BLOCK), dim3(ISS_BLOCK), 0, ctx->stream, t->gf, (const PtF *)t->pts,
                       (const uint32_t *)t->cell_start, t->n, r_nonmax, (const double *)d_sal.p, (uint32_t)min_neighbors, d_key.p);
    HIP_TRY(hipGetLastError());
    ev.mark(2, ctx->stream);
    HIP_TRY(hipMemcpyAsync(is_keypoint, d_key.p, n, hipMemcpyDeviceToHost, ctx->stream));
    if (saliency_or_null) HIP_TRY(hipMemcpyAsync(saliency_or_null, d_sal_orig.p, 8 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on) fprintf(stderr, "pcr_iss_times points %lld saliency_ms %.4f nms_ms %.4f\n", (long long)t->n, ev.ms(0), ev.ms(1));
    return PCR_OK;
}
