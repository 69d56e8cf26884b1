// Normals and covariances from a ball: the moments of every point's radius or hybrid neighbourhood within its own cloud.  The
// contract is in include/pcr.h ("radius and hybrid neighbourhoods").
//
//   pcr_target_ball_moments                  count, mean and raw covariance in the caller's order (the seam of the exact test)
//   pcr_target_estimate_normals_radius       fills the target's PtN records, as pcr_target_estimate_normals does
//   pcr_scan_estimate_normals_radius         ScanPayload<3>::estimate over the scan's self-index (pcr_scan_self_index)
//   pcr_target_estimate_covariances_radius   fills the target's GicpRec records, as pcr_target_estimate_covariances does
//   pcr_scan_estimate_covariances_radius     ScanPayload<6>::estimate
//
// One kernel, k_ball_moments<LIST>: one lane = one point in CELL-SORTED order, so the lanes of a wave are spatial neighbours, and
// one rad_ball_walk (radius_device.h), the walk of pcr_radius_query: the set IS what the radius search finds, the point itself
// and its exact duplicates included.  No atomics, the grid depends on n only: two calls return the same bits.
//   LIST 0   the radius set: RadMoments (radius_device.h, k_iss_saliency's sink) sums in the walk's order; the anchor, 9
//            float64 sums and the count stay in registers
//   LIST 1   the hybrid set, max_nn <= KNN_REG_K: the walk covers the whole ball -- it reads bound() once and cannot shrink --
//            and the sink keeps the max_nn best (squared distance, original index) keys in knn_device.h's register list KnnReg,
//            members queued in LDS and inserted for the whole wave when a lane's queue is full; the moments are summed after
//            the walk in list order
//   LIST 2   the same beyond KNN_REG_K with the sorted LDS list KnnList
// What a call wants of the moments is a set of pointers (BallOut); the branches on them are uniform over the launch.
#include "eigen3.h"
#include "gicp_weight.h"
#include "radius_device.h"
#include "scan_payload.h"

extern __shared__ __attribute__((aligned(16))) char ball_smem[];

#define BALL_BLOCK RAD_BLOCK
static_assert(BALL_BLOCK == KNN_BLOCK, "the lists are laid out for blocks of KNN_BLOCK lanes");
#define BALL_REG_BYTES (2 * sizeof(float) * (KNN_QCAP > 0 ? KNN_QCAP : 1) * KNN_BLOCK)

// every pointer may be NULL; "input order": at pt_orig of the record, the order of the array the index was built from
struct BallOut {
    uint32_t *count;         // [n]  input order: members of the set
    double *mean, *cov;      // [3 n], [6 n] input order: the mean and the raw covariance (xx xy xz yy yz zz)
    PtN *pn;                 // [n]  cell-sorted: point + normal records of a target
    float *nrm;              // [3 n] input order: the normal
    float *fcov;             // [6 n] input order: the covariance behind mode / eps (cov6_finish)
    int mode;
    double eps;
};

// the max_nn nearest members of the ball
template <typename LIST>
struct BallListSink {
    float r, b2;
    LIST L;
    float kth;
    uint32_t kth_o;
    __device__ __forceinline__ float bound() const { return b2; }
    __device__ __forceinline__ void offer(float d2f, uint32_t j, uint32_t orig) {
        // (a lane that queues has room: every lane that gets here takes part in the drain some lane of them needs)
        if constexpr (LIST::kQueued) {
            if (__any(L.qn >= KNN_QCAP)) L.flush(kth, kth_o);
        }
        if (d2f <= b2 && rad_member(d2f, r)) L.offer(d2f, j, orig, kth, kth_o);
    }
};

__device__ __forceinline__ void ball_finish(const BallOut &o, const PtF me, int64_t i, const RadMoments &S) {
    const size_t at = (size_t)pt_orig(me);
    double m[3], c[6];
    S.finish(m, c);
    if (o.count) o.count[at] = S.k;
    if (o.mean) {
        o.mean[3 * at] = S.k ? S.ax + m[0] : 0.0; o.mean[3 * at + 1] = S.k ? S.ay + m[1] : 0.0; o.mean[3 * at + 2] = S.k ? S.az + m[2] : 0.0;
    }
    if (o.cov) {
#pragma unroll
        for (int a = 0; a < 6; ++a) o.cov[6 * at + a] = c[a];
    }
    if (o.pn || o.nrm) {
        double nv[3] = {0.0, 0.0, 0.0};
        if (S.k >= 3u) smallest_eigvec3(c, nv);
        if (o.pn) {
            PtN rec;                                // the PlaneICP gather record: point + normal in 32 bytes
            rec.x = me.x; rec.y = me.y; rec.z = me.z; rec.orig = pt_orig(me);
            rec.nx = (float)nv[0]; rec.ny = (float)nv[1]; rec.nz = (float)nv[2]; rec.pad = 0;
            o.pn[i] = rec;
        }
        if (o.nrm) { o.nrm[3 * at] = (float)nv[0]; o.nrm[3 * at + 1] = (float)nv[1]; o.nrm[3 * at + 2] = (float)nv[2]; }
    }
    if (o.fcov) {
        cov6_finish(o.mode, o.eps, c);
#pragma unroll
        for (int a = 0; a < 6; ++a) o.fcov[6 * at + a] = (float)c[a];
    }
}

template <int LIST>
__global__ void __launch_bounds__(BALL_BLOCK) k_ball_moments(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n, float r, int max_nn,
                                                             BallOut o) {
    const int64_t i = (int64_t)blockIdx.x * BALL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    const bool finite = rad_finite(me.x, me.y, me.z);
    RadMoments S;
    S.init(r, pts);
    if (LIST == 0) {
        if (finite) rad_ball_walk(g, pts, cs, me.x, me.y, me.z, r, S);
    } else if (LIST == 1) {
        BallListSink<KnnReg> K;
        K.r = r; K.b2 = rad_bound2(r); K.kth = __int_as_float(0x7f800000); K.kth_o = PCR_NONE;
        K.L.init(max_nn, pts, ball_smem);
        if (finite) rad_ball_walk(g, pts, cs, me.x, me.y, me.z, r, K);
        K.L.flush(K.kth, K.kth_o);
        K.L.for_each([&](int, float, uint32_t js) { S.add(pts[js]); });
    } else {
        BallListSink<KnnList> K;
        K.r = r; K.b2 = rad_bound2(r); K.kth = __int_as_float(0x7f800000); K.kth_o = PCR_NONE;
        K.L = knn_list(ball_smem, max_nn, pts);
        if (finite) rad_ball_walk(g, pts, cs, me.x, me.y, me.z, r, K);
        K.L.for_each([&](int, float, uint32_t js) { S.add(pts[js]); });
    }
    ball_finish(o, me, i, S);
}

// scan payloads between caller and device order (scan_payload.h)
template <int C, bool TO_DEVICE>
__global__ void __launch_bounds__(256) k_ball_perm(const float *__restrict__ in, int64_t n, const uint32_t *__restrict__ order, float *out) {
    payload_perm<C, TO_DEVICE>(in, n, order, out);
}
static const ScanPayload<3> ball_scan_nrm{&pcr_scan::nrm, k_ball_perm<3, true>, k_ball_perm<3, false>};
static const ScanPayload<6> ball_scan_cov{&pcr_scan::cov, k_ball_perm<6, true>, k_ball_perm<6, false>};
// a target's covariance records from the estimate in the caller's order (the layout of gicp.hip's GicpRec: the index's PtF,
// xx xy xz yy | yz zz, padding -- one 64-byte line)
__global__ void __launch_bounds__(256) k_ball_tcov_in(const float *__restrict__ in, int64_t n, const PtF *__restrict__ pts, float4 *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const PtF p = pts[j];
    const float *c = in + 6 * (size_t)pt_orig(p);
    out[4 * j] = p;
    out[4 * j + 1] = make_float4(c[0], c[1], c[2], c[3]);
    out[4 * j + 2] = make_float4(c[4], c[5], 0.f, 0.f);
    out[4 * j + 3] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// PCR_BALL_TIMES=1 (developer, tools/ball_time.py): a launch is bracketed with events (StageTimes) and its milliseconds
// reported on stderr

// r finite and >= 0, 0 <= max_nn <= KNN_MAX_K
static pcr_status ball_check(float r, int max_nn, const char *who) {
    PCR_TRY(check_radius<float>(r, who));
    if (max_nn < 0 || max_nn > KNN_MAX_K) {
        pcr_set_error("invalid argument: %s needs max_nn in [0, %d] (0: the whole ball)", who, KNN_MAX_K);
        return PCR_ERR_INVALID;
    }
    return PCR_OK;
}

// the moments of the n points behind the index (g, pts, cs); enqueued on the context's stream
static pcr_status ball_launch(pcr_context *ctx, const Geom<float> &g, const PtF *pts, const uint32_t *cs, int64_t n, float r, int max_nn,
                              const BallOut &o, const char *who) {
    if (n <= 0) return PCR_OK;
    static const bool times = env_flag("PCR_BALL_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    const dim3 grid = grid_for(n, BALL_BLOCK), block(BALL_BLOCK);
    if (max_nn == 0)
        hipLaunchKernelGGL(k_ball_moments<0>, grid, block, 0, ctx->stream, g, pts, cs, n, r, max_nn, o);
    else if (max_nn <= KNN_REG_K)
        hipLaunchKernelGGL(k_ball_moments<1>, grid, block, BALL_REG_BYTES, ctx->stream, g, pts, cs, n, r, max_nn, o);
    else
        hipLaunchKernelGGL(k_ball_moments<2>, grid, block, 2 * sizeof(float) * (size_t)max_nn * KNN_BLOCK, ctx->stream, g, pts, cs, n, r, max_nn, o);
    HIP_TRY(hipGetLastError());
    ev.mark(1, ctx->stream);
    if (ev.on) fprintf(stderr, "pcr_ball_times %s points %lld max_nn %d moments_ms %.4f\n", who, (long long)n, max_nn, ev.ms(0));
    return PCR_OK;
}

static BallOut ball_out() { return BallOut{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, PCR_COV_RAW, 0.0}; }

extern "C" pcr_status pcr_target_ball_moments(pcr_target *t, float r, int max_nn, int64_t *count, double *mean3, double *cov6) {
    const char *who = "pcr_target_ball_moments";
    PCR_REQUIRE(t && ((count && mean3 && cov6) || t->n == 0), "NULL argument");
    PCR_TRY(ball_check(r, max_nn, who));
    PCR_TRY(check_point_target(t, who));
    if (t->n == 0) return PCR_OK;
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t n = (size_t)t->n;
    DevBuf<uint32_t> d_k;
    DevBuf<double> d_mean, d_cov;
    HIP_TRY(d_k.alloc(n));
    HIP_TRY(d_mean.alloc(3 * n));
    HIP_TRY(d_cov.alloc(6 * n));
    BallOut o = ball_out();
    o.count = d_k.p; o.mean = d_mean.p; o.cov = d_cov.p;
    PCR_TRY(ball_launch(ctx, t->gf, t->pts, t->cell_start, t->n, r, max_nn, o, who));
    HIP_TRY(hipMemcpyAsync(mean3, d_mean.p, 8 * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(cov6, d_cov.p, 8 * 6 * n, hipMemcpyDeviceToHost, ctx->stream));
    return download_u32_as_i64(ctx, d_k.p, n, count);
}

extern "C" pcr_status pcr_target_estimate_normals_radius(pcr_target *t, float r, int max_nn, float *normals_out_or_null,
                                                         int64_t *count_out_or_null) {
    const char *who = "pcr_target_estimate_normals_radius";
    PCR_REQUIRE(t, "NULL argument");
    PCR_TRY(ball_check(r, max_nn, who));
    PCR_TRY(check_point_target(t, who));
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    pcr_target_drop_color(t);       // (colour gradients lie in the tangent planes of the OLD normals)
    if (!t->pn) HIP_TRY(pcr_persist_alloc((void **)&t->pn, sizeof(PtN) * (size_t)(t->n ? t->n : 1)));
    if (t->n == 0) return PCR_OK;
    DevBuf<uint32_t> d_k;
    if (count_out_or_null) HIP_TRY(d_k.alloc((size_t)t->n));
    BallOut o = ball_out();
    o.pn = t->pn; o.count = count_out_or_null ? d_k.p : nullptr;
    PCR_TRY(ball_launch(ctx, t->gf, t->pts, t->cell_start, t->n, r, max_nn, o, who));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (count_out_or_null) PCR_TRY(download_u32_as_i64(ctx, d_k.p, (size_t)t->n, count_out_or_null));
    if (normals_out_or_null) return pcr_target_get_normals(t, normals_out_or_null);
    return PCR_OK;
}

extern "C" pcr_status pcr_target_estimate_covariances_radius(pcr_target *t, float r, int max_nn, int mode, double eps, float *cov_out_or_null,
                                                             int64_t *count_out_or_null) {
    const char *who = "pcr_target_estimate_covariances_radius";
    PCR_REQUIRE(t, "NULL argument");
    PCR_TRY(ball_check(r, max_nn, who));
    PCR_TRY(check_cov_mode(mode, eps));
    PCR_TRY(check_point_target(t, who));
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    if (!t->gcov) HIP_TRY(pcr_persist_alloc((void **)&t->gcov, 64 * (size_t)(t->n ? t->n : 1)));
    if (t->n == 0) return PCR_OK;
    const size_t n = (size_t)t->n;
    DevBuf<float> d_cov;                             // caller order
    DevBuf<uint32_t> d_k;
    HIP_TRY(d_cov.alloc(6 * n));
    if (count_out_or_null) HIP_TRY(d_k.alloc(n));
    BallOut o = ball_out();
    o.fcov = d_cov.p; o.mode = mode; o.eps = eps; o.count = count_out_or_null ? d_k.p : nullptr;
    PCR_TRY(ball_launch(ctx, t->gf, t->pts, t->cell_start, t->n, r, max_nn, o, who));
    hipLaunchKernelGGL(k_ball_tcov_in, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const float *)d_cov.p, t->n, (const PtF *)t->pts,
                       (float4 *)t->gcov);
    HIP_TRY(hipGetLastError());
    if (cov_out_or_null) HIP_TRY(hipMemcpyAsync(cov_out_or_null, d_cov.p, 24 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (count_out_or_null) PCR_TRY(download_u32_as_i64(ctx, d_k.p, n, count_out_or_null));
    return PCR_OK;
}

// the counts of a scan's estimate: device order -> the caller's
__global__ void __launch_bounds__(256) k_ball_count_perm(const uint32_t *__restrict__ in, int64_t n, const uint32_t *__restrict__ order, uint32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[order ? (size_t)order[i] : (size_t)i] = in[i];
}

// what the two scan entry points share behind their checks: the estimate through the payload, the counts beside it
template <int C>
static pcr_status ball_scan_estimate(const ScanPayload<C> &payload, pcr_scan *s, float r, int max_nn, int mode, double eps, float *out_or_null,
                                     int64_t *count_out_or_null, const char *who) {
    pcr_context *ctx = s->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t n = (size_t)s->n;
    DevBuf<uint32_t> d_k, d_kc;                      // device order, caller order
    if (count_out_or_null && n) { HIP_TRY(d_k.alloc(n)); HIP_TRY(d_kc.alloc(n)); }
    PCR_TRY(payload.estimate(s, out_or_null, [&](const pcr_target *idx, float *dst) -> pcr_status {
        BallOut o = ball_out();
        (C == 3 ? o.nrm : o.fcov) = dst;
        o.mode = mode; o.eps = eps; o.count = d_k.p;
        return ball_launch(ctx, idx->gf, idx->pts, idx->cell_start, s->n, r, max_nn, o, who);
    }));
    if (count_out_or_null && n) {
        hipLaunchKernelGGL(k_ball_count_perm, grid_for(s->n, 256), dim3(256), 0, ctx->stream, (const uint32_t *)d_k.p, s->n,
                           (const uint32_t *)s->order, d_kc.p);
        HIP_TRY(hipGetLastError());
        PCR_TRY(download_u32_as_i64(ctx, d_kc.p, n, count_out_or_null));
    }
    return PCR_OK;
}

extern "C" pcr_status pcr_scan_estimate_normals_radius(pcr_scan *s, float r, int max_nn, float *normals_out_or_null, int64_t *count_out_or_null) {
    const char *who = "pcr_scan_estimate_normals_radius";
    PCR_REQUIRE(s, "NULL argument");
    PCR_TRY(ball_check(r, max_nn, who));
    PCR_REQUIRE((!normals_out_or_null && !count_out_or_null) || pcr_scan_knows_order(s), PCR_NEED_ORDER);
    return ball_scan_estimate(ball_scan_nrm, s, r, max_nn, PCR_COV_RAW, 0.0, normals_out_or_null, count_out_or_null, who);
}

extern "C" pcr_status pcr_scan_estimate_covariances_radius(pcr_scan *s, float r, int max_nn, int mode, double eps, float *cov_out_or_null,
                                                           int64_t *count_out_or_null) {
    const char *who = "pcr_scan_estimate_covariances_radius";
    PCR_REQUIRE(s, "NULL argument");
    PCR_TRY(ball_check(r, max_nn, who));
    PCR_TRY(check_cov_mode(mode, eps));
    PCR_REQUIRE((!cov_out_or_null && !count_out_or_null) || pcr_scan_knows_order(s), PCR_NEED_ORDER);
    return ball_scan_estimate(ball_scan_cov, s, r, max_nn, mode, eps, cov_out_or_null, count_out_or_null, who);
}
