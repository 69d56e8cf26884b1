// A pass over a match list, stated once: the three-phase reduce loop, the fold, the ONE place that launches a fold, the host
// driver around it, the pcr_pass_fn around that and the entry points in front of it.  Behind GICP, VGICP, SymmetricICP and
// ColoredICP (gicp.hip, vgicp.hip, symm.hip, color.hip) and behind VGICP's direct voxel neighbourhoods (vgicp_direct.hip), whose
// "match list" is a lookup inside the kernel.  A unit is a SIDE and a UNIT; it keeps its own __global__ one-liners (k_gicp_* /
// k_vgicp_* / k_symm_* / k_color_* / k_vgicp_direct*), its *_W and its extern "C" names, each ONE call of a template here.
//
// A UNIT (GicpUnit, VgicpUnit, SymmUnit, ColorUnit; DirectUnit<NB>, derived from VgicpUnit) names what the entry points of a
// unit differ in -- and nothing else:
//   Side                      its SIDE
//   Params, check(&p, raw...) the checked per-call parameter block, for plain and robust calls alike, and the check that fills
//                             it from the caller's own parameter (MatchUnit: none; symm.hip: min_cos; color.hip: the two roots;
//                             vgicp_direct.hip: neighbors, checked and carried by the instantiation)
//   kind                      the search: PCR_ICP, or PCR_VPLANE
//   payloads(t, s)            PCR_ERR_NO_TARGET and its message where target or scan lack what the pass reads
//   no_match(t, s, max_dist, &none)                 MatchUnit: never; vgicp_side.h: a target with no kept voxel
//   matches(&a, &nn, t, s, kind, T, max_dist, flags, caller_order)
//                             where the correspondences of a call come from: fills LinArgs and the match buffer, or refuses.
//                             MatchUnit: the full search of `kind` (pass.hip: pcr_rows_search) -- the four units do not mention
//                             it; vgicp_direct.hip: the lookup data and the LinArgs of the call, no launch
//   side(t, s, p)             the SIDE of a call, everything but rows; made behind `matches`
//   reduce, robust, fold, residuals                 the four __global__ one-liners, launched through launch_side, which a unit
//                             whose kernels take the parts of its SIDE as separate arguments overloads
//   keys, adaptive                                  the two of the adaptive pass: a key per scan point, the reduce behind the selection
//   reduce_range, robust_range, residuals_range, adaptive_range     their roctx range names
//   times(), print_times(ev, n)                     MatchUnit: no bracket; vgicp_direct.hip: PCR_DIRECT_TIMES and its line
//
// A SIDE is a unit's kernel-argument struct (GicpArgs, VgicpArgs, SymmArgs, ColorArgs): its arrays, its parameters, rows -- and
//   Scan                      what phase A carries per scan point beside index and coordinates
//   load(i, Scan&)            the loads of scan point i (device order); nothing else
//   Match                     what phase B carries per correspondence
//   gather(a, j, Match&)      the loads of one match at cell-sorted index j; nothing else
//   each(a, P, x, y, z, tx, ty, tz, scan, match, f)
//                             what ONE correspondence yields, stated once: residual and gates, then f on its row(s) (J, r) or on
//                             (M, d); nothing is handed to f when a gate drops the correspondence; (tx, ty, tz) = xform(P, x, y, z)
//   Plain, Weighted, Resid    the three f: the sums of the plain pass, the sums under a robust weight, the squared residual(s)
//   M                         squared residuals per correspondence (1; ColoredICP 2)
//   add(acc, a, P, x, y, z, tx, ty, tz, scan, match)
//                             each with Plain.  RobustSide<SIDE> is the SIDE whose add is each with Weighted
#pragma once

#include <math.h>

#include "host_util.h"
#include "pass_device.h"
#include "select.h"

// ---- robust weights (include/pcr.h: "robust kernels") ---------------------------------------------------------------------
// kind, c and c2 = c * c (taken once on the host) travel by value
struct RobustK {
    int kind;
    double c, c2;
};

// w(s): float64, nothing contracted.  The switch is wave-uniform: kind is a kernel argument
__device__ __forceinline__ double robust_weight(const RobustK &rb, double s) {
    switch (rb.kind) {
    case PCR_ROBUST_HUBER: return s <= rb.c2 ? 1.0 : rb.c / __builtin_sqrt(s);
    case PCR_ROBUST_CAUCHY: return 1.0 / (1.0 + s / rb.c2);
    case PCR_ROBUST_TUKEY: { const double u = 1.0 - s / rb.c2; return s <= rb.c2 ? u * u : 0.0; }
    default: { const double l = rb.c2 / (rb.c2 + s); return l * l; }                  // PCR_ROBUST_GM
    }
}

// acc_rank1 under a weight: Jw = w J and rw = w r, one product each, then acc_rank1's fmas with them on the left
__device__ __forceinline__ void acc_rank1_w(double *acc, const double J[6], double r, double w) {
    double Jw[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) Jw[i] = w * J[i];
    int p = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { acc[p] = fma(Jw[i], J[j], acc[p]); ++p; }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] = fma(Jw[i], r, acc[21 + i]);
    acc[27] = fma(w * r, r, acc[27]);
    acc[28] += 1.0;
}

// The three f of a SIDE of rows (symm.hip, color.hip): f(row, J, r), rows in order.  acc_rank1 counts rows and out[28] counts
// correspondences: a row past the first puts the count back
struct RowsPlain {
    double *acc;
    __device__ __forceinline__ RowsPlain(double *acc_, const PoseK &, float, float, float) : acc(acc_) {}
    __device__ __forceinline__ void operator()(int row, const double J[6], double r) const {
        const double count = acc[28];
        acc_rank1(acc, J, r);
        if (row > 0) acc[28] = count;
    }
};
struct RowsWeighted {
    double *acc;
    const RobustK &rb;
    __device__ __forceinline__ RowsWeighted(double *acc_, const PoseK &, float, float, float, const RobustK &rb_) : acc(acc_), rb(rb_) {}
    __device__ __forceinline__ void operator()(int row, const double J[6], double r) const {
        const double count = acc[28];
        acc_rank1_w(acc, J, r, robust_weight(rb, r * r));
        if (row > 0) acc[28] = count;
    }
};
struct RowsResid {
    double *s;
    __device__ __forceinline__ RowsResid(double *s_, const PoseK &, float, float, float) : s(s_) {}
    __device__ __forceinline__ void operator()(int row, const double *, double r) const { s[row] = r * r; }
};

// the SIDE whose add weighs every correspondence
template <typename SIDE>
struct RobustSide : SIDE {
    RobustK rb;
    __device__ __forceinline__ void add(double *acc, const LinArgs &a, const PoseK &P, float x, float y, float z, float tx, float ty, float tz,
                                        const typename SIDE::Scan &s, const typename SIDE::Match &m) const {
        this->each(a, P, x, y, z, tx, ty, tz, s, m, typename SIDE::Weighted(acc, P, x, y, z, rb));
    }
};

// The SIDE of the adaptive pass (include/pcr.h: "adaptive pass"): RobustSide with the kernel read from what the selection left
// on the device (select.h: w_kind, w_c, w_c2) by the kernel before the loop (adaptive_side) -- wave-uniform by construction and
// kept in scalar registers, as the by-value RobustK of the robust kernels is.  The variants of the pass are data there: a trim
// is the kernel whose weight is exactly 1 over a match list from which the selection dropped the keys above tau, the limit for
// c -> 0 is Huber's at c = 0
template <typename SIDE>
struct AdaptiveSide : RobustSide<SIDE> {
    const SelectState *st;
};
template <typename SIDE>
__device__ __forceinline__ AdaptiveSide<SIDE> adaptive_side(AdaptiveSide<SIDE> sd) {
    sd.rb.kind = __builtin_amdgcn_readfirstlane(sd.st->w_kind);
    sd.rb.c = uniform_f64(sd.st->w_c); sd.rb.c2 = uniform_f64(sd.st->w_c2);
    return sd;
}

// W points per lane in flight, the phases of reduce_stream (pass_device.h):
//   phase A  index, coordinates and Scan of all W points.  A point past the end reads the lane's first point.
//   phase B  the W matches.  No match: element 0 through a select on the index -- always there -- and skipped in phase C;
//            no branch between the gathers.
//   phase C  SIDE::add -- in index order.
// Fold: wave shuffles in a fixed order, LDS across the waves in wave order, ONE row of 32 doubles per block with plain
// stores (block_store_partials).  No tickets, no atomics, no in-launch hand-off.
template <int W, typename SIDE>
__device__ __forceinline__ void match_reduce(const LinArgs &a, const SIDE &sd) {
    const PoseK &P = a.hp;                           // host-driven: the pose came by value
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x; t0 < a.n; t0 += W * stride) {
        uint32_t j[W];
        float x[W], y[W], z[W];
        typename SIDE::Scan sc[W];
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
            sd.load(i, sc[u]);
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
            xform(P, x[u], y[u], z[u], tx, ty, tz);
            sd.add(acc, a, P, x[u], y[u], z[u], tx, ty, tz, sc[u], m[u]);
        }
    }
    block_store_partials<false>(acc, sd.rows);
}

// one block: thread e < 29 adds rows 0 .. nb-1 in order.  The kernel boundary is the only ordering between the two launches;
// the grid depends on n and the device only, so two calls return the same bits.
__device__ __forceinline__ void match_fold(const double *__restrict__ rows, int nb, double *out) {
    const int e = threadIdx.x;
    if (e >= 29) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += rows[(size_t)b * 32 + e];
    out[e] = s;
}

// The sibling of match_reduce that writes instead of accumulating: SIDE::M squared residuals per scan point, +inf where the
// point has no match or a gate drops it, at the point's CALLER index through `order` (pcr_scan::order; NULL: the device order
// is the caller's), as k_rows scatters.  One point per lane and trip: nothing is folded, nothing depends on the grid.
// KEY: the key of the adaptive pass instead -- ONE double per point, the sum of its SIDE::M squared residuals in row order
// (ColoredICP: s_G + s_C, one addition), in device order; `order` is not read
template <typename SIDE, bool KEY = false>
__device__ __forceinline__ void match_residuals(const LinArgs &a, const SIDE &sd, const uint32_t *__restrict__ order, double *__restrict__ out) {
    const PoseK &P = a.hp;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
        double s[SIDE::M];
#pragma unroll
        for (int k = 0; k < SIDE::M; ++k) s[k] = (double)INFINITY;
        const uint32_t j = a.nn_j[i];
        if (j != PCR_NONE) {
            const float x = a.sx[i], y = a.sy[i], z = a.sz[i];
            typename SIDE::Scan sc;
            typename SIDE::Match m;
            sd.load(i, sc);
            sd.gather(a, j, m);
            float tx, ty, tz;
            xform(P, x, y, z, tx, ty, tz);
            sd.each(a, P, x, y, z, tx, ty, tz, sc, m, typename SIDE::Resid(s, P, x, y, z));
        }
        if constexpr (KEY) {
            double key = s[0];
#pragma unroll
            for (int k = 1; k < SIDE::M; ++k) key = key + s[k];
            out[i] = key;
        } else {
            const int64_t dest = order ? (int64_t)order[i] : i;
#pragma unroll
            for (int k = 0; k < SIDE::M; ++k) out[SIDE::M * dest + k] = s[k];
        }
    }
}

// How a kernel of the (LinArgs, SIDE, more...) shape is launched, on blocks of 256.  A unit whose kernels take the parts of its
// SIDE as separate arguments overloads this for its kernel type (vgicp_direct.hip)
template <typename SIDE, typename... More>
static void launch_side(void (*kernel)(const LinArgs, const SIDE, More...), dim3 grid, hipStream_t stream, const LinArgs &a, const SIDE &sd,
                        More... more) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, a, sd, more...);
}

// The ONE place that launches a fold: `reduce` over sd on nb blocks of 256, then `fold` -- one block -- of sd.rows into sums.
// ev, where a unit hands one in: a mark before the reduce, one between the two launches, one after the fold
template <typename KERNEL, typename SIDE>
static void launch_reduce_fold(pcr_context *ctx, KERNEL reduce, void (*fold)(const double *, int, double *),
                               const LinArgs &a, const SIDE &sd, int nb, double *sums, StageTimes *ev = nullptr) {
    if (ev) ev->mark(0, ctx->stream);
    launch_side(reduce, dim3((unsigned)nb), ctx->stream, a, sd);
    if (ev) ev->mark(1, ctx->stream);
    hipLaunchKernelGGL(fold, dim3(1), dim3(64), 0, ctx->stream, (const double *)sd.rows, nb, sums);
    if (ev) ev->mark(2, ctx->stream);
}

// reduce + fold + 29 doubles back behind the matches of `a`: one stream synchronisation, device blocks from the context's
// block cache.  sd comes with everything but rows set.
template <typename KERNEL, typename SIDE>
static pcr_status match_launch(pcr_context *ctx, const char *range_name, KERNEL reduce,
                               void (*fold)(const double *, int, double *), const LinArgs &a, SIDE sd, int64_t n, double out[29], StageTimes *ev) {
    const int nb = choose_blocks(ctx, n);            // n and the device only
    DevBuf<double> rows, sums;
    HIP_TRY(rows.alloc(32 * (size_t)nb)); HIP_TRY(sums.alloc(32));
    sd.rows = rows.p;
    {
        RoctxRange range(range_name);
        launch_reduce_fold(ctx, reduce, fold, a, sd, nb, sums.p, ev);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sums.p, 29 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// ---- the entry points, stated once: a UNIT and the templates over it ------------------------------------------------------
// What a UNIT leaves unsaid (it derives from this): no parameter of its own between max_dist and the flags, no target
// without a match, its correspondences from the full search of its kind, no bracket around its launches
struct MatchUnit {
    struct Params {};
    static pcr_status check(Params *) { return PCR_OK; }
    static pcr_status no_match(const pcr_target *, const pcr_scan *, double, bool *none) { *none = false; return PCR_OK; }
    // where the correspondences of a call come from: fills *a (and the match buffer behind a->nn_j), or refuses.  The full
    // search of `kind` (pass.hip: pcr_rows_search) into a match buffer of the call
    static pcr_status matches(LinArgs *a, DevBuf<uint32_t> *nn, pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist,
                              unsigned flags, bool caller_order) {
        return pcr_rows_search(a, nn, t, s, kind, T, max_dist, flags, caller_order);
    }
    // events around reduce and fold of a linearize / align pass (launch_reduce_fold), and the line that reports them
    static bool times() { return false; }
    static void print_times(StageTimes &, int64_t) {}
};

// the caller's pcr_robust -> RobustK.  NULL or PCR_ROBUST_NONE: the plain pass (kind 0; the scale is not read)
static inline pcr_status robust_args(const pcr_robust *rb, RobustK *k) {
    k->kind = PCR_ROBUST_NONE; k->c = 1.0; k->c2 = 1.0;
    if (!rb || rb->kind == PCR_ROBUST_NONE) return PCR_OK;
    PCR_REQUIRE(rb->kind >= PCR_ROBUST_HUBER && rb->kind <= PCR_ROBUST_GM, "robust kind must be one of PCR_ROBUST_*");
    const double c = rb->scale, c2 = c * c;
    PCR_REQUIRE(c > 0.0 && isfinite(c) && c2 > 0.0 && isfinite(c2), "robust scale must be finite and > 0, and so must its square");   // (false for NaN)
    k->kind = rb->kind; k->c = c; k->c2 = c2;
    return PCR_OK;
}

// The pcr_pass_fn of a unit (`kind` is not read: the matches are U::kind's).  params: what U::check made of the caller's own
// parameter, and the checked kernel of the call -- PCR_ROBUST_NONE: the plain kernel, the plain bits
template <typename U>
struct MatchParams {
    typename U::Params unit;
    RobustK rb;
};
// U::matches, 29 zeros, and -- for a scan with points -- the SIDE of the call and match_launch of the call's kernel over it
template <typename U>
static pcr_status match_run(pcr_target *t, pcr_scan *s, int, const double T[16], double max_dist, unsigned flags, const void *params, double out[29]) {
    const MatchParams<U> *p = (const MatchParams<U> *)params;
    PCR_TRY(U::payloads(t, s));
    bool none;
    PCR_TRY(U::no_match(t, s, max_dist, &none));
    LinArgs a;
    DevBuf<uint32_t> nn;
    if (!none) PCR_TRY(U::matches(&a, &nn, t, s, U::kind, T, max_dist, flags, false));
    for (int i = 0; i < 29; ++i) out[i] = 0.0;
    if (none || s->n == 0) return PCR_OK;
    const typename U::Side sd = U::side(t, s, p->unit);
    StageTimes ev;
    HIP_TRY(ev.init(U::times()));
    if (p->rb.kind == PCR_ROBUST_NONE) PCR_TRY(match_launch(t->ctx, U::reduce_range, U::reduce, U::fold, a, sd, s->n, out, ev.on ? &ev : nullptr));
    else PCR_TRY(match_launch(t->ctx, U::robust_range, U::robust, U::fold, a, RobustSide<typename U::Side>{sd, p->rb}, s->n, out, ev.on ? &ev : nullptr));
    if (ev.on) U::print_times(ev, s->n);
    return PCR_OK;
}

// The three entry points of a unit behind its five extern "C" names: rb is NULL from the plain ones, raw is the caller's own
// parameter of the unit (none, min_cos, lambda_geometric, neighbors).  The order of refusals, the same for every unit: NULL arguments,
// the unit's parameter, the kernel, (residuals) a scan that knows the caller's order, the payloads, what the search refuses.
// A refused call writes nothing
template <typename U, typename... Raw>
static pcr_status match_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_robust *rb, unsigned flags,
                                  double out[29], Raw... raw) {
    PCR_REQUIRE(t && s && T && out, "NULL argument");
    MatchParams<U> p;
    PCR_TRY(U::check(&p.unit, raw...));
    PCR_TRY(robust_args(rb, &p.rb));
    CtxScope scope(t->ctx);
    return match_run<U>(t, s, U::kind, T, max_dist, flags, &p, out);
}

// the host-driven Gauss-Newton loop of pcr_align (api.hip: pcr_align_host_loop) over the pass: same gn_step, same trace rows
template <typename U, typename... Raw>
static pcr_status match_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist, const pcr_robust *rb,
                              unsigned flags, double T_out[16], int *iterations, double *trace_or_null, Raw... raw) {
    PCR_REQUIRE(t && s && T_init && T_out, "NULL argument");
    MatchParams<U> p;
    PCR_TRY(U::check(&p.unit, raw...));
    PCR_TRY(robust_args(rb, &p.rb));
    CtxScope scope(t->ctx);
    return pcr_align_host_loop(match_run<U>, t, s, U::kind, &p, T_init, max_iter, tol, max_dist, flags, T_out, iterations, trace_or_null);
}

// U::matches, as match_run, and the residual kernel into Side::M doubles per scan point in the caller's order; +inf for every
// point of a target without a match, whatever else
template <typename U, typename... Raw>
static pcr_status match_residuals_entry(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double *s_out, Raw... raw) {
    PCR_REQUIRE(t && s && T && (s_out || s->n == 0), "NULL argument");
    typename U::Params p;
    PCR_TRY(U::check(&p, raw...));
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    pcr_context *ctx = t->ctx;
    CtxScope scope(ctx);
    PCR_TRY(U::payloads(t, s));
    bool none;
    PCR_TRY(U::no_match(t, s, max_dist, &none));
    const size_t count = (size_t)U::Side::M * (size_t)s->n;
    if (none) {
        for (size_t i = 0; i < count; ++i) s_out[i] = (double)INFINITY;
        return PCR_OK;
    }
    LinArgs a;
    DevBuf<uint32_t> nn;
    PCR_TRY(U::matches(&a, &nn, t, s, U::kind, T, max_dist, flags, true));
    if (s->n == 0) return PCR_OK;
    const typename U::Side sd = U::side(t, s, p);
    DevBuf<double> d;
    HIP_TRY(d.alloc(count));
    {
        RoctxRange range(U::residuals_range);
        launch_side(U::residuals, dim3((unsigned)choose_blocks(ctx, s->n)), ctx->stream, a, sd, (const uint32_t *)s->order, d.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s_out, d.p, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}


// ---- the adaptive pass (include/pcr.h: "adaptive pass") --------------------------------------------------------------------
// the caller's pcr_adaptive, checked
static inline pcr_status adaptive_args(const pcr_adaptive *ad, pcr_adaptive *k) {
    PCR_REQUIRE(ad->kind >= PCR_ROBUST_HUBER && ad->kind <= PCR_ROBUST_TRIM, "adaptive kind must be PCR_ROBUST_HUBER .. PCR_ROBUST_TRIM");
    PCR_REQUIRE(ad->quantile > 0.0 && ad->quantile <= 1.0, "adaptive quantile must be in (0, 1]");                         // (false for NaN)
    PCR_REQUIRE(ad->kind == PCR_ROBUST_TRIM || (ad->factor > 0.0 && isfinite(ad->factor)), "adaptive factor must be finite and > 0");
    *k = *ad;
    return PCR_OK;
}

// (m = 0, and what a pass without a launch returns)
static inline void adaptive_nothing(double out[29], double stats[4]) {
    for (int i = 0; i < 29; ++i) out[i] = 0.0;
    stats[0] = (double)INFINITY; stats[1] = stats[2] = stats[3] = 0.0;
}

// What a call hands to every pass: the unit's block, the checked kernel, and -- from *_align_adaptive -- where the stats of
// the next pass go (4 doubles per pass, advanced by the pass)
template <typename U>
struct AdaptiveParams {
    typename U::Params unit;
    pcr_adaptive ad;
    mutable double *stats_rows;
};

// matches -> key -> select (-> drop, under PCR_ROBUST_TRIM: the correspondences whose stored key is above tau leave the match
// list of the call) -> reduce -> fold, and 29 + 5 doubles back: one stream synchronisation.  out[28] is m, the number of keys
// < +inf, which is what the reduce counts -- but for a trim, where it counts the kept ones: n_le by construction
template <typename U>
static pcr_status adaptive_pass(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, const AdaptiveParams<U> &p,
                                double out[29], double stats[4]) {
    PCR_TRY(U::payloads(t, s));
    bool none;
    PCR_TRY(U::no_match(t, s, max_dist, &none));
    if (none) { adaptive_nothing(out, stats); return PCR_OK; }
    LinArgs a;
    DevBuf<uint32_t> nn;
    PCR_TRY(U::matches(&a, &nn, t, s, U::kind, T, max_dist, flags, false));
    adaptive_nothing(out, stats);
    if (s->n == 0) return PCR_OK;
    pcr_context *ctx = t->ctx;
    const int nb = choose_blocks(ctx, s->n);         // n and the device only
    DevBuf<double> keys, rows, sums;
    DevBuf<SelectState> st;
    HIP_TRY(keys.alloc((size_t)s->n)); HIP_TRY(rows.alloc(32 * (size_t)nb)); HIP_TRY(sums.alloc(40)); HIP_TRY(st.alloc(1));
    const typename U::Side sd = U::side(t, s, p.unit);
    AdaptiveSide<typename U::Side> asd{{sd, RobustK{PCR_ROBUST_HUBER, 0.0, 0.0}}, st.p};
    asd.rows = rows.p;
    // PCR_ADAPTIVE_TIMES=1 (developer, tools/adaptive_time.py): events around the key kernel and the selection, the two phases
    // the pass has beyond the robust one; their milliseconds on stderr
    static const bool times = env_flag("PCR_ADAPTIVE_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    {
        RoctxRange range(U::adaptive_range);
        ev.mark(0, ctx->stream);
        hipLaunchKernelGGL(U::keys, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a, sd, keys.p);
        ev.mark(1, ctx->stream);
        PCR_TRY(pcr_select_launch(ctx, keys.p, s->n, p.ad.quantile, 0, p.ad.kind, p.ad.factor, st.p, sums.p + 32));
        if (p.ad.kind == PCR_ROBUST_TRIM) PCR_TRY(pcr_select_drop_launch(ctx, keys.p, s->n, st.p, nn.p, PCR_NONE));
        ev.mark(2, ctx->stream);
        launch_reduce_fold(ctx, U::adaptive, U::fold, a, asd, nb, sums.p);
    }
    HIP_TRY(hipGetLastError());
    double h[37];
    HIP_TRY(hipMemcpyAsync(h, sums.p, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on) fprintf(stderr, "pcr_adaptive_times %s n %lld keys_ms %.4f select_ms %.4f\n", U::adaptive_range, (long long)s->n, ev.ms(0), ev.ms(1));
    for (int i = 0; i < 29; ++i) out[i] = h[i];
    for (int i = 0; i < 4; ++i) stats[i] = h[32 + i];
    out[28] = h[36];
    return PCR_OK;
}

// the pcr_pass_fn of the adaptive pass
template <typename U>
static pcr_status adaptive_run(pcr_target *t, pcr_scan *s, int, const double T[16], double max_dist, unsigned flags, const void *params, double out[29]) {
    const AdaptiveParams<U> *p = (const AdaptiveParams<U> *)params;
    double stats[4];
    PCR_TRY(adaptive_pass<U>(t, s, T, max_dist, flags, *p, out, stats));
    if (p->stats_rows) {
        for (int i = 0; i < 4; ++i) p->stats_rows[i] = stats[i];
        p->stats_rows += 4;
    }
    return PCR_OK;
}

// The two entry points of a unit behind its *_linearize_adaptive and *_align_adaptive: the order of refusals of
// match_linearize, the adaptive kernel in the place of the robust one
template <typename U, typename... Raw>
static pcr_status match_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_adaptive *ad, unsigned flags,
                                           double out[29], double stats[4], Raw... raw) {
    PCR_REQUIRE(t && s && T && out && stats && ad, "NULL argument");
    AdaptiveParams<U> p;
    PCR_TRY(U::check(&p.unit, raw...));
    PCR_TRY(adaptive_args(ad, &p.ad));
    p.stats_rows = nullptr;
    CtxScope scope(t->ctx);
    double o[29], st[4];                             // (a pass refused behind the search writes nothing)
    PCR_TRY(adaptive_pass<U>(t, s, T, max_dist, flags, p, o, st));
    for (int i = 0; i < 29; ++i) out[i] = o[i];
    for (int i = 0; i < 4; ++i) stats[i] = st[i];
    return PCR_OK;
}

template <typename U, typename... Raw>
static pcr_status match_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                       const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations, double *trace_or_null,
                                       double *stats_or_null, Raw... raw) {
    PCR_REQUIRE(t && s && T_init && T_out && ad, "NULL argument");
    AdaptiveParams<U> p;
    PCR_TRY(U::check(&p.unit, raw...));
    PCR_TRY(adaptive_args(ad, &p.ad));
    p.stats_rows = stats_or_null;
    CtxScope scope(t->ctx);
    return pcr_align_host_loop(adaptive_run<U>, t, s, U::kind, &p, T_init, max_iter, tol, max_dist, flags, T_out, iterations, trace_or_null);
}
