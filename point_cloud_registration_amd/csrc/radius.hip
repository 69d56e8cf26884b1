// Exact fixed-radius search over a point target's cell grid, and the mean k-NN distance of a cloud's own points.
//
//   pcr_radius_count / _query        float32 queries against the float32 records (gf / pts)
//   pcr_radius_count_dd / _query_dd  float64 queries against the float64 coordinates (gq / pts64)
//   pcr_knn_mean_distance            k_knn_mean_dist<REG>: knn_self (knn_device.h) with its own finish, as k_gicp_cov / k_knn_normals
//
// One lane = one query, no atomics, the grid depends on the query count only.  k_radius<Real, MODE> walks the cell box of the
// query's ball: MODE 0 counts the members, MODE 1 writes them into the lane's own segment [off[i], off[i + 1]) of the
// caller's CSR layout, every store guarded by the segment's length; a lane that finds more or fewer members than its segment
// holds raises one flag word (a plain store, every lane the same value), which the host reads before it copies anything out.
//
// Membership is decided by the distance pcr_knn_query / pcr_knn_query_f64 would report for the pair:
//   float32   d2 = dist2_f32(q - p) (nn_device.h), member iff __builtin_sqrtf(d2) <= r
//   float64   d2 = (dx*dx + dy*dy) + dz*dz, no contraction, member iff sqrt(d2) <= r
// so r == 0 finds coincident points and a query with a non-finite coordinate finds nothing.
//
// Each segment is then ordered by (d2, original index) ascending -- the k-NN's order, by d2 and not by the rounded distance:
//   float32   one key (bits(d2) << 32) | orig per entry, rocprim::segmented_radix_sort_keys, k_radius_unpack
//   float64   two stable segmented passes: by original index, then by the bits of d2
// Keys are unique within a segment (float32) or tied only between passes that are stable (float64): two calls return the
// same bits.
//
// The float64 walk is s64_ball_walk (seam64_device.h) with a counting / emitting sink.  The float32 walk (radius_device.h,
// shared with fpfh.hip) has its form: slabs, rows skipped by their (y, z) gap, each row's x range clipped by sqrt(B - dyz2) + slack, cells clamped into the grid,
// records fetched KNN_BATCH at a time and none past the end of a range offered (knn_scan_range's rule).  A ball that misses
// the grid box returns before the first row look-up: nothing here counts rings from a far query's own cell (seam64.hip).
//
// Device memory: a call holds at most PCR_RADIUS_CHUNK entries (default 2^26) at a time; queries are taken in chunks of
// consecutive queries whose segments fit, a single larger query as a chunk of its own.  Entries never move between
// segments, so the results do not depend on the chunking.
#include <stdlib.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "radius_device.h"
#include "seam64_device.h"

extern __shared__ __attribute__((aligned(16))) char rad_smem[];

// ---- the sinks (membership: rad_member / rad_bound2, radius_device.h) ---------------------------------------------------------
__device__ __forceinline__ uint64_t rad_key(float d2, uint32_t o) { return ((uint64_t)__float_as_uint(d2) << 32) | o; }
__device__ __forceinline__ uint64_t rad_key(double d2, uint32_t) { return (uint64_t)__double_as_longlong(d2); }

template <typename Real, int MODE>
struct RadSink {
    Real r, b2;
    uint32_t cnt, len;
    uint64_t *keys;      // the lane's segment: float32 (bits(d2) << 32) | orig; float64 bits(d2) ...
    uint32_t *vals;      // ... and orig (float64 only)
    __device__ __forceinline__ Real bound() const { return b2; }
    __device__ __forceinline__ void offer(Real d2, uint32_t, uint32_t o) {
        if (d2 <= b2 && rad_member(d2, r)) {                               // (NaN fails the pre-test)
            if (MODE == 1 && cnt < len) {
                keys[cnt] = rad_key(d2, o);
                if (sizeof(Real) == 8) vals[cnt] = o;
            }
            ++cnt;
        }
    }
};

// ---- the float64 walk (the float32 one: radius_device.h) ------------------------------------------------------------------
template <typename SINK>
__device__ __forceinline__ void rad_ball_walk(const Geom<double> &g, const PtD *__restrict__ pts, const uint32_t *__restrict__ cs,
                                              double qx, double qy, double qz, double r, SINK &S) {
    s64_ball_walk(g, pts, cs, qx, qy, qz, r * 1.0000001 + g.slack, S);
}

template <typename Real> struct RadPt;
template <> struct RadPt<float> { typedef PtF type; };
template <> struct RadPt<double> { typedef PtD type; };

// MODE 0: count[i] = members of query i.  MODE 1: the members into keys / vals at [off[i], off[i + 1]) in walk order; *flag = 1
// when a lane's count is not its segment's length.
template <typename Real, int MODE>
__global__ void __launch_bounds__(RAD_BLOCK) k_radius(Geom<Real> g, const typename RadPt<Real>::type *pts, const uint32_t *cs, const Real *q,
                                                      int64_t m, Real r, int64_t *count, const uint32_t *off, uint64_t *keys, uint32_t *vals,
                                                      uint32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * RAD_BLOCK + threadIdx.x;
    if (i >= m) return;
    const Real qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
    RadSink<Real, MODE> S;
    S.r = r; S.b2 = rad_bound2(r); S.cnt = 0; S.len = 0; S.keys = nullptr; S.vals = nullptr;
    if (MODE == 1) {
        const uint32_t o = off[i];
        S.len = off[i + 1] - o;
        S.keys = keys + o;
        S.vals = vals ? vals + o : nullptr;
    }
    if (rad_finite(qx, qy, qz)) rad_ball_walk(g, pts, cs, qx, qy, qz, r, S);
    if (MODE == 0) count[i] = (int64_t)S.cnt;
    else if (S.cnt != S.len) *flag = 1u;
}

// sorted keys -> (distance, original index)
__global__ void __launch_bounds__(256) k_radius_unpack(const uint64_t *__restrict__ keys, int64_t n, float *dist, int64_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    dist[i] = __builtin_sqrtf(__uint_as_float((uint32_t)(k >> 32)));
    idx[i] = (int64_t)(uint32_t)k;
}
__global__ void __launch_bounds__(256) k_radius_unpack_dd(const uint64_t *__restrict__ d2, const uint32_t *__restrict__ orig, int64_t n,
                                                          double *dist, int64_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    dist[i] = __builtin_sqrt(__longlong_as_double((long long)d2[i]));
    idx[i] = (int64_t)orig[i];
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// entries a call holds on the device at a time (PCR_RADIUS_CHUNK, read once; unset or below 1: 2^26)
static int64_t radius_budget() {
    static const int64_t v = env_i64("PCR_RADIUS_CHUNK", 0, 0, INT64_MAX);
    return v >= 1 ? v : (int64_t)1 << 26;
}
// PCR_RADIUS_TIMES=1 (developer, tools/radius_time.py): a count call brackets its kernel, a query call fill / sort / unpack of
// every chunk, with events (StageTimes) and reports their milliseconds on stderr

template <typename Real> struct RadTarget;
template <> struct RadTarget<float> {
    static const Geom<float> &geom(const pcr_target *t) { return t->gf; }
    static const PtF *pts(const pcr_target *t) { return t->pts; }
};
template <> struct RadTarget<double> {
    static const Geom<double> &geom(const pcr_target *t) { return t->gq; }
    static const PtD *pts(const pcr_target *t) { return t->pts64; }
};

template <typename Real>
static pcr_status radius_check(const pcr_target *t, Real r, const char *who) {
    PCR_TRY(check_point_target(t, who));
    if (sizeof(Real) == 8 && t->n > 0 && t->pts64 == nullptr) {
        pcr_set_error("invalid argument: %s needs a point target with float64 coordinates (pcr_target_points_set_f64)", who);
        return PCR_ERR_INVALID;
    }
    return check_radius<Real>(r, who);
}

template <typename Real>
static void radius_launch_count(pcr_target *t, const Real *d_q, int64_t m, Real r, int64_t *d_count) {
    hipLaunchKernelGGL((k_radius<Real, 0>), grid_for(m, RAD_BLOCK), dim3(RAD_BLOCK), 0, t->ctx->stream, RadTarget<Real>::geom(t), RadTarget<Real>::pts(t),
                       (const uint32_t *)t->cell_start, d_q, m, r, d_count, (const uint32_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                       (uint32_t *)nullptr);
}

template <typename Real>
static pcr_status radius_count(pcr_target *t, const Real *q, int64_t m, Real r, int64_t *count, const char *who) {
    PCR_REQUIRE(t && (q || m == 0) && (count || m == 0), "NULL argument");
    PCR_REQUIRE(m >= 0, "negative query count");
    PCR_TRY(radius_check<Real>(t, r, who));
    if (m == 0) return PCR_OK;
    if (t->n == 0) { for (int64_t i = 0; i < m; ++i) count[i] = 0; return PCR_OK; }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    DevBuf<Real> d_q;
    DevBuf<int64_t> d_count;
    HIP_TRY(d_q.alloc(3 * (size_t)m));
    HIP_TRY(d_count.alloc((size_t)m));
    HIP_TRY(hipMemcpyAsync(d_q.p, q, sizeof(Real) * 3 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    static const bool times = env_flag("PCR_RADIUS_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    radius_launch_count<Real>(t, d_q.p, m, r, d_count.p);
    HIP_TRY(hipGetLastError());
    ev.mark(1, ctx->stream);
    HIP_TRY(hipMemcpyAsync(count, d_count.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on) fprintf(stderr, "pcr_radius_times %s queries %lld count_ms %.4f\n", who, (long long)m, ev.ms(0));
    return PCR_OK;
}

// order the E entries of a chunk's segments by (d2, original index); *keys_out / *vals_out: where the result lies
static pcr_status radius_sort(pcr_context *ctx, bool f64, uint64_t *k0, uint64_t *k1, uint32_t *v0, uint32_t *v1, unsigned E, unsigned segs,
                              const uint32_t *d_off, uint64_t **keys_out, uint32_t **vals_out) {
    DevBuf<char> tmp;
    size_t bytes = 0;
    if (!f64) {
        rocprim::double_buffer<uint64_t> keys(k0, k1);
        HIP_TRY(rocprim::segmented_radix_sort_keys(nullptr, bytes, keys, E, segs, d_off, d_off + 1, 0, 64, ctx->stream));
        HIP_TRY(tmp.alloc_bytes(bytes));
        HIP_TRY(rocprim::segmented_radix_sort_keys(tmp.p, bytes, keys, E, segs, d_off, d_off + 1, 0, 64, ctx->stream));
        *keys_out = keys.current(); *vals_out = nullptr;
        return PCR_OK;
    }
    // by original index, then (stable) by the bits of d2
    rocprim::double_buffer<uint32_t> o(v0, v1);
    rocprim::double_buffer<uint64_t> d(k0, k1);
    HIP_TRY(rocprim::segmented_radix_sort_pairs(nullptr, bytes, o, d, E, segs, d_off, d_off + 1, 0, 32, ctx->stream));
    HIP_TRY(tmp.alloc_bytes(bytes));
    HIP_TRY(rocprim::segmented_radix_sort_pairs(tmp.p, bytes, o, d, E, segs, d_off, d_off + 1, 0, 32, ctx->stream));
    size_t bytes2 = 0;
    HIP_TRY(rocprim::segmented_radix_sort_pairs(nullptr, bytes2, d, o, E, segs, d_off, d_off + 1, 0, 64, ctx->stream));
    if (bytes2 > bytes) { HIP_TRY(hipStreamSynchronize(ctx->stream)); HIP_TRY(tmp.alloc_bytes(bytes2)); }
    HIP_TRY(rocprim::segmented_radix_sort_pairs(tmp.p, bytes2, d, o, E, segs, d_off, d_off + 1, 0, 64, ctx->stream));
    *keys_out = d.current(); *vals_out = o.current();
    return PCR_OK;
}

template <typename Real>
static pcr_status radius_query(pcr_target *t, const Real *q, int64_t m, Real r, const int64_t *offsets, Real *dist, int64_t *idx, const char *who) {
    PCR_REQUIRE(t && (q || m == 0) && offsets, "NULL argument");
    PCR_REQUIRE(m >= 0, "negative query count");
    PCR_TRY(radius_check<Real>(t, r, who));
    // the CSR layout: starts at 0, never decreases
    PCR_REQUIRE(offsets[0] == 0, "offsets must start at 0");
    for (int64_t i = 0; i < m; ++i) PCR_REQUIRE(offsets[i + 1] >= offsets[i], "offsets must not decrease");
    PCR_REQUIRE(offsets[m] == 0 || (dist && idx), "NULL argument");
    if (m == 0) return PCR_OK;
    if (t->n == 0) { PCR_REQUIRE(offsets[m] == 0, "offsets are not the prefix sum of the counts"); return PCR_OK; }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const bool f64 = sizeof(Real) == 8;
    const int64_t budget = radius_budget();
    DevBuf<Real> d_q;
    HIP_TRY(d_q.alloc(3 * (size_t)m));
    HIP_TRY(hipMemcpyAsync(d_q.p, q, sizeof(Real) * 3 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));

    // chunks of consecutive queries [cut[c], cut[c + 1]) whose segments fit the budget; a larger query alone
    std::vector<int64_t> cut{0};
    int64_t e_max = 0;
    for (int64_t a = 0; a < m;) {
        int64_t b = a + 1;
        while (b < m && offsets[b + 1] - offsets[a] <= budget) ++b;
        cut.push_back(b);
        if (offsets[b] - offsets[a] > e_max) e_max = offsets[b] - offsets[a];
        a = b;
    }
    PCR_REQUIRE(e_max < ((int64_t)1 << 32), "a chunk of segments holds 2^32 entries or more");
    const size_t n_chunks = cut.size() - 1;
    int64_t m_max = 0;
    for (size_t c = 0; c < n_chunks; ++c) m_max = cut[c + 1] - cut[c] > m_max ? cut[c + 1] - cut[c] : m_max;

    if (n_chunks > 1) {
        // results of an earlier chunk reach the caller before a later chunk's flag is known: check every length first
        DevBuf<int64_t> d_count;
        HIP_TRY(d_count.alloc((size_t)m));
        radius_launch_count<Real>(t, d_q.p, m, r, d_count.p);
        HIP_TRY(hipGetLastError());
        std::vector<int64_t> cnt((size_t)m);
        HIP_TRY(hipMemcpyAsync(cnt.data(), d_count.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < m; ++i) PCR_REQUIRE(cnt[i] == offsets[i + 1] - offsets[i], "offsets are not the prefix sum of the counts");
    }

    const size_t cap = (size_t)(e_max > 0 ? e_max : 1);
    DevBuf<uint64_t> k0, k1;
    DevBuf<uint32_t> v0, v1, d_off, d_flag;
    DevBuf<Real> d_dist;
    DevBuf<int64_t> d_idx;
    HIP_TRY(k0.alloc(cap)); HIP_TRY(k1.alloc(cap));
    if (f64) { HIP_TRY(v0.alloc(cap)); HIP_TRY(v1.alloc(cap)); }
    HIP_TRY(d_off.alloc((size_t)m_max + 1)); HIP_TRY(d_flag.alloc(1));
    HIP_TRY(d_dist.alloc(cap)); HIP_TRY(d_idx.alloc(cap));
    std::vector<uint32_t> rel((size_t)m_max + 1);
    static const bool times = env_flag("PCR_RADIUS_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));

    for (size_t c = 0; c < n_chunks; ++c) {
        const int64_t a = cut[c], b = cut[c + 1], mc = b - a, E = offsets[b] - offsets[a];
        for (int64_t i = 0; i <= mc; ++i) rel[(size_t)i] = (uint32_t)(offsets[a + i] - offsets[a]);
        HIP_TRY(hipMemcpyAsync(d_off.p, rel.data(), 4 * (size_t)(mc + 1), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(d_flag.p, 0, 4, ctx->stream));
        ev.mark(0, ctx->stream);
        hipLaunchKernelGGL((k_radius<Real, 1>), grid_for(mc, RAD_BLOCK), dim3(RAD_BLOCK), 0, ctx->stream, RadTarget<Real>::geom(t), RadTarget<Real>::pts(t),
                           (const uint32_t *)t->cell_start, (const Real *)(d_q.p + 3 * a), mc, r, (int64_t *)nullptr, (const uint32_t *)d_off.p,
                           k0.p, v0.p, d_flag.p);
        HIP_TRY(hipGetLastError());
        ev.mark(1, ctx->stream);
        if (E > 0) {
            uint64_t *ks = nullptr;
            uint32_t *vs = nullptr;
            PCR_TRY(radius_sort(ctx, f64, k0.p, k1.p, v0.p, v1.p, (unsigned)E, (unsigned)mc, d_off.p, &ks, &vs));
            ev.mark(2, ctx->stream);
            if (f64)
                hipLaunchKernelGGL(k_radius_unpack_dd, grid_for(E, 256), dim3(256), 0, ctx->stream, (const uint64_t *)ks,
                                   (const uint32_t *)vs, E, (double *)d_dist.p, d_idx.p);
            else
                hipLaunchKernelGGL(k_radius_unpack, grid_for(E, 256), dim3(256), 0, ctx->stream, (const uint64_t *)ks, E,
                                   (float *)d_dist.p, d_idx.p);
            HIP_TRY(hipGetLastError());
        } else {
            ev.mark(2, ctx->stream);
        }
        ev.mark(3, ctx->stream);
        // the host copies happen only after the flag reads clean
        uint32_t flag = 0;
        HIP_TRY(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        PCR_REQUIRE(flag == 0, "offsets are not the prefix sum of the counts");
        if (ev.on)
            fprintf(stderr, "pcr_radius_times %s queries %lld entries %lld fill_ms %.4f sort_ms %.4f unpack_ms %.4f\n", who, (long long)mc,
                    (long long)E, ev.ms(0), ev.ms(1), ev.ms(2));
        if (E > 0) {
            HIP_TRY(hipMemcpyAsync(dist + offsets[a], d_dist.p, sizeof(Real) * (size_t)E, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipMemcpyAsync(idx + offsets[a], d_idx.p, 8 * (size_t)E, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
    }
    return PCR_OK;
}

extern "C" pcr_status pcr_radius_count(pcr_target *t, const float *q, int64_t m, float r, int64_t *count) {
    return radius_count<float>(t, q, m, r, count, "pcr_radius_count");
}
extern "C" pcr_status pcr_radius_query(pcr_target *t, const float *q, int64_t m, float r, const int64_t *offsets, float *dist, int64_t *idx) {
    return radius_query<float>(t, q, m, r, offsets, dist, idx, "pcr_radius_query");
}
extern "C" pcr_status pcr_radius_count_dd(pcr_target *t, const double *q, int64_t m, double r, int64_t *count) {
    return radius_count<double>(t, q, m, r, count, "pcr_radius_count_dd");
}
extern "C" pcr_status pcr_radius_query_dd(pcr_target *t, const double *q, int64_t m, double r, const int64_t *offsets, double *dist,
                                          int64_t *idx) {
    return radius_query<double>(t, q, m, r, offsets, dist, idx, "pcr_radius_query_dd");
}

// ---- mean k-NN distance ---------------------------------------------------------------------------------------------------
template <typename LIST>
__device__ __forceinline__ void knn_mean_finish(const PtF me, double *mean, LIST &L) {
    // the distances pcr_knn_query reports, summed in float64 nearest first, over the neighbours found
    double s = 0;
    L.for_each([&](int, float d2, uint32_t) { s += (double)__builtin_sqrtf(d2); });
    mean[pt_orig(me)] = s / (double)(L.cnt > 0 ? L.cnt : 1);
}

// REG = 1: the collect path (k <= 16); 0: the LDS list (knn_self, knn_device.h)
template <int REG>
__global__ void __launch_bounds__(KNN_BLOCK) k_knn_mean_dist(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n, int k, double *mean) {
    const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    knn_self<REG>(g, pts, cs, me, k, rad_smem, [&](auto &L) { knn_mean_finish(me, mean, L); });
}

extern "C" pcr_status pcr_knn_mean_distance(pcr_target *t, int k, double *mean_out) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_REQUIRE(!t->is_voxel, "the mean k-NN distance belongs to point targets");
    if (k < 1 || k > KNN_MAX_K) { pcr_set_error("k must be in [1, %d]", KNN_MAX_K); return PCR_ERR_INVALID; }
    PCR_REQUIRE(mean_out || t->n == 0, "NULL argument");
    if (t->n == 0) return PCR_OK;
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    DevBuf<double> d_mean;
    HIP_TRY(d_mean.alloc((size_t)t->n));
    knn_launch(k_knn_mean_dist<1>, k_knn_mean_dist<0>, k <= KNN_REG_K, t->n, k, ctx->stream, t->gf, (const PtF *)t->pts,
               (const uint32_t *)t->cell_start, t->n, k, d_mean.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(mean_out, d_mean.p, 8 * (size_t)t->n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}
