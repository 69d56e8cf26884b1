// Direct voxel neighbourhoods for VGICP (include/pcr.h: "direct voxel neighbourhoods"): a scan point is associated with the
// kept voxel that CONTAINS its transformed position and with that voxel's neighbours -- 1, 7 or 27 voxels, found by integer
// lookup in the target's sorted hash keys -- and every voxel found contributes one distribution-to-distribution term, exactly
// the term a correspondence of vgicp.hip contributes (VgicpArgs, vgicp_side.h; DistSide::each, gicp_weight.h).  No search, no
// match list.  Built BESIDE the hot path like vgicp.hip: kernels.hip, pass.hip, rows.hip, gicp.hip, seam64.hip do not change.
//
//   k_keys_ascend             st_keys ascend strictly (checked once per target)
//   k_direct_inverse          key_inv[key-order index] = position in `means` / vcov (the inverse of what means[j].w records), so
//                             the pass gathers from the arrays the nearest-centroid pass gathers from: a later
//                             pcr_target_voxels_set_covariances is seen without anything being rebuilt
//   k_voxel_lookup<NB>        one lane per query: NB key-order indices, -1 where there is no kept voxel
//   k_vgicp_direct<NB>        the pass, one lane per scan point in device order, grid-stride: transform, ALL lookups (the binary
//   k_vgicp_direct_robust<NB> searches of a point's rows advance together, a step of every row in flight at a time), the hits
//                             compacted in offset order into a per-lane list in LDS, then one gather + DistSide::each per hit.
//                             32 float64 accumulators per lane, block_store_partials, folded by k_vgicp_fold (vgicp.hip): no
//                             atomics, the grid depends on the scan size and the device only -- two calls return the same bits
//   k_vgicp_direct_residuals<NB>   d^T M d of every (point, offset) in the caller's order, +inf where there is no kept pair
//
// The lookup.  key(c) = row(cy, cz) + cx with row = ((cz P mod M) + cy) P mod M (voxel_build.hip: k_voxel_keys), so the three
// x-neighbours of a row are the keys k - 1, k, k + 1 and, the keys being sorted and distinct, sit next to each other behind
// lower_bound(k - 1): one search serves three offsets (9 searches for 27 voxels, 5 for 7).  The rows of the neighbours follow
// from the point's own row by modular arithmetic, row(cy + dy, cz + dz) = (row + dy P + dz P^2) mod M, exact in integers:
// two 64-bit divisions per point instead of eighteen.
#include <math.h>
#include <string.h>

#include "gicp_weight.h"
#include "match_pass.h"
#include "vgicp_side.h"

__global__ void k_vgicp_fold(const double *__restrict__ rows, int nb, double *out);      // vgicp.hip

#define DIRECT_P 116101LL
#define DIRECT_M 10000000000LL
#define DIRECT_P2 3479442201LL              // P * P mod M
#define DIRECT_NONE 0xffffffffu

struct DirectArgs {
    const long long *keys;   // st_keys: ascending, distinct
    const uint32_t *inv;     // key-order index -> position in means / vcov (k_voxel_lookup: not read)
    uint32_t nk;             // kept voxels, > 0
    uint32_t top;            // the largest power of two <= nk: the first step of the search
    double vs;               // voxel size
};

// ---- lookup data ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_keys_ascend(const long long *__restrict__ keys, int64_t n, int *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i + 1 < n && keys[i] >= keys[i + 1]) *bad = 1;       // (every writer stores the same value)
}

__global__ void __launch_bounds__(256) k_direct_inverse(const PtD *__restrict__ means, int64_t n, uint32_t *inv) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t i = (size_t)__double_as_longlong(means[j].w);
    if (i < (size_t)n) inv[i] = (uint32_t)j;
}

// the lookup data of a voxel target with kept voxels, built by the first call that asks
static pcr_status direct_prepare(pcr_target *t) {
    if (t->key_inv) return PCR_OK;
    pcr_context *ctx = t->ctx;
    DevBuf<int> bad;
    HIP_TRY(bad.alloc(1));
    HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_keys_ascend, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const long long *)t->st_keys, t->n, bad.p);
    HIP_TRY(hipGetLastError());
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, bad.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    PCR_REQUIRE(h == 0, "the keys of the voxel target do not ascend strictly");
    uint32_t *inv = nullptr;
    HIP_TRY(pcr_persist_alloc((void **)&inv, sizeof(uint32_t) * (size_t)t->n));
    hipLaunchKernelGGL(k_direct_inverse, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const PtD *)t->means, t->n, inv);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { pcr_persist_free(ctx, inv); HIP_TRY(e); }
    t->key_inv = inv;
    return PCR_OK;
}

static pcr_status direct_has_keys(const pcr_target *t) {
    if (!t->is_voxel) { pcr_set_error("a direct voxel lookup needs a voxel target"); return PCR_ERR_NO_TARGET; }
    if (!t->st_keys) { pcr_set_error("voxel target holds no keys (pcr_target_voxels_set_keys)"); return PCR_ERR_NO_TARGET; }
    return PCR_OK;
}

static DirectArgs direct_args(const pcr_target *t) {
    uint32_t top = 1;
    while ((uint64_t)top * 2 <= (uint64_t)t->n) top *= 2;
    return {(const long long *)t->st_keys, t->key_inv, (uint32_t)t->n, top, t->voxel_size};
}

extern "C" pcr_status pcr_target_voxels_set_keys(pcr_target *t, const int64_t *keys) {
    PCR_REQUIRE(t && (keys || t->n == 0), "NULL argument");
    if (!t->is_voxel) { pcr_set_error("keys belong to voxel targets"); return PCR_ERR_NO_TARGET; }
    PCR_REQUIRE(!t->st_counts, "the keys of a target built from points are the build's own");
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    if (!t->st_keys) HIP_TRY(pcr_persist_alloc((void **)&t->st_keys, sizeof(int64_t) * (size_t)(t->n ? t->n : 1)));
    pcr_persist_free(ctx, t->key_inv);                    // (the next lookup checks the new keys)
    t->key_inv = nullptr;
    if (t->n > 0) HIP_TRY(hipMemcpyAsync(t->st_keys, keys, sizeof(int64_t) * (size_t)t->n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// ---- the lookup of one point -----------------------------------------------------------------------------------------------
// the rows of a neighbourhood, in offset order: (dy, dz) and whether the row takes all three dx
template <int NB> struct Nbhd;
template <> struct Nbhd<1> {
    static constexpr int ROWS = 1;
    static __device__ constexpr int dy(int) { return 0; }
    static __device__ constexpr int dz(int) { return 0; }
    static __device__ constexpr bool triple(int) { return false; }
};
template <> struct Nbhd<7> {       // (0,0,0) (-1,0,0) (+1,0,0) | (0,-1,0) | (0,+1,0) | (0,0,-1) | (0,0,+1)
    static constexpr int ROWS = 5;
    static __device__ constexpr int dy(int r) { return r == 1 ? -1 : (r == 2 ? 1 : 0); }
    static __device__ constexpr int dz(int r) { return r == 3 ? -1 : (r == 4 ? 1 : 0); }
    static __device__ constexpr bool triple(int r) { return r == 0; }
};
template <> struct Nbhd<27> {      // dz outer, dy middle, dx inner
    static constexpr int ROWS = 9;
    static __device__ constexpr int dy(int r) { return r % 3 - 1; }
    static __device__ constexpr int dz(int r) { return r / 3 - 1; }
    static __device__ constexpr bool triple(int) { return true; }
};

__device__ __forceinline__ long long direct_pymod(long long a) {
    const long long r = a % DIRECT_M;
    return r < 0 ? r + DIRECT_M : r;
}

// c = floor((double)t / voxel_size), IEEE division; false: no voxel (not finite, or |c| > 2^40)
__device__ __forceinline__ bool direct_cell(double vs, float t, long long &c) {
    const double q = floor((double)t / vs);
    const bool ok = fabs(q) <= 0x1p40;                    // (false for NaN)
    c = ok ? (long long)q : 0;
    return ok;
}

// idx[o] = key-order index of the kept voxel at offset o of the cell of (tx, ty, tz), -1: none
template <int NB>
__device__ __forceinline__ void direct_lookup(const DirectArgs &da, float tx, float ty, float tz, int idx[NB]) {
    typedef Nbhd<NB> N;
    constexpr int ROWS = N::ROWS;
    long long cx, cy, cz;
    const bool okx = direct_cell(da.vs, tx, cx), oky = direct_cell(da.vs, ty, cy), okz = direct_cell(da.vs, tz, cz);
    const bool ok = okx && oky && okz;
    const long long row0 = direct_pymod((direct_pymod(cz * DIRECT_P) + cy) * DIRECT_P);
    long long first[ROWS];           // the smallest key wanted of the row
    uint32_t pos[ROWS];              // keys below it
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        long long row = row0 + N::dy(r) * DIRECT_P + N::dz(r) * DIRECT_P2;       // in (-M, 2 M)
        row = row < 0 ? row + DIRECT_M : (row >= DIRECT_M ? row - DIRECT_M : row);
        first[r] = row + cx - (N::triple(r) ? 1 : 0);
        pos[r] = 0;
    }
    // lower_bound, branch-free and the same steps for every row and lane
    for (uint32_t s = da.top; s > 0; s >>= 1) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const uint32_t p = pos[r] + s;
            const long long e = da.keys[(p < da.nk ? p : da.nk) - 1];
            if (p <= da.nk && e < first[r]) pos[r] = p;
        }
    }
    const uint32_t last = da.nk - 1;
    long long e[ROWS][3];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int k = 0; k < (N::triple(r) ? 3 : 1); ++k) e[r][k] = da.keys[pos[r] + k < last ? pos[r] + k : last];
    int o = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint32_t p0 = pos[r];
        const bool f0 = ok && p0 < da.nk && e[r][0] == first[r];
        if (!N::triple(r)) { idx[o++] = f0 ? (int)p0 : -1; continue; }
        const uint32_t p1 = p0 + (f0 ? 1u : 0u);
        const bool f1 = ok && p1 < da.nk && (f0 ? e[r][1] : e[r][0]) == first[r] + 1;
        const uint32_t p2 = p1 + (f1 ? 1u : 0u);
        const long long v2 = p2 == p0 ? e[r][0] : (p2 == p0 + 1 ? e[r][1] : e[r][2]);
        const bool f2 = ok && p2 < da.nk && v2 == first[r] + 2;
        const int i0 = f0 ? (int)p0 : -1, i1 = f1 ? (int)p1 : -1, i2 = f2 ? (int)p2 : -1;      // dx = -1, 0, +1
        if (NB == 7) { idx[o] = i1; idx[o + 1] = i0; idx[o + 2] = i2; }
        else { idx[o] = i0; idx[o + 1] = i1; idx[o + 2] = i2; }
        o += 3;
    }
}

template <int NB>
__global__ void __launch_bounds__(256) k_voxel_lookup(const float *__restrict__ xyz, int64_t m, const DirectArgs da, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    int idx[NB];
    direct_lookup<NB>(da, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], idx);
#pragma unroll
    for (int o = 0; o < NB; ++o) out[NB * i + o] = (int64_t)idx[o];
}

// ---- the pass ---------------------------------------------------------------------------------------------------------------
// the positions in means / vcov of the voxels found, DIRECT_NONE where there is none: every load in flight before the first is used
template <int NB>
__device__ __forceinline__ void direct_positions(const DirectArgs &da, const int idx[NB], uint32_t j[NB]) {
#pragma unroll
    for (int o = 0; o < NB; ++o) j[o] = da.inv[idx[o] >= 0 ? idx[o] : 0];
#pragma unroll
    for (int o = 0; o < NB; ++o) j[o] = idx[o] >= 0 ? j[o] : DIRECT_NONE;
}

template <int NB, typename SIDE>
__device__ __forceinline__ void direct_reduce(const LinArgs &a, const SIDE &sd, const DirectArgs &da) {
    __shared__ uint32_t hits[NB * 256];          // [c][thread]: a lane reads what it wrote, nothing is shared
    const PoseK &P = a.hp;
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
        const float x = a.sx[i], y = a.sy[i], z = a.sz[i];
        typename SIDE::Scan sc;
        sd.load(i, sc);
        float tx, ty, tz;
        xform(P, x, y, z, tx, ty, tz);
        int idx[NB];
        direct_lookup<NB>(da, tx, ty, tz, idx);
        uint32_t j[NB];
        direct_positions<NB>(da, idx, j);
        int cnt = 0;
#pragma unroll
        for (int o = 0; o < NB; ++o)
            if (j[o] != DIRECT_NONE) { hits[cnt * 256 + threadIdx.x] = j[o]; ++cnt; }
#pragma unroll 1
        for (int c = 0; c < cnt; ++c) {
            typename SIDE::Match m;
            sd.gather(a, hits[c * 256 + threadIdx.x], m);
            sd.add(acc, a, P, x, y, z, tx, ty, tz, sc, m);
        }
    }
    block_store_partials<false>(acc, sd.rows);
}

template <int NB>
__global__ void __launch_bounds__(256) k_vgicp_direct(const LinArgs a, const VgicpArgs va, const DirectArgs da) { direct_reduce<NB>(a, va, da); }
template <int NB>
__global__ void __launch_bounds__(256) k_vgicp_direct_robust(const LinArgs a, const RobustSide<VgicpArgs> va, const DirectArgs da) {
    direct_reduce<NB>(a, va, da);
}

template <int NB>
__global__ void __launch_bounds__(256) k_vgicp_direct_residuals(const LinArgs a, const VgicpArgs va, const DirectArgs da,
                                                                const uint32_t *__restrict__ order, double *__restrict__ out) {
    __shared__ uint32_t slots[NB * 256];         // [o][thread]
    const PoseK &P = a.hp;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
        const float x = a.sx[i], y = a.sy[i], z = a.sz[i];
        VgicpArgs::Scan sc;
        va.load(i, sc);
        float tx, ty, tz;
        xform(P, x, y, z, tx, ty, tz);
        int idx[NB];
        direct_lookup<NB>(da, tx, ty, tz, idx);
        uint32_t j[NB];
        direct_positions<NB>(da, idx, j);
#pragma unroll
        for (int o = 0; o < NB; ++o) slots[o * 256 + threadIdx.x] = j[o];
        const int64_t dest = order ? (int64_t)order[i] : i;
#pragma unroll 1
        for (int o = 0; o < NB; ++o) {
            double s = (double)INFINITY;
            const uint32_t jo = slots[o * 256 + threadIdx.x];
            if (jo != DIRECT_NONE) {
                VgicpArgs::Match m;
                va.gather(a, jo, m);
                va.each(a, P, x, y, z, tx, ty, tz, sc, m, VgicpArgs::Resid(&s, P, x, y, z));
            }
            out[NB * dest + o] = s;
        }
    }
}

// ---- the driver ---------------------------------------------------------------------------------------------------------------
static pcr_status check_neighbors(int nb) {
    PCR_REQUIRE(nb == 1 || nb == 7 || nb == 27, "neighbors must be 1, 7 or 27");
    return PCR_OK;
}

// STATEMENT with NB = the checked nb as a constant
#define DIRECT_WITH_NB(nb, STATEMENT)                                  \
    do {                                                               \
        if ((nb) == 1) { constexpr int NB = 1; STATEMENT; }            \
        else if ((nb) == 7) { constexpr int NB = 7; STATEMENT; }       \
        else { constexpr int NB = 27; STATEMENT; }                     \
    } while (0)

struct DirectParams {
    int nb;
    RobustK rb;
};

// what a direct call refuses behind its own parameters, in the order the nearest-centroid entry points refuse it: the payloads,
// then what their search refuses
static pcr_status direct_refuse(const pcr_target *t, const pcr_scan *s, double max_dist) {
    if (!t->is_voxel) { pcr_set_error("VGICP needs a voxel target"); return PCR_ERR_NO_TARGET; }
    if (!t->vcov) { pcr_set_error("VGICP target has no covariances (pcr_target_voxels_set_covariances)"); return PCR_ERR_NO_TARGET; }
    if (!s->cov) { pcr_set_error("VGICP scan has no covariances (pcr_scan_estimate_covariances / _set_covariances)"); return PCR_ERR_NO_TARGET; }
    PCR_TRY(direct_has_keys(t));
    PCR_REQUIRE(s->ctx == t->ctx, "scan and target belong to different contexts");
    PCR_REQUIRE(max_dist > 0, "max_dist must be positive");
    if (t->ctx->comm != nullptr) { pcr_set_error("VGICP passes are not available on a context with a communicator attached"); return PCR_ERR_UNSUPPORTED; }
    return PCR_OK;
}

// what the kernels read of a call (LinArgs: the scan, the centroids, the gate, the pose).  The pose is rounded as pass.hip's
// host_pose_k rounds it for every host-driven pass (R as it is, r32 / t32 = (float) of the entry; that function is local to
// pass.hip, which this unit leaves alone -- tests/test_gpu_direct.py holds the two together: the pairs of a pass are those of
// the lookup at the float32 transform).  No flag bit of the caller reaches the kernels: nothing here reads LinArgs::flags, and
// its upper bits are internal switches of the pass kernels
static void direct_lin(const pcr_target *t, const pcr_scan *s, const double T[16], double max_dist, LinArgs *a) {
    memset(a, 0, sizeof *a);
    a->sx = s->x; a->sy = s->y; a->sz = s->z; a->n = s->n;
    a->means = t->means;
    a->md_f = (float)max_dist; a->md_d = max_dist;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { a->hp.R[3 * i + j] = T[4 * i + j]; a->hp.r32[3 * i + j] = (float)T[4 * i + j]; }
        a->hp.t32[i] = (float)T[4 * i + 3];
    }
}

// the pcr_pass_fn: one launch and the fold
static pcr_status direct_run(pcr_target *t, pcr_scan *s, int, const double T[16], double max_dist, unsigned, const void *params, double out[29]) {
    const DirectParams *p = (const DirectParams *)params;
    PCR_TRY(direct_refuse(t, s, max_dist));
    double o[29];                                    // (a pass refused further down writes nothing)
    for (int i = 0; i < 29; ++i) o[i] = 0.0;
    if (t->n > 0 && s->n > 0) {
        pcr_context *ctx = t->ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        PCR_TRY(pcr_ensure_scratch(ctx, s->n));
        PCR_TRY(direct_prepare(t));
        LinArgs a;
        direct_lin(t, s, T, max_dist, &a);
        const DirectArgs da = direct_args(t);
        const int nb = choose_blocks(ctx, s->n);         // n and the device only
        DevBuf<double> rows, sums;
        HIP_TRY(rows.alloc(32 * (size_t)nb)); HIP_TRY(sums.alloc(32));
        const VgicpArgs sd = {{s->cov}, t->vcov, rows.p};
        const RobustK rb = p->rb;
        // PCR_DIRECT_TIMES=1 (developer, tools/direct_time.py): events around the pass kernel and the fold, their milliseconds on stderr
        static const bool times = env_flag("PCR_DIRECT_TIMES");
        StageTimes ev;
        HIP_TRY(ev.init(times));
        {
            RoctxRange range(rb.kind == PCR_ROBUST_NONE ? "pcr:vgicp_direct" : "pcr:vgicp_direct_robust");
            const RobustSide<VgicpArgs> rsd = {sd, rb};
            ev.mark(0, ctx->stream);
            if (rb.kind == PCR_ROBUST_NONE) DIRECT_WITH_NB(p->nb, hipLaunchKernelGGL(k_vgicp_direct<NB>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a, sd, da));
            else DIRECT_WITH_NB(p->nb, hipLaunchKernelGGL(k_vgicp_direct_robust<NB>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a, rsd, da));
            ev.mark(1, ctx->stream);
            hipLaunchKernelGGL(k_vgicp_fold, dim3(1), dim3(64), 0, ctx->stream, (const double *)rows.p, nb, sums.p);
            ev.mark(2, ctx->stream);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(o, sums.p, 29 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ev.on) fprintf(stderr, "pcr_direct_times n %lld neighbors %d kernel_ms %.4f fold_ms %.4f\n", (long long)s->n, p->nb, ev.ms(0), ev.ms(1));
    }
    for (int i = 0; i < 29; ++i) out[i] = o[i];
    return PCR_OK;
}

extern "C" pcr_status pcr_vgicp_direct_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, int neighbors,
                                                 const pcr_robust *rb_or_null, unsigned flags, double out[29]) {
    PCR_REQUIRE(t && s && T && out, "NULL argument");
    DirectParams p;
    PCR_TRY(check_neighbors(neighbors));
    p.nb = neighbors;
    PCR_TRY(robust_args(rb_or_null, &p.rb));
    CtxScope scope(t->ctx);
    return direct_run(t, s, PCR_VPLANE, T, max_dist, flags, &p, out);
}

extern "C" pcr_status pcr_vgicp_direct_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             int neighbors, const pcr_robust *rb_or_null, unsigned flags, double T_out[16], int *iterations,
                                             double *trace_or_null) {
    PCR_REQUIRE(t && s && T_init && T_out, "NULL argument");
    DirectParams p;
    PCR_TRY(check_neighbors(neighbors));
    p.nb = neighbors;
    PCR_TRY(robust_args(rb_or_null, &p.rb));
    CtxScope scope(t->ctx);
    return pcr_align_host_loop(direct_run, t, s, PCR_VPLANE, &p, T_init, max_iter, tol, max_dist, flags, T_out, iterations, trace_or_null);
}

extern "C" pcr_status pcr_vgicp_direct_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, int neighbors, unsigned flags,
                                                 double *s_out) {
    (void)flags;                                     // (no flag changes what this call computes)
    PCR_REQUIRE(t && s && T && (s_out || s->n == 0), "NULL argument");
    PCR_TRY(check_neighbors(neighbors));
    PCR_REQUIRE(pcr_scan_knows_order(s), PCR_NEED_ORDER);
    CtxScope scope(t->ctx);
    PCR_TRY(direct_refuse(t, s, max_dist));
    if (s->n == 0) return PCR_OK;
    const size_t count = (size_t)neighbors * (size_t)s->n;
    if (t->n == 0) {
        for (size_t i = 0; i < count; ++i) s_out[i] = (double)INFINITY;
        return PCR_OK;
    }
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    PCR_TRY(pcr_ensure_scratch(ctx, s->n));
    PCR_TRY(direct_prepare(t));
    LinArgs a;
    direct_lin(t, s, T, max_dist, &a);
    const DirectArgs da = direct_args(t);
    const VgicpArgs sd = {{s->cov}, t->vcov, nullptr};
    DevBuf<double> d;
    HIP_TRY(d.alloc(count));
    {
        RoctxRange range("pcr:vgicp_direct_residuals");
        const dim3 grid((unsigned)choose_blocks(ctx, s->n));
        DIRECT_WITH_NB(neighbors, hipLaunchKernelGGL(k_vgicp_direct_residuals<NB>, grid, dim3(256), 0, ctx->stream, a, sd, da, (const uint32_t *)s->order, d.p));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s_out, d.p, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_voxels_lookup(pcr_target *t, const float *xyz, int64_t m, int neighbors, int64_t *idx) {
    PCR_REQUIRE(t && m >= 0 && ((xyz && idx) || m == 0), "NULL argument");
    PCR_TRY(check_neighbors(neighbors));
    PCR_TRY(direct_has_keys(t));
    if (m == 0) return PCR_OK;
    const size_t count = (size_t)neighbors * (size_t)m;
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    if (t->n == 0) {
        for (size_t i = 0; i < count; ++i) idx[i] = -1;
        return PCR_OK;
    }
    PCR_TRY(direct_prepare(t));
    const DirectArgs da = direct_args(t);
    DevBuf<float> q;
    DevBuf<int64_t> d;
    HIP_TRY(q.alloc(3 * (size_t)m)); HIP_TRY(d.alloc(count));
    HIP_TRY(hipMemcpyAsync(q.p, xyz, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    DIRECT_WITH_NB(neighbors, hipLaunchKernelGGL(k_voxel_lookup<NB>, grid_for(m, 256), dim3(256), 0, ctx->stream, (const float *)q.p, m, da, d.p));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); HIP_TRY(e); }
    HIP_TRY(hipMemcpyAsync(idx, d.p, count * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}
