// Direct voxel neighbourhoods for VGICP (include/pcr.h: "direct voxel neighbourhoods"): a scan point is associated with the
// kept voxel that CONTAINS its transformed position and with that voxel's neighbours -- 1, 7 or 27 voxels, found by integer
// lookup in the target's sorted hash keys -- and every voxel found contributes one distribution-to-distribution term, exactly
// the term a correspondence of vgicp.hip contributes (VgicpArgs, vgicp_side.h; DistSide::each, gicp_weight.h).  No search, no
// match list -- and a unit of match_pass.h all the same: DirectUnit<NB> is VgicpUnit with the lookup where the search was
// (MatchUnit::matches), so the refusals, the pose, reduce and fold launches, the read-back, the Gauss-Newton loop and the
// residual read-back are the scaffold's.  This file holds the lookup, the kernels and what the unit differs in.
//
//   k_keys_ascend             st_keys ascend strictly (checked once per target)
//   k_direct_inverse          key_inv[key-order index] = position in `means` / vcov (the inverse of what means[j].w records), so
//                             the pass gathers from the arrays the nearest-centroid pass gathers from: a later
//                             pcr_target_voxels_set_covariances is seen without anything being rebuilt
//   k_voxel_lookup<NB>        one lane per query: NB key-order indices, -1 where there is no kept voxel
//   k_vgicp_direct<NB>        the pass, one lane per scan point in device order, grid-stride: transform, ALL lookups (the binary
//   k_vgicp_direct_robust<NB> searches of a point's rows advance together, a step of every row in flight at a time), the hits
//                             compacted in offset order into a per-lane list in LDS, then one gather + DistSide::each per hit.
//                             32 float64 accumulators per lane, block_store_partials, folded by k_vgicp_fold (vgicp.hip) from
//                             the one place that launches a fold (match_pass.h: launch_reduce_fold): no atomics, the grid
//                             depends on the scan size and the device only -- two calls return the same bits
//   k_vgicp_direct_residuals<NB>   d^T M d of every (point, offset) in the caller's order, +inf where there is no kept pair
//   DirectSide<NB, S>         the SIDE of a call on the host: S and the lookup arguments, M = NB residuals per point; the kernels
//                             take the two as separate arguments (launch_side here)
//   DirectUnit<NB>            the UNIT; the three extern "C" names dispatch on `neighbors` to an instantiation
//
// The lookup.  key(c) = row(cy, cz) + cx with row = ((cz P mod M) + cy) P mod M (voxel_build.hip: k_voxel_keys), so the three
// x-neighbours of a row are the keys k - 1, k, k + 1 and, the keys being sorted and distinct, sit next to each other behind
// lower_bound(k - 1): one search serves three offsets (9 searches for 27 voxels, 5 for 7).  The rows of the neighbours follow
// from the point's own row by modular arithmetic, row(cy + dy, cz + dz) = (row + dy P + dz P^2) mod M, exact in integers:
// two 64-bit divisions per point instead of eighteen.
#include <math.h>
#include <string.h>

#include "vgicp_side.h"

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
    const size_t i = key_index(means[j]);
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
// The SIDE of a direct call on the host: S and the lookup arguments, NB squared residuals per scan point.  The kernels take the
// two apart, (LinArgs, S, DirectArgs, ...) -- with the lookup arguments inside the SIDE the 27-voxel pass kernel measured 2 %
// slower (docs/EXPERIMENTS.md) -- and launch_side below hands them over that way
template <int NB, typename S>
struct DirectSide : S {
    static constexpr int M = NB;
    DirectArgs da;
};

// What both kernels do with scan point i before they part: its loads, its transformed position and j[o] = the position in
// means / vcov of the kept voxel at offset o, DIRECT_NONE where there is none (every load of `inv` in flight before the first
// is used)
template <int NB, typename SIDE>
__device__ __forceinline__ void direct_point(const LinArgs &a, const SIDE &sd, const DirectArgs &da, int64_t i, float &x, float &y, float &z, typename SIDE::Scan &sc,
                                             float &tx, float &ty, float &tz, uint32_t j[NB]) {
    x = a.sx[i]; y = a.sy[i]; z = a.sz[i];
    sd.load(i, sc);
    xform(a.hp, x, y, z, tx, ty, tz);
    int idx[NB];
    direct_lookup<NB>(da, tx, ty, tz, idx);
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
        float x, y, z, tx, ty, tz;
        typename SIDE::Scan sc;
        uint32_t j[NB];
        direct_point<NB>(a, sd, da, i, x, y, z, sc, tx, ty, tz, j);
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
__global__ void __launch_bounds__(256) k_vgicp_direct_residuals(const LinArgs a, const VgicpArgs sd, const DirectArgs da,
                                                                const uint32_t *__restrict__ order, double *__restrict__ out) {
    __shared__ uint32_t slots[NB * 256];         // [o][thread]
    const PoseK &P = a.hp;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
        float x, y, z, tx, ty, tz;
        VgicpArgs::Scan sc;
        uint32_t j[NB];
        direct_point<NB>(a, sd, da, i, x, y, z, sc, tx, ty, tz, j);
#pragma unroll
        for (int o = 0; o < NB; ++o) slots[o * 256 + threadIdx.x] = j[o];
        const int64_t dest = order ? (int64_t)order[i] : i;
#pragma unroll 1
        for (int o = 0; o < NB; ++o) {
            double s = (double)INFINITY;
            const uint32_t jo = slots[o * 256 + threadIdx.x];
            if (jo != DIRECT_NONE) {
                VgicpArgs::Match m;
                sd.gather(a, jo, m);
                sd.each(a, P, x, y, z, tx, ty, tz, sc, m, VgicpArgs::Resid(&s, P, x, y, z));
            }
            out[NB * dest + o] = s;
        }
    }
}

// The launch adapter: a direct kernel by its host-side SIDE (launch_side of match_pass.h, overloaded on the kernel's shape)
template <int NB, typename S, typename... More>
static void launch_side(void (*kernel)(const LinArgs, const S, const DirectArgs, More...), dim3 grid, hipStream_t stream, const LinArgs &a,
                        const DirectSide<NB, S> &sd, More... more) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, a, (const S &)sd, sd.da, more...);
}
template <int NB, typename S>
static void launch_side(void (*kernel)(const LinArgs, const RobustSide<S>, const DirectArgs), dim3 grid, hipStream_t stream, const LinArgs &a,
                        const RobustSide<DirectSide<NB, S>> &sd) {
    const RobustSide<S> rsd = {(const S &)sd, sd.rb};
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, a, rsd, sd.da);
}

// ---- the entry points: a UNIT of match_pass.h, derived from VGICP's ---------------------------------------------------------------
static pcr_status check_neighbors(int nb) {
    PCR_REQUIRE(nb == 1 || nb == 7 || nb == 27, "neighbors must be 1, 7 or 27");
    return PCR_OK;
}

// STATEMENT with NB = nb as a constant (an nb that check_neighbors refuses: any one of them)
#define DIRECT_WITH_NB(nb, STATEMENT)                                  \
    do {                                                               \
        if ((nb) == 1) { constexpr int NB = 1; STATEMENT; }            \
        else if ((nb) == 7) { constexpr int NB = 7; STATEMENT; }       \
        else { constexpr int NB = 27; STATEMENT; }                     \
    } while (0)

// PCR_DIRECT_TIMES=1 (developer, tools/direct_time.py): events around the pass kernel and the fold, their milliseconds on
// stderr.  Read once per process, whatever the neighbourhoods
static bool direct_times() {
    static const bool times = env_flag("PCR_DIRECT_TIMES");
    return times;
}

// VgicpUnit with the lookup in the place of the search: its payloads and the keys; what the search would refuse, refused here
// for EVERY target; `matches` launches nothing; fold and loop are VGICP's.  (keys / adaptive are not this unit's: there is no
// adaptive direct pass.)
template <int NB>
struct DirectUnit : VgicpUnit {
    typedef DirectSide<NB, VgicpArgs> Side;
    static pcr_status check(Params *, int neighbors) { return check_neighbors(neighbors); }
    static pcr_status payloads(const pcr_target *t, const pcr_scan *s) {
        PCR_TRY(VgicpUnit::payloads(t, s));
        return direct_has_keys(t);
    }
    static pcr_status no_match(const pcr_target *t, const pcr_scan *s, double max_dist, bool *none) {
        PCR_TRY(refuse_as_search(t, s, max_dist));
        *none = t->n == 0;
        return PCR_OK;
    }
    // What the kernels read of a call (LinArgs: the scan, the centroids, the gate, the pose), behind the lookup data of the
    // target, which the first call builds -- or refuses -- before the SIDE of the call is made.  An empty scan builds nothing.
    // No flag bit of the caller reaches the kernels: nothing here reads LinArgs::flags, and its upper bits are internal
    // switches of the pass kernels
    static pcr_status matches(LinArgs *a, DevBuf<uint32_t> *, pcr_target *t, pcr_scan *s, int, const double T[16], double max_dist, unsigned, bool) {
        if (s->n == 0) return PCR_OK;
        pcr_context *ctx = t->ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        PCR_TRY(pcr_ensure_scratch(ctx, s->n));          // (fixes ctx->max_blocks: before choose_blocks)
        PCR_TRY(direct_prepare(t));
        memset(a, 0, sizeof *a);
        a->sx = s->x; a->sy = s->y; a->sz = s->z; a->n = s->n;
        a->means = t->means;
        a->md_f = (float)max_dist; a->md_d = max_dist;
        host_pose_k(T, &a->hp);
        return PCR_OK;
    }
    static Side side(const pcr_target *t, const pcr_scan *s, const Params &p) { return {VgicpUnit::side(t, s, p), direct_args(t)}; }
    static constexpr auto reduce = k_vgicp_direct<NB>;
    static constexpr auto robust = k_vgicp_direct_robust<NB>;
    static constexpr auto residuals = k_vgicp_direct_residuals<NB>;
    static constexpr const char *reduce_range = "pcr:vgicp_direct", *robust_range = "pcr:vgicp_direct_robust",
                                *residuals_range = "pcr:vgicp_direct_residuals";
    static bool times() { return direct_times(); }
    static void print_times(StageTimes &ev, int64_t n) {
        fprintf(stderr, "pcr_direct_times n %lld neighbors %d kernel_ms %.4f fold_ms %.4f\n", (long long)n, NB, ev.ms(0), ev.ms(1));
    }
};

extern "C" pcr_status pcr_vgicp_direct_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, int neighbors,
                                                 const pcr_robust *rb_or_null, unsigned flags, double out[29]) {
    DIRECT_WITH_NB(neighbors, return match_linearize<DirectUnit<NB>>(t, s, T, max_dist, rb_or_null, flags, out, neighbors));
}

extern "C" pcr_status pcr_vgicp_direct_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                             int neighbors, const pcr_robust *rb_or_null, unsigned flags, double T_out[16], int *iterations,
                                             double *trace_or_null) {
    DIRECT_WITH_NB(neighbors, return match_align<DirectUnit<NB>>(t, s, T_init, max_iter, tol, max_dist, rb_or_null, flags, T_out, iterations,
                                                                 trace_or_null, neighbors));
}

extern "C" pcr_status pcr_vgicp_direct_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, int neighbors, unsigned flags,
                                                 double *s_out) {
    DIRECT_WITH_NB(neighbors, return match_residuals_entry<DirectUnit<NB>>(t, s, T, max_dist, flags, s_out, neighbors));
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
