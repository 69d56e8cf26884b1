// Fast global registration (Zhou, Park, Koltun 2016): a pose from matches by Gauss-Newton under a Geman-McClure line process
// whose scale mu is annealed.  The contract is in include/pcr.h.
//
//   pcr_fgr_linearize   k_fgr_reduce, k_fgr_fold (+ k_fgr_weight)
//   pcr_fgr_pose        max_iter x (k_fgr_reduce, k_fgr_update) back to back on the stream, one synchronisation per
//                       FGR_QUEUE iterations (+ k_fgr_weight); PCR_FLAG_HOST_LOOP: k_fgr_reduce, k_fgr_fold and the host's
//                       fgr_step per iteration -- the same arithmetic
//   pcr_fgr_tuples      per chunk of tuples: k_fgr_tuples
//
// k_fgr_reduce: one lane = one match, streaming: six float32 and the multiplicity are the only loads, FGR_W matches per lane
// in flight.  The pose and mu come from FgrDev, read once per block into scalar registers.  The unit of summation is the TILE
// of 256 consecutive matches: a lane's 29 float64 terms are folded per tile -- wave shuffles in a fixed order, LDS across the
// four waves in wave order -- and every tile writes ONE row of 32 doubles with plain stores.  Which block folds a tile does
// not enter, so the rows do not depend on the grid.  No atomics.
//
// k_fgr_update / k_fgr_fold: one block adds the rows in ascending tile order, one lane per column; k_fgr_update then solves,
// applies gn_se3_lplus, advances mu and the iteration counter and writes the trace row -- fgr_step, the code the host loop
// runs.  Both kernels of the loop return at once when FgrDev::done is set.
//
// k_fgr_tuples: one lane = one tuple, rs_sample / rs_edge_ok of ransac_device.h; a valid tuple adds 1 to the multiplicity
// of its three rows by integer atomic add: an integer count does not depend on the order.
//
// k_fgr_solo (developer builds): the whole loop in one launch of one block over matches held in LDS.
//
// Environment, read at every call (developer / test switches): PCR_FGR_BLOCKS caps the grid of k_fgr_reduce (default and
// maximum FGR_MAX_BLOCKS), PCR_FGR_CHUNK sets the tuples per launch (default 2^20), PCR_FGR_SOLO=1 selects k_fgr_solo where
// the build has it and the matches fit, PCR_FGR_TIMES=1 reports the loop's milliseconds on stderr.
#include "host_util.h"
#include "gn_math.h"
#include "pass_device.h"       // uniform_f64, wave_fold32
#include "ransac_device.h"

#define FGR_TILE PCR_FGR_TILE
#define FGR_W PCR_FGR_WIDTH          // tiles per block and trip: matches per lane in flight
#define FGR_MAX_BLOCKS 1024
#define FGR_QUEUE 256                // iterations enqueued between two looks at FgrDev::done
#define FGR_M_MAX ((int64_t)1 << 24)
#ifdef PCR_DEV
#define FGR_HAVE_SOLO 1              // k_fgr_solo: developer builds only, measured slower than the loop of launches (docs/EXPERIMENTS.md)
#else
#define FGR_HAVE_SOLO 0
#endif
#define FGR_H_MAX ((int64_t)1 << 26)

// the state of the loop on the device: k_fgr_reduce reads it, k_fgr_update rewrites it
struct FgrDev {
    double T[16];
    double mu, mu_min, division, tol;
    int period, max_iter;
    int iter;            // passes completed = trace rows written
    int done;            // 0 running, 1 finished: status says how
    int status;          // 0 ran out, 1 converged, 2 singular
    int pad;
};

// ---- one step from the 29 sums: host loop and k_fgr_update -----------------------------------------------------------------
// dx = -solve(H, g); converged when tol > 0, mu has reached mu_min and |dx| < tol (the test precedes the update: T stays);
// else T <- lplus(T, dx) and mu follows its schedule.  Sets done / status, counts the pass.
PCR_HD static inline void fgr_step(double (*A)[7], const double o[29], FgrDev *s) {
    double H[36], g[6], dx[6];
    int p = 0;
    for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { H[6 * i + j] = o[p]; H[6 * j + i] = o[p]; ++p; }
    for (int i = 0; i < 6; ++i) g[i] = o[21 + i];
    const int it = s->iter;
    s->iter = it + 1;
    if (gn_solve6(A, H, g, dx)) { s->done = 1; s->status = 2; return; }
    double nrm = 0;
    for (int i = 0; i < 6; ++i) { dx[i] = -dx[i]; nrm += dx[i] * dx[i]; }
    if (s->tol > 0 && s->mu == s->mu_min && sqrt(nrm) < s->tol) { s->done = 1; s->status = 1; return; }
    gn_se3_lplus(s->T, dx);
    if ((it + 1) % s->period == 0 && s->mu > s->mu_min) {
        const double next = s->mu / s->division;
        s->mu = next > s->mu_min ? next : s->mu_min;
    }
    if (it + 1 >= s->max_iter) { s->done = 1; s->status = 0; }
}

// ---- the pass ---------------------------------------------------------------------------------------------------------------
struct FgrPose { double R[9], t[3], mu; };

__device__ __forceinline__ void fgr_load_pose(const FgrDev *__restrict__ s, FgrPose &P) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) P.R[3 * i + j] = uniform_f64(s->T[4 * i + j]);
        P.t[i] = uniform_f64(s->T[4 * i + 3]);
    }
    P.mu = uniform_f64(s->mu);
}

// x = T p, r = x - q, r2 = |r|^2, the line-process weight l * l: include/pcr.h, this order of operations
__device__ __forceinline__ double fgr_residual(const FgrPose &P, const float *p, const float *q, double x[3], double r[3], double &r2) {
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        x[i] = ((P.R[3 * i] * px + P.R[3 * i + 1] * py) + P.R[3 * i + 2] * pz) + P.t[i];
        r[i] = x[i] - (double)q[i];
    }
    r2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
    const double l = P.mu / (P.mu + r2);
    return l * l;
}

// the 29 terms of one match with weight w = c * (l * l); acc[29 .. 31] stay 0
__device__ __forceinline__ void fgr_terms(double *acc, double w, const double x[3], const double r[3], double r2) {
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    acc[0] = w;   acc[1] = 0.0; acc[2] = 0.0;  acc[3] = 0.0;          acc[4] = w * x2;      acc[5] = w * -x1;
    acc[6] = w;   acc[7] = 0.0; acc[8] = w * -x2;  acc[9] = 0.0;      acc[10] = w * x0;
    acc[11] = w;  acc[12] = w * x1;  acc[13] = w * -x0;  acc[14] = 0.0;
    acc[15] = w * (x1 * x1 + x2 * x2);  acc[16] = w * -(x0 * x1);  acc[17] = w * -(x0 * x2);
    acc[18] = w * (x0 * x0 + x2 * x2);  acc[19] = w * -(x1 * x2);
    acc[20] = w * (x0 * x0 + x1 * x1);
    acc[21] = w * r[0];  acc[22] = w * r[1];  acc[23] = w * r[2];
    acc[24] = w * (x1 * r[2] - x2 * r[1]);
    acc[25] = w * (x2 * r[0] - x0 * r[2]);
    acc[26] = w * (x0 * r[1] - x1 * r[0]);
    acc[27] = w * r2;
    acc[28] = w;
    acc[29] = 0.0; acc[30] = 0.0; acc[31] = 0.0;
}

// One tile: this lane's match (live: it exists) -> its 29 terms, folded over the block in block_store_partials' order: wave
// shuffles, then the four waves in wave order through ws.  Lane e < 32 of the block returns column e of the tile's row.  The
// caller alternates two ws buffers, so that a wave may start the next tile while wave 0 still reads this one.
__device__ __forceinline__ double fgr_tile_row(const FgrPose &P, const float *p, const float *q, int c, bool live, double (*ws)[32]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[32], x[3], r[3], r2;
    const double ll = fgr_residual(P, p, q, x, r, r2);
    fgr_terms(acc, live ? (double)c * ll : 0.0, x, r, r2);
    wave_fold32(acc, lane);
    if ((lane & 1) == 0) ws[wave][lane >> 1] = acc[0];
    __syncthreads();
    const int e = threadIdx.x & 31;
    return ((ws[0][e] + ws[1][e]) + ws[2][e]) + ws[3][e];
}

// tiles g, g + 1, .. of a group of FGR_W belong to one block and trip; rows[tile * 32 + e]
__global__ void __launch_bounds__(256) k_fgr_reduce(const float *__restrict__ src, const float *__restrict__ dst, const int32_t *__restrict__ mult,
                                                    int64_t m, int ntiles, const FgrDev *__restrict__ st, double *__restrict__ rows) {
    if (__builtin_amdgcn_readfirstlane(st->done) != 0) return;
    __shared__ double wsum[2][4][32];
    FgrPose P;
    fgr_load_pose(st, P);
    for (int g0 = (int)blockIdx.x * FGR_W; g0 < ntiles; g0 += (int)gridDim.x * FGR_W) {
        float p[FGR_W][3], q[FGR_W][3];
        int c[FGR_W];
        bool use[FGR_W];
        // the loads of all FGR_W matches of this lane; a match past the end reads row 0 (m >= 1) and counts 0
#pragma unroll
        for (int u = 0; u < FGR_W; ++u) {
            const int64_t j = (int64_t)(g0 + u) * FGR_TILE + threadIdx.x;
            use[u] = j < m;
            const int64_t i = use[u] ? j : 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { p[u][k] = src[3 * i + k]; q[u][k] = dst[3 * i + k]; }
            c[u] = mult ? mult[i] : 1;
        }
        reduce_phase();
#pragma unroll
        for (int u = 0; u < FGR_W; ++u) {
            if (g0 + u >= ntiles) break;                       // uniform over the block
            const double s = fgr_tile_row(P, p[u], q[u], c[u], use[u], wsum[u & 1]);
            if (threadIdx.x < 32) rows[(size_t)(g0 + u) * 32 + threadIdx.x] = s;
        }
        if (FGR_W & 1) __syncthreads();                        // (an odd FGR_W would reuse buffer 0 at once)
    }
}

// the weights l * l of every match at the pose and mu of *st (the multiplicity takes no part)
__global__ void __launch_bounds__(256) k_fgr_weight(const float *__restrict__ src, const float *__restrict__ dst, int64_t m,
                                                    const FgrDev *__restrict__ st, double *__restrict__ weight) {
    FgrPose P;
    fgr_load_pose(st, P);
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    double x[3], r[3], r2;
    weight[j] = fgr_residual(P, src + 3 * j, dst + 3 * j, x, r, r2);
}

// column e of the rows in ascending tile order: sixteen loads in flight, the additions one after the other
__device__ __forceinline__ double fgr_fold_rows(const double *__restrict__ rows, int ntiles, int e) {
    double s = 0.0;
    int b = 0;
    for (; b + 16 <= ntiles; b += 16) {
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = rows[(size_t)(b + k) * 32 + e];
#pragma unroll
        for (int k = 0; k < 16; ++k) s += v[k];
    }
    for (; b < ntiles; ++b) s += rows[(size_t)b * 32 + e];
    return s;
}

__global__ void __launch_bounds__(64) k_fgr_fold(const double *__restrict__ rows, int ntiles, double *__restrict__ out) {
    if (threadIdx.x < 32) out[threadIdx.x] = fgr_fold_rows(rows, ntiles, threadIdx.x);
}

// trace row of this iteration: T before the step (16), the 29 sums, mu
__global__ void __launch_bounds__(64) k_fgr_update(const double *__restrict__ rows, int ntiles, FgrDev *st, double *trace) {
    if (__builtin_amdgcn_readfirstlane(st->done) != 0) return;
    __shared__ double sums[32];
    if (threadIdx.x < 32) sums[threadIdx.x] = fgr_fold_rows(rows, ntiles, threadIdx.x);
    __syncthreads();
    if (trace) {
        double *row = trace + (size_t)st->iter * PCR_FGR_TRACE;
        if (threadIdx.x < 16) row[threadIdx.x] = st->T[threadIdx.x];
        else if (threadIdx.x < 45) row[threadIdx.x] = sums[threadIdx.x - 16];
        else if (threadIdx.x == 45) row[45] = st->mu;
    }
    __syncthreads();                                           // the trace has read T and mu
    if (threadIdx.x == 0) {
        double A[6][7], o[29];
#pragma unroll
        for (int i = 0; i < 29; ++i) o[i] = sums[i];
        FgrDev s = *st;
        fgr_step(A, o, &s);
        *st = s;
    }
}

#if FGR_HAVE_SOLO
// The whole loop in ONE launch of ONE block, for match lists that fit into the LDS of a workgroup: the matches are loaded
// into LDS once (src, dst as floats, then mult), every iteration walks the tiles with fgr_tile_row, lane e < 32 adds column e
// of the tile rows as they come -- ascending tile order, from 0, as fgr_fold_rows adds them -- and lane 0 runs fgr_step; block
// barriers only.  Same terms, same folds, same order: the same bits as the loop of launches.
__global__ void __launch_bounds__(256) k_fgr_solo(const float *__restrict__ src, const float *__restrict__ dst, const int32_t *__restrict__ mult,
                                                  int m, int ntiles, FgrDev *st, double *trace) {
    extern __shared__ __attribute__((aligned(16))) float s_pts[];      // src 3 m | dst 3 m | mult m
    __shared__ double wsum[2][4][32];
    __shared__ double sums[32];
    __shared__ FgrDev s_st;
    float *s_src = s_pts, *s_dst = s_pts + 3 * (size_t)m;
    int32_t *s_mult = (int32_t *)(s_pts + 6 * (size_t)m);
    for (int i = threadIdx.x; i < 3 * m; i += 256) { s_src[i] = src[i]; s_dst[i] = dst[i]; }
    for (int i = threadIdx.x; i < m; i += 256) s_mult[i] = mult ? mult[i] : 1;
    if (threadIdx.x == 0) s_st = *st;
    __syncthreads();
    while (__builtin_amdgcn_readfirstlane(s_st.done) == 0) {
        FgrPose P;
        fgr_load_pose(&s_st, P);
        double col = 0.0;
        for (int t = 0; t < ntiles; ++t) {
            const int j = t * FGR_TILE + (int)threadIdx.x;
            const bool live = j < m;
            const int i = live ? j : 0;
            const double s = fgr_tile_row(P, s_src + 3 * i, s_dst + 3 * i, s_mult[i], live, wsum[t & 1]);
            col += s;
        }
        if (threadIdx.x < 32) sums[threadIdx.x] = col;
        __syncthreads();                                       // (also: wave 0 has read the last tile before buffer 0 is written again)
        if (trace) {
            double *row = trace + (size_t)s_st.iter * PCR_FGR_TRACE;
            if (threadIdx.x < 16) row[threadIdx.x] = s_st.T[threadIdx.x];
            else if (threadIdx.x < 45) row[threadIdx.x] = sums[threadIdx.x - 16];
            else if (threadIdx.x == 45) row[45] = s_st.mu;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double A[6][7], o[29];
#pragma unroll
            for (int i = 0; i < 29; ++i) o[i] = sums[i];
            FgrDev s = s_st;
            fgr_step(A, o, &s);
            s_st = s;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *st = s_st;
}
#endif

// ---- the tuple test ---------------------------------------------------------------------------------------------------------
// tuples h0 .. h0 + n - 1; acc[0] += the valid ones
__global__ void __launch_bounds__(256) k_fgr_tuples(const float *__restrict__ src, const float *__restrict__ dst, int64_t m, int64_t h0, int64_t n,
                                                    uint64_t s, double sim2, double e2min, int32_t *mult, unsigned long long *acc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (i < n) {
        uint32_t c0, c1, c2;
        rs_sample(s, (uint64_t)(h0 + i), (uint64_t)m, c0, c1, c2);
        const RsV3 p0 = rs_ld(src, c0), p1 = rs_ld(src, c1), p2 = rs_ld(src, c2);
        const RsV3 q0 = rs_ld(dst, c0), q1 = rs_ld(dst, c1), q2 = rs_ld(dst, c2);
        ok = rs_edge_ok(p0, p1, q0, q1, sim2, e2min) && rs_edge_ok(p1, p2, q1, q2, sim2, e2min) && rs_edge_ok(p2, p0, q2, q0, sim2, e2min) &&
             rs_triangle_ok(p0, p1, p2) && rs_triangle_ok(q0, q1, q2);
        if (ok) { atomicAdd(mult + c0, 1); atomicAdd(mult + c1, 1); atomicAdd(mult + c2, 1); }
    }
    const unsigned long long nv = (unsigned long long)__popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && nv) atomicAdd(acc, nv);
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// the grid of k_fgr_reduce: from m and PCR_FGR_BLOCKS alone (no device)
static int fgr_blocks(int64_t m) {
    const int64_t tiles = (m + FGR_TILE - 1) / FGR_TILE, groups = (tiles + FGR_W - 1) / FGR_W;
    const int64_t cap = env_i64("PCR_FGR_BLOCKS", FGR_MAX_BLOCKS, 1, FGR_MAX_BLOCKS);
    return (int)(groups < cap ? (groups > 0 ? groups : 1) : cap);
}
extern "C" int pcr_fgr_blocks(int64_t m) { return fgr_blocks(m < 0 ? 0 : m); }

// the largest match list k_fgr_solo serves: src, dst and mult (28 bytes a match) beside the kernel's own 4 KiB within the LDS
// one workgroup may use, as the device reports it; 0 in a build without the kernel
static pcr_status fgr_solo_max(const pcr_context *ctx, int64_t *m_max) {
    *m_max = 0;
#if FGR_HAVE_SOLO
    int lds = 0;
    HIP_TRY(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    if (lds > 4096) *m_max = ((int64_t)lds - 4096) / 28;
#endif
    return PCR_OK;
}
extern "C" pcr_status pcr_fgr_solo_max(pcr_context *ctx, int64_t *m_max) {
    PCR_REQUIRE(ctx && m_max, "NULL argument");
    return fgr_solo_max(ctx, m_max);
}

static bool fgr_positive(double v) { return v > 0 && v <= DBL_MAX; }

static pcr_status fgr_check_pairs(const float *src, const float *dst, int64_t m, const int32_t *mult, const char *who) {
    if (m < 0 || m > FGR_M_MAX) { pcr_set_error("invalid argument: %s needs 0 <= m <= 2^24", who); return PCR_ERR_INVALID; }
    if (m == 0) return PCR_OK;
    PCR_REQUIRE(src && dst, "NULL argument");
    PCR_TRY(check_finite(src, 3 * (size_t)m, "src and dst"));
    PCR_TRY(check_finite(dst, 3 * (size_t)m, "src and dst"));
    if (mult)
        for (int64_t i = 0; i < m; ++i)
            if (mult[i] < 0) { pcr_set_error("invalid argument: %s needs mult >= 0", who); return PCR_ERR_INVALID; }
    return PCR_OK;
}

// the device side of one call: the matches, the state, the tile rows
struct FgrCall {
    pcr_context *ctx = nullptr;
    int64_t m = 0;
    int ntiles = 0, nblocks = 0;
    DevBuf<float> src, dst;
    DevBuf<int32_t> mult;
    DevBuf<FgrDev> st;
    DevBuf<double> rows, sums, weight;

    pcr_status upload(pcr_context *c, const float *h_src, const float *h_dst, int64_t m_, const int32_t *h_mult) {
        ctx = c; m = m_;
        ntiles = (int)((m + FGR_TILE - 1) / FGR_TILE);
        nblocks = fgr_blocks(m);
        HIP_TRY(src.alloc(3 * (size_t)m)); HIP_TRY(dst.alloc(3 * (size_t)m)); HIP_TRY(st.alloc(1));
        HIP_TRY(rows.alloc(32 * (size_t)ntiles)); HIP_TRY(sums.alloc(32));
        HIP_TRY(hipMemcpyAsync(src.p, h_src, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dst.p, h_dst, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        if (h_mult) {
            HIP_TRY(mult.alloc((size_t)m));
            HIP_TRY(hipMemcpyAsync(mult.p, h_mult, 4 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        }
        return PCR_OK;
    }
    pcr_status put_state(const FgrDev *s) {
        HIP_TRY(hipMemcpyAsync(st.p, s, sizeof(FgrDev), hipMemcpyHostToDevice, ctx->stream));
        return PCR_OK;
    }
    pcr_status reduce() {
        hipLaunchKernelGGL(k_fgr_reduce, dim3((unsigned)nblocks), dim3(256), 0, ctx->stream, (const float *)src.p, (const float *)dst.p,
                           (const int32_t *)mult.p, m, ntiles, (const FgrDev *)st.p, rows.p);
        HIP_TRY(hipGetLastError());
        return PCR_OK;
    }
    // reduce + fold -> 29 doubles on the host, enqueued: the caller synchronises
    pcr_status pass(double out[29]) {
        PCR_TRY(reduce());
        hipLaunchKernelGGL(k_fgr_fold, dim3(1), dim3(64), 0, ctx->stream, (const double *)rows.p, ntiles, sums.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, sums.p, 29 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        return PCR_OK;
    }
    // the weights at the state on the device -> host, enqueued: the caller synchronises
    pcr_status weights(double *out) {
        HIP_TRY(weight.alloc((size_t)m));
        hipLaunchKernelGGL(k_fgr_weight, grid_for(m, 256), dim3(256), 0, ctx->stream, (const float *)src.p, (const float *)dst.p, m,
                           (const FgrDev *)st.p, weight.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, weight.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        return PCR_OK;
    }
    pcr_status sync() {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PCR_OK;
    }
};

extern "C" pcr_status pcr_fgr_linearize(pcr_context *ctx, const float *src, const float *dst, int64_t m, const int32_t *mult_or_null,
                                        const double T[16], double mu, double out[29], double *weight_or_null) {
    PCR_REQUIRE(ctx && T && out, "NULL argument");
    PCR_TRY(fgr_check_pairs(src, dst, m, mult_or_null, "pcr_fgr_linearize"));
    if (!fgr_positive(mu)) { pcr_set_error("invalid argument: pcr_fgr_linearize needs a finite mu > 0"); return PCR_ERR_INVALID; }
    if (m == 0) {
        for (int i = 0; i < 29; ++i) out[i] = 0.0;
        return PCR_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    FgrCall call;
    PCR_TRY(call.upload(ctx, src, dst, m, mult_or_null));
    FgrDev s = {};
    for (int i = 0; i < 16; ++i) s.T[i] = T[i];
    s.mu = s.mu_min = mu; s.division = 2; s.period = 1; s.max_iter = 1;
    PCR_TRY(call.put_state(&s));
    double o[29];
    std::vector<double> w;
    PCR_TRY(call.pass(o));
    if (weight_or_null) {
        w.resize((size_t)m);
        PCR_TRY(call.weights(w.data()));
    }
    PCR_TRY(call.sync());
    for (int i = 0; i < 29; ++i) out[i] = o[i];
    if (weight_or_null) for (int64_t i = 0; i < m; ++i) weight_or_null[i] = w[(size_t)i];
    return PCR_OK;
}

extern "C" pcr_status pcr_fgr_pose(pcr_context *ctx, const float *src, const float *dst, int64_t m, const int32_t *mult_or_null,
                                   const double T_init[16], double mu0, double mu_min, double division, int period, int max_iter, double tol,
                                   unsigned flags, double T_out[16], int *iterations, int *status, double *mu_final, double *weight_or_null,
                                   double *trace_or_null) {
    PCR_REQUIRE(ctx && T_init && T_out && iterations && status && mu_final, "NULL argument");
    PCR_TRY(fgr_check_pairs(src, dst, m, mult_or_null, "pcr_fgr_pose"));
    if (!fgr_positive(mu0) || !fgr_positive(mu_min)) { pcr_set_error("invalid argument: pcr_fgr_pose needs finite mu0 and mu_min > 0"); return PCR_ERR_INVALID; }
    if (!(division > 1 && division <= DBL_MAX)) { pcr_set_error("invalid argument: pcr_fgr_pose needs a finite division > 1"); return PCR_ERR_INVALID; }
    if (period < 1) { pcr_set_error("invalid argument: pcr_fgr_pose needs period >= 1"); return PCR_ERR_INVALID; }
    if (max_iter < 0) { pcr_set_error("invalid argument: pcr_fgr_pose needs max_iter >= 0"); return PCR_ERR_INVALID; }
    FgrDev s = {};
    for (int i = 0; i < 16; ++i) s.T[i] = T_init[i];
    s.mu = mu0; s.mu_min = mu_min; s.division = division; s.tol = tol; s.period = period; s.max_iter = max_iter;
    auto finish = [&]() {
        for (int i = 0; i < 16; ++i) T_out[i] = s.T[i];
        *iterations = s.iter; *status = s.status; *mu_final = s.mu;
    };
    if (m == 0 || max_iter == 0) {                             // no launch; the weights of no pass are 1: nothing has been down-weighted
        if (weight_or_null) for (int64_t i = 0; i < m; ++i) weight_or_null[i] = 1.0;
        if (trace_or_null) for (size_t i = 0; i < (size_t)max_iter * PCR_FGR_TRACE; ++i) trace_or_null[i] = 0.0;
        finish();
        return PCR_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    FgrCall call;
    PCR_TRY(call.upload(ctx, src, dst, m, mult_or_null));
    PCR_TRY(call.put_state(&s));
    std::vector<double> trace;
    if (trace_or_null) trace.assign((size_t)max_iter * PCR_FGR_TRACE, 0.0);
    DevBuf<double> d_trace;
    const bool host_loop = (flags & PCR_FLAG_HOST_LOOP) != 0;
    const bool times = env_flag("PCR_FGR_TIMES");              // developer (tools/fgr_time.py): the loop's milliseconds on stderr
    StageTimes ev;
    HIP_TRY(ev.init(times));
    bool solo = false;
    ev.mark(0, ctx->stream);
    if (host_loop) {
        double A[6][7], o[29];
        while (!s.done) {
            PCR_TRY(call.pass(o));
            PCR_TRY(call.sync());
            if (trace_or_null) {
                double *row = trace.data() + (size_t)s.iter * PCR_FGR_TRACE;
                for (int i = 0; i < 16; ++i) row[i] = s.T[i];
                for (int i = 0; i < 29; ++i) row[16 + i] = o[i];
                row[45] = s.mu;
            }
            fgr_step(A, o, &s);
            PCR_TRY(call.put_state(&s));
            PCR_TRY(call.sync());                              // s changes again before a pending copy would have read it
        }
    } else {
        if (trace_or_null) {
            HIP_TRY(d_trace.alloc(trace.size()));
            HIP_TRY(hipMemsetAsync(d_trace.p, 0, 8 * trace.size(), ctx->stream));
        }
        double *const d_tr = trace_or_null ? d_trace.p : (double *)nullptr;
#if FGR_HAVE_SOLO
        // PCR_FGR_SOLO=1 selects it for every list that fits: it lost the A/B, so the developer build too runs the launches unasked
        const size_t lds_bytes = 28 * (size_t)m;
        int64_t solo_max = 0;
        if (env_i64("PCR_FGR_SOLO", 0, 0, 1) == 1) PCR_TRY(fgr_solo_max(ctx, &solo_max));
        solo = m <= solo_max;
        if (solo) {
            HIP_TRY(hipFuncSetAttribute((const void *)k_fgr_solo, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
            hipLaunchKernelGGL(k_fgr_solo, dim3(1), dim3(256), lds_bytes, ctx->stream, (const float *)call.src.p, (const float *)call.dst.p,
                               (const int32_t *)call.mult.p, (int)m, call.ntiles, call.st.p, d_tr);
            HIP_TRY(hipGetLastError());
        }
#endif
        // every iteration enqueued back to back; a loop of more than FGR_QUEUE iterations looks at `done` in between
        for (int it = 0; !solo && it < max_iter; ) {
            const int n = max_iter - it < FGR_QUEUE ? max_iter - it : FGR_QUEUE;
            for (int k = 0; k < n; ++k) {
                PCR_TRY(call.reduce());
                hipLaunchKernelGGL(k_fgr_update, dim3(1), dim3(64), 0, ctx->stream, (const double *)call.rows.p, call.ntiles, call.st.p, d_tr);
            }
            HIP_TRY(hipGetLastError());
            it += n;
            if (it >= max_iter) break;
            HIP_TRY(hipMemcpyAsync(&s, call.st.p, sizeof(FgrDev), hipMemcpyDeviceToHost, ctx->stream));
            PCR_TRY(call.sync());
            if (s.done) break;
        }
    }
    ev.mark(1, ctx->stream);
    // what the call hands back rides behind the loop: ONE synchronisation
    std::vector<double> w;
    if (weight_or_null) {
        w.resize((size_t)m);
        PCR_TRY(call.weights(w.data()));
    }
    if (!host_loop) {
        if (trace_or_null) HIP_TRY(hipMemcpyAsync(trace.data(), d_trace.p, 8 * trace.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(&s, call.st.p, sizeof(FgrDev), hipMemcpyDeviceToHost, ctx->stream));
    }
    PCR_TRY(call.sync());
    if (ev.on)
        fprintf(stderr, "pcr_fgr_times pose m %lld iterations %d form %s blocks %d loop_ms %.4f\n", (long long)m, s.iter,
                host_loop ? "host" : (solo ? "solo" : "device"), call.nblocks, ev.ms(0));
    // nothing can fail from here: the outputs are written together
    if (weight_or_null) for (int64_t i = 0; i < m; ++i) weight_or_null[i] = w[(size_t)i];
    if (trace_or_null) for (size_t i = 0; i < trace.size(); ++i) trace_or_null[i] = trace[i];
    finish();
    return PCR_OK;
}

extern "C" pcr_status pcr_fgr_tuples(pcr_context *ctx, const float *src, const float *dst, int64_t m, int64_t n_tuples, uint64_t seed,
                                     float tuple_scale, float min_edge, int32_t *mult, int64_t *n_valid) {
    PCR_REQUIRE(ctx && n_valid, "NULL argument");
    if (n_tuples < 0 || n_tuples > FGR_H_MAX) { pcr_set_error("invalid argument: pcr_fgr_tuples needs 0 <= n_tuples <= 2^26"); return PCR_ERR_INVALID; }
    PCR_TRY(fgr_check_pairs(src, dst, m, nullptr, "pcr_fgr_tuples"));
    if (!(min_edge >= 0 && min_edge <= FLT_MAX)) { pcr_set_error("invalid argument: pcr_fgr_tuples needs a finite min_edge >= 0"); return PCR_ERR_INVALID; }
    if (!(tuple_scale >= 0 && tuple_scale <= 1)) { pcr_set_error("invalid argument: pcr_fgr_tuples needs 0 <= tuple_scale <= 1"); return PCR_ERR_INVALID; }
    PCR_REQUIRE(m == 0 || mult, "NULL argument");
    if (m < 3 || n_tuples == 0) {                              // no tuples
        for (int64_t i = 0; i < m; ++i) mult[i] = 0;
        *n_valid = 0;
        return PCR_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const double sim2 = (double)tuple_scale * (double)tuple_scale, e2min = (double)min_edge * (double)min_edge;
    const uint64_t s = rs_mix(seed);
    const int64_t chunk = env_i64("PCR_FGR_CHUNK", (int64_t)1 << 20, 1, FGR_H_MAX);
    DevBuf<float> d_src, d_dst;
    DevBuf<int32_t> d_mult;
    DevBuf<unsigned long long> d_acc;
    HIP_TRY(d_src.alloc(3 * (size_t)m)); HIP_TRY(d_dst.alloc(3 * (size_t)m)); HIP_TRY(d_mult.alloc((size_t)m)); HIP_TRY(d_acc.alloc(1));
    HIP_TRY(hipMemcpyAsync(d_src.p, src, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_dst.p, dst, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_mult.p, 0, 4 * (size_t)m, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_acc.p, 0, 8, ctx->stream));
    for (int64_t h0 = 0; h0 < n_tuples; h0 += chunk) {
        const int64_t n = n_tuples - h0 < chunk ? n_tuples - h0 : chunk;
        hipLaunchKernelGGL(k_fgr_tuples, grid_for(n, 256), dim3(256), 0, ctx->stream, (const float *)d_src.p, (const float *)d_dst.p, m, h0, n, s, sim2,
                           e2min, d_mult.p, d_acc.p);
        HIP_TRY(hipGetLastError());
    }
    std::vector<int32_t> h_mult((size_t)m);
    unsigned long long acc = 0;
    HIP_TRY(hipMemcpyAsync(h_mult.data(), d_mult.p, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&acc, d_acc.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < m; ++i) mult[i] = h_mult[(size_t)i];
    *n_valid = (int64_t)acc;
    return PCR_OK;
}
