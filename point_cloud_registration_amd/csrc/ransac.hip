// Pose hypotheses from correspondences (RANSAC) and pose scoring.  The contract is in include/pcr.h.
//
//   pcr_pose_score      k_pose_score
//   pcr_ransac_poses    per chunk of hypotheses: k_ransac_fit, k_pose_score, k_ransac_best
//
// k_ransac_fit: one lane = one hypothesis: the counter-based sample of three rows, the edge checks and the triad fit in float64
// (+, -, x, / and sqrt only, no contraction: this unit is built with -ffp-contract=off), 12 float32 out.  Six gathered points
// per lane; not the hot kernel.
//
// k_pose_score: one lane holds one pose in 12 registers (each value twice: 24 VGPRs) and walks all the rows, which reach the
// wave through LDS tiles read at one address by every lane: a broadcast.  The inlier rule is float32 without fma, two rows at
// a time in the halves of packed float32 operations (each half rounds as the scalar operation does).  The count is an
// integer, so splitting the rows over blockIdx.y and adding the partial counts with an integer atomic is exact.  Padding rows
// are NaN: a NaN is never an inlier, so the tail of a tile needs no test in the loop.  Measured alternatives (wave-uniform
// scalar loads instead of LDS, two poses per lane, 64- and 128-lane blocks) were slower: docs/EXPERIMENTS.md.
//
// k_ransac_best: the maximum over the 64-bit key (count + 1, ~h) of the valid hypotheses -- the largest count, ties to the
// smallest h -- by wave shuffles and one integer atomic maximum per wave: associative, so the winner does not depend on the
// grid or on the chunks.
#include "host_util.h"
#include "ransac_device.h"     // rs_mix, rs_sample, RsV3, rs_edge_ok: shared with fgr.hip

#define RS_TILE PCR_RANSAC_TILE      // rows per LDS tile
#define RS_BLOCK 256                 // poses per block, one per lane
#define RS_MAX_SPLIT 256
#define RS_FILL_BLOCKS 1024
#define RS_M_MAX ((int64_t)1 << 24)
#define RS_H_MAX ((int64_t)1 << 26)

typedef float rs_v2 __attribute__((ext_vector_type(2)));
typedef float rs_v4 __attribute__((ext_vector_type(4)));

// ---- the fit ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ RsV3 rs_div(RsV3 a, double s) { return RsV3{a.x / s, a.y / s, a.z / s}; }

// the triad of (p0, p1, p2): u1 along e1, u3 along e1 x e2, u2 = u3 x u1; false when the triangle is degenerate
__device__ __forceinline__ bool rs_triad(RsV3 p0, RsV3 p1, RsV3 p2, RsV3 &u1, RsV3 &u2, RsV3 &u3) {
    const RsV3 e1 = rs_sub(p1, p0), e2 = rs_sub(p2, p0), w = rs_cross(e1, e2);
    const double n1 = rs_dot(e1, e1), nw = rs_dot(w, w);
    if (!(n1 > 0.0 && nw > 0.0)) return false;
    u1 = rs_div(e1, __builtin_sqrt(n1));
    u3 = rs_div(w, __builtin_sqrt(nw));
    u2 = rs_cross(u3, u1);
    return true;
}

// hypotheses h0 .. h0 + n - 1 -> poses[i * 12] (all NaN: invalid), samples[i * 3] when not NULL
__global__ void __launch_bounds__(256) k_ransac_fit(const float *__restrict__ src, const float *__restrict__ dst, int64_t m, int64_t h0, int64_t n,
                                                    uint64_t s, double sim2, double e2min, float *poses, int32_t *samples) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t c0, c1, c2;
    rs_sample(s, (uint64_t)(h0 + i), (uint64_t)m, c0, c1, c2);
    if (samples) { samples[3 * i] = (int32_t)c0; samples[3 * i + 1] = (int32_t)c1; samples[3 * i + 2] = (int32_t)c2; }
    const RsV3 p0 = rs_ld(src, c0), p1 = rs_ld(src, c1), p2 = rs_ld(src, c2);
    const RsV3 q0 = rs_ld(dst, c0), q1 = rs_ld(dst, c1), q2 = rs_ld(dst, c2);
    bool ok = rs_edge_ok(p0, p1, q0, q1, sim2, e2min) && rs_edge_ok(p1, p2, q1, q2, sim2, e2min) && rs_edge_ok(p2, p0, q2, q0, sim2, e2min);
    RsV3 u1, u2, u3, v1, v2, v3;
    u1 = u2 = u3 = v1 = v2 = v3 = RsV3{0.0, 0.0, 0.0};
    ok = ok && rs_triad(p0, p1, p2, u1, u2, u3);
    ok = ok && rs_triad(q0, q1, q2, v1, v2, v3);
    float *out = poses + 12 * i;
    if (!ok) {
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 12; ++k) out[k] = nan;
        return;
    }
    const double a1[3] = {v1.x, v1.y, v1.z}, a2[3] = {v2.x, v2.y, v2.z}, a3[3] = {v3.x, v3.y, v3.z};
    const double b1[3] = {u1.x, u1.y, u1.z}, b2[3] = {u2.x, u2.y, u2.z}, b3[3] = {u3.x, u3.y, u3.z};
    const double cp[3] = {((p0.x + p1.x) + p2.x) / 3.0, ((p0.y + p1.y) + p2.y) / 3.0, ((p0.z + p1.z) + p2.z) / 3.0};
    const double cq[3] = {((q0.x + q1.x) + q2.x) / 3.0, ((q0.y + q1.y) + q2.y) / 3.0, ((q0.z + q1.z) + q2.z) / 3.0};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double R[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            R[c] = (a1[r] * b1[c] + a2[r] * b2[c]) + a3[r] * b3[c];
            out[3 * r + c] = (float)R[c];
        }
        out[9 + r] = (float)(cq[r] - ((R[0] * cp[0] + R[1] * cp[1]) + R[2] * cp[2]));
    }
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------
// the squared residuals of two (pose, row) pairs, one per half
__device__ __forceinline__ rs_v2 rs_d2(const rs_v2 *P, rs_v2 px, rs_v2 py, rs_v2 pz, rs_v2 qx, rs_v2 qy, rs_v2 qz) {
    const rs_v2 x = ((P[0] * px + P[1] * py) + P[2] * pz) + P[9];
    const rs_v2 y = ((P[3] * px + P[4] * py) + P[5] * pz) + P[10];
    const rs_v2 z = ((P[6] * px + P[7] * py) + P[8] * pz) + P[11];
    const rs_v2 dx = x - qx, dy = y - qy, dz = z - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// One pose per lane, two rows per packed operation.  Rows [blockIdx.y * rows_per_split, ...) of m; count[i] is stored when
// gridDim.y == 1, else added to (the caller zeroes it).  mask (MASK): b x m bytes.
template <bool MASK>
__global__ void __launch_bounds__(RS_BLOCK) k_pose_score(const float *__restrict__ src, const float *__restrict__ dst, int64_t m,
                                                         const float *__restrict__ poses, int64_t b, float thr, int64_t rows_per_split,
                                                         int32_t *count, uint8_t *mask) {
    __shared__ rs_v4 s_tile[RS_TILE / 2 * 3];
    float *tile = (float *)s_tile;
    const float nan = __int_as_float(0x7fc00000);
    const int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    const int64_t j_lo = (int64_t)blockIdx.y * rows_per_split;
    const int64_t j_hi = j_lo + rows_per_split < m ? j_lo + rows_per_split : m;
    rs_v2 P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float a = i < b ? poses[i * 12 + k] : nan;
        P[k] = (rs_v2){a, a};
    }
    int n0 = 0, n1 = 0;
    for (int64_t j0 = j_lo; j0 < j_hi; j0 += RS_TILE) {
        const int rows = (int)(j_hi - j0 < RS_TILE ? j_hi - j0 : RS_TILE);
        __syncthreads();                               // the previous tile has been read by every lane
        // rows 2 r and 2 r + 1 interleaved: {pxa pxb pya pyb} {pza pzb qxa qxb} {qya qyb qza qzb}
        for (int e = threadIdx.x; e < RS_TILE; e += RS_BLOCK) {
            float *t = tile + (e >> 1) * 12 + (e & 1);
            const bool in = e < rows;
            const float *p = src + (j0 + e) * 3, *q = dst + (j0 + e) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                t[2 * c] = in ? p[c] : nan;
                t[6 + 2 * c] = in ? q[c] : nan;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int row = 0; row < rows; row += 2) {
            const rs_v4 *t = s_tile + (row >> 1) * 3;
            const rs_v4 A = t[0], B = t[1], Cq = t[2];
            const rs_v2 d2 = rs_d2(P, A.xy, A.zw, B.xy, B.zw, Cq.xy, Cq.zw);
            const int ia = d2.x <= thr, ib = d2.y <= thr;
            n0 += ia; n1 += ib;
            if (MASK && i < b) {
                mask[i * m + j0 + row] = (uint8_t)ia;
                if (row + 1 < rows) mask[i * m + j0 + row + 1] = (uint8_t)ib;
            }
        }
    }
    if (i < b) {
        if (gridDim.y == 1) count[i] = n0 + n1;
        else atomicAdd(count + i, n0 + n1);
    }
}

// ---- the best hypothesis ----------------------------------------------------------------------------------------------------
// counts[i] = -1 for the invalid hypotheses (an all-NaN pose); acc[0] = max key, acc[1] += valid hypotheses
__global__ void __launch_bounds__(256) k_ransac_best(const float *__restrict__ poses, int32_t *counts, int64_t h0, int64_t n,
                                                     unsigned long long *acc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long key = 0ull;
    bool valid = false;
    if (i < n) {
        const float r00 = poses[12 * i];
        valid = r00 == r00;
        if (valid) key = ((unsigned long long)(uint32_t)(counts[i] + 1) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)(h0 + i));
        else counts[i] = -1;
    }
    const unsigned long long nv = (unsigned long long)__popcll(__ballot(valid));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) {
        if (key) atomicMax(acc, key);
        if (nv) atomicAdd(acc + 1, nv);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// PCR_RANSAC_TIMES=1 (developer, tools/ransac_time.py): the calls bracket their kernels with events and report the milliseconds
// on stderr (StageTimes).  PCR_RANSAC_CHUNK: hypotheses per chunk (default 2^20).  Both are read once per process.

// splits of the rows: with few poses, enough blocks to fill the chip (RS_FILL_BLOCKS: on 256 CUs, 16 poses over 10^6 rows take
// 49 ms unsplit, 0.81 ms in 64 splits, 0.23 ms in 245), whole tiles per split; from b and m alone
static int rs_splits(int64_t m, int64_t b, int64_t *rows_out) {
    int64_t rows = m;
    int ny = 1;
    if (m > 0 && b > 0) {
        const int64_t gx = (b + RS_BLOCK - 1) / RS_BLOCK, tiles = (m + RS_TILE - 1) / RS_TILE;
        int64_t want = (RS_FILL_BLOCKS + gx - 1) / gx;
        if (want > RS_MAX_SPLIT) want = RS_MAX_SPLIT;
        if (want > tiles) want = tiles;
        if (want > 1) {
            rows = (m + want - 1) / want;
            rows = (rows + RS_TILE - 1) / RS_TILE * RS_TILE;
            ny = (int)((m + rows - 1) / rows);
        }
    }
    if (rows_out) *rows_out = rows;
    return ny;
}

extern "C" int pcr_pose_score_splits(int64_t m, int64_t b) { return rs_splits(m, b, nullptr); }

// device arrays throughout; m >= 1, b >= 1
static pcr_status rs_score(pcr_context *ctx, const float *d_src, const float *d_dst, int64_t m, const float *d_poses, int64_t b, float thr,
                           int32_t *d_count, uint8_t *d_mask, int *splits_out) {
    int64_t rows = m;
    const int ny = rs_splits(m, b, &rows);
    if (ny > 1) HIP_TRY(hipMemsetAsync(d_count, 0, 4 * (size_t)b, ctx->stream));
    const dim3 grid(grid_for(b, RS_BLOCK).x, (unsigned)ny), blk(RS_BLOCK);
    if (d_mask) hipLaunchKernelGGL(k_pose_score<true>, grid, blk, 0, ctx->stream, d_src, d_dst, m, d_poses, b, thr, rows, d_count, d_mask);
    else hipLaunchKernelGGL(k_pose_score<false>, grid, blk, 0, ctx->stream, d_src, d_dst, m, d_poses, b, thr, rows, d_count, d_mask);
    HIP_TRY(hipGetLastError());
    if (splits_out) *splits_out = ny;
    return PCR_OK;
}

static bool rs_all_finite(const float *a, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!(a[i] >= -FLT_MAX && a[i] <= FLT_MAX)) return false;
    return true;
}

static pcr_status rs_check_pairs(const float *src, const float *dst, int64_t m, float max_dist, const char *who) {
    if (m < 0 || m > RS_M_MAX) { pcr_set_error("invalid argument: %s needs 0 <= m <= 2^24", who); return PCR_ERR_INVALID; }
    if (!(max_dist >= 0 && max_dist <= FLT_MAX)) { pcr_set_error("invalid argument: %s needs a finite max_dist >= 0", who); return PCR_ERR_INVALID; }
    if (m > 0) {
        PCR_REQUIRE(src && dst, "NULL argument");
        if (!rs_all_finite(src, 3 * m) || !rs_all_finite(dst, 3 * m)) {
            pcr_set_error("invalid argument: %s needs finite src and dst", who);
            return PCR_ERR_INVALID;
        }
    }
    return PCR_OK;
}

extern "C" pcr_status pcr_pose_score(pcr_context *ctx, const float *src, const float *dst, int64_t m, const float *poses, int64_t b,
                                     float max_dist, int32_t *count, uint8_t *mask_or_null) {
    PCR_REQUIRE(ctx, "NULL argument");
    PCR_REQUIRE(b >= 0 && b <= RS_H_MAX, "pcr_pose_score needs 0 <= b <= 2^26");
    PCR_TRY(rs_check_pairs(src, dst, m, max_dist, "pcr_pose_score"));
    if (b == 0) return PCR_OK;
    PCR_REQUIRE(poses && count, "NULL argument");
    if (m == 0) {
        for (int64_t i = 0; i < b; ++i) count[i] = 0;
        return PCR_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const float thr = max_dist * max_dist;
    DevBuf<float> d_src, d_dst, d_poses;
    DevBuf<int32_t> d_count;
    DevBuf<uint8_t> d_mask;
    HIP_TRY(d_src.alloc(3 * (size_t)m)); HIP_TRY(d_dst.alloc(3 * (size_t)m)); HIP_TRY(d_poses.alloc(12 * (size_t)b));
    HIP_TRY(d_count.alloc((size_t)b));
    if (mask_or_null) HIP_TRY(d_mask.alloc((size_t)b * (size_t)m));
    HIP_TRY(hipMemcpyAsync(d_src.p, src, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_dst.p, dst, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_poses.p, poses, 48 * (size_t)b, hipMemcpyHostToDevice, ctx->stream));
    static const bool times = env_flag("PCR_RANSAC_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    int ny = 1;
    ev.mark(0, ctx->stream);
    PCR_TRY(rs_score(ctx, d_src.p, d_dst.p, m, d_poses.p, b, thr, d_count.p, mask_or_null ? d_mask.p : (uint8_t *)nullptr, &ny));
    ev.mark(1, ctx->stream);
    HIP_TRY(hipMemcpyAsync(count, d_count.p, 4 * (size_t)b, hipMemcpyDeviceToHost, ctx->stream));
    if (mask_or_null) HIP_TRY(hipMemcpyAsync(mask_or_null, d_mask.p, (size_t)b * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on)
        fprintf(stderr, "pcr_ransac_times score m %lld b %lld splits %d score_ms %.4f\n", (long long)m, (long long)b, ny, ev.ms(0));
    return PCR_OK;
}

extern "C" pcr_status pcr_ransac_poses(pcr_context *ctx, const float *src, const float *dst, int64_t m, int64_t n_hyp, uint64_t seed,
                                       float max_dist, float edge_similarity, float min_edge, int64_t *best, float best_pose[12],
                                       int32_t *best_count, int64_t *n_valid, int32_t *samples_or_null, float *poses_or_null,
                                       int32_t *counts_or_null) {
    PCR_REQUIRE(ctx, "NULL argument");
    if (n_hyp < 0 || n_hyp > RS_H_MAX) { pcr_set_error("invalid argument: pcr_ransac_poses needs 0 <= n_hyp <= 2^26"); return PCR_ERR_INVALID; }
    PCR_TRY(rs_check_pairs(src, dst, m, max_dist, "pcr_ransac_poses"));
    if (!(min_edge >= 0 && min_edge <= FLT_MAX)) { pcr_set_error("invalid argument: pcr_ransac_poses needs a finite min_edge >= 0"); return PCR_ERR_INVALID; }
    if (!(edge_similarity >= 0 && edge_similarity <= 1)) {
        pcr_set_error("invalid argument: pcr_ransac_poses needs 0 <= edge_similarity <= 1");
        return PCR_ERR_INVALID;
    }
    PCR_REQUIRE(best && best_pose && best_count && n_valid, "NULL argument");
    *best = -1; *best_count = 0; *n_valid = 0;
    for (int k = 0; k < 12; ++k) best_pose[k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f;
    if (n_hyp == 0) return PCR_OK;
    if (m < 3) {                                          // no hypotheses: every one of them reads as invalid
        for (int64_t i = 0; i < n_hyp; ++i) {
            if (samples_or_null) samples_or_null[3 * i] = samples_or_null[3 * i + 1] = samples_or_null[3 * i + 2] = -1;
            if (poses_or_null) for (int k = 0; k < 12; ++k) poses_or_null[12 * i + k] = __builtin_nanf("");
            if (counts_or_null) counts_or_null[i] = -1;
        }
        return PCR_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const float thr = max_dist * max_dist;
    const double sim2 = (double)edge_similarity * (double)edge_similarity, e2min = (double)min_edge * (double)min_edge;
    const uint64_t s = rs_mix(seed);
    static const int64_t chunk_max = env_i64("PCR_RANSAC_CHUNK", (int64_t)1 << 20, 1, RS_H_MAX);
    const int64_t chunk = chunk_max < n_hyp ? chunk_max : n_hyp;
    DevBuf<float> d_src, d_dst, d_poses;
    DevBuf<int32_t> d_count, d_samples;
    DevBuf<unsigned long long> d_acc;
    HIP_TRY(d_src.alloc(3 * (size_t)m)); HIP_TRY(d_dst.alloc(3 * (size_t)m));
    HIP_TRY(d_poses.alloc(12 * (size_t)chunk)); HIP_TRY(d_count.alloc((size_t)chunk)); HIP_TRY(d_acc.alloc(2));
    if (samples_or_null) HIP_TRY(d_samples.alloc(3 * (size_t)chunk));
    HIP_TRY(hipMemcpyAsync(d_src.p, src, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_dst.p, dst, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_acc.p, 0, 16, ctx->stream));
    static const bool times = env_flag("PCR_RANSAC_TIMES");
    double fit_ms = 0, score_ms = 0, best_ms = 0;
    for (int64_t h0 = 0; h0 < n_hyp; h0 += chunk) {
        const int64_t n = n_hyp - h0 < chunk ? n_hyp - h0 : chunk;
        const dim3 grid = grid_for(n, 256);
        StageTimes ev;                                    // fit | score | best
        HIP_TRY(ev.init(times));
        ev.mark(0, ctx->stream);
        hipLaunchKernelGGL(k_ransac_fit, grid, dim3(256), 0, ctx->stream, (const float *)d_src.p, (const float *)d_dst.p, m, h0, n, s, sim2, e2min,
                           d_poses.p, samples_or_null ? d_samples.p : (int32_t *)nullptr);
        HIP_TRY(hipGetLastError());
        ev.mark(1, ctx->stream);
        PCR_TRY(rs_score(ctx, d_src.p, d_dst.p, m, d_poses.p, n, thr, d_count.p, nullptr, nullptr));
        ev.mark(2, ctx->stream);
        hipLaunchKernelGGL(k_ransac_best, grid, dim3(256), 0, ctx->stream, (const float *)d_poses.p, d_count.p, h0, n, d_acc.p);
        HIP_TRY(hipGetLastError());
        ev.mark(3, ctx->stream);
        if (samples_or_null) HIP_TRY(hipMemcpyAsync(samples_or_null + 3 * h0, d_samples.p, 12 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        if (poses_or_null) HIP_TRY(hipMemcpyAsync(poses_or_null + 12 * h0, d_poses.p, 48 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        if (counts_or_null) HIP_TRY(hipMemcpyAsync(counts_or_null + h0, d_count.p, 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        if (times) { fit_ms += ev.ms(0); score_ms += ev.ms(1); best_ms += ev.ms(2); }
    }
    unsigned long long acc[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(acc, d_acc.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_valid = (int64_t)acc[1];
    if (acc[0]) {
        const int64_t h = (int64_t)(0xffffffffu - (uint32_t)acc[0]);
        *best = h;
        *best_count = (int32_t)(uint32_t)(acc[0] >> 32) - 1;
        // the winner's pose again: a hypothesis depends on (seed, h, m) only
        hipLaunchKernelGGL(k_ransac_fit, dim3(1), dim3(256), 0, ctx->stream, (const float *)d_src.p, (const float *)d_dst.p, m, h, (int64_t)1, s, sim2,
                           e2min, d_poses.p, (int32_t *)nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(best_pose, d_poses.p, 48, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (times)
        fprintf(stderr, "pcr_ransac_times ransac m %lld n_hyp %lld chunk %lld fit_ms %.4f score_ms %.4f best_ms %.4f\n", (long long)m,
                (long long)n_hyp, (long long)chunk, fit_ms, score_ms, best_ms);
    return PCR_OK;
}
