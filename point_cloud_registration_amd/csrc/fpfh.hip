// FPFH descriptors (Rusu, Blodow, Beetz: Fast Point Feature Histograms for 3D registration, ICRA 2009; the Open3D form) of a
// point target that has normals, and exact nearest-neighbour matching of descriptors.  The contract is in include/pcr.h.
//
//   pcr_target_spfh     k_spfh<1>                       counts and k in the caller's order (the seam of the exact test)
//   pcr_target_fpfh     k_spfh<0>, k_fpfh               float32 (n, 33) in the caller's order
//   pcr_target_fpfh_rows  k_spfh<0>, k_fpfh_row_index, k_fpfh_rows   float32 (m, 33): the descriptors of m chosen rows
//   pcr_feature_match   k_feature_nn<D>, k_feature_merge
//
// k_spfh / k_fpfh: one lane = one point in CELL-SORTED order, so the lanes of a wave are spatial neighbours; both walk the
// point's ball with rad_ball_walk (radius_device.h), the walk of pcr_radius_query, so the neighbourhood IS the radius search's
// minus the pairs at d2 == 0.  No atomics, the grid depends on n only: two calls return the same bits.
//   k_spfh   the sink gathers pn[j] (point + normal, one 32-byte sector), forms the pair feature in float64 and bumps three of
//            the lane's 33 counters.  The counters are dynamically indexed, so they live in LDS as [bin][lane]: a lane's column
//            is its own bank (8448 bytes per 64-lane block), nothing is shared, nothing has to be synchronised.
//   k_fpfh   the same walk again; the sink gathers the neighbour's 33 counts and k at its cell-sorted index and adds
//            S_j[b] / d2 into 33 float64 accumulators (statically indexed: registers), then normalises per 11-bin block, adds
//            the lane's own SPFH, rounds to float32 and stores at the point's original index.
// The integer counts make the first pass independent of the visiting order; the second sums at most a few hundred float64
// terms in walk order, ~1e-14 relative, far below half a float32 ulp.
//
// k_feature_nn: one lane holds one row of A in registers, the rows of B pass through LDS in tiles of FNN_TILE rows (every
// lane reads the same address: a broadcast), d2 is the float32 sum over the columns in order -- separate subtract, multiply
// and add, this unit is built with -ffp-contract=off; two rows of B at a time in the halves of packed float32 operations --
// and each lane keeps the two smallest keys (bits(d2) << 32) | j; a NaN distance maps to the largest key and never wins.
// B is split over blockIdx.y so that a few ten thousand rows of A still fill the chip; a minimum over keys is associative,
// so k_feature_merge's merge of the per-split top-2 is exact and the result does not depend on the split.  D = 33 is its own
// instantiation; every other width runs the D = 64 one over rows padded with zeros ((0 - 0)^2 added to a float32 sum changes
// no bit).
#include "radius_device.h"

#define FPFH_BINS 33
#define FPFH_BLOCK RAD_BLOCK

// ---- the pair feature -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fp_dot(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}
// clamp(floor(c), 0, 10); NaN -> 0
__device__ __forceinline__ int fp_bin(double c) { return c >= 1.0 ? (c >= 10.0 ? 10 : (int)c) : 0; }

// p = the point, q = its neighbour, d2 = |q - p|^2 > 0 as (dx*dx + dy*dy) + dz*dz: the three bins (alpha, phi, theta)
__device__ __forceinline__ void fp_pair_bins(const PtN &p, const PtN &q, double dx, double dy, double dz, double d2, int &ba, int &bp, int &bt) {
    const double L = __builtin_sqrt(d2);
    const double a1 = fp_dot((double)p.nx, (double)p.ny, (double)p.nz, dx, dy, dz);
    const double a2 = fp_dot((double)q.nx, (double)q.ny, (double)q.nz, dx, dy, dz);
    const bool swap = fabs(a1) < fabs(a2);
    const double n1x = swap ? (double)q.nx : (double)p.nx, n1y = swap ? (double)q.ny : (double)p.ny, n1z = swap ? (double)q.nz : (double)p.nz;
    const double n2x = swap ? (double)p.nx : (double)q.nx, n2y = swap ? (double)p.ny : (double)q.ny, n2z = swap ? (double)p.nz : (double)q.nz;
    if (swap) { dx = -dx; dy = -dy; dz = -dz; }
    const double phi = fp_dot(n1x, n1y, n1z, dx, dy, dz) / L;
    double vx = dy * n1z - dz * n1y, vy = dz * n1x - dx * n1z, vz = dx * n1y - dy * n1x;
    const double vv = fp_dot(vx, vy, vz, vx, vy, vz);
    double alpha = 0.0, theta = 0.0;
    if (vv != 0.0) {
        const double vn = __builtin_sqrt(vv);
        vx = vx / vn; vy = vy / vn; vz = vz / vn;
        const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
        alpha = fp_dot(vx, vy, vz, n2x, n2y, n2z);
        theta = atan2(fp_dot(wx, wy, wz, n2x, n2y, n2z), fp_dot(n1x, n1y, n1z, n2x, n2y, n2z));
    }
    const double pi = 3.141592653589793;
    ba = fp_bin(11.0 * (alpha + 1.0) / 2.0);
    bp = fp_bin(11.0 * (phi + 1.0) / 2.0);
    bt = fp_bin(11.0 * (theta + pi) / (2.0 * pi));
}

// ---- the sinks ------------------------------------------------------------------------------------------------------------
struct SpfhSink {
    float r, b2;
    PtN me;
    const PtN *pn;
    uint32_t *cnt;       // the lane's column of the block's [bin][lane] counters
    uint32_t k;
    __device__ __forceinline__ float bound() const { return b2; }
    __device__ __forceinline__ void offer(float d2f, uint32_t j, uint32_t) {
        if (d2f <= b2 && rad_member(d2f, r)) {                               // (NaN fails the pre-test)
            const PtN q = pn[j];
            const double dx = (double)q.x - (double)me.x, dy = (double)q.y - (double)me.y, dz = (double)q.z - (double)me.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 != 0.0) {
                int ba, bp, bt;
                fp_pair_bins(me, q, dx, dy, dz, d2, ba, bp, bt);
                cnt[ba * FPFH_BLOCK] += 1u;
                cnt[(11 + bp) * FPFH_BLOCK] += 1u;
                cnt[(22 + bt) * FPFH_BLOCK] += 1u;
                ++k;
            }
        }
    }
};

struct FpfhSink {
    float r, b2;
    float mx, my, mz;
    const PtF *pts;
    const uint32_t *counts;     // [n][33], cell-sorted
    const uint32_t *kk;         // [n], cell-sorted
    double acc[FPFH_BINS];
    __device__ __forceinline__ float bound() const { return b2; }
    __device__ __forceinline__ void offer(float d2f, uint32_t j, uint32_t) {
        if (d2f <= b2 && rad_member(d2f, r)) {
            const PtF q = pts[j];
            const double dx = (double)q.x - (double)mx, dy = (double)q.y - (double)my, dz = (double)q.z - (double)mz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const uint32_t kj = kk[j];
            if (d2 != 0.0 && kj != 0u) {
                const uint32_t *c = counts + (size_t)j * FPFH_BINS;
                const double kd = (double)kj;
#pragma unroll
                for (int b = 0; b < FPFH_BINS; ++b) acc[b] += ((100.0 * (double)c[b]) / kd) / d2;
            }
        }
    }
};

// ORIG = 0: counts / k at the lane's cell-sorted index (what k_fpfh gathers); 1: at the point's original index
template <int ORIG>
__global__ void __launch_bounds__(FPFH_BLOCK) k_spfh(Geom<float> g, const PtF *pts, const PtN *pn, const uint32_t *cs, int64_t n, float r,
                                                     uint32_t *counts, uint32_t *kk) {
    __shared__ uint32_t s_cnt[FPFH_BINS * FPFH_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * FPFH_BLOCK + threadIdx.x;
    if (i >= n) return;
    SpfhSink S;
    S.r = r; S.b2 = rad_bound2(r); S.me = pn[i]; S.pn = pn; S.cnt = s_cnt + threadIdx.x; S.k = 0;
#pragma unroll
    for (int b = 0; b < FPFH_BINS; ++b) S.cnt[b * FPFH_BLOCK] = 0u;
    if (rad_finite(S.me.x, S.me.y, S.me.z)) rad_ball_walk(g, pts, cs, S.me.x, S.me.y, S.me.z, r, S);
    const int64_t o = ORIG ? (int64_t)S.me.orig : i;
#pragma unroll
    for (int b = 0; b < FPFH_BINS; ++b) counts[o * FPFH_BINS + b] = S.cnt[b * FPFH_BLOCK];
    kk[o] = S.k;
}

// the end of k_fpfh and k_fpfh_rows: the lane's own SPFH (counts c, k = ki) plus its normalised sums, one float32 row
__device__ __forceinline__ void fpfh_finish(const FpfhSink &S, const uint32_t *c, uint32_t ki, float *row) {
    const double kd = (double)(ki ? ki : 1u);
#pragma unroll
    for (int blk = 0; blk < 3; ++blk) {
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < 11; ++b) sum += S.acc[11 * blk + b];
#pragma unroll
        for (int b = 0; b < 11; ++b) {
            const double own = (100.0 * (double)c[11 * blk + b]) / kd;        // (k == 0: every count is 0)
            const double nb = sum > 0.0 ? (100.0 * S.acc[11 * blk + b]) / sum : 0.0;
            row[11 * blk + b] = (float)(own + nb);
        }
    }
}

// the walk of k_fpfh and k_fpfh_rows for the point at cell-sorted index i
__device__ __forceinline__ void fpfh_walk(const Geom<float> &g, const PtF *pts, const uint32_t *cs, float r, const uint32_t *counts,
                                          const uint32_t *kk, const PtF &me, FpfhSink &S) {
    S.r = r; S.b2 = rad_bound2(r); S.mx = me.x; S.my = me.y; S.mz = me.z; S.pts = pts; S.counts = counts; S.kk = kk;
#pragma unroll
    for (int b = 0; b < FPFH_BINS; ++b) S.acc[b] = 0.0;
    if (rad_finite(me.x, me.y, me.z)) rad_ball_walk(g, pts, cs, me.x, me.y, me.z, r, S);
}

__global__ void __launch_bounds__(FPFH_BLOCK) k_fpfh(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n, float r,
                                                     const uint32_t *counts, const uint32_t *kk, float *out, int64_t *k_out) {
    const int64_t i = (int64_t)blockIdx.x * FPFH_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    FpfhSink S;
    fpfh_walk(g, pts, cs, r, counts, kk, me, S);
    const uint32_t ki = kk[i];
    fpfh_finish(S, counts + (size_t)i * FPFH_BINS, ki, out + (size_t)pt_orig(me) * FPFH_BINS);
    if (k_out) k_out[pt_orig(me)] = (int64_t)ki;
}

// descriptors at chosen rows.  slot_of[original index] = the row's place in the caller's list, or -1: every selected point
// stores its cell-sorted index at its slot (the slots are unique: a plain store)
__global__ void __launch_bounds__(256) k_fpfh_row_index(const PtF *pts, int64_t n, const int32_t *slot_of, uint32_t *sel) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t s = slot_of[pt_orig(pts[i])];
    if (s >= 0) sel[s] = (uint32_t)i;
}

// one lane = one selected row, in the caller's (ascending) order; the walk, its order and the finish are k_fpfh's, so row
// `slot` equals row rows[slot] of pcr_target_fpfh bit for bit
__global__ void __launch_bounds__(FPFH_BLOCK) k_fpfh_rows(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t m, float r,
                                                          const uint32_t *counts, const uint32_t *kk, const uint32_t *sel, float *out,
                                                          int64_t *k_out) {
    const int64_t slot = (int64_t)blockIdx.x * FPFH_BLOCK + threadIdx.x;
    if (slot >= m) return;
    const size_t i = sel[slot];
    const PtF me = pts[i];
    FpfhSink S;
    fpfh_walk(g, pts, cs, r, counts, kk, me, S);
    const uint32_t ki = kk[i];
    fpfh_finish(S, counts + i * FPFH_BINS, ki, out + (size_t)slot * FPFH_BINS);
    if (k_out) k_out[slot] = (int64_t)ki;
}

// ---- feature matching -----------------------------------------------------------------------------------------------------
#define FNN_BLOCK 256        // rows of A per block, one per lane
#define FNN_TILE 64          // rows of B per LDS tile
#define FNN_MAX_SPLIT 64
#define FNN_KEY_NONE 0xffffffffffffffffull

__device__ __forceinline__ void fnn_insert(uint64_t key, uint64_t &k1, uint64_t &k2) {
    const bool first = key < k1;
    const uint64_t lose = first ? k1 : key;      // whichever of the two is not the smallest
    k1 = first ? key : k1;
    k2 = lose < k2 ? lose : k2;
}

__device__ __forceinline__ uint64_t fnn_key(float d2, int64_t j) {
    return d2 == d2 ? ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)(uint32_t)j : FNN_KEY_NONE;
}

// rows [j_lo, j_hi) of B against row i of A; D columns computed, `dim` of them real and the rest zero.  A lane takes the rows
// of B two at a time, as the two halves of float2 operations (v_pk_add_f32 / v_pk_mul_f32: each half rounds as the scalar
// operation does, and there is no packed fma to contract into): the tile holds rows 2 p and 2 p + 1 interleaved column by
// column, a[] holds every value of the lane's row twice.  part[(i * gridDim.y + y) * 2 + {0, 1}] = the two smallest keys of
// split y.
typedef float fnn_v2 __attribute__((ext_vector_type(2)));
typedef float fnn_v4 __attribute__((ext_vector_type(4)));
template <int D>
__global__ void __launch_bounds__(FNN_BLOCK) k_feature_nn(const float *__restrict__ A, int64_t na, const float *__restrict__ B, int64_t nb, int dim,
                                                          int64_t chunk, uint64_t *part) {
    constexpr int DP = (D + 1) & ~1;                 // columns of a row pair: two columns (of two rows) to a 16-byte slot
    __shared__ fnn_v4 s_tile[FNN_TILE / 2 * DP / 2];
    float *tile = (float *)s_tile;
    const int64_t i = (int64_t)blockIdx.x * FNN_BLOCK + threadIdx.x;
    const int64_t j_lo = (int64_t)blockIdx.y * chunk;
    const int64_t j_hi = j_lo + chunk < nb ? j_lo + chunk : nb;
    fnn_v2 a[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const float v = (i < na && c < dim) ? A[i * dim + c] : 0.f;
        a[c] = (fnn_v2){v, v};
    }
    uint64_t k1 = FNN_KEY_NONE, k2 = FNN_KEY_NONE;
    for (int64_t j0 = j_lo; j0 < j_hi; j0 += FNN_TILE) {
        const int rows = (int)(j_hi - j0 < FNN_TILE ? j_hi - j0 : FNN_TILE);
        __syncthreads();                               // the previous tile has been read by every lane
        for (int e = threadIdx.x; e < FNN_TILE * DP; e += FNN_BLOCK) {
            const int row = e / DP, c = e - row * DP;
            tile[((row >> 1) * DP + c) * 2 + (row & 1)] = (row < rows && c < dim) ? B[(j0 + row) * dim + c] : 0.f;
        }
        __syncthreads();
        for (int row = 0; row < rows; row += 2) {
            const fnn_v4 *b4 = s_tile + (row >> 1) * (DP / 2);
            fnn_v2 d2 = {0.f, 0.f};
#pragma unroll
            for (int c2 = 0; c2 < DP / 2; ++c2) {
                const fnn_v4 b = b4[c2];
                const fnn_v2 t0 = a[2 * c2] - b.xy;
                d2 = d2 + t0 * t0;
                if (2 * c2 + 1 < D) {
                    const fnn_v2 t1 = a[2 * c2 + 1] - b.zw;
                    d2 = d2 + t1 * t1;
                }
            }
            fnn_insert(fnn_key(d2.x, j0 + row), k1, k2);
            if (row + 1 < rows) fnn_insert(fnn_key(d2.y, j0 + row + 1), k1, k2);      // (an odd tail: the other half is padding)
        }
    }
    if (i < na) {
        uint64_t *p = part + ((size_t)i * gridDim.y + blockIdx.y) * 2;
        p[0] = k1; p[1] = k2;
    }
}

__global__ void __launch_bounds__(256) k_feature_merge(const uint64_t *__restrict__ part, int64_t na, int splits, int64_t *idx, float *d2_first,
                                                       float *d2_second) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    uint64_t k1 = FNN_KEY_NONE, k2 = FNN_KEY_NONE;
    const uint64_t *p = part + (size_t)i * splits * 2;
    for (int s = 0; s < 2 * splits; ++s) fnn_insert(p[s], k1, k2);
    const float inf = __int_as_float(0x7f800000);
    idx[i] = k1 == FNN_KEY_NONE ? (int64_t)-1 : (int64_t)(uint32_t)k1;
    d2_first[i] = k1 == FNN_KEY_NONE ? inf : __uint_as_float((uint32_t)(k1 >> 32));
    d2_second[i] = k2 == FNN_KEY_NONE ? inf : __uint_as_float((uint32_t)(k2 >> 32));
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// PCR_FPFH_TIMES=1 (developer, tools/fpfh_time.py, tools/iss_time.py): the calls bracket their kernels with events (StageTimes)
// and report the milliseconds on stderr

// a point target (else PCR_ERR_INVALID), a finite radius >= 0, normals (else PCR_ERR_NO_TARGET; an empty target has nothing
// that could lack one)
static pcr_status fpfh_check(const pcr_target *t, float r, const char *who) {
    PCR_TRY(check_point_target(t, who));
    PCR_TRY(check_radius<float>(r, who));
    if (t->n > 0 && !t->pn) { pcr_set_error("%s: the target has no per-point normals", who); return PCR_ERR_NO_TARGET; }
    return PCR_OK;
}

// the first pass over the whole target: counts [n][33] and k [n], at the cell-sorted index (ORIG = 0) or the original one
template <int ORIG>
static void spfh_launch(pcr_target *t, float r, uint32_t *d_counts, uint32_t *d_k) {
    hipLaunchKernelGGL(k_spfh<ORIG>, grid_for(t->n, FPFH_BLOCK), dim3(FPFH_BLOCK), 0, t->ctx->stream, t->gf, (const PtF *)t->pts, (const PtN *)t->pn,
                       (const uint32_t *)t->cell_start, t->n, r, d_counts, d_k);
}

extern "C" pcr_status pcr_target_spfh(pcr_target *t, float r, uint32_t *counts, int64_t *k) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_TRY(fpfh_check(t, r, "pcr_target_spfh"));
    if (t->n == 0) return PCR_OK;
    PCR_REQUIRE(counts && k, "NULL argument");
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t n = (size_t)t->n;
    DevBuf<uint32_t> d_counts, d_k;
    HIP_TRY(d_counts.alloc(n * FPFH_BINS));
    HIP_TRY(d_k.alloc(n));
    spfh_launch<1>(t, r, d_counts.p, d_k.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts, d_counts.p, 4 * n * FPFH_BINS, hipMemcpyDeviceToHost, ctx->stream));
    return download_u32_as_i64(ctx, d_k.p, n, k);
}

// the descriptors of every point (rows == NULL: m = n, in the caller's order) or of the m > 0 checked rows, in their order
static pcr_status fpfh_run(pcr_target *t, float r, const int64_t *rows, int64_t m, float *fpfh, int64_t *k_or_null) {
    PCR_REQUIRE(fpfh, "NULL argument");
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const size_t n = (size_t)t->n;
    DevBuf<uint32_t> d_counts, d_k, d_sel;
    DevBuf<int32_t> d_slot;
    DevBuf<float> d_out;
    DevBuf<int64_t> d_kout;
    HIP_TRY(d_counts.alloc(n * FPFH_BINS));
    HIP_TRY(d_k.alloc(n));
    std::vector<int32_t> slot_of;                  // slot_of[original index] = the row's place in the caller's list, or -1
    if (rows) {
        slot_of.assign(n, -1);
        for (int64_t s = 0; s < m; ++s) slot_of[(size_t)rows[s]] = (int32_t)s;
        HIP_TRY(d_slot.alloc(n));
        HIP_TRY(d_sel.alloc((size_t)m));
        HIP_TRY(hipMemcpyAsync(d_slot.p, slot_of.data(), 4 * n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(d_sel.p, 0, 4 * (size_t)m, ctx->stream));    // (every slot is stored below; never an index out of range)
    }
    HIP_TRY(d_out.alloc((size_t)m * FPFH_BINS));
    if (k_or_null) HIP_TRY(d_kout.alloc((size_t)m));
    int64_t *d_kp = k_or_null ? d_kout.p : (int64_t *)nullptr;
    static const bool times = env_flag("PCR_FPFH_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    spfh_launch<0>(t, r, d_counts.p, d_k.p);
    HIP_TRY(hipGetLastError());
    ev.mark(1, ctx->stream);
    if (rows) {
        hipLaunchKernelGGL(k_fpfh_row_index, grid_for(t->n, 256), dim3(256), 0, ctx->stream, (const PtF *)t->pts, t->n, (const int32_t *)d_slot.p,
                           d_sel.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_fpfh_rows, grid_for(m, FPFH_BLOCK), dim3(FPFH_BLOCK), 0, ctx->stream, t->gf, (const PtF *)t->pts,
                           (const uint32_t *)t->cell_start, m, r, (const uint32_t *)d_counts.p, (const uint32_t *)d_k.p, (const uint32_t *)d_sel.p,
                           d_out.p, d_kp);
    } else {
        hipLaunchKernelGGL(k_fpfh, grid_for(t->n, FPFH_BLOCK), dim3(FPFH_BLOCK), 0, ctx->stream, t->gf, (const PtF *)t->pts,
                           (const uint32_t *)t->cell_start, t->n, r, (const uint32_t *)d_counts.p, (const uint32_t *)d_k.p, d_out.p, d_kp);
    }
    HIP_TRY(hipGetLastError());
    ev.mark(2, ctx->stream);
    HIP_TRY(hipMemcpyAsync(fpfh, d_out.p, 4 * (size_t)m * FPFH_BINS, hipMemcpyDeviceToHost, ctx->stream));
    if (k_or_null) HIP_TRY(hipMemcpyAsync(k_or_null, d_kout.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on && rows)
        fprintf(stderr, "pcr_fpfh_times points %lld rows %lld spfh_ms %.4f fpfh_rows_ms %.4f\n", (long long)t->n, (long long)m, ev.ms(0), ev.ms(1));
    else if (ev.on)
        fprintf(stderr, "pcr_fpfh_times points %lld spfh_ms %.4f fpfh_ms %.4f\n", (long long)t->n, ev.ms(0), ev.ms(1));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_fpfh(pcr_target *t, float r, float *fpfh, int64_t *k_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_TRY(fpfh_check(t, r, "pcr_target_fpfh"));
    if (t->n == 0) return PCR_OK;
    return fpfh_run(t, r, nullptr, t->n, fpfh, k_or_null);
}

extern "C" pcr_status pcr_target_fpfh_rows(pcr_target *t, float r, const int64_t *rows, int64_t m, float *fpfh, int64_t *k_or_null) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_TRY(fpfh_check(t, r, "pcr_target_fpfh_rows"));
    PCR_REQUIRE(m >= 0, "negative row count");
    PCR_REQUIRE(rows || m == 0, "NULL argument");
    for (int64_t s = 0; s < m; ++s) {
        if (rows[s] < 0 || rows[s] >= t->n || (s > 0 && rows[s] <= rows[s - 1])) {
            pcr_set_error("invalid argument: pcr_target_fpfh_rows needs strictly ascending rows inside [0, n)");
            return PCR_ERR_INVALID;
        }
    }
    if (m == 0) return PCR_OK;
    return fpfh_run(t, r, rows, m, fpfh, k_or_null);
}

// splits of B: enough blocks to fill the chip when A is short, every split at least two tiles long (a one-tile block has no
// load to overlap with anything); from na and nb alone
static int fnn_splits(int64_t na, int64_t nb) {
    const int64_t gx = (na + FNN_BLOCK - 1) / FNN_BLOCK, tiles = (nb + FNN_TILE - 1) / FNN_TILE;
    int64_t want = (2048 + gx - 1) / gx;
    if (want > FNN_MAX_SPLIT) want = FNN_MAX_SPLIT;
    if (want > tiles / 2) want = tiles / 2;
    return (int)(want < 1 ? 1 : want);
}

extern "C" pcr_status pcr_feature_match(pcr_context *ctx, const float *A, int64_t na, const float *B, int64_t nb, int dim, int64_t *idx,
                                        float *d2_first, float *d2_second) {
    PCR_REQUIRE(ctx, "NULL argument");
    PCR_REQUIRE(na >= 0 && nb >= 0, "negative row count");
    if (dim < 1 || dim > 64) { pcr_set_error("invalid argument: pcr_feature_match needs 1 <= dim <= 64"); return PCR_ERR_INVALID; }
    PCR_REQUIRE(nb < ((int64_t)1 << 31) && na < ((int64_t)1 << 31), "2^31 rows or more");
    if (na == 0) return PCR_OK;
    PCR_REQUIRE(A && idx && d2_first && d2_second && (B || nb == 0), "NULL argument");
    if (nb == 0) {                                    // nothing to match against: no launch
        for (int64_t i = 0; i < na; ++i) { idx[i] = -1; d2_first[i] = d2_second[i] = __builtin_inff(); }
        return PCR_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const int splits = fnn_splits(na, nb);
    // rows of B per split: whole tiles
    int64_t chunk = (nb + splits - 1) / splits;
    chunk = (chunk + FNN_TILE - 1) / FNN_TILE * FNN_TILE;
    const int ny = (int)((nb + chunk - 1) / chunk);
    DevBuf<float> d_A, d_B, d_d1, d_d2;
    DevBuf<int64_t> d_idx;
    DevBuf<uint64_t> d_part;
    HIP_TRY(d_A.alloc((size_t)na * dim)); HIP_TRY(d_B.alloc((size_t)nb * dim));
    HIP_TRY(d_d1.alloc((size_t)na)); HIP_TRY(d_d2.alloc((size_t)na)); HIP_TRY(d_idx.alloc((size_t)na));
    HIP_TRY(d_part.alloc((size_t)na * ny * 2));
    HIP_TRY(hipMemcpyAsync(d_A.p, A, 4 * (size_t)na * dim, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_B.p, B, 4 * (size_t)nb * dim, hipMemcpyHostToDevice, ctx->stream));
    static const bool times = env_flag("PCR_FPFH_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    const dim3 grid(grid_for(na, FNN_BLOCK).x, (unsigned)ny);
    if (dim == 33)
        hipLaunchKernelGGL(k_feature_nn<33>, grid, dim3(FNN_BLOCK), 0, ctx->stream, (const float *)d_A.p, na, (const float *)d_B.p, nb, dim, chunk,
                           d_part.p);
    else
        hipLaunchKernelGGL(k_feature_nn<64>, grid, dim3(FNN_BLOCK), 0, ctx->stream, (const float *)d_A.p, na, (const float *)d_B.p, nb, dim, chunk,
                           d_part.p);
    HIP_TRY(hipGetLastError());
    ev.mark(1, ctx->stream);
    hipLaunchKernelGGL(k_feature_merge, grid_for(na, 256), dim3(256), 0, ctx->stream, (const uint64_t *)d_part.p, na, ny, d_idx.p,
                       d_d1.p, d_d2.p);
    HIP_TRY(hipGetLastError());
    ev.mark(2, ctx->stream);
    HIP_TRY(hipMemcpyAsync(idx, d_idx.p, 8 * (size_t)na, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d2_first, d_d1.p, 4 * (size_t)na, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d2_second, d_d2.p, 4 * (size_t)na, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on)
        fprintf(stderr, "pcr_fpfh_times match na %lld nb %lld dim %d splits %d nn_ms %.4f merge_ms %.4f\n", (long long)na, (long long)nb, dim, ny,
                ev.ms(0), ev.ms(1));
    return PCR_OK;
}
