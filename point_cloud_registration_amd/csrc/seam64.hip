// The float64 side of the search seam: KDTree(float64 data).query(float64 points, k) and VoxelGrid.query of the reference
// (kdtree.py:18-21, voxel.py:165,171-179) with the query kept in float64 from the caller's array to the result.
//
//   pcr_nn_query_dd    k = 1.  Point target with float64 coordinates: the float32 search over the index, run on the ROUNDED
//                      query, only nominates; nn_box_f64 with the true query decides by (float64 distance, original index).
//                      Voxel target: nn_search<double> over the centroids.
//   pcr_knn_query_f64  1 <= k <= 64.  The float32 k-NN over the rounded query gives a radius that holds at least k points in
//                      float64 too; the ball of that radius is walked as nn_box_f64 walks it and every record inserted, at its
//                      float64 distance, into a sorted per-lane list in LDS.  The walk shrinks to the list's k-th distance
//                      once the list is full.
//
// One lane = one query.  Distances are (dx*dx + dy*dy) + dz*dz with dx = q - p in float64, no contraction -- nn_test<double>'s
// expression -- and ties go to the smaller original index, so a NumPy brute force is a bit-for-bit yardstick.
//
// Queries the grid searches cannot place -- far outside the grid box (the ring loops of nn_device.h count rings from the
// query's own cell: 1e12 m away that is 1e9 rings), NaN, a voxel target's k-NN (no float32 index in every case), fewer than
// k nominees -- take s64_ring_search: float64 rings around the query's cell CLAMPED into the grid, every pruning bound
// the distance expression itself evaluated on per-axis gaps (monotone under rounding, so a bound never exceeds the computed
// distance of a record behind it, whatever the magnitudes).
#include "seam64_device.h"

// ---- k = 1 -------------------------------------------------------------------------------------------------------------
// FORM 1: a point target with float64 coordinates (g / pts = gq / pts64 behind the float32 index gf / pts32); 0: a voxel
// target (g / pts = gd / means; gf / pts32 unused).  rmax = +inf: unbounded.
template <int FORM, bool HALO>
__global__ void __launch_bounds__(256) k_nn_query_dd(Geom<float> gf, const PtF *pts32, Geom<double> g, const PtD *pts, const uint32_t *cs,
                                                     double band, const double *q, int64_t m, double rmax, double *dist, int64_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const double qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
    const bool bounded = rmax < s64_inf();
    S64Best S;
    S.init(s64_inf());
    bool have = false;
    if (FORM == 1) {
        const float fx = (float)qx, fy = (float)qy, fz = (float)qz;
        if (s64_placeable<float>(gf, fx, fy, fz)) {
            // the float32 search must reach every point whose FLOAT64 position lies within r_max of the FLOAT64 query: the
            // point's record moved by at most band, the query by its own rounding
            const double b = (rmax + band + s64_displacement(qx, qy, qz, fx, fy, fz)) * 1.00002;
            const float bound2 = bounded ? (float)(b * b * 1.000001) : __int_as_float(0x7f800000);
            float best; uint32_t bj, bo;
            nn_search<float, PtF, false, false, HALO>(gf, pts32, cs, fx, fy, fz, bound2, best, bj, bo);
            if (bo != PCR_NONE) nn_box_f64(g, pts, cs, qx, qy, qz, bj, S.bd, S.bj, S.bo);
            have = bo != PCR_NONE || bounded;              // (bounded and no nominee: nothing within r_max)
        }
    } else if (s64_placeable<double>(g, qx, qy, qz)) {
        const double b = rmax * (1.0 + 1e-6);
        nn_search<double, PtD>(g, pts, cs, qx, qy, qz, bounded ? b * b : s64_inf(), S.bd, S.bj, S.bo);
        have = true;
    }
    if (!have) {
        const double b = rmax * (1.0 + 1e-6);
        S.init(bounded ? b * b : s64_inf());
        s64_ring_search(g, pts, cs, qx, qy, qz, S);
    }
    const double d = __builtin_sqrt(S.bd);
    const bool ok = S.bo != PCR_NONE && d < rmax;
    dist[i] = ok ? d : s64_inf();
    idx[i] = ok ? (int64_t)S.bo : (int64_t)-1;
}

// ---- 1 <= k <= KNN_MAX_K ------------------------------------------------------------------------------------------------
extern __shared__ __attribute__((aligned(16))) char s64_smem[];

// MODE 0: no float32 index (voxel targets): the ring search alone.  1: k <= KNN_REG_K, the float32 bound from knn_collect;
// 2: from knn_search with its LDS list.  The float32 search's LDS is the list's: a barrier separates the two uses.
template <int MODE>
__global__ void __launch_bounds__(S64_BLOCK) k_knn_query_f64(Geom<float> gf, const PtF *pts32, Geom<double> g, const PtD *pts,
                                                             const uint32_t *cs, int64_t n, double band, const double *q, int64_t m,
                                                             int k, double *dist, int64_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * S64_BLOCK + threadIdx.x;
    const bool valid = i < m;
    double qx = 0, qy = 0, qz = 0;
    if (valid) { qx = q[3 * i]; qy = q[3 * i + 1]; qz = q[3 * i + 2]; }
    double R = -1.0;                    // radius that holds at least k points in float64 (< 0: none)
    if (MODE != 0) {
        const float fx = (float)qx, fy = (float)qy, fz = (float)qz;
        if (valid && s64_placeable<float>(gf, fx, fy, fz)) {
            float r2 = -1.f;            // the k-th float32 squared distance
            if (MODE == 1) {
                KnnOut O;
                O.init(s64_smem);
                knn_collect(gf, pts32, cs, fx, fy, fz, k, O);
                if (O.cnt == k) r2 = O.qd[(int)O.ord[(k - 1) * KNN_BLOCK] * KNN_BLOCK];
            } else {
                KnnList L;
                L.k = k; L.cnt = 0; L.lane = threadIdx.x; L.pts = pts32;
                L.d = (float *)s64_smem;
                L.j = (uint32_t *)(s64_smem + sizeof(float) * k * KNN_BLOCK);
                knn_search(gf, pts32, cs, fx, fy, fz, L);
                if (L.cnt == k) r2 = L.D(k - 1);
            }
            // k records within r32 of the rounded query: their float64 positions lie within r32 + band + the query's own
            // displacement of the float64 query (1e-6: the float32 rounding of r32 itself, several hundred times over)
            if (r2 >= 0.f) R = (double)__builtin_sqrtf(r2) * (1.0 + 1e-6) + band + s64_displacement(qx, qy, qz, fx, fy, fz);
        }
        __syncthreads();
    }
    S64List L;
    L.init(s64_smem, k, pts);
    if (valid) {
        bool done = false;
        if (R >= 0.0 && R < 1.0e300) {
            const double r = R * 1.0000001;
            L.reset(r * r);
            s64_ball_walk(g, pts, cs, qx, qy, qz, r + g.slack, L);
            done = L.cnt == k;
        }
        if (!done) {
            L.reset(s64_inf());
            s64_ring_search(g, pts, cs, qx, qy, qz, L);
        }
        for (int s = 0; s < k; ++s) {                                       // padding as pcr_knn_query's: inf / n
            const bool in = s < L.cnt;
            dist[i * k + s] = in ? __builtin_sqrt(L.D(s)) : s64_inf();
            idx[i * k + s] = in ? (int64_t)L.O(s) : n;
        }
    }
}

__global__ void __launch_bounds__(256) k_s64_fill(int64_t count, double *dist, int64_t *idx, int64_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) { dist[i] = s64_inf(); idx[i] = v; }
}

static pcr_status s64_target_ok(const pcr_target *t, const char *who) {
    if (!t->is_voxel && t->pts64 == nullptr) {
        pcr_set_error("invalid argument: %s needs a voxel target or a point target with float64 coordinates (pcr_target_points_set_f64)", who);
        return PCR_ERR_INVALID;
    }
    return PCR_OK;
}

pcr_status pcr_run_nn_dd(pcr_target *t, const double *d_q, int64_t m, double r_max, double *d_dist, int64_t *d_idx) {
    PCR_TRY(s64_target_ok(t, "pcr_nn_query_dd"));
    pcr_context *ctx = t->ctx;
    if (m == 0) return PCR_OK;
    const bool bounded = r_max > 0 && r_max < 1e300 * 1e300;
    const double rmax = bounded ? r_max : __builtin_inf();
    const dim3 grid((unsigned)((m + 255) / 256));
    ProfEvent ev;
    ctx->prof_this_pass = ctx->prof_on;
    pcr_prof_begin(ctx, PCR_K_NN, &ev);
    if (t->n == 0)
        hipLaunchKernelGGL(k_s64_fill, grid, dim3(256), 0, ctx->stream, m, d_dist, d_idx, (int64_t)-1);
    else if (t->is_voxel)
        hipLaunchKernelGGL((k_nn_query_dd<0, false>), grid, dim3(256), 0, ctx->stream, t->gf, (const PtF *)nullptr, t->gd, (const PtD *)t->means,
                           (const uint32_t *)t->cell_start, 0.0, d_q, m, rmax, d_dist, d_idx);
    else if (t->cs_h != nullptr)
        hipLaunchKernelGGL((k_nn_query_dd<1, true>), grid, dim3(256), 0, ctx->stream, t->gf, (const PtF *)t->pts, t->gq, (const PtD *)t->pts64,
                           (const uint32_t *)t->cell_start, t->band64, d_q, m, rmax, d_dist, d_idx);
    else
        hipLaunchKernelGGL((k_nn_query_dd<1, false>), grid, dim3(256), 0, ctx->stream, t->gf, (const PtF *)t->pts, t->gq, (const PtD *)t->pts64,
                           (const uint32_t *)t->cell_start, t->band64, d_q, m, rmax, d_dist, d_idx);
    pcr_prof_end(ctx, &ev);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

pcr_status pcr_run_knn_f64(pcr_target *t, const double *d_q, int64_t m, int k, double *d_dist, int64_t *d_idx) {
    PCR_TRY(s64_target_ok(t, "pcr_knn_query_f64"));
    if (k < 1 || k > KNN_MAX_K) { pcr_set_error("k must be in [1, %d]", KNN_MAX_K); return PCR_ERR_INVALID; }
    pcr_context *ctx = t->ctx;
    if (m == 0) return PCR_OK;
    const dim3 grid((unsigned)((m + S64_BLOCK - 1) / S64_BLOCK));
    // the list, or the float32 search's arrays in front of it where those are larger (k <= 16)
    const size_t list = (sizeof(double) + sizeof(uint32_t)) * (size_t)k * S64_BLOCK;
    ProfEvent ev;
    ctx->prof_this_pass = ctx->prof_on;
    pcr_prof_begin(ctx, PCR_K_NN, &ev);
    if (t->n == 0) {
        const int64_t count = m * k;
        hipLaunchKernelGGL(k_s64_fill, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, count, d_dist, d_idx, (int64_t)0);
    } else if (t->is_voxel) {
        hipLaunchKernelGGL(k_knn_query_f64<0>, grid, dim3(S64_BLOCK), list, ctx->stream, t->gf, (const PtF *)nullptr, t->gd, (const PtD *)t->means,
                           (const uint32_t *)t->cell_start, t->n, 0.0, d_q, m, k, d_dist, d_idx);
    } else if (k <= KNN_REG_K) {
        const size_t smem = list > KNN_COLLECT_BYTES ? list : KNN_COLLECT_BYTES;
        hipLaunchKernelGGL(k_knn_query_f64<1>, grid, dim3(S64_BLOCK), smem, ctx->stream, t->gf, (const PtF *)t->pts, t->gq, (const PtD *)t->pts64,
                           (const uint32_t *)t->cell_start, t->n, t->band64, d_q, m, k, d_dist, d_idx);
    } else {
        hipLaunchKernelGGL(k_knn_query_f64<2>, grid, dim3(S64_BLOCK), list, ctx->stream, t->gf, (const PtF *)t->pts, t->gq, (const PtD *)t->pts64,
                           (const uint32_t *)t->cell_start, t->n, t->band64, d_q, m, k, d_dist, d_idx);
    }
    pcr_prof_end(ctx, &ev);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}
