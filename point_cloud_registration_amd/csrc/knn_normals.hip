// Exact k nearest neighbours over the target's cell grid and k-NN PCA normals.
//
//   pcr_knn_query               KDTree(data).query(points, k) of the reference (kdtree.py:18-65)
//   pcr_target_estimate_normals estimate_norm_with_tree (estimate_normals.py:27-87): k-NN of every
//                               target point, covariance of the neighbours, eigenvector of the
//                               smallest eigenvalue
//
// The searches themselves (knn_collect for k <= 16, knn_search with the LDS list beyond) are in knn_device.h.
#include "eigen3.h"
#include "knn_device.h"

extern __shared__ __attribute__((aligned(16))) char knn_smem[];

template <typename LIST>
__device__ __forceinline__ void knn_query_finish(const PtF *pts, int64_t n_target, int64_t i, int k, float *dist, int64_t *idx, LIST &L) {
    for (int s = L.cnt; s < k; ++s) { dist[i * k + s] = __int_as_float(0x7f800000); idx[i * k + s] = n_target; }
    L.for_each([&](int s, float ds, uint32_t js) {
        dist[i * k + s] = __builtin_sqrtf(ds);
        idx[i * k + s] = (int64_t)pt_orig(pts[js]);
    });
}

// REG = 1: the collect path (k <= 16); 0: the LDS list
template <int REG>
__global__ void __launch_bounds__(KNN_BLOCK) k_knn_query(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n_target,
                                                         const float *q, int64_t m, int k, float *dist, int64_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
    if (i >= m) return;
    if (REG) {
        KnnOut L;
        L.init(knn_smem);
        knn_collect(g, pts, cs, q[3 * i], q[3 * i + 1], q[3 * i + 2], k, L);
        knn_query_finish(pts, n_target, i, k, dist, idx, L);
    } else {
        KnnList L = knn_list(knn_smem, k, pts);
        knn_search(g, pts, cs, q[3 * i], q[3 * i + 1], q[3 * i + 2], L);
        knn_query_finish(pts, n_target, i, k, dist, idx, L);
    }
}

template <typename LIST>
__device__ __forceinline__ void knn_normals_finish(const PtF *pts, const PtF me, int64_t i, int k, int compat, PtN *pn, LIST &L) {
    double c[6];
    if (compat) {
        // estimate_normals.py:56-72: float32 running sums over the neighbours (nearest first),
        // cov = E[pp^T] - mu mu^T in float32
        float sx = 0, sy = 0, sz = 0, xx = 0, xy = 0, xz = 0, yy = 0, yz = 0, zz = 0;
        L.for_each([&](int, float, uint32_t js) {
            const PtF p = pts[js];
            sx += p.x; sy += p.y; sz += p.z;
            xx += p.x * p.x; xy += p.x * p.y; xz += p.x * p.z; yy += p.y * p.y; yz += p.y * p.z; zz += p.z * p.z;
        });
        const float kf = (float)k;
        const float mx = sx / kf, my = sy / kf, mz = sz / kf;
        c[0] = xx / kf - mx * mx; c[1] = xy / kf - mx * my; c[2] = xz / kf - mx * mz;
        c[3] = yy / kf - my * my; c[4] = yz / kf - my * mz; c[5] = zz / kf - mz * mz;
    } else {
        knn_cov6_f64(L, pts, c);
    }
    double nv[3];
    smallest_eigvec3(c, nv);
    PtN r;                                      // the PlaneICP gather record: point + normal in 32 bytes
    r.x = me.x; r.y = me.y; r.z = me.z; r.orig = pt_orig(me);
    r.nx = (float)nv[0]; r.ny = (float)nv[1]; r.nz = (float)nv[2]; r.pad = 0;
    pn[i] = r;
}

// points in the 27-cell block around a position (from cell_start alone)
#ifndef KNN_SPARSE_T
#define KNN_SPARSE_T 30
#endif
__device__ __forceinline__ uint32_t knn_block_count(const Geom<float> &g, const uint32_t *__restrict__ cs, float qx, float qy, float qz) {
    const float lim = 1.0e9f;
    const int cx = (int)floorf(fminf(fmaxf((qx - g.ox) * g.inv_h, -lim), lim)), cy = (int)floorf(fminf(fmaxf((qy - g.oy) * g.inv_h, -lim), lim)),
              cz = (int)floorf(fminf(fmaxf((qz - g.oz) * g.inv_h, -lim), lim));
    if (!(cx >= 0 && cx < g.nx && cy >= 0 && cy < g.ny && cz >= 0 && cz < g.nz)) return 0;
    const int xl = max(cx - 1, 0), xh = min(cx + 1, g.nx - 1);
    uint32_t t = 0;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); ++y) {
            const size_t row = ((size_t)z * (size_t)g.ny + (size_t)y) * (size_t)g.nx;
            t += (cs[row + xh + 1] & g.cs_mask) - (cs[row + xl] & g.cs_mask);
        }
    return t;
}

// Sparse neighbourhoods first: a wave of such points lives several times as long as the others (ring search over hundreds of
// rows), and the cell-sorted order tends to keep them together at one end of the array -- at the far end they were the kernel's
// tail (1.06 M-point street cloud: 0.82 ms in array order, 0.71 reversed).  order[] = the blocks whose FIRST point has fewer
// than KNN_SPARSE_T points in its 27-cell block, then the others (cnt: two zeroed counters).
__global__ void __launch_bounds__(256) k_knn_order(Geom<float> g, const PtF *pts, const uint32_t *cs, uint32_t nb, uint32_t *order,
                                                   uint32_t *cnt) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    const bool valid = b < nb;
    bool sparse = false;
    if (valid) {
        const PtF p0 = pts[(int64_t)b * KNN_BLOCK];
        sparse = knn_block_count(g, cs, p0.x, p0.y, p0.z) < KNN_SPARSE_T;
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long ms = __ballot(valid && sparse), md = __ballot(valid && !sparse);
    uint32_t bs = 0, bd = 0;
    if (lane == 0) { if (ms) bs = atomicAdd(&cnt[0], (uint32_t)__popcll(ms)); if (md) bd = atomicAdd(&cnt[1], (uint32_t)__popcll(md)); }
    bs = __shfl(bs, 0, 64); bd = __shfl(bd, 0, 64);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (valid && sparse) order[bs + (uint32_t)__popcll(ms & below)] = b;
    if (valid && !sparse) order[nb - 1u - (bd + (uint32_t)__popcll(md & below))] = b;
}

// normals of the target's own points, processed (and written) in cell-sorted order
template <int REG>
__global__ void __launch_bounds__(KNN_BLOCK) k_knn_normals(Geom<float> g, const PtF *pts, const uint32_t *cs, int64_t n,
                                                           int k, int compat, PtN *pn, const uint32_t *__restrict__ order) {
    const int64_t i = (int64_t)(order ? order[blockIdx.x] : blockIdx.x) * KNN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PtF me = pts[i];
    knn_self<REG>(g, pts, cs, me, k, knn_smem, [&](auto &L) { knn_normals_finish(pts, me, i, k, compat, pn, L); });
}

// k <= 16: the register list (PCR_KNN_REG=0: the LDS list for every k, for A/B)
static bool knn_use_registers(int k) {
    static const bool allow = env_i64("PCR_KNN_REG", 1, INT64_MIN, INT64_MAX) != 0;
    return allow && k <= KNN_REG_K;
}

static pcr_status check_k(int k) {
    if (k < 1 || k > KNN_MAX_K) { pcr_set_error("k must be in [1, %d]", KNN_MAX_K); return PCR_ERR_INVALID; }
    return PCR_OK;
}

extern "C" pcr_status pcr_knn_query(pcr_target *t, const float *q, int64_t m, int k, float *dist, int64_t *idx) {
    PCR_REQUIRE(t && (q || m == 0) && (dist || m == 0) && (idx || m == 0), "NULL argument");
    PCR_REQUIRE(!t->is_voxel, "k-NN needs a point target");
    PCR_TRY(check_k(k));
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (m == 0) return PCR_OK;
    CtxScope scope(ctx);
    DevBuf<float> d_q, d_dist;
    DevBuf<int64_t> d_idx;
    HIP_TRY(d_q.alloc(3 * (size_t)m));
    HIP_TRY(d_dist.alloc((size_t)m * k));
    HIP_TRY(d_idx.alloc((size_t)m * k));
    HIP_TRY(hipMemcpyAsync(d_q.p, q, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
    knn_launch(k_knn_query<1>, k_knn_query<0>, knn_use_registers(k), m, k, ctx->stream, t->gf, t->pts, t->cell_start, t->n, (const float *)d_q.p, m,
               k, d_dist.p, d_idx.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dist, d_dist.p, 4 * (size_t)m * k, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(idx, d_idx.p, 8 * (size_t)m * k, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

extern "C" pcr_status pcr_target_estimate_normals(pcr_target *t, int k, int compat, float *normals_out) {
    PCR_REQUIRE(t, "NULL argument");
    PCR_REQUIRE(!t->is_voxel, "normals belong to point targets");
    PCR_TRY(check_k(k));
    pcr_context *ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    pcr_target_drop_color(t);       // (colour gradients lie in the tangent planes of the OLD normals)
    if (!t->pn) HIP_TRY(pcr_persist_alloc((void **)&t->pn, sizeof(PtN) * (size_t)(t->n ? t->n : 1)));
    if (t->n > 0) {
        const Geom<float> &g = t->gf;
        const unsigned nb = grid_for(t->n, KNN_BLOCK).x;
        static const bool sparse_first = env_i64("PCR_KNN_SPARSE_FIRST", 1, INT64_MIN, INT64_MAX) != 0;
        const bool reg = knn_use_registers(k);
        DevBuf<uint32_t> order, cnt;
        // (only where the tail is a visible share of the kernel: at 1e7 / 1e8 points the reordering costs 3 % in locality)
        if (reg && sparse_first && nb > 1024 && nb <= 65536) {
            HIP_TRY(order.alloc(nb)); HIP_TRY(cnt.alloc(2));
            HIP_TRY(hipMemsetAsync(cnt.p, 0, 2 * sizeof(uint32_t), ctx->stream));
            hipLaunchKernelGGL(k_knn_order, grid_for(nb, 256), dim3(256), 0, ctx->stream, g, t->pts, t->cell_start, nb, order.p, cnt.p);
        }
        knn_launch(k_knn_normals<1>, k_knn_normals<0>, reg, t->n, k, ctx->stream, g, t->pts, t->cell_start, t->n, k, compat, t->pn,
                   (const uint32_t *)order.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (normals_out) return pcr_target_get_normals(t, normals_out);
    return PCR_OK;
}
