// Gauss-Newton coresets: create_gn_set and fast_caratheodory (caratheodory.py:36-138; K. Koide, "Exact Point Cloud
// Downsampling for Fast and Accurate Global Trajectory Optimization", arXiv 2307.02948).
//
// Device side: the O(N M) passes -- the per-point products of create_gn_set (k_gn_set), the weighted chunk sums of every
// level of fast_caratheodory (k_chunk_sums + k_chunk_fold: partial sums per block, folded in a fixed order, no
// floating-point atomics), the member lists of the next level (k_member_gather) and the selected columns (k_take_columns).
// P stays in HBM for the whole call; a level carries only its member list (ascending indices into P + weights).
// Host side: the Caratheodory elimination of the k chunk means (at most 91 x k numbers, independent of N) in float64,
// one point per step, with the null vector taken from a Householder QR with column pivoting (no LAPACK).
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "host_util.h"

#define CS_BLOCK 256
#define CS_MAX_D 12          // M = D (D + 1) / 2 + D + 1 <= 91

static inline int gn_rows(int d) { return d * (d + 1) / 2 + d + 1; }

// D of a Gauss-Newton set with M rows, 0 when M is not of that form
static int gn_dim(int m) {
    for (int d = 1; d <= CS_MAX_D; ++d)
        if (gn_rows(d) == m) return d;
    return 0;
}

// ---- create_gn_set (caratheodory.py:118-138) -------------------------------------------------------------------------
// One lane = one row of (J, r).  Each product is rounded once in the type C++ gives it -- float x float in float,
// anything with a double in double -- which is NumPy's promotion (einsum / J * r[:, None] / r ** 2 in the reference), and
// the build has -ffp-contract=off, so the values are the reference's bit for bit.  The reference takes the J J products
// with np.einsum, which adds each product to a zeroed output: a product of -0.0 is +0.0 there (J r and r^2 are plain
// products and keep the sign), hence the `+ 0` on those rows alone.  P is (M, n) row-major: lane i writes column i of
// every row, so each row is written coalesced.
template <typename TJ, typename TR, int D>
__global__ void __launch_bounds__(CS_BLOCK) k_gn_set(const TJ *__restrict__ J, const TR *__restrict__ r, int64_t n,
                                                     double *__restrict__ P) {
    for (int64_t i = (int64_t)blockIdx.x * CS_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CS_BLOCK) {
        TJ j[D];
#pragma unroll
        for (int a = 0; a < D; ++a) j[a] = J[i * D + a];
        const TR ri = r[i];
        int64_t row = 0;
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = a; b < D; ++b) {                 // np.triu_indices(D) order
                const TJ p = j[a] * j[b];
                P[row++ * n + i] = (double)(p + (TJ)0);      // -0.0 -> +0.0, nothing else changes
            }
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const auto p = j[a] * ri;
            P[row++ * n + i] = (double)p;
        }
        const TR e = ri * ri;
        P[row * n + i] = (double)e;
    }
}

template <typename TJ, typename TR>
static pcr_status launch_gn_set(pcr_context *ctx, const void *J, const void *r, int64_t n, int d, double *P) {
    const int64_t want = (n + CS_BLOCK - 1) / CS_BLOCK;
    const dim3 grid((unsigned)std::min<int64_t>(want, (int64_t)ctx->num_cu * 8));
    const TJ *j = (const TJ *)J;
    const TR *rr = (const TR *)r;
    switch (d) {
#define CS_GN_CASE(D) case D: hipLaunchKernelGGL((k_gn_set<TJ, TR, D>), grid, dim3(CS_BLOCK), 0, ctx->stream, j, rr, n, P); break;
        CS_GN_CASE(1) CS_GN_CASE(2) CS_GN_CASE(3) CS_GN_CASE(4) CS_GN_CASE(5) CS_GN_CASE(6)
        CS_GN_CASE(7) CS_GN_CASE(8) CS_GN_CASE(9) CS_GN_CASE(10) CS_GN_CASE(11) CS_GN_CASE(12)
#undef CS_GN_CASE
        default: pcr_set_error("invalid argument: d must be in [1, %d]", CS_MAX_D); return PCR_ERR_INVALID;
    }
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

// ---- fast_caratheodory: chunk sums of one level (caratheodory.py:87-90) -------------------------------------------------
__device__ __forceinline__ double cs_shfl_xor(double v, int mask) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return __hiloint2double(hi, lo);
}

// Chunk c = member positions [bounds[c], bounds[c + 1]) is cut into `bpc` equal sub-ranges, one block each (the first level
// of a 1.06 M-point set has only 64 chunks: this keeps every CU streaming).  Member q is column idx[q] of P (q itself when
// idx == nullptr: the first level) with weight u[q].  A block writes M + 1 partial sums: sum u P[m, .] for m < M, then
// sum u.  Each lane adds its members in order, lanes fold by a xor butterfly, waves in index order: a fixed order.
template <int M>
__global__ void __launch_bounds__(CS_BLOCK) k_chunk_sums(const double *__restrict__ P, int64_t stride, const int64_t *__restrict__ idx,
                                                         const double *__restrict__ u, const int64_t *__restrict__ bounds, int bpc,
                                                         double *__restrict__ partials) {
    __shared__ double red[CS_BLOCK / 64][M + 1];
    const int c = blockIdx.x / bpc, b = blockIdx.x % bpc;
    const int64_t lo = bounds[c], len = bounds[c + 1] - lo;
    const int64_t q0 = lo + len * b / bpc, q1 = lo + len * (b + 1) / bpc;
    double acc[M + 1];
#pragma unroll
    for (int m = 0; m <= M; ++m) acc[m] = 0.0;
    for (int64_t q = q0 + threadIdx.x; q < q1; q += CS_BLOCK) {
        const double w = u[q];
        const double *col = P + (idx ? idx[q] : q);
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m] = fma(w, col[m * stride], acc[m]);
        acc[M] += w;
    }
#pragma unroll
    for (int m = 0; m <= M; ++m)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[m] += cs_shfl_xor(acc[m], off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m <= M; ++m) red[wave][m] = acc[m];
    }
    __syncthreads();
    for (int m = threadIdx.x; m <= M; m += CS_BLOCK) {
        double s = red[0][m];
        for (int w = 1; w < CS_BLOCK / 64; ++w) s += red[w][m];
        partials[(int64_t)blockIdx.x * (M + 1) + m] = s;
    }
}

// sums[c][m] = the bpc partial sums of chunk c, added in block order
__global__ void __launch_bounds__(CS_BLOCK) k_chunk_fold(const double *__restrict__ partials, int k, int bpc, int m1,
                                                         double *__restrict__ sums) {
    const int64_t t = (int64_t)blockIdx.x * CS_BLOCK + threadIdx.x;
    if (t >= (int64_t)k * m1) return;
    const int64_t c = t / m1, m = t % m1;
    double s = 0.0;
    for (int b = 0; b < bpc; ++b) s += partials[(c * bpc + b) * m1 + m];
    sums[t] = s;
}

template <int M>
static void launch_chunk_sums(pcr_context *ctx, const double *P, int64_t stride, const int64_t *idx, const double *u,
                              const int64_t *bounds, int k, int bpc, double *partials) {
    hipLaunchKernelGGL(k_chunk_sums<M>, dim3((unsigned)(k * bpc)), dim3(CS_BLOCK), 0, ctx->stream, P, stride, idx, u, bounds, bpc,
                       partials);
}

static pcr_status chunk_sums(pcr_context *ctx, int d, const double *P, int64_t stride, const int64_t *idx, const double *u,
                             const int64_t *bounds, int k, int bpc, double *partials) {
    switch (d) {
#define CS_SUM_CASE(D) case D: launch_chunk_sums<D * (D + 1) / 2 + D + 1>(ctx, P, stride, idx, u, bounds, k, bpc, partials); break;
        CS_SUM_CASE(1) CS_SUM_CASE(2) CS_SUM_CASE(3) CS_SUM_CASE(4) CS_SUM_CASE(5) CS_SUM_CASE(6)
        CS_SUM_CASE(7) CS_SUM_CASE(8) CS_SUM_CASE(9) CS_SUM_CASE(10) CS_SUM_CASE(11) CS_SUM_CASE(12)
#undef CS_SUM_CASE
        default: pcr_set_error("invalid argument: unsupported number of rows"); return PCR_ERR_INVALID;
    }
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

// ---- the next level's member list (caratheodory.py:100-111) -----------------------------------------------------------
// One surviving chunk: its members start at old position `src` and go to new position `dst` (ascending; a chunk ends where
// the next one starts), their weights multiplied by factor = w_sub / u_sub of the chunk.
struct CsSeg {
    int64_t src, dst;
    double factor;
};

__global__ void __launch_bounds__(CS_BLOCK) k_member_gather(const int64_t *__restrict__ idx_old, const double *__restrict__ u_old,
                                                            const CsSeg *__restrict__ segs, int nseg, int64_t n_new,
                                                            int64_t *__restrict__ idx_new, double *__restrict__ u_new) {
    for (int64_t q = (int64_t)blockIdx.x * CS_BLOCK + threadIdx.x; q < n_new; q += (int64_t)gridDim.x * CS_BLOCK) {
        int lo = 0, hi = nseg - 1;                  // last segment with dst <= q
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segs[mid].dst <= q) lo = mid;
            else hi = mid - 1;
        }
        const int64_t src = segs[lo].src + (q - segs[lo].dst);
        idx_new[q] = idx_old ? idx_old[src] : src;
        u_new[q] = segs[lo].factor * u_old[src];    // w_factors * u[selected_indices] (caratheodory.py:110)
    }
}

// P_sel = P[:, idx]: out is (m, n_out) row-major
__global__ void __launch_bounds__(CS_BLOCK) k_take_columns(const double *__restrict__ P, int64_t stride, int m,
                                                           const int64_t *__restrict__ idx, int64_t n_out, double *__restrict__ out) {
    for (int64_t q = (int64_t)blockIdx.x * CS_BLOCK + threadIdx.x; q < n_out; q += (int64_t)gridDim.x * CS_BLOCK) {
        const int64_t j = idx[q];
        for (int r = 0; r < m; ++r) out[(int64_t)r * n_out + q] = P[(int64_t)r * stride + j];
    }
}

// ---- host: Caratheodory elimination (caratheodory.py:24-60) -------------------------------------------------------------
// A vector y != 0 with A y = 0, A = m x c column-major (c > m, so one exists).  Householder QR with column pivoting
// (the largest remaining column first) stops at the numerical rank r; with the first free column f = r of the permuted
// order, y = Pi [-R11^{-1} R12[:, f]; e_f].
static void null_vector(std::vector<double> &A, int m, int c, std::vector<double> &y) {
    std::vector<int> perm(c);
    for (int j = 0; j < c; ++j) perm[j] = j;
    double scale = 0.0;
    for (int j = 0; j < c; ++j) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += A[(size_t)j * m + i] * A[(size_t)j * m + i];
        scale = std::max(scale, s);
    }
    const double tol = sqrt(scale) * 2.220446049250313e-16 * std::max(m, c);
    std::vector<double> v(m);
    int rank = 0;
    for (int s = 0; s < std::min(m, c); ++s) {
        int best = s;
        double bn = -1.0;
        for (int j = s; j < c; ++j) {
            double nj = 0.0;
            for (int i = s; i < m; ++i) nj += A[(size_t)j * m + i] * A[(size_t)j * m + i];
            if (nj > bn) { bn = nj; best = j; }
        }
        if (!(sqrt(bn) > tol)) break;
        if (best != s) {
            for (int i = 0; i < m; ++i) std::swap(A[(size_t)s * m + i], A[(size_t)best * m + i]);
            std::swap(perm[s], perm[best]);
        }
        // reflector H = I - 2 v v^T / (v^T v) mapping A[s:, s] to alpha e_0
        double *x = &A[(size_t)s * m];
        const double alpha = -copysign(sqrt(bn), x[s]);
        double vv = 0.0;
        for (int i = s; i < m; ++i) { v[i] = x[i]; }
        v[s] -= alpha;
        for (int i = s; i < m; ++i) vv += v[i] * v[i];
        for (int j = s + 1; j < c; ++j) {
            double *a = &A[(size_t)j * m];
            double dot = 0.0;
            for (int i = s; i < m; ++i) dot += v[i] * a[i];
            const double f = 2.0 * dot / vv;
            for (int i = s; i < m; ++i) a[i] -= f * v[i];
        }
        x[s] = alpha;
        for (int i = s + 1; i < m; ++i) x[i] = 0.0;
        rank = s + 1;
    }
    // back substitution R11 z = -R12[:, f]
    const int f = rank;
    std::vector<double> z(c, 0.0);
    z[f] = 1.0;
    for (int i = rank - 1; i >= 0; --i) {
        double s = -A[(size_t)f * m + i];
        for (int j = i + 1; j < rank; ++j) s -= A[(size_t)j * m + i] * z[j];
        z[i] = s / A[(size_t)i * m + i];
    }
    y.assign(c, 0.0);
    for (int j = 0; j < c; ++j) y[perm[j]] = z[j];
}

// Reduce n weighted points (columns of Ps, m x n column-major; weights u > 0) to `target` points with the same weighted sum
// and the same total weight.  Each step takes v with sum_i v_i P_i = 0 and sum_i v_i = 0 -- v = [-sum y, y] for a null
// vector y of A = [P_1 - P_0, ..., P_{n-1} - P_0] -- and moves the weights by the smallest step alpha v that drives one of
// them to zero (alpha = u_i / v_i of the smallest |u_i / v_i|: every other weight stays >= 0), then drops that point.
// alive: the surviving column numbers, ascending; w: their weights.
static void caratheodory_host(const std::vector<double> &Ps, int m, int n, const std::vector<double> &u, int target,
                              std::vector<int> &alive, std::vector<double> &w) {
    alive.resize(n);
    for (int i = 0; i < n; ++i) alive[i] = i;
    w = u;
    std::vector<double> A, y, v;
    while ((int)alive.size() > target) {
        const int na = (int)alive.size(), c = na - 1;
        A.resize((size_t)m * c);
        const double *p0 = &Ps[(size_t)alive[0] * m];
        for (int j = 0; j < c; ++j) {
            const double *pj = &Ps[(size_t)alive[j + 1] * m];
            for (int i = 0; i < m; ++i) A[(size_t)j * m + i] = pj[i] - p0[i];
        }
        null_vector(A, m, c, y);
        v.resize(na);
        double sy = 0.0;
        for (int j = 0; j < c; ++j) sy += y[j];
        v[0] = -sy;
        for (int j = 0; j < c; ++j) v[j + 1] = y[j];
        int pick = -1;
        double best = 0.0;
        for (int i = 0; i < na; ++i) {
            if (v[i] == 0.0) continue;
            const double a = fabs(w[i] / v[i]);
            if (pick < 0 || a < best) { best = a; pick = i; }
        }
        const double alpha = w[pick] / v[pick];
        for (int i = 0; i < na; ++i) w[i] -= alpha * v[i];
        alive.erase(alive.begin() + pick);
        w.erase(w.begin() + pick);
    }
}

// ---- entry points -------------------------------------------------------------------------------------------------------
extern "C" pcr_status pcr_gn_set(pcr_context *ctx, const void *J, int J_is_f64, const void *r, int r_is_f64, int64_t n, int d,
                                 double *P_out) {
    PCR_REQUIRE(ctx && n >= 0 && (n == 0 || (J && r && P_out)), "NULL argument or negative n");
    PCR_REQUIRE(d >= 1 && d <= CS_MAX_D, "d must be in [1, 12]");
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return PCR_OK;
    CtxScope scope(ctx);
    const int m = gn_rows(d);
    const size_t sj = J_is_f64 ? 8 : 4, sr = r_is_f64 ? 8 : 4;
    DevBuf<char> d_J, d_r;
    DevBuf<double> d_P;
    HIP_TRY(d_J.alloc_bytes(sj * d * (size_t)n));
    HIP_TRY(d_r.alloc_bytes(sr * (size_t)n));
    HIP_TRY(d_P.alloc((size_t)m * n));
    HIP_TRY(hipMemcpyAsync(d_J.p, J, sj * d * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_r.p, r, sr * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (J_is_f64 && r_is_f64) PCR_TRY((launch_gn_set<double, double>(ctx, d_J.p, d_r.p, n, d, d_P.p)));
    else if (J_is_f64) PCR_TRY((launch_gn_set<double, float>(ctx, d_J.p, d_r.p, n, d, d_P.p)));
    else if (r_is_f64) PCR_TRY((launch_gn_set<float, double>(ctx, d_J.p, d_r.p, n, d, d_P.p)));
    else PCR_TRY((launch_gn_set<float, float>(ctx, d_J.p, d_r.p, n, d, d_P.p)));
    HIP_TRY(hipMemcpyAsync(P_out, d_P.p, 8 * (size_t)m * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// out[q] = map[idx[q]]
__global__ void __launch_bounds__(CS_BLOCK) k_take_i64(const int64_t *__restrict__ map, const int64_t *__restrict__ idx, int64_t n_out,
                                                       int64_t *__restrict__ out) {
    for (int64_t q = (int64_t)blockIdx.x * CS_BLOCK + threadIdx.x; q < n_out; q += (int64_t)gridDim.x * CS_BLOCK)
        out[q] = idx ? map[idx[q]] : map[q];
}

// u[q] = weights[map[q]] (fill: u[q] = value)
__global__ void __launch_bounds__(CS_BLOCK) k_gather_f64(const double *__restrict__ weights, const int64_t *__restrict__ map, int64_t n,
                                                         double value, double *__restrict__ u) {
    for (int64_t q = (int64_t)blockIdx.x * CS_BLOCK + threadIdx.x; q < n; q += (int64_t)gridDim.x * CS_BLOCK)
        u[q] = weights ? weights[map[q]] : value;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The levels of fast_caratheodory over a DEVICE-RESIDENT set: columns 0 .. n-1 of d_P (m rows, `stride` doubles apart) with
// weights d_u0, n > n_target.  Shared by pcr_coreset (P uploaded by the caller) and pcr_scan_coreset (P written by the terms
// kernel).  d_col_map (or NULL): idx_out names the selected columns through it; P_sel_out may be NULL.
static pcr_status coreset_core(pcr_context *ctx, int d, int m, const double *d_P, int64_t stride, int64_t n, const double *d_u0, int k,
                               int64_t n_target, const int64_t *d_col_map, int64_t *n_out, double *w_out, int64_t *idx_out,
                               double *P_sel_out, double *ms_elim, double *ms_down, int *levels) {
    const int m1 = m + 1;
    DevBuf<double> d_u[2], d_part, d_sums, d_sel;
    DevBuf<int64_t> d_idx[2], d_bounds, d_named;
    DevBuf<CsSeg> d_segs;
    auto t0 = std::chrono::steady_clock::now();
    const int64_t *idx_cur = nullptr;                     // level 0: member q is column q
    const double *u_cur = d_u0;
    int64_t cur = n;
    int ping = 0;
    std::vector<int64_t> bounds;
    std::vector<double> sums, Ps, u_sub, w_sub;
    std::vector<int> alive;
    std::vector<CsSeg> segs;
    while (cur > n_target) {
        // caratheodory.py:75-80: k chunks, bounds = np.linspace(0, cur_N, k + 1, dtype=int) -- floor(i * (cur_N / k)), last = cur_N
        const int kk = (int)std::min<int64_t>(k, cur);
        bounds.resize(kk + 1);
        const double step = (double)cur / (double)kk;
        for (int i = 0; i < kk; ++i) bounds[i] = (int64_t)floor((double)i * step);
        bounds[kk] = cur;
        int64_t max_chunk = 0;
        for (int i = 0; i < kk; ++i) max_chunk = std::max(max_chunk, bounds[i + 1] - bounds[i]);
        // blocks per chunk: ~4 blocks per CU in all, ~1024 members per block at least
        const int64_t bpc64 = std::min<int64_t>((4 * (int64_t)ctx->num_cu + kk - 1) / kk, (max_chunk + 1023) / 1024);
        const int bpc = (int)std::max<int64_t>(1, bpc64);
        HIP_TRY(d_bounds.alloc(kk + 1));
        HIP_TRY(d_part.alloc((size_t)kk * bpc * m1));
        HIP_TRY(d_sums.alloc((size_t)kk * m1));
        HIP_TRY(hipMemcpyAsync(d_bounds.p, bounds.data(), 8 * (size_t)(kk + 1), hipMemcpyHostToDevice, ctx->stream));
        PCR_TRY(chunk_sums(ctx, d, d_P, stride, idx_cur, u_cur, d_bounds.p, kk, bpc, d_part.p));
        hipLaunchKernelGGL(k_chunk_fold, dim3((unsigned)(((int64_t)kk * m1 + CS_BLOCK - 1) / CS_BLOCK)), dim3(CS_BLOCK), 0, ctx->stream,
                           (const double *)d_part.p, kk, bpc, m1, d_sums.p);
        HIP_TRY(hipGetLastError());
        sums.resize((size_t)kk * m1);
        t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipMemcpyAsync(sums.data(), d_sums.p, 8 * sums.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        *ms_down += ms_since(t0);
        if (*levels == 0) {
            // every column of P is in some chunk and u > 0: a non-finite entry of P makes its chunk's sums non-finite
            for (double s : sums)
                if (!isfinite(s)) {
                    pcr_set_error("invalid argument: P holds non-finite values (or its weighted sums overflow)");
                    return PCR_ERR_INVALID;
                }
        }
        t0 = std::chrono::steady_clock::now();
        // chunk weights and weighted means (caratheodory.py:89-90), column-major m x kk
        u_sub.resize(kk);
        Ps.resize((size_t)kk * m);
        for (int c = 0; c < kk; ++c) {
            u_sub[c] = sums[(size_t)c * m1 + m];
            for (int i = 0; i < m; ++i) Ps[(size_t)c * m + i] = sums[(size_t)c * m1 + i] / u_sub[c];
        }
        // caratheodory.py:93-96
        int64_t n_sub = m + 1;
        if (n_sub * max_chunk < n_target) n_sub = n_target / max_chunk;
        caratheodory_host(Ps, m, kk, u_sub, (int)n_sub, alive, w_sub);
        segs.resize(alive.size());
        int64_t dst = 0;
        for (size_t s = 0; s < alive.size(); ++s) {
            const int c = alive[s];
            segs[s] = {bounds[c], dst, w_sub[s] / u_sub[c]};
            dst += bounds[c + 1] - bounds[c];
        }
        *ms_elim += ms_since(t0);
        HIP_TRY(d_segs.alloc(segs.size()));
        if (!d_idx[ping].p) HIP_TRY(d_idx[ping].alloc(dst));
        if (!d_u[ping].p) HIP_TRY(d_u[ping].alloc(dst));
        HIP_TRY(hipMemcpyAsync(d_segs.p, segs.data(), sizeof(CsSeg) * segs.size(), hipMemcpyHostToDevice, ctx->stream));
        const dim3 ggrid((unsigned)std::min<int64_t>((dst + CS_BLOCK - 1) / CS_BLOCK, (int64_t)ctx->num_cu * 8));
        hipLaunchKernelGGL(k_member_gather, ggrid, dim3(CS_BLOCK), 0, ctx->stream, idx_cur, u_cur, (const CsSeg *)d_segs.p,
                           (int)segs.size(), dst, d_idx[ping].p, d_u[ping].p);
        HIP_TRY(hipGetLastError());
        idx_cur = d_idx[ping].p;
        u_cur = d_u[ping].p;
        ping ^= 1;
        cur = dst;
        ++*levels;
    }
    const dim3 tgrid((unsigned)std::min<int64_t>((cur + CS_BLOCK - 1) / CS_BLOCK, (int64_t)ctx->num_cu * 8));
    if (P_sel_out) {                                       // P_sel = P[:, idx]
        HIP_TRY(d_sel.alloc((size_t)m * cur));
        hipLaunchKernelGGL(k_take_columns, tgrid, dim3(CS_BLOCK), 0, ctx->stream, d_P, stride, m, idx_cur, cur, d_sel.p);
        HIP_TRY(hipGetLastError());
    }
    if (d_col_map) {                                       // columns -> what the caller calls them (ascending, like the columns)
        HIP_TRY(d_named.alloc((size_t)cur));
        hipLaunchKernelGGL(k_take_i64, tgrid, dim3(CS_BLOCK), 0, ctx->stream, d_col_map, idx_cur, cur, d_named.p);
        HIP_TRY(hipGetLastError());
    }
    t0 = std::chrono::steady_clock::now();
    if (P_sel_out) HIP_TRY(hipMemcpyAsync(P_sel_out, d_sel.p, 8 * (size_t)m * cur, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(w_out, u_cur, 8 * (size_t)cur, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(idx_out, d_col_map ? (const int64_t *)d_named.p : idx_cur, 8 * (size_t)cur, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *ms_down += ms_since(t0);
    *n_out = cur;
    return PCR_OK;
}

extern "C" pcr_status pcr_coreset(pcr_context *ctx, const double *P, int m, int64_t n, const double *u, int k, int64_t n_target,
                                  int64_t *n_out, double *w_out, int64_t *idx_out, double *P_sel_out) {
    PCR_REQUIRE(ctx && n_out && n >= 0 && (n == 0 || (P && u)), "NULL argument or negative n");
    const int d = gn_dim(m);
    PCR_REQUIRE(d > 0, "m must be D (D + 1) / 2 + D + 1 for some D in [1, 12]");
    PCR_REQUIRE(k > m + 1, "k must exceed m + 1");
    PCR_REQUIRE(n_target >= m + 1, "n_target must be at least m + 1");
    PCR_REQUIRE(w_out && idx_out && P_sel_out, "NULL output");
    for (int64_t i = 0; i < n; ++i)
        PCR_REQUIRE(isfinite(u[i]) && u[i] > 0.0, "u must be finite and positive");
    if (n <= n_target) {                                   // caratheodory.py:67-69
        for (int64_t i = 0; i < n; ++i) { w_out[i] = u[i]; idx_out[i] = i; }
        std::copy(P, P + (size_t)m * n, P_sel_out);
        *n_out = n;
        return PCR_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    static const bool stats = env_flag("PCR_CORESET_STATS");
    const auto t_all = std::chrono::steady_clock::now();
    double ms_up = 0, ms_elim = 0, ms_down = 0;
    int levels = 0;
    DevBuf<double> d_P, d_u0;
    HIP_TRY(d_P.alloc((size_t)m * n));
    HIP_TRY(d_u0.alloc(n));
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(d_P.p, P, 8 * (size_t)m * n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_u0.p, u, 8 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (stats) { HIP_TRY(hipStreamSynchronize(ctx->stream)); ms_up = ms_since(t0); }
    PCR_TRY(coreset_core(ctx, d, m, d_P.p, n, n, d_u0.p, k, n_target, nullptr, n_out, w_out, idx_out, P_sel_out, &ms_elim, &ms_down,
                         &levels));
    if (stats)
        fprintf(stderr, "pcr_coreset: n %lld m %d levels %d -> %lld points; total %.3f ms: upload %.3f, host elimination %.3f, "
                        "read-backs (incl. waiting for the kernels before them) %.3f\n",
                (long long)n, m, levels, (long long)*n_out, ms_since(t_all), ms_up, ms_elim, ms_down);
    return PCR_OK;
}

// ---- the scan routes: the terms kernel's columns never leave HBM ---------------------------------------------------------
// sum_c weights[col_idx[c]] P[:, c] and the sum of those weights: k_chunk_sums with ONE chunk (fixed order, no float atomics)
pcr_status pcr_terms_weighted_sum(pcr_context *ctx, const double *d_P, int64_t stride, const int64_t *d_col_idx, int64_t n_in,
                                  const double *weights, int64_t n, double out[29]) {
    for (int i = 0; i < 29; ++i) out[i] = 0.0;
    if (n_in == 0) return PCR_OK;
    DevBuf<double> d_w, d_u, d_part, d_sums;
    DevBuf<int64_t> d_bounds;
    HIP_TRY(d_w.alloc((size_t)n)); HIP_TRY(d_u.alloc((size_t)n_in));
    HIP_TRY(hipMemcpyAsync(d_w.p, weights, 8 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((unsigned)std::min<int64_t>((n_in + CS_BLOCK - 1) / CS_BLOCK, (int64_t)ctx->num_cu * 8));
    hipLaunchKernelGGL(k_gather_f64, grid, dim3(CS_BLOCK), 0, ctx->stream, (const double *)d_w.p, d_col_idx, n_in, 0.0, d_u.p);
    HIP_TRY(hipGetLastError());
    const int64_t bounds[2] = {0, n_in};
    const int bpc = (int)std::max<int64_t>(1, std::min<int64_t>(4 * (int64_t)ctx->num_cu, (n_in + 1023) / 1024));
    HIP_TRY(d_bounds.alloc(2)); HIP_TRY(d_part.alloc((size_t)bpc * 29)); HIP_TRY(d_sums.alloc(29));
    HIP_TRY(hipMemcpyAsync(d_bounds.p, bounds, sizeof bounds, hipMemcpyHostToDevice, ctx->stream));
    PCR_TRY(chunk_sums(ctx, 6, d_P, stride, nullptr, d_u.p, d_bounds.p, 1, bpc, d_part.p));
    hipLaunchKernelGGL(k_chunk_fold, dim3(1), dim3(CS_BLOCK), 0, ctx->stream, (const double *)d_part.p, 1, bpc, 29, d_sums.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_sums.p, 8 * 29, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

pcr_status pcr_terms_coreset(pcr_context *ctx, const double *d_P, int64_t stride, const int64_t *d_col_idx, int64_t n_in, int k,
                             int64_t n_target, int64_t *idx_out, double *w_out, int64_t *n_out) {
    static const bool stats = env_flag("PCR_CORESET_STATS");
    const auto t_all = std::chrono::steady_clock::now();
    double ms_elim = 0, ms_down = 0;
    int levels = 0;
    if (n_in <= n_target) {                                // every gated-in point, weight 1
        if (n_in > 0) {
            HIP_TRY(hipMemcpyAsync(idx_out, d_col_idx, 8 * (size_t)n_in, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        for (int64_t i = 0; i < n_in; ++i) w_out[i] = 1.0;
        *n_out = n_in;
    } else {
        DevBuf<double> d_u0;
        HIP_TRY(d_u0.alloc((size_t)n_in));
        const dim3 grid((unsigned)std::min<int64_t>((n_in + CS_BLOCK - 1) / CS_BLOCK, (int64_t)ctx->num_cu * 8));
        hipLaunchKernelGGL(k_gather_f64, grid, dim3(CS_BLOCK), 0, ctx->stream, (const double *)nullptr, (const int64_t *)nullptr, n_in, 1.0,
                           d_u0.p);
        HIP_TRY(hipGetLastError());
        PCR_TRY(coreset_core(ctx, 6, 28, d_P, stride, n_in, d_u0.p, k, n_target, d_col_idx, n_out, w_out, idx_out, nullptr, &ms_elim,
                             &ms_down, &levels));
    }
    if (stats)
        fprintf(stderr, "pcr_scan_coreset: n %lld m 28 levels %d -> %lld points; after the terms kernel %.3f ms: upload 0.000, "
                        "host elimination %.3f, read-backs (incl. waiting for the kernels before them) %.3f\n",
                (long long)n_in, levels, (long long)*n_out, ms_since(t_all), ms_elim, ms_down);
    return PCR_OK;
}
