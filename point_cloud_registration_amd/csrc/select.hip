// An exact order statistic on the device: the radix select of select.h.
//
//   k_select_hist   round d of 8: every key < +inf whose ordered pattern shares the digits chosen so far adds 1 to the bin of
//                   its digit d -- in the block's LDS histogram (integer LDS atomics), then one integer add per non-empty bin
//                   and block into SelectState::hist[d].  Integer adds are exact in any order, so the histogram does not
//                   depend on the grid.
//   k_select_pick   one block of 256 lanes, lane = bin: an inclusive scan of the 256 counts in LDS; the one lane whose bin
//                   holds the rank writes the digit into the prefix and narrows rank and below.  Round 0 also takes m (the
//                   total of its histogram) and the rank; round 7 turns the prefix back into the key, tau, counts the keys
//                   <= tau (below + the scan up to its bin), takes c = factor * sqrt(tau), c2 = c * c, and states
//                   what the reduce behind it reads (select.h: w_kind, w_c, w_c2).
//   k_select_drop   behind the selection, for a trim: the entries of a match list whose stored key is not <= tau leave it.
//
// The order of float64 `<` on the bit pattern: -0.0 is taken as +0.0 (they are equal under `<`), then a negative pattern is
// inverted and a positive one gets its sign bit set -- the usual flip.  NaN and +inf are outside: not (key < +inf).
#include <math.h>

#include <vector>

#include "select.h"

__device__ __forceinline__ bool select_ordered(double key, unsigned long long &u) {
    if (!(key < (double)INFINITY)) return false;                      // +inf, NaN
    const unsigned long long b = key == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(key);
    u = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return true;
}
__device__ __forceinline__ double select_key(unsigned long long u) {
    const unsigned long long b = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    return __longlong_as_double((long long)b);
}

__global__ void __launch_bounds__(256) k_select_hist(const double *__restrict__ keys, int64_t n, SelectState *st, int round) {
    __shared__ unsigned int h[PCR_SELECT_BINS];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * round;
    const unsigned long long prefix = st->prefix;
    // the digits above this round's: all ones from bit shift + 8 up (none in round 0)
    const unsigned long long above = round == 0 ? 0ull : ~0ull << (shift + 8);
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        unsigned long long u;
        if (!select_ordered(keys[i], u)) continue;
        if ((u & above) != (prefix & above)) continue;
        atomicAdd(&h[(unsigned)(u >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned int c = h[threadIdx.x];
    if (c) atomicAdd(&st->hist[round][threadIdx.x], (unsigned long long)c);
}

__global__ void __launch_bounds__(256) k_select_pick(SelectState *st, int round, double quantile, unsigned long long k_fixed, int kind, double factor,
                                                     double *stats) {
    __shared__ unsigned long long scan[PCR_SELECT_BINS];
    const int b = threadIdx.x;
    const unsigned long long mine = st->hist[round][b];
    // what an earlier launch left, read by every lane BEFORE the barriers below: the one lane that writes does so behind them
    const unsigned long long m0 = round == 0 ? 1ull : st->m, rank0 = st->rank, below0 = st->below, prefix0 = st->prefix;
    scan[b] = mine;
    __syncthreads();
    // inclusive scan (Hillis-Steele: 8 steps, each read behind a barrier)
    for (int d = 1; d < PCR_SELECT_BINS; d <<= 1) {
        const unsigned long long add = b >= d ? scan[b - d] : 0ull;
        __syncthreads();
        scan[b] += add;
        __syncthreads();
    }
    const unsigned long long incl = scan[b], excl = incl - mine, total = scan[PCR_SELECT_BINS - 1];
    unsigned long long rank, below;
    if (round == 0) {
        // every lane takes the same m and rank: nothing is read back from the state
        unsigned long long k = k_fixed;
        if (k == 0ull) {
            k = (unsigned long long)floor(quantile * (double)total);
            if (k < 1ull) k = 1ull;
        }
        if (k > total) k = total;
        if (b == 0) {
            st->m = total; st->k = k;
            if (total == 0ull) {
                st->tau = (double)INFINITY; st->c = 0.0; st->c2 = 0.0; st->kind = kind; st->n_le = 0ull;
                st->w_kind = PCR_ROBUST_HUBER; st->w_c = 0.0; st->w_c2 = 0.0;      // (no term reads them)
                if (stats) { stats[0] = (double)INFINITY; stats[1] = 0.0; stats[2] = 0.0; stats[3] = 0.0; stats[4] = 0.0; }
            }
        }
        rank = k; below = 0ull;
    } else {
        if (m0 == 0ull) return;
        rank = rank0; below = below0;
    }
    if (!(mine != 0ull && excl < rank && rank <= incl)) return;
    // the one lane whose bin holds the rank
    const int shift = 56 - 8 * round;
    const unsigned long long prefix = (round == 0 ? 0ull : prefix0) | ((unsigned long long)b << shift);
    st->prefix = prefix;
    st->rank = rank - excl;
    st->below = below + excl;
    if (round != PCR_SELECT_DIGITS - 1) return;
    const double tau = select_key(prefix);
    const unsigned long long n_le = below + incl;
    double c = 0.0;
    if (kind != PCR_ROBUST_TRIM) c = factor * __builtin_sqrt(tau);
    const double c2 = c * c;
    st->tau = tau; st->c = c; st->c2 = c2; st->kind = kind; st->n_le = n_le;
    const bool trim = kind == PCR_ROBUST_TRIM, limit = !(c2 > 0.0);
    st->w_kind = trim || limit ? PCR_ROBUST_HUBER : kind;
    st->w_c = trim || limit ? 0.0 : c;
    st->w_c2 = trim ? (double)INFINITY : (limit ? 0.0 : c2);
    if (stats) { stats[0] = tau; stats[1] = c; stats[2] = (double)n_le; stats[3] = (double)st->k; stats[4] = (double)st->m; }
}

// (a NaN or +inf key fails the compare: its entry is `none` already, or becomes it)
__global__ void __launch_bounds__(256) k_select_drop(const double *__restrict__ keys, int64_t n, const SelectState *__restrict__ st, uint32_t *idx,
                                                     uint32_t none) {
    const double tau = st->tau;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        if (!(keys[i] <= tau)) idx[i] = none;
}

pcr_status pcr_select_launch(pcr_context *ctx, const double *keys, int64_t n, double quantile, int64_t k_fixed, int kind, double factor,
                             SelectState *st, double *stats_or_null) {
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(SelectState), ctx->stream));
    const int64_t want = (n + 255) / 256;
    const unsigned nb = (unsigned)(want < PCR_SELECT_MAX_BLOCKS ? want : PCR_SELECT_MAX_BLOCKS);
    {
        RoctxRange range("pcr:select");
        for (int round = 0; round < PCR_SELECT_DIGITS; ++round) {
            hipLaunchKernelGGL(k_select_hist, dim3(nb), dim3(256), 0, ctx->stream, keys, n, st, round);
            hipLaunchKernelGGL(k_select_pick, dim3(1), dim3(256), 0, ctx->stream, st, round, quantile, (unsigned long long)k_fixed, kind, factor,
                               stats_or_null);
        }
    }
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

pcr_status pcr_select_drop_launch(pcr_context *ctx, const double *keys, int64_t n, const SelectState *st, uint32_t *idx, uint32_t none) {
    const int64_t want = (n + 255) / 256;
    const unsigned nb = (unsigned)(want < PCR_SELECT_MAX_BLOCKS ? want : PCR_SELECT_MAX_BLOCKS);
    hipLaunchKernelGGL(k_select_drop, dim3(nb), dim3(256), 0, ctx->stream, keys, n, st, idx, none);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

extern "C" pcr_status pcr_order_statistic(pcr_context *ctx, const double *keys, int64_t n, int64_t k, double *value, int64_t *n_le) {
    PCR_REQUIRE(ctx && keys && value && n_le, "NULL argument");
    PCR_REQUIRE(n >= 1, "n must be at least 1");
    PCR_REQUIRE(k >= 1, "k must be at least 1");
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) m += keys[i] < (double)INFINITY;
    PCR_REQUIRE(k <= m, "k exceeds the number of keys < +inf");
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    DevBuf<double> d_keys;
    DevBuf<SelectState> st;
    HIP_TRY(d_keys.alloc((size_t)n)); HIP_TRY(st.alloc(1));
    HIP_TRY(hipMemcpyAsync(d_keys.p, keys, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    PCR_TRY(pcr_select_launch(ctx, d_keys.p, n, 1.0, k, PCR_ROBUST_TRIM, 0.0, st.p, nullptr));
    // (the state's tail: m .. kind)
    struct { unsigned long long m, k, n_le; double tau; } r;
    HIP_TRY(hipMemcpyAsync(&r, &st.p->m, sizeof r, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *value = r.tau;
    *n_le = (int64_t)r.n_le;
    return PCR_OK;
}
