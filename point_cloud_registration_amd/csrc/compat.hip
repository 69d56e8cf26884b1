// The compatibility graph of a match list and its second-order measure (SC2-PCR, Chen et al. 2022; TEASER's graph): which
// pairs of matches keep their length under a rigid motion, how many compatible neighbours two compatible matches share, and
// the consensus sets around the best-connected matches.  The contract is in include/pcr.h.
//
//   pcr_compat_bits        k_compat_bits
//   pcr_compat_degrees     k_compat_bits, k_compat_degrees
//   pcr_compat_consensus   k_compat_bits, k_compat_degrees, the seeds on the host, k_compat_consensus
//
// k_compat_bits: one wave = CP_ROWS rows i of the matrix, one lane = one column j of the current word: the lane keeps its
// match j in registers for the CP_ROWS tests (float64, two square roots each, no contraction: this unit is built with
// -ffp-contract=off), the rows' own matches are wave-uniform.  A ballot IS the 64-bit word; lane w & 63 keeps word w, and every
// 64 words the wave stores 512 consecutive bytes per row: each word is written once, by one lane, with a plain vector store.
//
// k_compat_degrees<R> (the hot kernel): one wave = R rows i (1; 4 for the longest lists), held in registers (W <= 512 words:
// 8 per lane and row).  It
// walks the set bits of its rows -- ballot over the lanes with a non-zero word, readlane, count-trailing-zeros: all scalar --
// and reads row j coalesced, once for all its rows that have bit j, two rows j in flight; AND, population count, one wave
// reduction per row at the end.  Everything is an integer.
//
// k_compat_consensus: one block = one seed s.  row s sits in LDS; the four waves take the set bits of row s in turn and leave
// score_sj (a 16-bit number: score <= m - 2 < 2^15) in an LDS array over j, 0xffff where C_sj = 0.  Then k - 1 rounds of the
// block-wide maximum of the 64-bit key (score << 32) | (0xffffffff - j) below the previous winner: keys are distinct, so the
// rounds hand out the candidates by score descending, ties to the smaller j.
//
// Environment: PCR_COMPAT_TIMES=1 (developer, tools/compat_time.py; read once per process) reports the kernels' milliseconds
// on stderr.
#include <algorithm>

#include "host_util.h"

#define CP_ROWS 4                    // rows per wave of k_compat_bits
#define CP_M_MAX PCR_COMPAT_M_MAX
#define CP_W_MAX (CP_M_MAX / 64)
#define CP_NONE 0xffffu              // k_compat_consensus: no score, C_sj = 0
static_assert(CP_M_MAX % 64 == 0 && CP_M_MAX - 2 < CP_NONE, "a score fits 16 bits beside the marker");

__device__ __forceinline__ int cp_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ uint64_t cp_readlane(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t cp_uniform(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long cp_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- the bit matrix ---------------------------------------------------------------------------------------------------------
struct CpV3 { double x, y, z; };
__device__ __forceinline__ CpV3 cp_ld(const float *__restrict__ a, int r) {
    return CpV3{(double)a[3 * (size_t)r], (double)a[3 * (size_t)r + 1], (double)a[3 * (size_t)r + 2]};
}
// |a - b|, the dot product as rs_dot writes it
__device__ __forceinline__ double cp_len(CpV3 a, CpV3 b) {
    const double x = a.x - b.x, y = a.y - b.y, z = a.z - b.z;
    return __builtin_sqrt((x * x + y * y) + z * z);
}

// rows [4 wave, 4 wave + 4) x all W words; m >= 1
__global__ void __launch_bounds__(256) k_compat_bits(const float *__restrict__ src, const float *__restrict__ dst, int m, int W, double d,
                                                     uint64_t *__restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int i0 = ((int)blockIdx.x * 4 + cp_wave()) * CP_ROWS;
    if (i0 >= m) return;                                       // the whole wave
    CpV3 pi[CP_ROWS], qi[CP_ROWS];
#pragma unroll
    for (int r = 0; r < CP_ROWS; ++r) {                        // a row past the end tests row m - 1 again and stores nothing
        const int i = i0 + r < m ? i0 + r : m - 1;
        pi[r] = cp_ld(src, i); qi[r] = cp_ld(dst, i);
    }
    uint64_t keep[CP_ROWS];
#pragma unroll
    for (int r = 0; r < CP_ROWS; ++r) keep[r] = 0;
    for (int w = 0; w < W; ++w) {
        const int j = w * 64 + lane;
        const int jj = j < m ? j : m - 1;
        const CpV3 pj = cp_ld(src, jj), qj = cp_ld(dst, jj);
#pragma unroll
        for (int r = 0; r < CP_ROWS; ++r) {
            const bool ok = j < m && j != i0 + r && __builtin_fabs(cp_len(pi[r], pj) - cp_len(qi[r], qj)) <= d;
            const uint64_t word = __ballot(ok);
            if (lane == (w & 63)) keep[r] = word;
        }
        if ((w & 63) == 63 || w == W - 1) {
            const int t = (w & ~63) + lane;
            if (t <= w) {
#pragma unroll
                for (int r = 0; r < CP_ROWS; ++r)
                    if (i0 + r < m) bits[(size_t)(i0 + r) * W + t] = keep[r];
            }
        }
    }
}

// ---- the degrees ------------------------------------------------------------------------------------------------------------
// rows [R wave, R wave + R) of the launch's waves, each in CP_NCH words per lane: word 64 k + lane is chunk k.  The wave walks
// the UNION of the set bits of its rows, loads row j once and adds it to every row of its own that has bit j (a scalar test):
// where the rows' sets coincide (a clean match list: C is dense) a row j is read once for R rows, where they are disjoint
// nothing is lost.  R = 4 takes 136 VGPRs and a quarter of the waves: it pays above CP_SHARE_MIN rows, up to there R = 1
// (docs/EXPERIMENTS.md).  The
// chunks a row of W words has are a wave-uniform count, so the unrolled loops over k skip the others with a scalar branch and
// the words stay in registers.  A lane's word past the end of the row (in its last chunk) is 0 on the side of row i and is read
// from word W - 1 on the side of row j: it adds nothing, and the inner loop has no per-lane test.  A row past m is all 0.
#define CP_NCH (CP_W_MAX / 64)
#define CP_SHARE_MIN 16384           // m above this: four rows per wave
template <int R>
__global__ void __launch_bounds__(256) k_compat_degrees(const uint64_t *__restrict__ bits, int m, int W, int64_t *__restrict__ deg1,
                                                        int64_t *__restrict__ deg2) {
    const int lane = threadIdx.x & 63;
    const int i0 = ((int)blockIdx.x * 4 + cp_wave()) * R;
    if (i0 >= m) return;
    uint64_t mine[R][CP_NCH];
    int col[CP_NCH];
    uint32_t d1[R], acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) d1[r] = acc[r] = 0;
#pragma unroll
    for (int k = 0; k < CP_NCH; ++k) {
        const int t = k * 64 + lane;
        col[k] = t < W ? t : W - 1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            mine[r][k] = t < W && i0 + r < m ? bits[(size_t)(i0 + r) * W + t] : 0;
            d1[r] += (uint32_t)__popcll(mine[r][k]);
        }
    }
#pragma unroll
    for (int k = 0; k < CP_NCH; ++k) {
        if (k * 64 >= W) break;
        uint64_t any = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) any |= mine[r][k];
        uint64_t lanes = __ballot(any != 0);
        while (lanes) {
            const int L = __builtin_ctzll(lanes);
            lanes &= lanes - 1;
            uint64_t w[R], word = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) { w[r] = cp_readlane(mine[r][k], L); word |= w[r]; }
            const int base = (k * 64 + L) * 64;
            while (word) {                                     // two rows j in flight
                const int b0 = __builtin_ctzll(word);
                word &= word - 1;
                const bool two = word != 0;
                const int b1 = two ? __builtin_ctzll(word) : b0;
                word &= word - 1;
                const uint64_t *r0 = bits + (size_t)(base + b0) * W, *r1 = bits + (size_t)(base + b1) * W;
                uint64_t a[CP_NCH], c[CP_NCH];
#pragma unroll
                for (int kk = 0; kk < CP_NCH; ++kk)
                    if (kk * 64 < W) { a[kk] = r0[col[kk]]; c[kk] = r1[col[kk]]; }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if ((w[r] >> b0) & 1) {
#pragma unroll
                        for (int kk = 0; kk < CP_NCH; ++kk)
                            if (kk * 64 < W) acc[r] += (uint32_t)__popcll(mine[r][kk] & a[kk]);
                    }
                    if (two && ((w[r] >> b1) & 1)) {
#pragma unroll
                        for (int kk = 0; kk < CP_NCH; ++kk)
                            if (kk * 64 < W) acc[r] += (uint32_t)__popcll(mine[r][kk] & c[kk]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned long long s1 = cp_wave_sum(d1[r]), s2 = cp_wave_sum(acc[r]);
        if (lane == 0 && i0 + r < m) { deg1[i0 + r] = (int64_t)s1; deg2[i0 + r] = (int64_t)s2; }
    }
}

// ---- the consensus sets -----------------------------------------------------------------------------------------------------
// block = seed; members / scores [blockIdx.x * k ..): the seed and its degree, then the k - 1 best candidates, then -1
__global__ void __launch_bounds__(256) k_compat_consensus(const uint64_t *__restrict__ bits, int m, int W, const int32_t *__restrict__ seeds, int k,
                                                          int32_t *__restrict__ members, int32_t *__restrict__ scores) {
    __shared__ uint64_t s_row[CP_W_MAX];
    __shared__ uint16_t s_score[CP_M_MAX];
    __shared__ unsigned long long s_best[4];
    const int lane = threadIdx.x & 63, wave = cp_wave();
    const int s = seeds[blockIdx.x];
    const uint64_t *row = bits + (size_t)s * W;
    for (int t = threadIdx.x; t < W; t += 256) s_row[t] = row[t];
    for (int j = threadIdx.x; j < m; j += 256) s_score[j] = CP_NONE;
    __syncthreads();
    // score_sj of every set bit j of row s: one wave per j, its words coalesced
    for (int t = wave; t < W; t += 4) {
        uint64_t word = cp_uniform(s_row[t]);
        while (word) {
            const int j = t * 64 + __builtin_ctzll(word);
            word &= word - 1;
            const uint64_t *rj = bits + (size_t)j * W;
            uint32_t n = 0;
            for (int u = lane; u < W; u += 64) n += (uint32_t)__popcll(s_row[u] & rj[u]);
            const unsigned long long total = cp_wave_sum(n);
            if (lane == 0) s_score[j] = (uint16_t)total;
        }
    }
    if (wave == 0) {                                           // slot 0: the seed, with score_ss = deg1_s
        uint32_t n = 0;
        for (int u = lane; u < W; u += 64) n += (uint32_t)__popcll(s_row[u]);
        const unsigned long long total = cp_wave_sum(n);
        if (lane == 0) { members[(size_t)blockIdx.x * k] = s; scores[(size_t)blockIdx.x * k] = (int32_t)total; }
    }
    __syncthreads();
    unsigned long long prev = ~0ull;
    for (int slot = 1; slot < k; ++slot) {
        unsigned long long best = 0;
        if (prev) {                                            // (uniform) nothing is left below key 0: the rest is padding
            for (int j = threadIdx.x; j < m; j += 256) {
                const uint32_t sc = s_score[j];
                const unsigned long long key = ((unsigned long long)sc << 32) | (unsigned long long)(0xffffffffu - (uint32_t)j);
                if (sc != CP_NONE && key < prev && key > best) best = key;
            }
#pragma unroll
            for (int dd = 32; dd >= 1; dd >>= 1) {
                const unsigned long long o = __shfl_xor(best, dd, 64);
                best = o > best ? o : best;
            }
            if (lane == 0) s_best[wave] = best;
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 4; ++v) best = s_best[v] > best ? s_best[v] : best;
            __syncthreads();                                   // s_best is written again in the next round
        }
        if (threadIdx.x == 0) {
            members[(size_t)blockIdx.x * k + slot] = best ? (int32_t)(0xffffffffu - (uint32_t)best) : -1;
            scores[(size_t)blockIdx.x * k + slot] = best ? (int32_t)(best >> 32) : -1;
        }
        prev = best;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
static pcr_status cp_check(const float *src, const float *dst, int64_t m, double d, const char *who) {
    if (m < 0 || m > CP_M_MAX) { pcr_set_error("invalid argument: %s needs 0 <= m <= %d (PCR_COMPAT_M_MAX)", who, CP_M_MAX); return PCR_ERR_INVALID; }
    if (!(d > 0 && d <= DBL_MAX)) { pcr_set_error("invalid argument: %s needs a finite d > 0", who); return PCR_ERR_INVALID; }
    PCR_REQUIRE(m == 0 || (src && dst), "NULL argument");
    return PCR_OK;
}

// pcr_compat_consensus: the n rows with the largest deg2, ties to the smaller row, in that order (n <= m)
static void cp_pick_seeds(const int64_t *deg2, int64_t m, int n, int32_t *seeds) {
    std::vector<int32_t> rows((size_t)m);
    for (int64_t i = 0; i < m; ++i) rows[(size_t)i] = (int32_t)i;
    std::partial_sort(rows.begin(), rows.begin() + n, rows.end(),
                      [deg2](int32_t a, int32_t b) { return deg2[a] != deg2[b] ? deg2[a] > deg2[b] : a < b; });
    for (int e = 0; e < n; ++e) seeds[e] = rows[(size_t)e];
}

// the device side of one call: the matches and the bit matrix; m >= 1
struct CompatCall {
    pcr_context *ctx = nullptr;
    int m = 0, W = 0;
    DevBuf<float> src, dst;
    DevBuf<uint64_t> bits;
    DevBuf<int64_t> deg1, deg2;

    size_t words() const { return (size_t)m * (size_t)W; }
    pcr_status upload(pcr_context *c, const float *h_src, const float *h_dst, int64_t m_) {
        ctx = c; m = (int)m_; W = (m + 63) / 64;
        HIP_TRY(src.alloc(3 * (size_t)m)); HIP_TRY(dst.alloc(3 * (size_t)m)); HIP_TRY(bits.alloc(words()));
        HIP_TRY(hipMemcpyAsync(src.p, h_src, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(dst.p, h_dst, 12 * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
        return PCR_OK;
    }
    pcr_status run_bits(double d) {
        hipLaunchKernelGGL(k_compat_bits, grid_for(m, 4 * CP_ROWS), dim3(256), 0, ctx->stream, (const float *)src.p, (const float *)dst.p, m, W, d,
                           bits.p);
        HIP_TRY(hipGetLastError());
        return PCR_OK;
    }
    pcr_status run_degrees() {
        HIP_TRY(deg1.alloc((size_t)m)); HIP_TRY(deg2.alloc((size_t)m));
        const uint64_t *b = bits.p;
        if (m > CP_SHARE_MIN) hipLaunchKernelGGL(k_compat_degrees<4>, grid_for(m, 16), dim3(256), 0, ctx->stream, b, m, W, deg1.p, deg2.p);
        else hipLaunchKernelGGL(k_compat_degrees<1>, grid_for(m, 4), dim3(256), 0, ctx->stream, b, m, W, deg1.p, deg2.p);
        HIP_TRY(hipGetLastError());
        return PCR_OK;
    }
};

extern "C" pcr_status pcr_compat_bits(pcr_context *ctx, const float *src, const float *dst, int64_t m, double d, uint64_t *bits) {
    PCR_REQUIRE(ctx, "NULL argument");
    PCR_TRY(cp_check(src, dst, m, d, "pcr_compat_bits"));
    if (m == 0) return PCR_OK;
    PCR_REQUIRE(bits, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    CompatCall call;
    PCR_TRY(call.upload(ctx, src, dst, m));
    static const bool times = env_flag("PCR_COMPAT_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    PCR_TRY(call.run_bits(d));
    ev.mark(1, ctx->stream);
    HIP_TRY(hipMemcpyAsync(bits, call.bits.p, 8 * call.words(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on) fprintf(stderr, "pcr_compat_times bits m %lld words %d bits_ms %.4f\n", (long long)m, call.W, ev.ms(0));
    return PCR_OK;
}

extern "C" pcr_status pcr_compat_degrees(pcr_context *ctx, const float *src, const float *dst, int64_t m, double d, int64_t *deg1, int64_t *deg2) {
    PCR_REQUIRE(ctx, "NULL argument");
    PCR_TRY(cp_check(src, dst, m, d, "pcr_compat_degrees"));
    if (m == 0) return PCR_OK;
    PCR_REQUIRE(deg1 && deg2, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    CompatCall call;
    PCR_TRY(call.upload(ctx, src, dst, m));
    static const bool times = env_flag("PCR_COMPAT_TIMES");
    StageTimes ev;
    HIP_TRY(ev.init(times));
    ev.mark(0, ctx->stream);
    PCR_TRY(call.run_bits(d));
    ev.mark(1, ctx->stream);
    PCR_TRY(call.run_degrees());
    ev.mark(2, ctx->stream);
    HIP_TRY(hipMemcpyAsync(deg1, call.deg1.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(deg2, call.deg2.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on)
        fprintf(stderr, "pcr_compat_times degrees m %lld words %d bits_ms %.4f degrees_ms %.4f\n", (long long)m, call.W, ev.ms(0), ev.ms(1));
    return PCR_OK;
}

extern "C" pcr_status pcr_compat_consensus(pcr_context *ctx, const float *src, const float *dst, int64_t m, double d, int n_seeds, int k,
                                           int64_t *deg1_or_null, int64_t *deg2_or_null, int32_t *seeds, int32_t *members, int32_t *scores,
                                           int *n_seeds_out) {
    PCR_REQUIRE(ctx, "NULL argument");
    PCR_TRY(cp_check(src, dst, m, d, "pcr_compat_consensus"));
    if (k < 2 || k > PCR_COMPAT_K_MAX) {
        pcr_set_error("invalid argument: pcr_compat_consensus needs 2 <= k <= %d (PCR_COMPAT_K_MAX)", PCR_COMPAT_K_MAX);
        return PCR_ERR_INVALID;
    }
    if (n_seeds < 1) { pcr_set_error("invalid argument: pcr_compat_consensus needs n_seeds >= 1"); return PCR_ERR_INVALID; }
    PCR_REQUIRE(n_seeds_out, "NULL argument");
    if (m == 0) { *n_seeds_out = 0; return PCR_OK; }
    PCR_REQUIRE(seeds && members && scores, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    CtxScope scope(ctx);
    const int n = (int64_t)n_seeds < m ? n_seeds : (int)m;
    CompatCall call;
    PCR_TRY(call.upload(ctx, src, dst, m));
    static const bool times = env_flag("PCR_COMPAT_TIMES");
    StageTimes ev, ev2;                                        // bits | degrees, then the seeds on the host, then consensus
    HIP_TRY(ev.init(times)); HIP_TRY(ev2.init(times));
    ev.mark(0, ctx->stream);
    PCR_TRY(call.run_bits(d));
    ev.mark(1, ctx->stream);
    PCR_TRY(call.run_degrees());
    ev.mark(2, ctx->stream);
    std::vector<int64_t> h_deg1((size_t)m), h_deg2((size_t)m);
    if (deg1_or_null) HIP_TRY(hipMemcpyAsync(h_deg1.data(), call.deg1.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_deg2.data(), call.deg2.p, 8 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> h_seeds((size_t)n), h_members((size_t)n * k), h_scores((size_t)n * k);
    cp_pick_seeds(h_deg2.data(), m, n, h_seeds.data());
    DevBuf<int32_t> d_seeds, d_members, d_scores;
    HIP_TRY(d_seeds.alloc((size_t)n)); HIP_TRY(d_members.alloc((size_t)n * k)); HIP_TRY(d_scores.alloc((size_t)n * k));
    HIP_TRY(hipMemcpyAsync(d_seeds.p, h_seeds.data(), 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    ev2.mark(0, ctx->stream);
    hipLaunchKernelGGL(k_compat_consensus, dim3((unsigned)n), dim3(256), 0, ctx->stream, (const uint64_t *)call.bits.p, call.m, call.W,
                       (const int32_t *)d_seeds.p, k, d_members.p, d_scores.p);
    HIP_TRY(hipGetLastError());
    ev2.mark(1, ctx->stream);
    HIP_TRY(hipMemcpyAsync(h_members.data(), d_members.p, 4 * (size_t)n * k, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_scores.data(), d_scores.p, 4 * (size_t)n * k, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ev.on)
        fprintf(stderr, "pcr_compat_times consensus m %lld words %d seeds %d k %d bits_ms %.4f degrees_ms %.4f consensus_ms %.4f\n", (long long)m,
                call.W, n, k, ev.ms(0), ev.ms(1), ev2.ms(0));
    // nothing can fail from here: the outputs are written together
    if (deg1_or_null) for (int64_t i = 0; i < m; ++i) deg1_or_null[i] = h_deg1[(size_t)i];
    if (deg2_or_null) for (int64_t i = 0; i < m; ++i) deg2_or_null[i] = h_deg2[(size_t)i];
    for (int e = 0; e < n; ++e) seeds[e] = h_seeds[(size_t)e];
    for (size_t e = 0; e < (size_t)n * k; ++e) { members[e] = h_members[e]; scores[e] = h_scores[e]; }
    *n_seeds_out = n;
    return PCR_OK;
}
