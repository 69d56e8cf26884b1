// A pass over a match list, stated once: the three-phase reduce loop, the fold, the host driver of the two launches and the
// scaffold of a pcr_pass_fn around them.  Behind GICP, VGICP, SymmetricICP and ColoredICP (gicp.hip, vgicp.hip, symm.hip,
// color.hip); each keeps its own __global__ one-liners (k_gicp_* / k_vgicp_* / k_symm_* / k_color_*) and its *_W.
//
// A SIDE is a unit's kernel-argument struct (GicpArgs, VgicpArgs, SymmArgs, ColorArgs): its arrays, its parameters, rows -- and
//   Scan                      what phase A carries per scan point beside index and coordinates
//   load(i, Scan&)            the loads of scan point i (device order); nothing else
//   Match                     what phase B carries per correspondence
//   gather(a, j, Match&)      the loads of one match at cell-sorted index j; nothing else
//   add(acc, a, P, x, y, z, tx, ty, tz, scan, match)
//                             residual, gate and sums of one correspondence; (tx, ty, tz) = xform(P, x, y, z)
#pragma once

#include "host_util.h"
#include "pass_device.h"

// W points per lane in flight, the phases of reduce_stream (pass_device.h):
//   phase A  index, coordinates and Scan of all W points.  A point past the end reads the lane's first point.
//   phase B  the W matches.  No match: element 0 through a select on the index -- always there -- and skipped in phase C;
//            no branch between the gathers.
//   phase C  SIDE::add -- in index order.
// Fold: wave shuffles in a fixed order, LDS across the waves in wave order, ONE row of 32 doubles per block with plain
// stores (block_store_partials).  No tickets, no atomics, no in-launch hand-off.
template <int W, typename SIDE>
__device__ __forceinline__ void match_reduce(const LinArgs &a, const SIDE &sd) {
    const PoseK &P = a.hp;                           // host-driven: the pose came by value
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x; t0 < a.n; t0 += W * stride) {
        uint32_t j[W];
        float x[W], y[W], z[W];
        typename SIDE::Scan sc[W];
        typename SIDE::Match m[W];
        bool use[W];
        // phase A
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const int64_t t = t0 + u * stride;
            use[u] = t < a.n;
            const int64_t i = use[u] ? t : t0;
            j[u] = a.nn_j[i];
            x[u] = a.sx[i]; y[u] = a.sy[i]; z[u] = a.sz[i];
            sd.load(i, sc[u]);
        }
        reduce_phase();
#pragma unroll
        for (int u = 0; u < W; ++u) reduce_pin(j[u]);
        // phase B
#pragma unroll
        for (int u = 0; u < W; ++u) {
            use[u] = use[u] && j[u] != PCR_NONE;
            sd.gather(a, use[u] ? j[u] : 0u, m[u]);
        }
        reduce_phase();
        // phase C
#pragma unroll
        for (int u = 0; u < W; ++u) {
            if (!use[u]) continue;
            float tx, ty, tz;
            xform(P, x[u], y[u], z[u], tx, ty, tz);
            sd.add(acc, a, P, x[u], y[u], z[u], tx, ty, tz, sc[u], m[u]);
        }
    }
    block_store_partials<false>(acc, sd.rows);
}

// one block: thread e < 29 adds rows 0 .. nb-1 in order.  The kernel boundary is the only ordering between the two launches;
// the grid depends on n and the device only, so two calls return the same bits.
__device__ __forceinline__ void match_fold(const double *__restrict__ rows, int nb, double *out) {
    const int e = threadIdx.x;
    if (e >= 29) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += rows[(size_t)b * 32 + e];
    out[e] = s;
}

// reduce + fold + 29 doubles back behind a search into `a`: one stream synchronisation, device blocks from the context's
// block cache.  sd comes with everything but rows set.
template <typename SIDE>
static pcr_status match_launch(pcr_context *ctx, const char *range_name, void (*reduce)(const LinArgs, const SIDE),
                               void (*fold)(const double *, int, double *), const LinArgs &a, SIDE sd, int64_t n, double out[29]) {
    const int nb = choose_blocks(ctx, n);            // n and the device only
    DevBuf<double> rows, sums;
    HIP_TRY(rows.alloc(32 * (size_t)nb)); HIP_TRY(sums.alloc(32));
    sd.rows = rows.p;
    {
        RoctxRange range(range_name);
        hipLaunchKernelGGL(reduce, dim3((unsigned)nb), dim3(256), 0, ctx->stream, a, sd);
        hipLaunchKernelGGL(fold, dim3(1), dim3(64), 0, ctx->stream, (const double *)rows.p, nb, sums.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sums.p, 29 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

// What a pcr_pass_fn does once the unit has checked its payloads: kind's full search (pass.hip: pcr_rows_search) into a match
// buffer of the call, 29 zeros, and -- for a scan with points -- match_launch
template <typename SIDE>
static pcr_status match_pass(pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist, unsigned flags, const char *range_name,
                             void (*reduce)(const LinArgs, const SIDE), void (*fold)(const double *, int, double *), const SIDE &sd,
                             double out[29]) {
    LinArgs a;
    DevBuf<uint32_t> nn;
    PCR_TRY(pcr_rows_search(&a, &nn, t, s, kind, T, max_dist, flags, false));
    for (int i = 0; i < 29; ++i) out[i] = 0.0;
    if (s->n == 0) return PCR_OK;
    return match_launch(t->ctx, range_name, reduce, fold, a, sd, s->n, out);
}
