// One per-point payload of a scan (pcr_scan::cov, ::nrm, ::inten; C = 6, 3, 1 floats per point), stated once: it lives in
// DEVICE order and crosses the boundary in the CALLER's order through pcr_scan::order.  gicp.hip, symm.hip and color.hip keep
// their __global__ wrappers (k_gicp_scov_perm / k_symm_perm / k_color_perm <TO_DEVICE>) around payload_perm and their
// extern "C" entry points with the argument checks; everything behind the checks is here.
#pragma once

#include "host_util.h"

// TO_DEVICE: dev[i] = caller[order[i]]; else caller[order[i]] = dev[i] (order NULL: the same order)
template <int C, bool TO_DEVICE>
__device__ __forceinline__ void payload_perm(const float *__restrict__ in, int64_t n, const uint32_t *__restrict__ order, float *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t c = order ? (size_t)order[i] : (size_t)i;
    const float *src = in + C * (TO_DEVICE ? c : (size_t)i);
    float *dst = out + C * (TO_DEVICE ? (size_t)i : c);
#pragma unroll
    for (int a = 0; a < C; ++a) dst[a] = src[a];
}

template <int C>
struct ScanPayload {
    typedef void (*perm_fn)(const float *, int64_t, const uint32_t *, float *);
    float *pcr_scan::*slot;             // the scan's array
    perm_fn to_device, to_caller;       // the unit's wrappers of payload_perm<C, true> / <C, false>, blocks of 256

    pcr_status alloc(pcr_scan *s) const {
        if (!(s->*slot)) HIP_TRY(pcr_scan_alloc(s, (void **)&(s->*slot), 4 * C * (size_t)(s->n ? s->n : 1)));
        return PCR_OK;
    }

    // the caller's array -> the scan (allocated if absent)
    pcr_status set(pcr_scan *s, const float *host) const {
        pcr_context *ctx = s->ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        CtxScope scope(ctx);
        PCR_TRY(alloc(s));
        if (s->n == 0) return PCR_OK;
        DevBuf<float> d;
        HIP_TRY(d.alloc(C * (size_t)s->n));
        HIP_TRY(hipMemcpyAsync(d.p, host, 4 * C * (size_t)s->n, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(to_device, grid_for(s->n, 256), dim3(256), 0, ctx->stream, (const float *)d.p, s->n, (const uint32_t *)s->order, s->*slot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PCR_OK;
    }

    // the scan's array -> the caller's
    pcr_status get(pcr_scan *s, float *host) const {
        pcr_context *ctx = s->ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        CtxScope scope(ctx);
        if (s->n == 0) return PCR_OK;
        DevBuf<float> d;
        HIP_TRY(d.alloc(C * (size_t)s->n));
        hipLaunchKernelGGL(to_caller, grid_for(s->n, 256), dim3(256), 0, ctx->stream, (const float *)(s->*slot), s->n, (const uint32_t *)s->order, d.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, d.p, 4 * C * (size_t)s->n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PCR_OK;
    }

    // fill(idx, dst) enqueues the estimate of every point over the scan's self-index (pcr_scan_self_index: its input order is
    // the scan's device order, so pt_orig lands a point's floats in dst directly).  Into the scan's array when it has one, else
    // into a block the scan takes over only once the estimate is complete: a failure on the way must not leave a scan that
    // "has" the payload holding uninitialised values
    template <typename FILL>
    pcr_status estimate(pcr_scan *s, float *host_or_null, FILL fill) const {
        pcr_context *ctx = s->ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        CtxScope scope(ctx);
        if (s->n == 0) return alloc(s);
        float *dst = s->*slot;
        const bool fresh = !dst;
        if (fresh) HIP_TRY(pcr_scan_alloc(s, (void **)&dst, 4 * C * (size_t)s->n));
        struct Undo {
            pcr_scan *s; float *p; bool armed;
            ~Undo() { if (armed) { pcr_scan_free(s, p); } }
        } undo{s, dst, true};
        s->*slot = nullptr;                          // (re-estimating: a failure leaves the scan without the payload)
        {
            TmpIndex idx;
            PCR_TRY(pcr_scan_self_index(s, &idx));
            PCR_TRY(fill(idx.t, dst));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        undo.armed = false;
        s->*slot = dst;
        if (host_or_null) return get(s, host_or_null);
        return PCR_OK;
    }
};
