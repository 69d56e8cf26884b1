// The host scaffold of the neighbourhood units (radius.hip, fpfh.hip, keypoints.hip, ransac.hip, knn_normals.hip, gicp.hip,
// vgicp.hip, coreset.hip): the event bracket behind the PCR_*_TIMES lines, the environment switches, the launch grid, the
// argument checks they share and the copy-back of a uint32 array the C ABI hands out as int64.  Host code only.
#pragma once

#include <float.h>
#include <math.h>
#include <stdlib.h>

#include "pcr_internal.h"

// ---- environment switches -----------------------------------------------------------------------------------------------
// Read once per process: a call site keeps the value in a function-local static.  An empty value counts as unset.
static inline bool env_flag(const char *name) {
    const char *v = getenv(name);
    return v && atoll(v) != 0;
}
static inline int64_t env_i64(const char *name, int64_t dflt, int64_t lo, int64_t hi) {
    const char *v = getenv(name);
    const int64_t x = v && *v ? (int64_t)atoll(v) : dflt;
    return x < lo ? lo : (x > hi ? hi : x);
}

// ---- stage times --------------------------------------------------------------------------------------------------------
// Up to 4 marks on a stream; ms(i) = the milliseconds between mark i and mark i + 1, waiting for the later one.  Without
// init(true) every call is a no-op, so a unit brackets its kernels unconditionally:
//     static const bool times = env_flag("PCR_X_TIMES");
//     StageTimes ev;  HIP_TRY(ev.init(times));  ev.mark(0, s);  launch;  ev.mark(1, s);  ...  if (ev.on) fprintf(stderr, ..., ev.ms(0));
struct StageTimes {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    StageTimes() = default;
    StageTimes(const StageTimes &) = delete;
    StageTimes &operator=(const StageTimes &) = delete;
    ~StageTimes() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t init(bool want) {
        on = want;
        if (want) for (hipEvent_t &e : ev) { const hipError_t s = hipEventCreate(&e); if (s != hipSuccess) return s; }
        return hipSuccess;
    }
    void mark(int i, hipStream_t s) { if (on) (void)hipEventRecord(ev[i], s); }
    float ms(int i) {
        float m = 0;
        if (on) { (void)hipEventSynchronize(ev[i + 1]); (void)hipEventElapsedTime(&m, ev[i], ev[i + 1]); }
        return m;
    }
};

// ---- launches -----------------------------------------------------------------------------------------------------------
// one lane per element, blocks of `block` lanes
static inline dim3 grid_for(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// ---- argument checks ----------------------------------------------------------------------------------------------------
static inline pcr_status check_point_target(const pcr_target *t, const char *who) {
    if (t->is_voxel) { pcr_set_error("invalid argument: %s needs a point target", who); return PCR_ERR_INVALID; }
    return PCR_OK;
}
// finite and >= 0 (false for NaN)
template <typename Real>
static inline pcr_status check_radius(Real r, const char *who) {
    if (!(r >= 0 && r <= (Real)(sizeof(Real) == 8 ? DBL_MAX : FLT_MAX))) {
        pcr_set_error("invalid argument: %s needs a finite radius >= 0", who);
        return PCR_ERR_INVALID;
    }
    return PCR_OK;
}

// every value of a caller's per-point payload (covariances, normals, intensities, gradients) is finite
template <typename T>
static inline pcr_status check_finite(const T *v, size_t count, const char *what) {
    for (size_t i = 0; i < count; ++i)
        if (!isfinite(v[i])) { pcr_set_error("invalid argument: %s must be finite", what); return PCR_ERR_INVALID; }
    return PCR_OK;
}

// ---- copy-back ----------------------------------------------------------------------------------------------------------
// n uint32 values of the device array d into out as int64; synchronises the context's stream
static inline pcr_status download_u32_as_i64(pcr_context *ctx, const uint32_t *d, size_t n, int64_t *out) {
    std::vector<uint32_t> v(n);
    HIP_TRY(hipMemcpyAsync(v.data(), d, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) out[i] = (int64_t)v[i];
    return PCR_OK;
}
