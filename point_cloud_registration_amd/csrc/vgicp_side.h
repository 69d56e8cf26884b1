// What the two VGICP units share (vgicp.hip: the nearest-centroid pass; vgicp_direct.hip: the direct voxel neighbourhoods,
// a unit derived from it).  VgicpArgs, the target side of a VGICP correspondence: what is gathered of a kept voxel and how
// residual and weight are formed from it -- the scan side and the ONE statement of a correspondence are DistSide's
// (gicp_weight.h).  VgicpUnit, the UNIT of match_pass.h: payloads, the refusals of a pass that runs no search, the kernels of
// vgicp.hip by name.
#pragma once

#include "gicp_weight.h"
#include "match_pass.h"

struct VgicpArgs : DistSide<VgicpArgs> {
    const double *vcov;      // voxel covariances, cell-sorted, 6 doubles per voxel (16-byte aligned rows)
    double *rows;            // [gridDim.x][32]

    // the match: the centroid (32 bytes of `means`, as halves) and the voxel covariance (48 bytes of vcov)
    struct Match { double2 m0, m1, cv[3]; };
    typedef double Res;
    __device__ __forceinline__ void gather(const LinArgs &a, uint32_t j, Match &m) const {
        const double2 *mp = reinterpret_cast<const double2 *>(a.means + j);
        const double2 *cq = reinterpret_cast<const double2 *>(vcov + 6 * (size_t)j);
        m.m0 = mp[0]; m.m1 = mp[1];
        m.cv[0] = cq[0]; m.cv[1] = cq[1]; m.cv[2] = cq[2];
    }
    __device__ __forceinline__ bool residual(const LinArgs &a, const Match &m, float tx, float ty, float tz, double &dx, double &dy, double &dz) const {
        return residual_f64<true>(a, make_double4(m.m0.x, m.m0.y, m.m1.x, m.m1.y), tx, ty, tz, dx, dy, dz);
    }
    __device__ __forceinline__ void weight(const PoseK &P, const float cp[6], const Match &m, double m6[6]) const {
        const double cq[6] = {m.cv[0].x, m.cv[0].y, m.cv[1].x, m.cv[1].y, m.cv[2].x, m.cv[2].y};
        gicp_weight(P, cp, cq, m6);
    }
};

// ---- the UNIT -----------------------------------------------------------------------------------------------------------
// its kernels: vgicp.hip
__global__ void __launch_bounds__(256) k_vgicp_reduce(const LinArgs a, const VgicpArgs va);
__global__ void __launch_bounds__(64) k_vgicp_fold(const double *__restrict__ rows, int nb, double *out);
__global__ void __launch_bounds__(256) k_vgicp_robust(const LinArgs a, const RobustSide<VgicpArgs> va);
__global__ void __launch_bounds__(256) k_vgicp_residuals(const LinArgs a, const VgicpArgs va, const uint32_t *order, double *out);
__global__ void __launch_bounds__(256) k_vgicp_keys(const LinArgs a, const VgicpArgs va, double *out);
__global__ void __launch_bounds__(256) k_vgicp_adaptive(const LinArgs a, const AdaptiveSide<VgicpArgs> va);

// The search is VPlaneICP's, over the centroids; a call has no parameter of the unit's own
struct VgicpUnit : MatchUnit {
    typedef VgicpArgs Side;
    static constexpr int kind = PCR_VPLANE;
    static pcr_status payloads(const pcr_target *t, const pcr_scan *s) {
        if (!t->is_voxel) { pcr_set_error("VGICP needs a voxel target"); return PCR_ERR_NO_TARGET; }
        if (!t->vcov) { pcr_set_error("VGICP target has no covariances (pcr_target_voxels_set_covariances)"); return PCR_ERR_NO_TARGET; }
        if (!s->cov) { pcr_set_error("VGICP scan has no covariances (pcr_scan_estimate_covariances / _set_covariances)"); return PCR_ERR_NO_TARGET; }
        return PCR_OK;
    }
    // what the search refuses of a VGICP call, for a pass that does not get to the search
    static pcr_status refuse_as_search(const pcr_target *t, const pcr_scan *s, double max_dist) {
        PCR_REQUIRE(s->ctx == t->ctx, "scan and target belong to different contexts");
        PCR_REQUIRE(max_dist > 0, "max_dist must be positive");
        if (t->ctx->comm != nullptr) { pcr_set_error("VGICP passes are not available on a context with a communicator attached"); return PCR_ERR_UNSUPPORTED; }
        return PCR_OK;
    }
    // no kept voxel: no match (and no voxel 0 for the select of phase B) -- once what the search refuses has been refused here
    static pcr_status no_match(const pcr_target *t, const pcr_scan *s, double max_dist, bool *none) {
        *none = t->n == 0;
        return *none ? refuse_as_search(t, s, max_dist) : PCR_OK;
    }
    static Side side(const pcr_target *t, const pcr_scan *s, const Params &) { return {{s->cov}, t->vcov, nullptr}; }
    static constexpr auto reduce = k_vgicp_reduce;
    static constexpr auto robust = k_vgicp_robust;
    static constexpr auto fold = k_vgicp_fold;
    static constexpr auto residuals = k_vgicp_residuals;
    static constexpr auto keys = k_vgicp_keys;
    static constexpr auto adaptive = k_vgicp_adaptive;
    static constexpr const char *reduce_range = "pcr:vgicp_reduce", *robust_range = "pcr:vgicp_robust", *residuals_range = "pcr:vgicp_residuals",
                                *adaptive_range = "pcr:vgicp_adaptive";
};
