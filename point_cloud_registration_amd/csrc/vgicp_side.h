// The target side of a VGICP correspondence, shared by the nearest-centroid pass (vgicp.hip) and the direct voxel
// neighbourhoods (vgicp_direct.hip): what is gathered of a kept voxel and how residual and weight are formed from it.  The scan
// side and the ONE statement of a correspondence are DistSide's (gicp_weight.h).
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
