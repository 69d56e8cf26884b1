// What RANSAC's hypotheses (ransac.hip: k_ransac_fit) and FGR's tuple test (fgr.hip: k_fgr_tuples) share: the counter-based
// sample of three rows and the edge-length rule, as include/pcr.h writes them.  Float64 over the widened float32 points, no
// contraction (the units are built with -ffp-contract=off).
#pragma once

#include <stdint.h>

// ---- sampling ---------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t rs_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ void rs_sample(uint64_t s, uint64_t h, uint64_t m, uint32_t &c0, uint32_t &c1, uint32_t &c2) {
    uint64_t a0 = __umul64hi(rs_mix(s ^ (4 * h + 0)), m);
    uint64_t a1 = __umul64hi(rs_mix(s ^ (4 * h + 1)), m - 1);
    uint64_t a2 = __umul64hi(rs_mix(s ^ (4 * h + 2)), m - 2);
    a1 += (a1 >= a0);
    const uint64_t lo = a0 < a1 ? a0 : a1, hi = a0 < a1 ? a1 : a0;
    a2 += (a2 >= lo);
    a2 += (a2 >= hi);
    c0 = (uint32_t)a0; c1 = (uint32_t)a1; c2 = (uint32_t)a2;
}

// ---- points and edges -------------------------------------------------------------------------------------------------------
struct RsV3 { double x, y, z; };
__device__ __forceinline__ RsV3 rs_ld(const float *__restrict__ a, uint32_t r) {
    return RsV3{(double)a[3 * (size_t)r], (double)a[3 * (size_t)r + 1], (double)a[3 * (size_t)r + 2]};
}
__device__ __forceinline__ RsV3 rs_sub(RsV3 a, RsV3 b) { return RsV3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double rs_dot(RsV3 a, RsV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ RsV3 rs_cross(RsV3 a, RsV3 b) { return RsV3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

__device__ __forceinline__ bool rs_edge_ok(RsV3 pi, RsV3 pj, RsV3 qi, RsV3 qj, double sim2, double e2min) {
    const RsV3 dp = rs_sub(pi, pj), dq = rs_sub(qi, qj);
    const double a2 = rs_dot(dp, dp), b2 = rs_dot(dq, dq);
    return a2 >= sim2 * b2 && b2 >= sim2 * a2 && a2 >= e2min && b2 >= e2min;
}

// |e1|^2 > 0 and |e1 x e2|^2 > 0: the triangle (p0, p1, p2) spans a plane
__device__ __forceinline__ bool rs_triangle_ok(RsV3 p0, RsV3 p1, RsV3 p2) {
    const RsV3 e1 = rs_sub(p1, p0), w = rs_cross(e1, rs_sub(p2, p0));
    return rs_dot(e1, e1) > 0.0 && rs_dot(w, w) > 0.0;
}
