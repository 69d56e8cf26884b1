// Hot-path kernels: transform -> exact NN -> gate -> residual/Jacobian -> 6x6 normal equations -> (in
// pcr_align) the Gauss-Newton step itself.
//
// One calc_H_g_e2 of the reference (icp.py:24-57, plane_icp.py:30-69,
// voxelized_plane_icp.py:23-64, ndt.py:24-57) = k_nn_scan + k_reduce_finalize<KIND>, or the one fused kernel
// k_linearize_finalize<KIND> on a small scan  (the unfused folds and the wave-cooperative search of the developer build
// live in kernels_dev.hip).  One iteration of Registration.align (registration.py:89-111) = that + the Gauss-Newton step
// (k_gn_update, or inline in the fused kernel).
//
// This file holds the kernels and, at its end, the launch functions (declared in pass_device.h) that map run-time
// arguments to a kernel instantiation -- the only code that names a kernel template.  The host side of a pass (set-up,
// enqueue, the pcr_run_* loops) is pass.hip.
//
// Data layout in HBM
//   scan      SoA x[], y[], z[] float32, Morton-sorted once per align()  -> 3 coalesced dword
//             streams, 12 B/point, neighbouring lanes are neighbouring points in space;
//             nn_j u32[]: the matched cell-sorted index of every scan point (search -> reduce)
//   target    cell-sorted float4 {x, y, z, orig idx} for the search; cell-sorted 32-byte
//             {point, normal} records for the PlaneICP gather; cell_start u32[ncells+1]; optional
//             halo lists (nn_device.h)   (voxel targets: double4 means, double[3] normals,
//             double[6] inverse covariances; a few MB, L2-resident)
//   output    per-block partial sums [nblocks + 8][32] double, folded in fixed order inside
//             k_reduce_finalize (deterministic: no floating-point atomics anywhere)
//
// Roofline: HBM-bound gather/stream work, no dense contraction -> no MFMA.  Algorithmic bytes
// per scan point: ICP 24, PlaneICP 36, VPlaneICP 36, NDT 48.
//
// Launch: 256-thread blocks (4 waves of 64).  The sorted scan is split into contiguous spans per XCD
// (block b runs on XCD b % 8), so each XCD sweeps one region of space and its private 4 MiB L2 holds
// that region's target cells (see TileIter / nn_tile_loop).  Per-lane accumulators are float64 (H
// entries reach 1e11 at 1e8 points, float32 would lose the 1e-5 parity bar); the 32 sums are folded
// across the wave with a halving butterfly (32 shuffles instead of 32 x 6), then across waves through LDS.
#include <type_traits>

#include "pass_device.h"
#ifdef PCR_DEV
#include "nn_mfma.h"      // (round 5: the MFMA-filtered search, measured slower than k_nn_scan at every pose: developer build only)
#endif

// ---- certified reuse of the previous pass' matches ------------------------------------------------
// Registration.align (registration.py:89-111) repeats the full search every iteration although the converged
// tail moves the scan by millimetres.  Between two passes over the same scan and target:
//   * the previous pass left, per scan point, its exact nearest neighbour x1 (nn_j) and lb2 <= |q - y| for every
//     other target point y, q being the point under the previous pose (a tracking search: nn_point<TRACK>);
//   * under the new pose the point sits at q', m = |q' - q| away, so |q' - y| >= lb2 - m for every y != x1
//     (triangle inequality);  if |q' - x1| < lb2 - m, x1 is still the strict, unique nearest neighbour --
//     exactly what a fresh search would return -- and lb2 - m is the new bound;
//   * a point that had nothing inside the search bound keeps that state while lb2 - m stays above the gate.
// k_certify evaluates this for every point (one gather of the old match, no search), writes the new bounds and
// a bit mask of the points it could NOT certify; k_nn_scan<LIST> then searches only those, compacted so that the
// lanes of a wave stay dense; the reduce kernel is the one of every other pass, so the sums are bit-identical to
// a pass that searched everything.  Everything is float32 arithmetic on the float32 positions the search itself
// uses; the relative slacks (1e-5) cover the rounding of the distances (~1e-7) many times over.
template <int VOXEL>
__global__ void __launch_bounds__(256) k_certify(const LinArgs a) {
    PoseK P;
    PoseQ Q;
    if (!load_pose<false>(a, P)) return;
    load_prev(a, Q);
    const TileIter it(a);
    const int lane = threadIdx.x & 63;
    uint32_t marked = 0;
    for (int64_t i0 = it.base - threadIdx.x; i0 < it.end; i0 += it.stride) {
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < it.end;
        bool cert = false;
        if (live) {
            const uint32_t j = a.nn_j[i];
            const float lb = a.lb2[i];
            const float x = a.sx[i], y = a.sy[i], z = a.sz[i];
            float tx, ty, tz, ux, uy, uz;
            xform(P, x, y, z, tx, ty, tz);
            xform(Q, x, y, z, ux, uy, uz);
            const float m = __builtin_sqrtf(dist2_f32(tx - ux, ty - uy, tz - uz)) * 1.00001f;
            const float lbn = (lb - m) * 0.999999f;
            if (j != PCR_NONE) {
                float d1;
                if (!VOXEL) {
                    const PtF q = a.pts[j];
                    d1 = __builtin_sqrtf(dist2_f32(tx - q.x, ty - q.y, tz - q.z));
                } else {
                    const PtD q = a.means[j];
                    const double dx = (double)tx - q.x, dy = (double)ty - q.y, dz = (double)tz - q.z;
                    d1 = (float)__builtin_sqrt((dx * dx + dy * dy) + dz * dz);
                }
                cert = d1 * 1.00002f < lbn;
            } else {
                cert = lbn > a.md_f * 1.00001f;            // still nothing inside the gate
            }
            if (cert) a.lb2[i] = lbn;
        }
        const unsigned long long mask = __ballot(live && !cert);
        const int64_t w0 = i0 + (threadIdx.x & ~63);          // first point of this wave's tile
        if (lane == 0 && w0 < it.end) a.umask[w0 >> 6] = mask;
        marked += (uint32_t)__popcll(mask);
    }
    __shared__ uint32_t blk_marked;
    if (threadIdx.x == 0) blk_marked = 0;
    __syncthreads();
    if (lane == 0) atomicAdd(&blk_marked, marked);
    __syncthreads();
    if (threadIdx.x == 0) a.ucnt[blockIdx.x] = blk_marked;
}

// A chunk of a LIST pass: PCR_LIST_CHUNK consecutive scan points = 16 mask words, handed to a BLOCK.  Wave 0 expands
// the set bits into a list in LDS (lane l takes 16 bits: word l >> 2, quarter l & 3); the block's four waves then
// search the listed points 64 at a time, round-robin -- the lanes stay dense however few points k_certify left
// over, and a chunk with everything marked still runs four rounds per wave, like a full search.
// (First version: one wave per chunk, 16 rounds in sequence -- 4.6x slower than the full search when nothing
// certified.)
template <int VOXEL, int HALO>
__device__ __forceinline__ void nn_chunk_list(const LinArgs &a, const PoseK &P, const PoseQ &Q, uint16_t *lst, uint32_t *lst_n,
                                              int64_t first, int64_t end) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        const int64_t w = (first >> 6) + (lane >> 2);
        const int64_t nwords = (a.n + 63) >> 6;
        unsigned long long word = 0;
        if (w < nwords && (w << 6) < end) word = a.umask[w];
        uint32_t bits = (uint32_t)(word >> (16 * (lane & 3))) & 0xffffu;
        const uint32_t cnt = (uint32_t)__popc(bits);
        uint32_t incl = cnt;                                        // inclusive prefix sum over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) *lst_n = incl;
        uint32_t pos = incl - cnt;
        while (bits) {
            const uint32_t b = (uint32_t)__builtin_ctz(bits);
            lst[pos++] = (uint16_t)((lane << 4) | b);
            bits &= bits - 1;
        }
    }
    __syncthreads();
    const uint32_t total = *lst_n;
    for (uint32_t e = threadIdx.x; e < total; e += 256) nn_point<VOXEL, HALO, 1>(a, a.gf, P, Q, first + (int64_t)lst[e]);
    __syncthreads();                                                // (the list is rewritten by the next chunk)
}

// block-level hand-out of the chunks of a LIST pass: the XCD's span of the scan is dealt to the XCD's blocks through
// one counter per XCD sub-span (same counters and the same sub-spans as nn_tile_loop; a block asks once per 1024
// points, so the atomics do not matter here)
template <typename Body>
__device__ __forceinline__ void nn_chunk_loop(const LinArgs &a, Body &&body) {
    const int xcd = (int)(blockIdx.x & 7);
    const uint32_t xb = blockIdx.x >> 3;
    const int64_t gspan = (((a.n + PCR_TILE_CTRS - 1) / PCR_TILE_CTRS) + (PCR_LIST_CHUNK - 1)) & ~(int64_t)(PCR_LIST_CHUNK - 1);
    __shared__ uint32_t chunk_t;
    for (int r = 0; r < PCR_TILE_SUB; ++r) {
        const int c = xcd + 8 * (int)((xb + r) % PCR_TILE_SUB);
        const int64_t lo = gspan * c;
        const int64_t end = lo + gspan < a.n ? lo + gspan : a.n;
        for (;;) {
            if (threadIdx.x == 0) chunk_t = atomicAdd(&a.tile_ctr[c * PCR_TILE_STRIDE], 1u);
            __syncthreads();
            const int64_t first = lo + (int64_t)chunk_t * PCR_LIST_CHUNK;
            __syncthreads();
            if (first >= end) break;
            body(first, first + PCR_LIST_CHUNK < end ? first + PCR_LIST_CHUNK : end);
        }
    }
}

// MODE: PCR_NN_FULL / PCR_NN_TRACK / PCR_NN_LIST
// VOXEL: 0 point target (float32 search), 1 centroid search with the plain row loop, 2 centroid search that takes the rows
// of a ring from the row-occupancy bitmap -- chosen per launch when the gate spans >= 5 rings of the centroid grid
// (vplane_10m: 0.5 m voxels, 2 m gate; ndt_10m with 1 m voxels keeps the row loop, which is faster there).
// (the float32 search needs < 80 VGPRs: 6 waves per SIMD.  The float64 centroid search with the row-occupancy
// bitmap wants ~110: bounded to 5 waves it spills 92 bytes per lane; at 4 waves it is the fastest form measured --
// nn time over the trajectory, base / bitmap from ring 2 at 5 waves / the same at 4 waves / bitmap from ring 1 at 4 waves:
// vplane_10m 7105 / 6538 / 6104 / 5978 us, ndt_10m 3777 / 4299 / 3982 / 3903 us)
#ifndef PCR_VOX_WAVES
#define PCR_VOX_WAVES 4
#endif
template <int VOXEL, int HALO, int LOCAL, int MODE, int LB = PCR_RANGE_PLAIN>
__global__ void __launch_bounds__(256, VOXEL == 2 ? PCR_VOX_WAVES : (LB == PCR_RANGE_BOXES ? 4 : 5)) k_nn_scan(const LinArgs a) {       // LB: see nn_point
    PoseK P;
    PoseQ Q;
    if (!load_pose<false>(a, P)) return;
    if (MODE != PCR_NN_FULL) load_prev(a, Q);
    if (MODE == PCR_NN_LIST) {
        __shared__ uint16_t lst[PCR_LIST_CHUNK];
        __shared__ uint32_t lst_n;
        nn_chunk_loop(a, [&](int64_t first, int64_t end) { nn_chunk_list<VOXEL, HALO>(a, P, Q, lst, &lst_n, first, end); });
    } else {
        // (the device-resident loop: the list set of this iteration was decided by k_gn_update.  Round 6: also under LOCAL == 1 --
        // since round 5's chunk interleave made the block-local hand-out the policy of every mid-size scan, the loop's searches
        // ran as LOCAL == 1 launches and read the FIRST list set at every iteration; select_lists is a no-op for host-driven passes)
        const Geom<float> gsel = (!VOXEL && HALO && LOCAL != 0 && MODE == PCR_NN_FULL) ? select_lists(a) : a.gf;
        auto body = [&](int64_t first, int64_t end) {
            const int64_t i = first + (threadIdx.x & 63);
            if (i < end) nn_point<VOXEL, HALO, MODE == PCR_NN_TRACK, LB>(a, gsel, P, Q, i);
        };
        if (LOCAL == 2) {       // device-resident loop: k_gn_update decided from the size of its step (PoseDev::tile_local)
            if (__builtin_amdgcn_readfirstlane(a.pose->tile_local)) nn_tile_loop<1, 64>(a, body);
            else nn_tile_loop<0, 64>(a, body);
        } else {
            nn_tile_loop<LOCAL, 64>(a, body);
        }
    }
}

#ifdef PCR_DEV
// Plain pass over a POINT target at a far pose: wave-cooperative search with an MFMA distance filter (nn_mfma.h); same
// matches as k_nn_scan<0, HALO, LOCAL, PCR_NN_FULL>, bit for bit
__global__ void __launch_bounds__(256) k_nn_bound(const LinArgs a) {
    PoseK P;
    if (!load_pose<false>(a, P)) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) nn_mfma_bound(a, a.gf, P, i);
}
template <int HALO, int LOCAL>
__global__ void __launch_bounds__(256, 4) k_nn_mfma(const LinArgs a) {
    PoseK P;
    if (!load_pose<false>(a, P)) return;
    __shared__ uint32_t cidx_all[4][PCR_MF_MAXC];
    __shared__ uint32_t defer_all[4][64];
    MfWave w;
    w.cidx = cidx_all[threadIdx.x >> 6]; w.defer = defer_all[threadIdx.x >> 6]; w.ndefer = 0;
    auto body = [&](int64_t first, int64_t end) { nn_tile_mfma<HALO, 1>(a, a.gf, P, w, a.pts_last, first, end); };
    nn_tile_loop<LOCAL, 64>(a, body);
    if (w.ndefer > 0) nn_mfma_flush<HALO>(a, a.gf, P, w);
}
#ifdef PCR_MF_STATS
extern "C" __attribute__((visibility("default"))) int pcr_mf_stats_read(unsigned long long out[16], int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mf_stats), 16 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_mf_stats), z, sizeof z) != hipSuccess) return 1; }
    return 0;
}
#endif
#endif

// Plain pass over a voxel target that has a float32 filter index (pass_device.h: nn_point_filter)
// (Two-way settling inside this kernel -- nn_point_filter<HALO, 1>: the search also tracks the runner-up and a third bound,
// +8 VALU operations per candidate -- was measured on both 10 M configs in round 4: search 570 -> 640 us and 380 -> 429 us per
// pass, more than the pending points cost anywhere.  The fused small-scan kernel, where one extra search chain doubles the
// longest wave, does use it.)
// Q6 (round 5): the same kernel in front of the float64 coordinates of a float64 POINT target (pass_device.h: nn_filter_core)
template <int HALO, int LOCAL, int Q6 = 0>
__global__ void __launch_bounds__(256, 5) k_nn_filter(const LinArgs a) {
    PoseK P;
    if (!load_pose<false>(a, P)) return;
    auto body = [&](int64_t first, int64_t end) {
        const int64_t i = first + (threadIdx.x & 63);
        if (i < end) nn_point_filter<HALO, 0, Q6>(a, P, i);
    };
    nn_tile_loop<LOCAL, 64>(a, body);
}
#ifdef PCR_DEV
// ... and the float64 search of what it could not certify as a launch of its own (round 3; now only in front of the
// unfused developer reduce kernels); returns at once when no lane of this pass asked
__global__ void __launch_bounds__(256) k_nn_fix(const LinArgs a) {
    PoseK P;
    if (!load_pose<false>(a, P)) return;
    if (__builtin_amdgcn_readfirstlane(*(volatile const uint32_t *)a.pending) != a.stamp) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const uint32_t j = a.nn_j[i];
        if (nn_is_pending(j)) nn_point_fix(a, P, i, j & ~PCR_PENDING_BIT);
    }
}
#endif

// The ONE writer of a pose in HBM: T and the copies the kernels read (float64 rotation for the Jacobians, float32 rotation /
// translation for the point transform).  Batched and single results are bit-identical because every pose goes through here
// (and through host_pose_k of pass_device.h, which rounds alike).
__device__ __forceinline__ void pose_write(PoseDev *p, const double *T) {
    for (int i = 0; i < 16; ++i) p->T[i] = T[i];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) { p->R[3 * i + j] = T[4 * i + j]; p->r32[3 * i + j] = (float)T[4 * i + j]; }
        p->t32[i] = (float)T[4 * i + 3];
    }
}
// ... and the start of a device-resident loop: the pose and the loop words
__device__ __forceinline__ void pose_arm(PoseDev *p, const double *T, int max_iter) {
    pose_write(p, T);
    p->iter = 0;
    p->done = max_iter > 0 ? PCR_LOOP_RUNNING : PCR_LOOP_MAXITER;
    p->tile_local = 0;
    p->halo_deep = PCR_DEEP_SETS;   // the first pass knows nothing about its distance to the target: the deepest lists there are
}

// The O(1) tail of an iteration on the device (ONE thread): record the trace row, dx = -solve(H, g),
// |dx| < tol test, T <- plus(T, dx), derived float32 / rotation copies for the next pass, progress
// words for the host.  out29 is complete and visible to this thread.
__device__ __forceinline__ void gn_update(const FinArgs &f, double (*A)[7]) {
    PoseDev *p = f.pose;
    const int it = p->iter;
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = p->T[i];
    if (f.trace) {
        double *row = f.trace + (size_t)it * 45;
        for (int i = 0; i < 16; ++i) row[i] = T[i];
        for (int i = 0; i < 29; ++i) row[16 + i] = f.out[i];
    }
    double T_old[16];
    for (int i = 0; i < 16; ++i) T_old[i] = T[i];
    const int r = gn_step(A, f.out, f.tol, T);
    // hand-out policy of the next search (see pass_enqueue): block-local once the scan moves by less than local_len
    const double moved = r == 0 ? gn_typical_motion(T_old, T, f.bb_c, f.bb_e) : 0.0;
    p->tile_local = (r == 0 && f.local_len > 0.0 && moved < f.local_len) ? 1 : 0;
    p->halo_deep = (r != 0 || moved >= f.out_len) ? 0 : (moved >= f.far_len ? 2 : (moved >= f.deep_len ? 1 : 0));
    int done = r == 2 ? PCR_LOOP_SINGULAR : (r == 1 ? PCR_LOOP_CONVERGED : PCR_LOOP_RUNNING);
    if (r == 0) pose_write(p, T);
    const int it1 = it + 1;
    if (done == PCR_LOOP_RUNNING && it1 >= f.max_iter) done = PCR_LOOP_MAXITER;
    p->iter = it1;
    p->done = done;
    if (f.host_T) {
        // progress word every iteration (the host keeps the queue two iterations ahead of it); the pose
        // itself crosses PCIe only once, with the final state
        if (done != PCR_LOOP_RUNNING) {
            for (int i = 0; i < 16; ++i) f.host_T[i] = T[i];
            __threadfence_system();
        }
        *f.host_state = ((unsigned long long)(unsigned)done << 32) | (unsigned)it1;
    }
}

// the step of the device-resident loop: a 1-wave launch behind the fold (single GPU) or behind the
// all-reduce of the 29 sums (multi-GPU: every rank computes the same update)
__global__ void __launch_bounds__(64) k_gn_update(const FinArgs f) {
    if (threadIdx.x != 0) return;
    if (f.pose->done == PCR_LOOP_RUNNING) {
        double A[6][7];                 // registers: gn_solve6 indexes it with compile-time constants only
        gn_update(f, A);
    } else if (f.pose->done == PCR_LOOP_COMMFAIL && f.host_state) {
        // the exchange in front of this launch gave up waiting for a peer: tell the host, which is watching this word
        *f.host_state = ((unsigned long long)(unsigned)PCR_LOOP_COMMFAIL << 32) | (unsigned)f.pose->iter;
    }
}

// start of pcr_align: the initial pose into HBM (kernel arguments: no host-to-device copy)
struct PoseInit { double T[16]; };
__global__ void __launch_bounds__(64) k_pose_init(PoseDev *p, const PoseInit init, int max_iter) {
    if (threadIdx.x != 0) return;
    pose_arm(p, init.T, max_iter);
}

// The pending points of a filter pass (1-2 per 1000) inside the range of scan points this thread is about to reduce.
// Searched one by one as they turn up, a wave runs one float64 search chain (~20 dependent round trips) per loop
// iteration in which ANY of its lanes has a pending point -- 3-4 chains in sequence per wave on vplane_10m, as long as the
// separate k_nn_fix launch took (measured: reduce 64 -> 144 us).  So the wave first COLLECTS its pending points in a
// small list in LDS (ballot + prefix count, no atomics) and searches them 64 at a time: one chain per wave in the
// ordinary case, dense waves when everything is pending (duplicated centroids).
__device__ __forceinline__ void fix_pending(const LinArgs &a, const PoseK &P, const TileIter &it) {
    __shared__ uint32_t fix_list[4][128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *lst = fix_list[wave];
    const int64_t base0 = it.base - threadIdx.x;               // first point of this block's first tile
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0;                                                // wave-uniform
    // FIX_UNROLL words of nn_j are requested before the first is looked at: one word per round trip made the walk itself a
    // chain of ~38 dependent loads per wave (10 M points over 1024 blocks), 55-60 us -- as long as the searches it feeds
    constexpr int FIX_UNROLL = 8;
    for (int64_t i0 = base0;; i0 += FIX_UNROLL * it.stride) {
        const bool more = i0 < it.end;                          // block-uniform
        if (more) {
            uint32_t jv[FIX_UNROLL];
#pragma unroll
            for (int u = 0; u < FIX_UNROLL; ++u) {
                const int64_t i = i0 + (int64_t)u * it.stride + threadIdx.x;
                jv[u] = i < it.end ? a.nn_j[i] : PCR_NONE;
            }
#pragma unroll
            for (int u = 0; u < FIX_UNROLL; ++u) {
                const bool pend = nn_is_pending(jv[u]);
                const unsigned long long m = __ballot(pend);
                if (m == 0) continue;
                if (pend) lst[cnt + __popcll(m & below)] = (uint32_t)(i0 + (int64_t)u * it.stride + threadIdx.x - base0);
                cnt += __popcll(m);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (cnt >= 64) {                                // a full wave of pending points: search them now
                    const int64_t ip = base0 + (int64_t)lst[lane];
#ifdef PCR_DEV
                    if (a.flags & (1u << 28)) a.nn_j[ip] &= ~PCR_PENDING_BIT;      // (PCR_FIX_DEBUG=1, timing only: the walk without the searches)
                    else
#endif
                    nn_point_fix(a, P, ip, a.nn_j[ip] & ~PCR_PENDING_BIT);
                    const uint32_t carry = lane + 64 < cnt ? lst[lane + 64] : 0u;
                    __builtin_amdgcn_wave_barrier();
                    lst[lane] = carry;
                    cnt -= 64;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            continue;
        }
        // the end of the range: what is still listed (fewer than 64)
        if (lane < cnt) {
            const int64_t ip = base0 + (int64_t)lst[lane];
#ifdef PCR_DEV
            if (a.flags & (1u << 28)) a.nn_j[ip] &= ~PCR_PENDING_BIT;
            else
#endif
            nn_point_fix(a, P, ip, a.nn_j[ip] & ~PCR_PENDING_BIT);
        }
        // (the words rewritten above are read back by OTHER lanes of this wave in reduce_stream -- same-wave global
        // store -> load ordering holds on gfx950, but say so to the compiler and the memory model explicitly)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        break;
    }
}

// k_reduce with the fold inside (the shipped reduce kernel)
// FIX (behind k_nn_filter): every thread first walks the scan points it is about to reduce and runs the float64 search
// for those the filter left PCR_PENDING (1-2 per 1000), rewriting nn_j; then it streams as usual.  Round 3 did this in a
// launch of its own (k_nn_fix: 40-65 us -- the latency of one float64 search chain with the rest of the chip idle, plus
// a 40 MB read of nn_j); here the chains of the few waves that have one overlap with the streaming of all the others,
// and the search's registers are dead before the 32 accumulators come alive.  The order of the sums is unchanged.
template <int KIND, int FIX>
// (FIX and the point kinds stay at <= 128 VGPRs: the 4 blocks per CU of the reduce grid are then one resident generation)
__global__ void __launch_bounds__(256, (FIX || KIND == PCR_ICP || KIND == PCR_PLANE) ? 4 : 1) k_reduce_finalize(const LinArgs a, const FinArgs f) {
    PoseK P;
    if (!load_pose<true>(a, P)) return;
    const TileIter it(a);
    if (FIX && KIND != PCR_ICP) {              // (PLANE: the float64 search of a float64 point target, quirk Q6)
        if ((uint32_t)__builtin_amdgcn_readfirstlane((int)*(volatile const uint32_t *)a.pending) == a.stamp)
            fix_pending(a, P, it);
    }
    double acc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) acc[i] = 0.0;
    // (<PLANE, FIX>, quirk Q6: one point less per trip -- five points' loads beside the sums do not fit its 128 registers
    // without scratch; the order of the sums does not depend on W)
    reduce_stream<KIND, (FIX && KIND == PCR_PLANE) ? PCR_RED_W - 1 : PCR_RED_W>(acc, a, P, it.base, it.end, it.stride);
    (void)ticket_fold_emit(acc, a, f);
    // (the Gauss-Newton step is NOT inlined here: its straight-line float64 code needs 136 VGPRs, which
    // would cap this streaming kernel at 3 blocks per CU; k_gn_update runs it as a 1-wave launch)
}

// GN (device-resident loop on one GPU): the block that emits also takes the Gauss-Newton step.  This kernel runs one
// tile per wave at 129-191 VGPRs anyway, so -- unlike in the streaming reduce kernel -- the step's registers cost no
// occupancy, and the iteration saves the k_gn_update launch (~8 us of a 46 us iteration on a 100 k-point scan).  Every
// other block read the pose before it contributed its ticket, so rewriting it here races with nothing.
template <int KIND, int HALO, int GN, int FILT, int LB = 0>
__global__ void __launch_bounds__(256) k_linearize_finalize(const LinArgs a, const FinArgs f) {
    PoseK P;
    if (!load_pose<true>(a, P)) return;
    double acc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) acc[i] = 0.0;
    linearize_body<KIND, HALO, FILT, LB>(a, P, acc);
    const bool last = ticket_fold_emit(acc, a, f);
    if (GN && last && threadIdx.x == 0 && f.pose->done == PCR_LOOP_RUNNING) {
        double A[6][7];
        gn_update(f, A);
    }
}

// The batched form of k_linearize_finalize (pcr_linearize_batch / pcr_align_batch): blockIdx.y = item of the batch,
// blockIdx.x = block within the item.  A 100 k-point scan fills a fraction of the chip with waves that wait on dependent cold
// misses; K such scans against ONE target are K times the waves in flight in one launch instead of K launches.  An instantiation
// of its own over the shared device functions (no run-time branch in the single-scan kernels): per item the scan slice, n,
// nblocks, rows, tickets, pose, sums and trace rows come from the item's descriptor, so TileIter, ticket_fold_emit and
// gn_update see exactly the arguments a single launch over that scan gives them -- every item's sums, trace rows and poses
// are bit-identical to the single path's.  GN = 1: the device-resident loop (pose from the item's PoseDev, step inline);
// GN = 0: a plain pass at the descriptor's pose.
template <int KIND, int HALO, int GN, int FILT, int LB = 0>
__global__ void __launch_bounds__(256) k_linearize_batch(const LinArgs a0, const FinArgs f0, const BatchItem *__restrict__ items) {
    const BatchItem *d = items + blockIdx.y;
    const int nblocks = __builtin_amdgcn_readfirstlane(d->nblocks);
    if ((int)blockIdx.x >= nblocks) return;
    LinArgs a = a0;
    FinArgs f = f0;
    a.sx = uniform_ptr(d->sx); a.sy = uniform_ptr(d->sy); a.sz = uniform_ptr(d->sz);
    {
        const long long n = (long long)d->n;
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)n);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)n >> 32));
        a.n = (int64_t)(((unsigned long long)hi << 32) | lo);
    }
    a.nblocks = nblocks; f.nblocks = nblocks;
    a.partials = uniform_ptr(d->partials); f.partials = a.partials;
    f.tickets = uniform_ptr(d->tickets);
    f.out = uniform_ptr(d->out);
    PoseK P;
    if (GN) {
        PoseDev *pose = uniform_ptr(d->pose);
        a.pose = pose; f.pose = pose;
        if (!load_pose<true>(a, P)) return;
    } else {
        a.pose = nullptr; f.pose = nullptr;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double v = uniform_f64(d->T[4 * i + j]);
                P.R[3 * i + j] = v; P.r32[3 * i + j] = (float)v; f.R[3 * i + j] = v;
            }
            P.t32[i] = (float)uniform_f64(d->T[4 * i + 3]);
        }
    }
    double acc[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) acc[i] = 0.0;
    linearize_body<KIND, HALO, FILT, LB>(a, P, acc);
    const bool last = ticket_fold_emit(acc, a, f);
    if (GN && last && threadIdx.x == 0 && f.pose->done == PCR_LOOP_RUNNING) {
        // (what only the step reads is fetched here, by the one thread that takes it)
        f.trace = d->trace; f.host_T = d->host_T; f.host_state = d->host_state;
        for (int i = 0; i < 3; ++i) { f.bb_c[i] = d->bb_c[i]; f.bb_e[i] = d->bb_e[i]; }
        double A[6][7];
        gn_update(f, A);
    }
}

// start of a batched call, one wave per item: the item's tickets and trace rows zeroed (the block they live in comes from the
// context's cache), its start pose into its PoseDev (kernel boundary in front of the first pass: no host-to-device copy of
// state beyond the descriptors)
__global__ void __launch_bounds__(64) k_batch_init(const BatchItem *__restrict__ items, int max_iter) {
    const BatchItem &d = items[blockIdx.x];
    for (int i = threadIdx.x; i < 9 * PCR_TICKET_STRIDE; i += 64) d.tickets[i] = 0u;
    if (d.trace) for (size_t i = threadIdx.x; i < (size_t)max_iter * 45; i += 64) d.trace[i] = 0.0;
    PoseDev *p = d.pose;
    if (threadIdx.x != 0 || p == nullptr) return;
    pose_arm(p, d.T, max_iter);
}

// after the RCCL all-reduce: hand the 29 doubles to the host the same zero-copy way k_finalize does
__global__ void __launch_bounds__(64) k_publish(const double *__restrict__ out, double *host_out,
                                                volatile uint32_t *host_flag, uint32_t seq) {
    if (threadIdx.x < 29) host_out[threadIdx.x] = out[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) *host_flag = seq;
}

// ---- fine seam: plain NN queries (no transform), original indices out -------------------------
template <typename Real, typename PT, bool HALO, int LB = PCR_RANGE_PLAIN>
__global__ void __launch_bounds__(256) k_nn_query(Geom<Real> g, const PT *pts, const uint32_t *cs,
                                                  const float *q, int64_t m, Real bound2, Real rmax,
                                                  Real *dist, int64_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    Real best; uint32_t bj, bo;
    nn_search<Real, PT, false, false, HALO, 0, false, PCR_NN_BATCH, LB>(g, pts, cs, (Real)q[3 * i], (Real)q[3 * i + 1], (Real)q[3 * i + 2], bound2, best, bj, bo);
    bj = bo;                                       // (only tested against PCR_NONE below)
    Real d = RealTraits<Real>::sqrt_rn(best);
    if (bj != PCR_NONE && rmax < RealTraits<Real>::inf() && !(d < rmax)) bj = PCR_NONE;
    dist[i] = bj == PCR_NONE ? RealTraits<Real>::inf() : d;
    idx[i] = bj == PCR_NONE ? (int64_t)-1 : (int64_t)bo;
}

// KDTree(float64 data).query (kdtree.py:18-21; quirk Q6): the float32 search over the index nominates, the float64 box search
// through the nominee (nn_box_f64: every point whose float64 position can lie inside that ball) decides by (float64
// distance, original index).  The fine seam: no certification shortcut, every query runs both.
template <bool HALO>
__global__ void __launch_bounds__(256) k_nn_query_q6(Geom<float> gf, const PtF *pts, const uint32_t *cs, Geom<double> gq, const PtD *pts64,
                                                     const float *q, int64_t m, float bound2_f, double rmax, double *dist, int64_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
    float best; uint32_t bj, bo;
    nn_search<float, PtF, false, false, HALO>(gf, pts, cs, qx, qy, qz, bound2_f, best, bj, bo);
    double bd = __longlong_as_double(0x7ff0000000000000LL);
    if (bo != PCR_NONE) nn_box_f64(gq, pts64, cs, (double)qx, (double)qy, (double)qz, bj, bd, bj, bo);
    const double d = __builtin_sqrt(bd);
    if (bo != PCR_NONE && !(d < rmax)) bo = PCR_NONE;
    dist[i] = bo == PCR_NONE ? __longlong_as_double(0x7ff0000000000000LL) : d;
    idx[i] = bo == PCR_NONE ? (int64_t)-1 : (int64_t)bo;
}

// =============================================================================================
// launch functions: run-time arguments -> kernel instantiation (declared in pass_device.h, called from pass.hip)
// =============================================================================================
static const dim3 kBlock(256);
// how the plain float32 search scans the ranges of this point target (nn_device.h)
static int range_mode(const Geom<float> &g) { return g.lbox != nullptr ? PCR_RANGE_BOXES : (g.xq > 0.f ? PCR_RANGE_XORDER : PCR_RANGE_PLAIN); }

void launch_certify(bool voxel, dim3 grid, hipStream_t st, const LinArgs &a) {
    with_const<2>(voxel, [&](auto V) { hipLaunchKernelGGL(k_certify<V()>, grid, kBlock, 0, st, a); });
}

// voxel: the VOXEL argument of k_nn_scan (0 / 1 / 2); local: 0 global counters, 1 block-local, 2 decided on the device -- plain
// searches of the device-resident loop only (a tracking search takes 2 as 1, a LIST pass deals chunks and ignores it)
void launch_nn_scan(int voxel, int mode, bool halo, int local, dim3 grid, hipStream_t st, const LinArgs &a) {
    const int l = mode == PCR_NN_LIST ? 0 : (mode == PCR_NN_FULL && local == 2) ? 2 : local != 0;
    // (LB: plain full searches of a point target with heavy cells, Geom::lbox, or with the x order, Geom::xq)
    const int lb = voxel == 0 && mode == PCR_NN_FULL ? range_mode(a.gf) : PCR_RANGE_PLAIN;
    with_const<3>(voxel, [&](auto V) {
        with_const<3>(mode, [&](auto M) {
            with_const<2>(halo && voxel == 0, [&](auto H) {
                with_const<3>(l, [&](auto L) {
                    with_const<3>(lb, [&](auto B) {
                        // lists and leaf boxes: point targets only; LB: full searches only.  (LOCAL == 2 exists for tracking and
                        // LIST searches too, as it always has, although `l` above never selects it: the set of kernels is
                        // held fixed here)
                        if constexpr (!(V() != 0 && (H() || B())) && !(M() != PCR_NN_FULL && B()))
                            hipLaunchKernelGGL((k_nn_scan<V(), H(), L(), M(), B()>), grid, kBlock, 0, st, a);
                    });
                });
            });
        });
    });
}

void launch_nn_filter(bool halo, int local, bool separate_fix, bool q6, dim3 grid, hipStream_t st, const LinArgs &a) {
    // (local == 2, "decided on the device from the size of the step", is not instantiated here: both tile loops in one
    // kernel around the tracking search spill 736 bytes per lane; the device-resident loop keeps the global counters)
    with_const<2>(halo, [&](auto H) {
        with_const<2>(local == 1, [&](auto L) {
            with_const<2>(q6, [&](auto Q) { hipLaunchKernelGGL((k_nn_filter<H(), L(), Q()>), grid, kBlock, 0, st, a); });
        });
    });
    // the float64 search of the pending points: the prologue of k_reduce_finalize<KIND, 1> (round 4); a launch of its own
    // only in front of the unfused developer reduce kernels
#ifdef PCR_DEV
    if (separate_fix) hipLaunchKernelGGL(k_nn_fix, grid, kBlock, 0, st, a);
#else
    (void)separate_fix;
#endif
}

#ifdef PCR_DEV
void launch_nn_mfma(bool halo, int local, dim3 grid, hipStream_t st, const LinArgs &a) {
    {   // the bounds first: a streaming launch over the scan
        int64_t nb = (a.n + 255) / 256;
        if (nb > 256 * 16) nb = 256 * 16;
        hipLaunchKernelGGL(k_nn_bound, dim3((unsigned)(nb > 0 ? nb : 1)), kBlock, 0, st, a);
    }
    with_const<2>(halo, [&](auto H) {
        with_const<2>(local == 1, [&](auto L) { hipLaunchKernelGGL((k_nn_mfma<H(), L()>), grid, kBlock, 0, st, a); });
    });
}
#endif

// the shipped reduce kernel; fix: behind a filter search (never for ICP, whose target has no float64 side)
void launch_reduce_kind(int kind, bool fix, dim3 grid, hipStream_t st, const LinArgs &a, const FinArgs &f) {
    with_const<4>(kind, [&](auto K) {
        with_const<2>(fix && kind != PCR_ICP, [&](auto X) {
            if constexpr (!(K() == PCR_ICP && X())) hipLaunchKernelGGL((k_reduce_finalize<K(), X()>), grid, kBlock, 0, st, a, f);
        });
    });
}

// The fused kernels, single and batched, over ONE ladder: go(K, HALO, GN, FILT, LB) for the instantiation that `v` names.
// A point target has no filter index; a voxel target has no leaf boxes, and lists only on its filter index.
template <typename F>
static void with_fused_variant(int kind, const FusedVariant &v, F &&go) {
    with_const<4>(kind, [&](auto K) {
        with_const<2>(v.halo, [&](auto H) {
            with_const<2>(v.gn, [&](auto G) {
                with_const<2>(v.filt, [&](auto FL) {
                    with_const<3>(v.lb, [&](auto LB) {
                        constexpr bool point = K() == PCR_ICP || K() == PCR_PLANE;
                        if constexpr (point ? !FL() : (!LB() && (FL() || !H()))) go(K, H, G, FL, LB);
                    });
                });
            });
        });
    });
}
void launch_fused(int kind, const FusedVariant &v, dim3 grid, hipStream_t st, const LinArgs &a, const FinArgs &f) {
    with_fused_variant(kind, v, [&](auto K, auto H, auto G, auto FL, auto LB) {
        hipLaunchKernelGGL((k_linearize_finalize<K(), H(), G(), FL(), LB()>), grid, kBlock, 0, st, a, f);
    });
}
void launch_fused_batch(int kind, const FusedVariant &v, dim3 grid, hipStream_t st, const LinArgs &a, const FinArgs &f,
                        const BatchItem *items) {
    // (the batched kernel has no x-ordered instantiation: it scans the ranges of an x-ordered target plainly, which is exact on
    // any order inside a cell and gives the single launch's matches and sums)
    FusedVariant vb = v;
    if (vb.lb == PCR_RANGE_XORDER) vb.lb = PCR_RANGE_PLAIN;
    with_fused_variant(kind, vb, [&](auto K, auto H, auto G, auto FL, auto LB) {
        if constexpr (LB() != PCR_RANGE_XORDER)
            hipLaunchKernelGGL((k_linearize_batch<K(), H(), G(), FL(), LB()>), grid, kBlock, 0, st, a, f, items);
    });
}

void launch_gn_update(hipStream_t st, const FinArgs &f) { hipLaunchKernelGGL(k_gn_update, dim3(1), dim3(64), 0, st, f); }
void launch_pose_init(hipStream_t st, PoseDev *pose, const double T[16], int max_iter) {
    PoseInit init;
    memcpy(init.T, T, sizeof init.T);
    hipLaunchKernelGGL(k_pose_init, dim3(1), dim3(64), 0, st, pose, init, max_iter);
}
void launch_batch_init(hipStream_t st, const BatchItem *items, unsigned n_items, int max_iter) {
    hipLaunchKernelGGL(k_batch_init, dim3(n_items), dim3(64), 0, st, items, max_iter);
}
void launch_publish(hipStream_t st, const double *out, double *host_out, volatile uint32_t *host_flag, uint32_t seq) {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, out, host_out, host_flag, seq);
}

// form 0: float32 search of a point target; 1: float64 search of a voxel target's centroids; 2: float64 result over a float64
// point target (quirk Q6).  bound2 / rmax are rounded to the search's own type here
void launch_nn_query(const pcr_target *t, int form, hipStream_t st, const float *q, int64_t m, double bound2, double rmax, void *dist,
                     int64_t *idx) {
    const dim3 grid((unsigned)((m + 255) / 256));
    if (form == 0) {
        with_const<2>(t->cs_h != nullptr, [&](auto H) {
            with_const<3>(range_mode(t->gf), [&](auto B) {
                hipLaunchKernelGGL((k_nn_query<float, PtF, H() != 0, B()>), grid, kBlock, 0, st, t->gf, t->pts, t->cell_start, q, m,
                                   (float)bound2, (float)rmax, (float *)dist, idx);
            });
        });
    } else if (form == 2) {
        with_const<2>(t->cs_h != nullptr, [&](auto H) {
            hipLaunchKernelGGL((k_nn_query_q6<H() != 0>), grid, kBlock, 0, st, t->gf, t->pts, t->cell_start, t->gq, t->pts64, q, m,
                               (float)bound2, rmax, (double *)dist, idx);
        });
    } else {
        hipLaunchKernelGGL((k_nn_query<double, PtD, false>), grid, kBlock, 0, st, t->gd, t->means, t->cell_start, q, m, bound2, rmax,
                           (double *)dist, idx);
    }
}

// resident 256-thread blocks per CU of the search kernel a grid is sized by (0: the query failed, the caller has a default)
int nn_blocks_per_cu(int which) {
    int nb = 0;
    hipError_t e = hipErrorInvalidValue;
    switch (which) {
    case PCR_OCC_POINT: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_nn_scan<0, 1, 0, 0>, 256, 0); break;
    case PCR_OCC_VOXEL: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_nn_scan<1, 0, 0, 0>, 256, 0); break;
    case PCR_OCC_FILTER: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_nn_filter<1, 0>, 256, 0); break;
    case PCR_OCC_POINT_LB: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_nn_scan<0, 1, 0, 0, PCR_RANGE_BOXES>, 256, 0); break;
#ifdef PCR_DEV
    case PCR_OCC_MFMA: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_nn_mfma<1, 0>, 256, 0); break;
#endif
    default: break;
    }
    return e == hipSuccess && nb > 0 ? nb : 0;
}
