// Index construction (set_target side, once per target / once per align for the scan):
//   - dense cell grid over the target points      (replaces the pykdtree build, icp.py:20,
//     plane_icp.py:22, reference kdtree.py:18-21)
//   - dense cell grid over the kept voxel centroids (replaces KDTree(means), voxel.py:165)
//   - Morton sort of the scan (registration.py:83 casts the scan once per align; here it is
//     also uploaded and ordered once, the per-iteration kernels then stream it)
//
// Sorting and prefix sums use rocPRIM through hipCUB (device-wide radix sort / scan); the
// kernels around them are hand-written.  Everything runs on the context's stream.
#include <hipcub/hipcub.hpp>
#include <rocprim/rocprim.hpp>

#include <math.h>
#include <cmath>
#include <vector>

#include "nn_device.h"
#include "gn_math.h"

// ---- bounding box ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static inline float ord2f(unsigned u) {
    const unsigned v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

// box[0..2] = min (ordered-uint encoding), box[3..5] = max over the FINITE points; box[6] = number of
// points with a NaN / inf coordinate (they are left out of the box: an inf would blow the grid up, a
// NaN is invisible to fmin/fmax anyway)
#define BBOX_SLOTS 64
#define BBOX_STRIDE 32                  // words: a slot per 128-byte line; line 0 holds the folded box
#define BBOX_WORDS (BBOX_STRIDE * (1 + BBOX_SLOTS))
template <typename T>
__global__ void __launch_bounds__(256) k_bbox(const T *__restrict__ xyz, int64_t n, unsigned *box) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const T v0 = xyz[3 * i], v1 = xyz[3 * i + 1], v2 = xyz[3 * i + 2];
        const T v[3] = {v0, v1, v2};
        const T big = (T)3.0e38;                                      // beyond float32 range counts as non-finite
        if (!(fabs(v0) <= big && fabs(v1) <= big && fabs(v2) <= big)) { ++bad; continue; }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // round outward when narrowing float64 centroids
            float fl = (float)v[a], fh = (float)v[a];
            if ((T)fl > v[a]) fl = nextafterf(fl, -INFINITY);
            if ((T)fh < v[a]) fh = nextafterf(fh, INFINITY);
            lo[a] = fminf(lo[a], fl); hi[a] = fmaxf(hi[a], fh);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int off = 32; off >= 1; off >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
        }
    }
    for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
    // one atomic per block and component (thousands of waves hammering six words serialise badly)
    __shared__ float slo[4][3], shi[4][3];
    __shared__ unsigned sbad[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { slo[wave][a] = lo[a]; shi[wave][a] = hi[a]; }
        sbad[wave] = bad;
    }
    __syncthreads();
    // (1024 blocks x 7 atomics on one cache line serialise in its L2 channel -- most of this kernel's 29 us at 1.06 M points:
    // the blocks spread over BBOX_SLOTS lines, k_bbox_final folds them into box[0..6])
    unsigned *slot = box + BBOX_STRIDE * (1 + blockIdx.x % BBOX_SLOTS);
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        const float l = fminf(fminf(slo[0][a], slo[1][a]), fminf(slo[2][a], slo[3][a]));
        const float h = fmaxf(fmaxf(shi[0][a], shi[1][a]), fmaxf(shi[2][a], shi[3][a]));
        atomicMin(&slot[a], f2ord(l));
        atomicMax(&slot[3 + a], f2ord(h));
    }
    if (threadIdx.x == 3) {
        const unsigned b = sbad[0] + sbad[1] + sbad[2] + sbad[3];
        if (b) atomicAdd(&slot[6], b);
    }
}

// lo / hi over the finite points (0 when there is none); *nonfinite = how many points were left out
__global__ void __launch_bounds__(64) k_bbox_init(unsigned *box) {           // one lane per slot
    unsigned *slot = box + BBOX_STRIDE * (1 + threadIdx.x);
#pragma unroll
    for (int a = 0; a < 7; ++a) slot[a] = a < 3 ? 0xffffffffu : 0u;
}
__global__ void __launch_bounds__(64) k_bbox_final(unsigned *box) {
    const unsigned *slot = box + BBOX_STRIDE * (1 + threadIdx.x);
    unsigned v[7];
#pragma unroll
    for (int a = 0; a < 7; ++a) v[a] = slot[a];
#pragma unroll
    for (int a = 0; a < 7; ++a)
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned o = __shfl_xor(v[a], off, 64);
            v[a] = a < 3 ? min(v[a], o) : (a < 6 ? max(v[a], o) : v[a] + o);
        }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 7; ++a) box[a] = v[a];
    }
}
static_assert(BBOX_SLOTS == 64, "k_bbox_init / k_bbox_final: one lane per slot");

// the box of k_bbox, launched only (box: BBOX_WORDS words on the device, the result in the first 7)
template <typename T>
static pcr_status device_bbox_launch(pcr_context *ctx, const T *d_xyz, int64_t n, unsigned *d_box) {
    hipLaunchKernelGGL(k_bbox_init, dim3(1), dim3(64), 0, ctx->stream, d_box);
    if (n > 0) {
        int64_t nb = (n + 255) / 256;
        if (nb > 1024) nb = 1024;
        hipLaunchKernelGGL(k_bbox<T>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, d_xyz, n, d_box);
    }
    hipLaunchKernelGGL(k_bbox_final, dim3(1), dim3(64), 0, ctx->stream, d_box);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

static void bbox_decode(const unsigned h[7], int64_t n, float lo[3], float hi[3]) {
    const bool any = n > 0 && (int64_t)h[6] < n;
    for (int a = 0; a < 3; ++a) {
        lo[a] = any ? ord2f(h[a]) : 0.f;
        hi[a] = any ? ord2f(h[3 + a]) : 0.f;
    }
}

template <typename T>
static pcr_status device_bbox(pcr_context *ctx, const T *d_xyz, int64_t n, float lo[3], float hi[3],
                              int64_t *nonfinite = nullptr) {
    DevBuf<unsigned> d_box;
    HIP_TRY(d_box.alloc(BBOX_WORDS));
    PCR_TRY(device_bbox_launch<T>(ctx, d_xyz, n, d_box.p));
    unsigned h[7];
    HIP_TRY(hipMemcpyAsync(h, d_box, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    bbox_decode(h, n, lo, hi);
    if (nonfinite) *nonfinite = (int64_t)h[6];
    return PCR_OK;
}

// ---- cell ids, histogram -----------------------------------------------------------------
template <typename Real>
__device__ __forceinline__ uint32_t cell_of(const Geom<Real> &g, Real x, Real y, Real z) {
    int cx = (int)floor((x - g.ox) * g.inv_h), cy = (int)floor((y - g.oy) * g.inv_h), cz = (int)floor((z - g.oz) * g.inv_h);
    cx = min(max(cx, 0), g.nx - 1); cy = min(max(cy, 0), g.ny - 1); cz = min(max(cz, 0), g.nz - 1);
    return (uint32_t)(((size_t)cz * g.ny + cy) * g.nx + cx);
}

// (thousands of blocks adding to ONE word serialise in its L2 channel: ~10 ns each, 41 us for the 4141 blocks of 1.06 M points --
// the count goes to OCC_SLOTS words on separate cache lines and the host adds them up)
#define OCC_SLOTS 64
#define OCC_STRIDE 16
#define OCC_WORDS (OCC_SLOTS * OCC_STRIDE)
static unsigned long long occ_total(const unsigned long long *h) {
    unsigned long long t = 0;
    for (int i = 0; i < OCC_SLOTS; ++i) t += h[i * OCC_STRIDE];
    return t;
}

// (occ: += the number of cells this launch touched first, i.e. the occupied cells of a histogram that started at zero -- one
// atomic per block; a separate counting pass over the cells cost as much as this kernel, round 5)
// Position of a point inside its cell as a Morton code of 3 x `b` bits (b <= 3): the minor sort key of a target with heavy
// cells, so that 8 / 64 consecutive records of a cell are a compact patch (leaf / group boxes, Geom::lbox)
template <typename Real>
__device__ __forceinline__ uint32_t sub_morton(const Geom<Real> &g, Real x, Real y, Real z, int b) {
    const Real s = (Real)(1 << b);
    const Real ux = (x - g.ox) * g.inv_h, uy = (y - g.oy) * g.inv_h, uz = (z - g.oz) * g.inv_h;
    const int m = (1 << b) - 1;
    const int ix = min(max((int)((ux - floor(ux)) * s), 0), m), iy = min(max((int)((uy - floor(uy)) * s), 0), m),
              iz = min(max((int)((uz - floor(uz)) * s), 0), m);
    uint32_t code = 0;
    for (int k = 0; k < b; ++k)
        code |= (((uint32_t)ix >> k) & 1u) << (3 * k) | (((uint32_t)iy >> k) & 1u) << (3 * k + 1) | (((uint32_t)iz >> k) & 1u) << (3 * k + 2);
    return code;
}

// Position of a point inside its cell along x, in quanta of cell / 65536: the minor sort key of an x-ordered target (Geom::xq).
// Non-decreasing in x over the points of a cell: (x - ox) * inv_h is monotone, the cell's own index is subtracted exactly, the
// scale is a power of two and the clamp keeps the order.  cx0 / span: the cells the key counts from and over -- the point's own
// cell (cell_of's x index) and 1 for the cell-sorted array; the extended list of cell cx holds points of the cells
// cx - 1 .. cx + 1 and is keyed from the lower face of cell cx - 1 over 3 cells.  Two records with equal keys differ in x by
// less than cell / 65536 plus the rounding of (x - ox) * inv_h, which Geom::slack covers.
#define PCR_XQ_BITS 16
template <typename Real>
__device__ __forceinline__ uint32_t sub_xq(const Geom<Real> &g, Real x, int cx0, int span) {
    const Real ux = (x - g.ox) * g.inv_h;
    const int q = (int)floor((ux - (Real)cx0) * (Real)(1 << PCR_XQ_BITS));
    return (uint32_t)min(max(q, 0), (span << PCR_XQ_BITS) - 1);
}
template <typename Real>
__device__ __forceinline__ uint32_t sub_xq_own(const Geom<Real> &g, Real x) {
    return sub_xq<Real>(g, x, min(max((int)floor((x - g.ox) * g.inv_h), 0), g.nx - 1), 1);
}

// (occ: += the number of cells this launch touched first, i.e. the occupied cells of a histogram that started at zero -- one
// atomic per block; a separate counting pass over the cells cost as much as this kernel, round 5)
// sub_bits > 0: cell_id = (cell << sub_bits) | Morton code of the position inside the cell.
// occ[slot + 1] (histogram passes): max over the block of the population its points saw their cells reach (round 6: the probe
// of the automatic cell size also tells whether some cells are far heavier than the average)
// K: the sort key's type -- uint32_t, or (round 6, heavy targets) 64 bits wide so that the sub-cell code gets 18 bits instead of
// the 6-9 a 32-bit key leaves behind a 24-bit cell id
template <typename Real, typename T, typename K = uint32_t>
__global__ void __launch_bounds__(256) k_cell_ids(const T *__restrict__ xyz, int64_t n, Geom<Real> g,
                                                  K *cell_id, uint32_t *idx, uint32_t *counts, unsigned long long *occ,
                                                  int sub_bits, bool xsub = false) {
    __shared__ unsigned firsts, popmax;
    if (threadIdx.x == 0) { firsts = 0; popmax = 0; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool first = false;
    unsigned pop = 0;
    uint32_t c = 0;
    if (i < n) {
        const Real x = (Real)xyz[3 * i], y = (Real)xyz[3 * i + 1], z = (Real)xyz[3 * i + 2];
        c = cell_of<Real>(g, x, y, z);
        if (cell_id) {
            // (xsub: the minor key is the x offset inside the cell, PCR_XQ_BITS wide, instead of the Morton code)
            cell_id[i] = sub_bits > 0 ? ((K)c << sub_bits) | (K)(xsub ? sub_xq_own<Real>(g, x) : sub_morton<Real>(g, x, y, z, sub_bits / 3)) : (K)c;
            idx[i] = (uint32_t)i;
        }
    }
    if (!counts) return;                 // (ids only: block-uniform)
    {
        // histogram pass.  One atomic per DISTINCT cell of the wave (round 6): on a LiDAR sweep hundreds of consecutive returns
        // fall into one cell, and 64 lanes queueing on one counter made a probing pass 244 us where the street cloud's takes 54.
        // The leader of each group of equal cells adds the group's size; `pop` = the population the cell reached, `first` = the
        // group that found it empty.
        const bool valid = i < n;
        unsigned long long todo = __ballot(valid);
        const int lane = threadIdx.x & 63;
        while (todo) {
            const int src = __builtin_ctzll(todo);
            const uint32_t c0 = (uint32_t)__shfl((int)c, src, 64);
            const unsigned long long same = __ballot(valid && c == c0) & todo;
            if (lane == src) {
                const unsigned cnt = (unsigned)__popcll(same);
                const unsigned old = atomicAdd(&counts[c0], cnt);
                pop = old + cnt; first = old == 0u;
            }
            todo &= ~same;
        }
    }
    const unsigned long long m = __ballot(first);
    for (int off = 32; off >= 1; off >>= 1) pop = max(pop, (unsigned)__shfl_xor((int)pop, off, 64));
    if ((threadIdx.x & 63) == 0) { if (m) atomicAdd(&firsts, (unsigned)__popcll(m)); atomicMax(&popmax, pop); }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (firsts) atomicAdd(&occ[(blockIdx.x % OCC_SLOTS) * OCC_STRIDE], (unsigned long long)firsts);
        atomicMax(&occ[(blockIdx.x % OCC_SLOTS) * OCC_STRIDE + 1], (unsigned long long)popmax);
    }
}
static unsigned long long occ_popmax(const unsigned long long *h) {
    unsigned long long t = 0;
    for (int i = 0; i < OCC_SLOTS; ++i) t = h[i * OCC_STRIDE + 1] > t ? h[i * OCC_STRIDE + 1] : t;
    return t;
}

// cell_start from the SORTED cell ids instead of an atomic histogram (the final pass' 1.06 M atomics on random cells took 58 us,
// these two steps 10 + 20): head[c] = position of the first record of cell c (the array starts as all-ones, head[ncells] = n);
// a reverse running minimum then gives every cell -- the empty ones included -- the position of the first record at or behind
// it, which IS the exclusive prefix of the counts.  occ += the occupied cells.
template <typename K = uint32_t>
__global__ void __launch_bounds__(256) k_cell_heads(const K *__restrict__ cid, int64_t n, int64_t ncells, uint32_t *head,
                                                    unsigned long long *occ, int shift) {
    __shared__ unsigned firsts;
    if (threadIdx.x == 0) firsts = 0;
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool first = false;
    if (j < n) {
        const uint32_t c = (uint32_t)(cid[j] >> shift);   // (shift: the sub-cell bits of a heavy target's sort key)
        first = j == 0 || (uint32_t)(cid[j - 1] >> shift) != c;
        if (first) head[c] = (uint32_t)j;
        if (j == 0) head[ncells] = (uint32_t)n;
    }
    const unsigned long long m = __ballot(first);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&firsts, (unsigned)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && firsts) atomicAdd(&occ[(blockIdx.x % OCC_SLOTS) * OCC_STRIDE], (unsigned long long)firsts);
}

static pcr_status reverse_min_scan_u32(pcr_context *ctx, uint32_t *d_inout, int64_t n) {
    auto it = rocprim::make_reverse_iterator(d_inout + n);
    size_t tmp_bytes = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, tmp_bytes, it, it, (size_t)n, rocprim::minimum<uint32_t>(), ctx->stream));
    DevBuf<char> tmp;
    HIP_TRY(tmp.alloc_bytes(tmp_bytes));
    HIP_TRY(rocprim::inclusive_scan(tmp.p, tmp_bytes, it, it, (size_t)n, rocprim::minimum<uint32_t>(), ctx->stream));
    return PCR_OK;
}

__global__ void __launch_bounds__(256) k_gather_f32(const float *__restrict__ xyz, const uint32_t *__restrict__ order,
                                                    int64_t n, PtF *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = order[j];
    out[j] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float(i));
}

__global__ void __launch_bounds__(256) k_gather_f64(const double *__restrict__ xyz, const uint32_t *__restrict__ order,
                                                    int64_t n, PtD *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = order[j];
    out[j] = make_double4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2],
                          __longlong_as_double((long long)i));
}

// ---- halo: extended per-cell lists (point targets) ------------------------------------------------
// Every point is listed in its own cell and in each of the 26 neighbours whose shared face / edge /
// corner it lies within `halo` of (margin widened by the grid's rounding slack: listing a point too
// often is harmless, too rarely would break the certification of nn_ring0).
template <typename F>
__device__ __forceinline__ void halo_cells(const Geom<float> &g, float x, float y, float z, F &&f) {
    const float q[3] = {x, y, z}, o[3] = {g.ox, g.oy, g.oz};
    const int nn[3] = {g.nx, g.ny, g.nz};
    int c[3], lo[3], hi[3];
    const float m = g.halo + g.slack;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int ci = (int)floor((q[a] - o[a]) * g.inv_h);
        ci = min(max(ci, 0), nn[a] - 1);
        c[a] = ci;
        const float dl = (q[a] - o[a]) - (float)ci * g.h;              // to the cell's lower face
        const float dh = (float)(ci + 1) * g.h - (q[a] - o[a]);        // to its upper face
        lo[a] = (dl <= m && ci > 0) ? -1 : 0;
        hi[a] = (dh <= m && ci < nn[a] - 1) ? 1 : 0;
    }
    for (int dz = lo[2]; dz <= hi[2]; ++dz)
        for (int dy = lo[1]; dy <= hi[1]; ++dy)
            for (int dx = lo[0]; dx <= hi[0]; ++dx)
                f((uint32_t)(((size_t)(c[2] + dz) * g.ny + (c[1] + dy)) * g.nx + (c[0] + dx)), (dx | dy | dz) == 0);
}

// A cell's list starts with its OWN points, in their cell-sorted order: their number and their places are known from
// cell_start, so only the copies into neighbouring cells (0.7 of the 1.7 entries per point at a 0.1-cell margin) go through
// atomics (round 5: k_halo_count 52 -> 17, k_halo_fill 85 -> 26 us at 1.06 M points).
__global__ void __launch_bounds__(256) k_halo_own(const uint32_t *__restrict__ cs, int64_t ncells, uint32_t mask, uint32_t *cnt) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c <= ncells) cnt[c] = c < ncells ? (cs[c + 1] & mask) - (cs[c] & mask) : 0u;
}

// cursor of a cell's neighbour copies = start of its list + its own points
__global__ void __launch_bounds__(256) k_halo_cursor(const uint32_t *__restrict__ cs, const uint32_t *__restrict__ cs_h, int64_t ncells,
                                                     uint32_t mask, uint32_t *cursor) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < ncells) cursor[c] = cs_h[c] + ((cs[c + 1] & mask) - (cs[c] & mask));
}

__global__ void __launch_bounds__(256) k_halo_count(const PtF *__restrict__ pts, int64_t n, Geom<float> g, uint32_t *cnt) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const PtF p = pts[j];
    halo_cells(g, p.x, p.y, p.z, [&](uint32_t c, bool own) { if (!own) atomicAdd(&cnt[c], 1u); });
}

__global__ void __launch_bounds__(256) k_halo_fill(const PtF *__restrict__ pts, int64_t n, Geom<float> g, const uint32_t *__restrict__ cs,
                                                   const uint32_t *__restrict__ cs_h, uint32_t *cursor, PtF *out, uint32_t *j_out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const PtF p = pts[j];
    halo_cells(g, p.x, p.y, p.z, [&](uint32_t c, bool own) {
        const uint32_t e = own ? cs_h[c] + ((uint32_t)j - (cs[c] & g.cs_mask)) : atomicAdd(&cursor[c], 1u);
        out[e] = p; j_out[e] = (uint32_t)j;
    });
}

// x-ordered targets (Geom::xq): a list must be ascending in x as a whole, its own points and the copies from its neighbours
// merged.  The fill writes (list cell, x offset from the lower face of the cell before it) keys and the cell-sorted indices into
// the same slots as k_halo_fill; one radix sort of the pairs then orders every list in place (the cell is the major key and every
// list keeps its number of entries), and the records are gathered behind it.
__global__ void __launch_bounds__(256) k_halo_fill_x(const PtF *__restrict__ pts, int64_t n, Geom<float> g, const uint32_t *__restrict__ cs,
                                                     const uint32_t *__restrict__ cs_h, uint32_t *cursor, unsigned long long *key_out,
                                                     uint32_t *j_out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const PtF p = pts[j];
    halo_cells(g, p.x, p.y, p.z, [&](uint32_t c, bool own) {
        const uint32_t e = own ? cs_h[c] + ((uint32_t)j - (cs[c] & g.cs_mask)) : atomicAdd(&cursor[c], 1u);
        const int lx = (int)(c % (uint32_t)g.nx);
        key_out[e] = ((unsigned long long)c << (PCR_XQ_BITS + 2)) | (unsigned long long)sub_xq<float>(g, p.x, lx - 1, 3);
        j_out[e] = (uint32_t)j;
    });
}
__global__ void __launch_bounds__(256) k_halo_gather(const PtF *__restrict__ pts, const uint32_t *__restrict__ j_h, int64_t n_h, PtF *out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n_h) out[e] = pts[j_h[e]];
}

// cs_h gets the gap bits of the finished cell_start (same cells are empty in both)
__global__ void __launch_bounds__(256) k_gap_copy(const uint32_t *__restrict__ cs, uint32_t *cs_h, int64_t n1, uint32_t mask) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n1) cs_h[c] = (cs_h[c] & mask) | (cs[c] & ~mask);
}

// ---- empty-space field: Chebyshev distance (in cells) to the nearest occupied cell -----------------
// gap(c) = min over occupied cells o of max(|dx|, |dy|, |dz|), capped at PCR_GAP_MAX.  The L-infinity
// distance separates: first the distance along x inside every row, then min over dy of max(that, |dy|),
// then the same along z -- three passes of at most 31 reads per cell with an early exit (a candidate at
// offset d cannot beat a value <= d), instead of 15 dilation passes over 27 neighbours each (65 ms for
// the 251 M cells of the 1e8-point target).  Every pass carries the cell the minimum came from; its
// first point becomes the seed of the empty cell.
#define GAP_INF 255
// x pass.  A block first turns the occupancy of its 256 cells (+ 64 on either side) into bits in LDS; a cell then finds the
// nearest occupied cell of its row with two bit scans over a 31-bit window instead of up to 62 reads of cell_start (round 5:
// 46 us -> per 3 M cells; an empty cell far from any point, the common case in a street scene, used to run the full loop).
static_assert(PCR_GAP_MAX <= 31, "the window of k_gap_x is one 64-bit word");
__global__ void __launch_bounds__(256) k_gap_x(const uint32_t *__restrict__ cs, int nx, int64_t ncells, uint8_t *gap,
                                               uint32_t *src) {
    __shared__ unsigned long long occ[6];                 // bit b of word w: cell c0 - 64 + 64 w + b
    const int64_t c0 = (int64_t)blockIdx.x * 256;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    auto occupied = [&](int64_t cc) { return cc >= 0 && cc < ncells && cs[cc + 1] != cs[cc]; };
    const unsigned long long m = __ballot(occupied(c0 + t));
    if (lane == 0) occ[1 + wave] = m;
    if (wave < 2) {
        const unsigned long long m2 = __ballot(occupied(wave == 0 ? c0 - 64 + lane : c0 + 256 + lane));
        if (lane == 0) occ[wave == 0 ? 0 : 5] = m2;
    }
    __syncthreads();
    const int64_t c = c0 + t;
    if (c >= ncells) return;
    const int x = (int)(c % nx);
    const int W = PCR_GAP_MAX;
    const int lo = 64 + t - W, wi = lo >> 6, sh = lo & 63;          // window bit i = cell c - W + i
    unsigned long long win = occ[wi] >> sh;
    if (sh) win |= occ[wi + 1] << (64 - sh);
    win &= (1ull << (2 * W + 1)) - 1ull;
    const int dl_max = min(x, W), dr_max = min(nx - 1 - x, W);       // stay inside the row
    win &= ~((1ull << (W - dl_max)) - 1ull);
    win &= (1ull << (W + dr_max + 1)) - 1ull;
    const unsigned left = (unsigned)(win & ((1ull << (W + 1)) - 1ull));     // bit W - d: the cell d to the left (d = 0: itself)
    const unsigned right = (unsigned)(win >> W);                            // bit d: the cell d to the right
    const int dl = left ? W - (31 - __clz((int)left)) : GAP_INF;
    const int dr = right ? __ffs((int)right) - 1 : GAP_INF;
    uint8_t g = GAP_INF;
    uint32_t from = 0xffffffffu;
    if (dl <= dr && dl != GAP_INF) { g = (uint8_t)dl; from = (uint32_t)(c - dl); }      // (equal distances: the left cell, as the loop had it)
    else if (dr != GAP_INF) { g = (uint8_t)dr; from = (uint32_t)(c + dr); }
    gap[c] = g; src[c] = from;
}

// along one more axis (stride = cells between neighbours on that axis, len = cells on it, pos = own index)
__global__ void __launch_bounds__(256) k_gap_axis(const uint8_t *__restrict__ gin, const uint32_t *__restrict__ sin,
                                                  int64_t ncells, int64_t stride, int len, int64_t period,
                                                  uint8_t *gout, uint32_t *sout) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncells) return;
    const int pos = (int)((c % period) / stride);
    int best = gin[c];
    uint32_t from = sin[c];
    for (int d = 1; d <= PCR_GAP_MAX && d < best; ++d) {          // a cell d away yields at least d
        if (pos - d >= 0) {
            const int v = max((int)gin[c - d * stride], d);
            if (v < best) { best = v; from = sin[c - d * stride]; }
        }
        if (pos + d < len) {
            const int v = max((int)gin[c + d * stride], d);
            if (v < best) { best = v; from = sin[c + d * stride]; }
        }
    }
    gout[c] = (uint8_t)best; sout[c] = from;
}

// gap bits into cell_start, source cell -> index of its first point (the seed)
__global__ void __launch_bounds__(256) k_gap_pack(uint32_t *cs, int64_t ncells, const uint8_t *__restrict__ gap,
                                                  const uint32_t *__restrict__ src, uint32_t *seed) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncells) return;
    const uint32_t g = gap[c] > PCR_GAP_MAX ? PCR_GAP_MAX : gap[c];
    const uint32_t from = src[c];
    // (cs of OTHER cells may already carry their gap bits: mask them off)
    seed[c] = from == 0xffffffffu ? 0xffffffffu : (cs[from] & ((1u << PCR_GAP_SHIFT) - 1u));
    cs[c] |= g << PCR_GAP_SHIFT;
}

static pcr_status pack_gap_field(pcr_context *ctx, uint32_t *cs, int nx, int ny, int nz, uint32_t **seed_out) {
    const int64_t ncells = (int64_t)nx * ny * nz;
    DevBuf<uint8_t> g1, g2;
    DevBuf<uint32_t> s1, s2, seed;
    HIP_TRY(g1.alloc((size_t)ncells)); HIP_TRY(g2.alloc((size_t)ncells));
    HIP_TRY(s1.alloc((size_t)ncells)); HIP_TRY(s2.alloc((size_t)ncells));
    HIP_TRY(seed.alloc_exact((size_t)ncells));
    const unsigned nb = (unsigned)((ncells + 255) / 256);
    hipLaunchKernelGGL(k_gap_x, dim3(nb), dim3(256), 0, ctx->stream, (const uint32_t *)cs, nx, ncells, g1.p, s1.p);
    hipLaunchKernelGGL(k_gap_axis, dim3(nb), dim3(256), 0, ctx->stream, (const uint8_t *)g1.p, (const uint32_t *)s1.p, ncells,
                       (int64_t)nx, ny, (int64_t)nx * ny, g2.p, s2.p);
    hipLaunchKernelGGL(k_gap_axis, dim3(nb), dim3(256), 0, ctx->stream, (const uint8_t *)g2.p, (const uint32_t *)s2.p, ncells,
                       (int64_t)nx * ny, nz, ncells, g1.p, s1.p);
    hipLaunchKernelGGL(k_gap_pack, dim3(nb), dim3(256), 0, ctx->stream, cs, ncells, (const uint8_t *)g1.p, (const uint32_t *)s1.p,
                       seed.p);
    HIP_TRY(hipGetLastError());
    *seed_out = seed.release();
    return PCR_OK;
}

// PCR_EDGE_SEED=0 (developer A/B switch, read once): queries outside the grid box start at the gate (GeomSwitches::edge_seed)
static uint32_t edge_seed_rule() {
    static const uint32_t on = [] { const char *e = getenv("PCR_EDGE_SEED"); return e && *e && atoi(e) == 0 ? 0u : 1u; }();
    return on;
}

template <typename Real>
static bool make_geom(const float lo[3], const float hi[3], double h, Geom<Real> *g, double *ncells) {
    g->ox = (Real)lo[0]; g->oy = (Real)lo[1]; g->oz = (Real)lo[2];
    g->h = (Real)h; g->inv_h = (Real)(1.0 / h);
    *ncells = INFINITY;
    if (!(h > 0.0) || !std::isfinite(h)) return false;
    double dims[3];
    for (int a = 0; a < 3; ++a) dims[a] = floor(((double)hi[a] - (double)lo[a]) / h) + 2.0;
    *ncells = dims[0] * dims[1] * dims[2];
    if (dims[0] > 2.0e9 || dims[1] > 2.0e9 || dims[2] > 2.0e9) return false;
    g->nx = (int)dims[0]; g->ny = (int)dims[1]; g->nz = (int)dims[2];
    double mag = 0;
    for (int a = 0; a < 3; ++a) { mag = fmax(mag, fabs((double)lo[a])); mag = fmax(mag, fabs((double)hi[a])); }
    const double eps = sizeof(Real) == 4 ? 1.2e-7 : 2.3e-16;
    g->slack = (Real)((double)PCR_SLACK_ULPS * eps * (mag + h) + 1e-30);
    g->cs_mask = 0xffffffffu;
    g->seed = nullptr;
    g->halo = (Real)0; g->cs_h = nullptr; g->pts_h = nullptr; g->j_h = nullptr; g->rowocc = nullptr; g->nyw = 0; g->nxb = 0; g->lbox = nullptr; g->gbox = nullptr; g->lbox_h = nullptr; g->gbox_h = nullptr;
    g->xq = (Real)0;
    if constexpr (sizeof(Real) == 4) g->sw.edge_seed = edge_seed_rule();
    return true;
}

// counts -> exclusive prefix (cell_start has ncells+1 entries; counts[ncells] must be 0)
static pcr_status exclusive_scan_u32(pcr_context *ctx, uint32_t *d_inout, int64_t n) {
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, d_inout, d_inout, (int)n, ctx->stream));
    DevBuf<char> tmp;
    HIP_TRY(tmp.alloc_bytes(tmp_bytes));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, d_inout, d_inout, (int)n, ctx->stream));
    // (no synchronisation: the temporary goes back to the context's block cache, whose next user runs on the same stream --
    // round 5, VERDICT r4 item 6b: a point-index build used to synchronise 11 times)
    return PCR_OK;
}

template <typename K>
static pcr_status sort_pairs(pcr_context *ctx, K *keys_in, K *keys_out, uint32_t *vals_in, uint32_t *vals_out, int64_t n,
                             int end_bit) {
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit,
                                               ctx->stream));
    DevBuf<char> tmp;
    HIP_TRY(tmp.alloc_bytes(tmp_bytes));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit,
                                               ctx->stream));
    return PCR_OK;
}

// The host-side rule: which targets store the records of a cell in ascending x.  float32 point targets (the centroid filter
// index of a voxel target is searched by tracking searches only and stays as it was) without heavy cells -- those keep the
// Morton order their leaf / group boxes need -- whose (cell, x offset) key fits 64 bits; PCR_XORDER=0 builds the old order
// (the A/B switch: read when a target is built, never on the pass path).
extern "C" int pcr_x_order_rule(int f32_point_target, int heavy, int64_t n, int cell_bits) {
    const char *e = getenv("PCR_XORDER");
    if (e && *e && atoi(e) == 0) return 0;
    return f32_point_target && !heavy && n > 0 && cell_bits + PCR_XQ_BITS <= 64 ? 1 : 0;
}

static int bits_for(double ncells) {
    int b = 1;
    while (b < 32 && ldexp(1.0, b) < ncells) ++b;
    return b;
}

// PCR_PTS_PAD sentinel records (+inf coordinates, index ~0) behind the last record of a point array
template <typename PT>
__global__ void __launch_bounds__(64) k_pad_sentinels(PT *p) {
    if (threadIdx.x >= PCR_PTS_PAD) return;
    PT v;
    v.x = v.y = v.z = __builtin_inff();
    if constexpr (sizeof(v.w) == 4) v.w = __uint_as_float(0xffffffffu);
    else v.w = __longlong_as_double(0xffffffffLL);
    p[threadIdx.x] = v;
}

// Extended per-cell lists of a finished point grid (cell-sorted points `pts`, cell_start `cs` with its gap bits) for
// a halo margin of halo_frac x cell.  n_h = 0 (and no buffers) when the copies would not fit the 28-bit offsets.
static pcr_status build_halo_lists(pcr_context *ctx, Geom<float> gh, const PtF *pts, int64_t n, const uint32_t *cs, double halo_frac,
                                   DevBuf<uint32_t> *cs_h, DevBuf<PtF> *pts_h, DevBuf<uint32_t> *j_h, int64_t *n_h_out) {
    *n_h_out = 0;
    const size_t ncells = (size_t)gh.nx * (size_t)gh.ny * (size_t)gh.nz;
    const unsigned nb = (unsigned)((n + 255) / 256);
    gh.halo = (float)(fmin(halo_frac, 1.0) * (double)gh.h);     // (1.0: a cell's list = all points of its 27-cell block)
    const size_t nc1 = ncells + 1;
    HIP_TRY(cs_h->alloc_exact(nc1));
    const unsigned nbc = (unsigned)((nc1 + 255) / 256);
    hipLaunchKernelGGL(k_halo_own, dim3(nbc), dim3(256), 0, ctx->stream, cs, (int64_t)ncells, gh.cs_mask, cs_h->p);
    hipLaunchKernelGGL(k_halo_count, dim3(nb), dim3(256), 0, ctx->stream, pts, n, gh, cs_h->p);
    HIP_TRY(hipGetLastError());
    PCR_TRY(exclusive_scan_u32(ctx, cs_h->p, (int64_t)nc1));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, cs_h->p + (nc1 - 1), sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if ((int64_t)total >= ((int64_t)1 << PCR_GAP_SHIFT)) {     // too many copies for 28-bit offsets: no lists
        cs_h->reset();
        return PCR_OK;
    }
    const int64_t n_h = (int64_t)total;
    DevBuf<uint32_t> cursor;
    HIP_TRY(cursor.alloc(nc1));
    hipLaunchKernelGGL(k_halo_cursor, dim3(nbc), dim3(256), 0, ctx->stream, cs, (const uint32_t *)cs_h->p, (int64_t)ncells, gh.cs_mask, cursor.p);
    HIP_TRY(pts_h->alloc_exact((size_t)n_h + PCR_PTS_PAD));
    HIP_TRY(j_h->alloc_exact((size_t)n_h + PCR_PTS_PAD));
    hipLaunchKernelGGL(k_pad_sentinels<PtF>, dim3(1), dim3(64), 0, ctx->stream, pts_h->p + (size_t)n_h);
    if (gh.xq > 0.f && n_h > 0) {
        DevBuf<unsigned long long> key, key2;
        DevBuf<uint32_t> j_tmp;
        HIP_TRY(key.alloc((size_t)n_h)); HIP_TRY(key2.alloc((size_t)n_h)); HIP_TRY(j_tmp.alloc((size_t)n_h));
        hipLaunchKernelGGL(k_halo_fill_x, dim3(nb), dim3(256), 0, ctx->stream, pts, n, gh, cs, (const uint32_t *)cs_h->p, cursor.p, key.p, j_tmp.p);
        PCR_TRY(sort_pairs<unsigned long long>(ctx, key, key2, j_tmp, j_h->p, n_h, bits_for((double)ncells) + PCR_XQ_BITS + 2));
        hipLaunchKernelGGL(k_halo_gather, dim3((unsigned)((n_h + 255) / 256)), dim3(256), 0, ctx->stream, pts, (const uint32_t *)j_h->p, n_h, pts_h->p);
    } else
        hipLaunchKernelGGL(k_halo_fill, dim3(nb), dim3(256), 0, ctx->stream, pts, n, gh, cs, (const uint32_t *)cs_h->p, cursor.p, pts_h->p, j_h->p);
    hipLaunchKernelGGL(k_gap_copy, dim3((unsigned)((nc1 + 255) / 256)), dim3(256), 0, ctx->stream, cs, cs_h->p, (int64_t)nc1, gh.cs_mask);
    HIP_TRY(hipGetLastError());
    *n_h_out = n_h;                 // (not synchronised: every caller synchronises the stream before it hands the lists out)
    return PCR_OK;
}

// Shared build: pick h (auto: average occupancy of the occupied cells in [3, 10]), histogram,
// prefix, stable radix sort by cell id, gather.
template <typename Real, typename T, typename PT>
static pcr_status build_grid(pcr_context *ctx, const T *d_xyz, int64_t n, double h, bool auto_h, Geom<Real> *geom,
                             uint32_t **cell_start_out, uint32_t **seed_out, PT **pts_out, int64_t *occupied_out,
                             double halo_frac, uint32_t **cs_h_out, PtF **pts_h_out, uint32_t **j_h_out, int64_t *n_h_out,
                             bool *heavy_out = nullptr) {
    if (heavy_out) *heavy_out = false;
    *seed_out = nullptr;
    *cs_h_out = nullptr; *pts_h_out = nullptr; *j_h_out = nullptr; *n_h_out = 0;
    PCR_REQUIRE(n < ((int64_t)1 << 31), "at most 2^31-1 points per target");
    HIP_TRY(hipSetDevice(ctx->device));
    float lo[3], hi[3];
    int64_t nonfinite = 0;
    PCR_TRY(device_bbox<T>(ctx, d_xyz, n, lo, hi, &nonfinite));
    if (nonfinite > 0) {
        // A target point with a NaN / inf coordinate (common in raw PCD files) has no cell and can be nobody's
        // nearest neighbour; the reference's KD-tree would return garbage or hang on it.  Refuse it here.
        pcr_set_error("target has %lld point(s) with a non-finite coordinate; drop them first "
                      "(e.g. xyz[np.isfinite(xyz).all(1)])", (long long)nonfinite);
        return PCR_ERR_INVALID;
    }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const double max_cells = fmin(1.0e9, (double)free_b / 4.0 / 8.0);   // cell_start may take 1/8 of free HBM

    DevBuf<uint32_t> d_counts;
    DevBuf<unsigned long long> d_nz;
    HIP_TRY(d_nz.alloc(OCC_WORDS));
    std::vector<unsigned long long> h_nz(OCC_WORDS);
    double ncells = 0;
    int64_t occupied = 0;
    const unsigned nb = (unsigned)((n + 255) / 256);
    int dir = 0;                  // auto cell size moves in one direction only: -1 shrinking, +1 growing
    bool capped = false;          // hit the memory cap: cannot shrink further
    // Round 6: the automatic cell never shrinks below the edge at which the dense grid would hold more than PCR_CELLS_PER_POINT
    // (default 8) cells per point.  "~5 points per occupied cell" is the right target for a cloud of constant density; on a
    // LiDAR sweep (ring lines, density ~ 1/r^2: synthetic.lidar_sweep) it drives the edge to 6 cm -- 7e8 cells for 1e6 points, and a
    // query one metre from its match walks 17 rings of them (22.9 ms for a pass that takes 0.22 ms on the street cloud).  Such
    // clouds keep cells of the sparse regime and their heavy cells are searched through leaf / group boxes instead (Geom::lbox).
    double h_floor = 0.0;
    unsigned long long pop_max = 0;
    bool probed = false, at_floor = false;
    if (auto_h && n > 0) {
        static const double cpp = getenv("PCR_CELLS_PER_POINT") && atof(getenv("PCR_CELLS_PER_POINT")) > 0 ? atof(getenv("PCR_CELLS_PER_POINT")) : 8.0;
        double vol = 1.0;
        for (int a = 0; a < 3; ++a) vol *= fmax((double)hi[a] - (double)lo[a], 0.0);
        h_floor = cbrt(vol / (cpp * (double)n));
        if (!std::isfinite(h_floor)) h_floor = 0.0;
    }
    // (a given cell size needs no probing pass: the final histogram below counts its occupied cells)
    for (int iter = 0; iter < 16 && auto_h && n > 0; ++iter) {
        Geom<Real> g;
        while (!make_geom<Real>(lo, hi, h, &g, &ncells) || ncells > max_cells) {
            h *= 2.0; capped = true;
            if (!std::isfinite(h) || h > 1.0e30) { pcr_set_error("cannot build a cell grid over this bounding box"); return PCR_ERR_INVALID; }
        }
        HIP_TRY(d_counts.alloc((size_t)ncells + 1));
        HIP_TRY(hipMemsetAsync(d_counts.p, 0, sizeof(uint32_t) * ((size_t)ncells + 1), ctx->stream));
        HIP_TRY(hipMemsetAsync(d_nz.p, 0, sizeof(unsigned long long) * OCC_WORDS, ctx->stream));
        hipLaunchKernelGGL((k_cell_ids<Real, T, uint32_t>), dim3(nb), dim3(256), 0, ctx->stream, d_xyz, n, g,
                           (uint32_t *)nullptr, (uint32_t *)nullptr, d_counts.p, d_nz.p, 0);
        HIP_TRY(hipMemcpyAsync(h_nz.data(), d_nz.p, sizeof(unsigned long long) * OCC_WORDS, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        occupied = (int64_t)occ_total(h_nz.data());
        pop_max = occ_popmax(h_nz.data());
        probed = true;
        const double occ = (double)n / (double)(occupied > 0 ? occupied : 1);
        if (occ > 10.0 && dir <= 0 && !capped) {
            if (h * 0.5 >= h_floor) { h *= 0.5; dir = -1; continue; }
            // (round 6, late: no further probe AT the floor -- there the fine adjustment below cannot move h, and whether the cloud
            // has heavy cells shows in this probe's largest against its average cell just as well; a probing pass over a LiDAR sweep
            // costs 220 us, four times the street cloud's, since hundreds of waves meet on the counters of its heaviest cells)
            if (h > h_floor * 1.05) { h = h_floor; at_floor = true; break; }
        }
        if (occ < 2.5 && dir >= 0) { h *= 2.0; dir = 1; continue; }
        break;
    }
    if (auto_h && n > 0 && occupied > 0 && !capped && !at_floor) {
        // fine adjustment: clouds are surfaces, so occupancy of occupied cells grows like h^2; aim at
        // ~5 points per cell (measured optimum on MI355X: fewer candidates per ring-0 cell, still few rows)
        const double occ = (double)n / (double)occupied;
        double f = sqrt(5.0 / occ);
        f = f < 0.70710678 ? 0.70710678 : (f > 1.41421356 ? 1.41421356 : f);
        h = fmax(h * f, fmin(h, h_floor));
    }
    // heavy cells?  (the probe's largest cell against its average cell; a given cell size has no probe: assume so.  Only the
    // float32 point index has the boxes; sort keys stay 32 bits wide)
    const double occ_mean = (double)n / (double)(occupied > 0 ? occupied : 1);
    bool heavy = heavy_out != nullptr && sizeof(Real) == 4 && n >= 4096 &&
                 (!probed || ((double)pop_max > 64.0 && (double)pop_max > 12.0 * occ_mean));
    {
        const char *he = getenv("PCR_HEAVY");                 // developer: 0 never, 1 always
        if (he && *he && heavy_out != nullptr && sizeof(Real) == 4 && n > 0) heavy = atoi(he) != 0;
    }
    // with the final h: ids + fresh histogram
    Geom<Real> g;
    while (!make_geom<Real>(lo, hi, h, &g, &ncells) || ncells > max_cells) {
        h *= 2.0;
        if (!std::isfinite(h) || h > 1.0e30) { pcr_set_error("cannot build a cell grid over this bounding box"); return PCR_ERR_INVALID; }
    }
    *geom = g;
    HIP_TRY(d_counts.alloc_exact((size_t)ncells + 1));
    HIP_TRY(hipMemsetAsync(d_counts.p, n > 0 ? 0xff : 0, sizeof(uint32_t) * ((size_t)ncells + 1), ctx->stream));
    DevBuf<uint32_t> d_cid, d_idx, d_cid2, d_idx2, d_seed;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    HIP_TRY(d_cid.alloc(nn)); HIP_TRY(d_idx.alloc(nn));
    HIP_TRY(d_cid2.alloc(nn)); HIP_TRY(d_idx2.alloc(nn));
    DevBuf<PT> d_pts;
    HIP_TRY(d_pts.alloc_exact(nn + PCR_PTS_PAD));
    // sentinel records behind the last point (see nn_scan_range): +inf coordinates, index ~0
    hipLaunchKernelGGL(k_pad_sentinels<PT>, dim3(1), dim3(64), 0, ctx->stream, d_pts.p + (size_t)n);
    HIP_TRY(hipMemsetAsync(d_nz.p, 0, sizeof(unsigned long long) * OCC_WORDS, ctx->stream));
    // Heavy targets: minor sort key = Morton code of the position inside the cell.  First version (round 6): as many bits as a
    // 32-bit key leaves -- 6 behind the 24-bit cell id of the 1.06 M-point LiDAR sweep, i.e. 4 x 4 x 4 sub-cells of 64 mm, each
    // holding ~60 returns of a ring line in ARBITRARY order: every leaf box of such a sub-cell spans all of it and a converged
    // query opens them all (67 loads, of which 43 re-tests).  Now a 64-bit key with PCR_HEAVY_SUB_BITS = 18 (64^3 sub-cells of 4 mm
    // there): 8 consecutive records are 8 neighbours along the line.  <= 9 keeps the 32-bit key.
    int sub_bits = 0;
    bool wide = false;
    // Targets WITHOUT heavy cells: minor sort key = the x offset inside the cell (Geom::xq), through the same 64-bit sort.
    const bool xorder = pcr_x_order_rule(heavy_out != nullptr && sizeof(Real) == 4, heavy, n, bits_for(ncells)) != 0;
    if (xorder) { sub_bits = PCR_XQ_BITS; wide = true; }
    if (heavy) {
        static const int want = getenv("PCR_HEAVY_SUB_BITS") ? atoi(getenv("PCR_HEAVY_SUB_BITS")) : 18;
        const int w = (want < 0 ? 0 : (want > 21 ? 21 : want)) / 3 * 3;
        if (w > 9 && bits_for(ncells) + w <= 64) { sub_bits = w; wide = true; }
        else {
            sub_bits = 32 - bits_for(ncells);
            sub_bits = sub_bits >= 9 ? 9 : (sub_bits / 3) * 3;
            if (w < sub_bits) sub_bits = w;
        }
    }
    if (n > 0 && wide) {
        DevBuf<unsigned long long> d_key, d_key2;
        HIP_TRY(d_key.alloc(nn)); HIP_TRY(d_key2.alloc(nn));
        hipLaunchKernelGGL((k_cell_ids<Real, T, unsigned long long>), dim3(nb), dim3(256), 0, ctx->stream, d_xyz, n, g, d_key.p, d_idx.p,
                           (uint32_t *)nullptr, (unsigned long long *)nullptr, sub_bits, xorder);
        PCR_TRY(sort_pairs<unsigned long long>(ctx, d_key, d_key2, d_idx, d_idx2, n, bits_for(ncells) + sub_bits));
        hipLaunchKernelGGL(k_cell_heads<unsigned long long>, dim3(nb), dim3(256), 0, ctx->stream, (const unsigned long long *)d_key2.p, n,
                           (int64_t)ncells, d_counts.p, d_nz.p, sub_bits);
    } else if (n > 0) {
        hipLaunchKernelGGL((k_cell_ids<Real, T, uint32_t>), dim3(nb), dim3(256), 0, ctx->stream, d_xyz, n, g, d_cid.p, d_idx.p,
                           (uint32_t *)nullptr, (unsigned long long *)nullptr, sub_bits);
        PCR_TRY(sort_pairs<uint32_t>(ctx, d_cid, d_cid2, d_idx, d_idx2, n, bits_for(ncells) + sub_bits));
        hipLaunchKernelGGL(k_cell_heads<uint32_t>, dim3(nb), dim3(256), 0, ctx->stream, (const uint32_t *)d_cid2.p, n, (int64_t)ncells, d_counts.p, d_nz.p, sub_bits);
    }
    if (n > 0) {
        if (sizeof(Real) == 4)
            hipLaunchKernelGGL(k_gather_f32, dim3(nb), dim3(256), 0, ctx->stream, (const float *)d_xyz,
                               (const uint32_t *)d_idx2.p, n, (PtF *)d_pts.p);
        else
            hipLaunchKernelGGL(k_gather_f64, dim3(nb), dim3(256), 0, ctx->stream, (const double *)d_xyz,
                               (const uint32_t *)d_idx2.p, n, (PtD *)d_pts.p);
    }
    if (n > 0) PCR_TRY(reverse_min_scan_u32(ctx, d_counts, (int64_t)ncells + 1));       // (n = 0: all zeros already)
    if (n > 0 && n < ((int64_t)1 << PCR_GAP_SHIFT)) {
        PCR_TRY(pack_gap_field(ctx, d_counts, g.nx, g.ny, g.nz, &d_seed.p));
        g.cs_mask = (1u << PCR_GAP_SHIFT) - 1u;
    }
    HIP_TRY(hipGetLastError());
    // (occupied cells of the final geometry: counted by k_cell_ids above, read back with the one synchronisation at the end)
    const bool nz2_pending = n > 0;
    // ---- halo lists (point targets with a gap field: both share the 28-bit offsets)
    g.halo = (Real)0; g.cs_h = nullptr; g.pts_h = nullptr; g.j_h = nullptr; g.rowocc = nullptr; g.nyw = 0; g.nxb = 0;
    g.lbox = nullptr; g.gbox = nullptr; g.lbox_h = nullptr; g.gbox_h = nullptr;
    g.xq = xorder ? (Real)((double)g.h / (double)(1 << PCR_XQ_BITS)) : (Real)0;
    DevBuf<uint32_t> d_cs_h, d_j_h;
    DevBuf<PtF> d_pts_h;
    int64_t n_h = 0;
    if (sizeof(Real) == 4 && halo_frac > 0 && n > 0 && g.cs_mask != 0xffffffffu) {
        Geom<float> gh;
        memcpy(&gh, &g, sizeof gh);                           // Real == float here
        PCR_TRY(build_halo_lists(ctx, gh, (const PtF *)d_pts.p, n, (const uint32_t *)d_counts.p, halo_frac, &d_cs_h, &d_pts_h, &d_j_h, &n_h));
        if (n_h > 0) { g.halo = (Real)(fmin(halo_frac, 1.0) * (double)g.h); g.cs_h = d_cs_h.p; g.pts_h = d_pts_h.p; g.j_h = d_j_h.p; }
    }
    // (build_halo_lists synchronised for its total when it ran; otherwise once here: the index is complete when we return)
    if (nz2_pending) HIP_TRY(hipMemcpyAsync(h_nz.data(), d_nz.p, sizeof(unsigned long long) * OCC_WORDS, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (nz2_pending) occupied = (int64_t)occ_total(h_nz.data());
    // success: hand the index over
    g.seed = d_seed.p;
    *geom = g;
    *n_h_out = n_h;
    *cs_h_out = d_cs_h.release();
    *pts_h_out = d_pts_h.release();
    *j_h_out = d_j_h.release();
    *seed_out = d_seed.release();
    *occupied_out = occupied;
    if (heavy_out) *heavy_out = heavy;
    *cell_start_out = d_counts.release();
    *pts_out = d_pts.release();
    return PCR_OK;
}

// row-occupancy bitmap (Geom::rowocc): one thread per word = 64 rows x one 16-cell x-block
__global__ void __launch_bounds__(256) k_row_occ(const uint32_t *__restrict__ cs, uint32_t mask, int nx, int ny, int nz, int nyw, int nxb,
                                                 unsigned long long *out) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= (int64_t)nz * nyw * nxb) return;
    const int xb = (int)(w % nxb), wy = (int)((w / nxb) % nyw), z = (int)(w / ((int64_t)nxb * nyw));
    const int x0 = xb * 16, x1 = min(x0 + 16, nx);
    unsigned long long bits = 0;
    for (int b = 0; b < 64; ++b) {
        const int y = wy * 64 + b;
        if (y >= ny) break;
        const size_t row = ((size_t)z * ny + y) * (size_t)nx;
        if ((cs[row + x1] & mask) != (cs[row + x0] & mask)) bits |= 1ull << b;
    }
    out[w] = bits;
}

template <typename Real>
static pcr_status make_row_occ(pcr_context *ctx, const uint32_t *cs, Geom<Real> *g, unsigned long long **out) {
    g->rowocc = nullptr; g->nyw = (g->ny + 63) / 64; g->nxb = (g->nx + 15) / 16;
    const int64_t words = (int64_t)g->nz * g->nyw * g->nxb;
    if (words <= 0) return PCR_OK;
    DevBuf<unsigned long long> buf;
    HIP_TRY(buf.alloc_exact((size_t)words));
    hipLaunchKernelGGL(k_row_occ, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, ctx->stream, cs, g->cs_mask, g->nx, g->ny, g->nz,
                       g->nyw, g->nxb, buf.p);
    HIP_TRY(hipGetLastError());
    *out = buf.release();             // (not synchronised: pcr_voxel_target_finish does, once, behind the permutations)
    g->rowocc = *out;
    return PCR_OK;
}

// leaf / group boxes (Geom::lbox, gbox): the box of every 8 and of every 64 consecutive records of a point array (its sentinel
// records excluded), ONE 16-byte record each: the min corner exactly, the extents as 10-bit counts of qe = cell / 256 rounded up
// plus one, 1023 = unbounded (nn_device.h: box_d2).  One thread per leaf; the 8 leaves of a group sit in 8 neighbouring lanes.
__device__ __forceinline__ uint32_t box_extent_q(float lo, float hi, float inv_qe, float extra) {
    // extra = 1 + the grid's rounding slack in counts: the decoded max corner fma(count, qe, lo) errs by an ulp of the COORDINATE,
    // which at |p| ~ 1e5 m exceeds qe; the slack (16 ulp of the largest coordinate) always covers it
    const float c = ceilf((hi - lo) * inv_qe) + extra;
    return c >= 1023.f || !(c == c) ? 1023u : (uint32_t)c;
}
__global__ void __launch_bounds__(256) k_leaf_boxes(const PtF *__restrict__ pts, int64_t n, float qe, float extra, float4 *__restrict__ lbox,
                                                    float4 *__restrict__ gbox) {
    const int64_t L = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nleaf = (n + 7) >> 3;
    const float inf = __builtin_inff();
    const float inv_qe = 1.f / qe;
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    if (L < nleaf) {
        const int64_t j1 = min((L << 3) + 8, n);
        for (int64_t j = L << 3; j < j1; ++j) {
            const PtF p = pts[j];
            lo[0] = fminf(lo[0], p.x); hi[0] = fmaxf(hi[0], p.x);
            lo[1] = fminf(lo[1], p.y); hi[1] = fmaxf(hi[1], p.y);
            lo[2] = fminf(lo[2], p.z); hi[2] = fmaxf(hi[2], p.z);
        }
        const uint32_t w = box_extent_q(lo[0], hi[0], inv_qe, extra) | box_extent_q(lo[1], hi[1], inv_qe, extra) << 10 | box_extent_q(lo[2], hi[2], inv_qe, extra) << 20;
        lbox[L] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(w));
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
        }
    }
    if ((threadIdx.x & 7) == 0 && L < nleaf) {
        const uint32_t w = box_extent_q(lo[0], hi[0], inv_qe, extra) | box_extent_q(lo[1], hi[1], inv_qe, extra) << 10 | box_extent_q(lo[2], hi[2], inv_qe, extra) << 20;
        gbox[L >> 3] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(w));
    }
}

// boxes over `n` records (+ a few records of padding: the batched scan clamps its indices, nothing reads beyond the last box)
static pcr_status make_leaf_boxes(pcr_context *ctx, const PtF *pts, int64_t n, float cell, float slack, float4 **lbox_out, float4 **gbox_out) {
    *lbox_out = nullptr; *gbox_out = nullptr;
    if (n <= 0) return PCR_OK;
    const int64_t nleaf = (n + 7) >> 3, ngroup = (nleaf + 7) >> 3;
    DevBuf<float4> lb, gb;
    HIP_TRY(lb.alloc_exact((size_t)(nleaf + 8)));
    HIP_TRY(gb.alloc_exact((size_t)(ngroup + 8)));
    hipLaunchKernelGGL(k_leaf_boxes, dim3((unsigned)((nleaf + 255) / 256)), dim3(256), 0, ctx->stream, pts, n, cell * 0.00390625f,
                       1.f + ceilf(slack / (cell * 0.00390625f)), lb.p, gb.p);
    HIP_TRY(hipGetLastError());
    *lbox_out = lb.release(); *gbox_out = gb.release();
    return PCR_OK;
}

// population of the occupied cells: counts of cells by population (exact up to 1023, then one bin per power of two) + the maximum
__global__ void __launch_bounds__(256) k_cell_pop(const uint32_t *__restrict__ cs, uint32_t mask, int64_t ncells, unsigned long long *hist,
                                                  unsigned long long *pmax) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncells) return;
    const uint32_t pop = (cs[c + 1] & mask) - (cs[c] & mask);
    if (pop == 0) return;
    const int bin = pop < 1024u ? (int)pop : 1024 + (31 - __builtin_clz(pop));
    atomicAdd(&hist[bin], 1ull);
    atomicMax(pmax, (unsigned long long)pop);
}

pcr_status pcr_cell_population(pcr_context *ctx, pcr_target *t) {
    if (t->pop_max > 0 || t->n <= 0) return PCR_OK;
    const int64_t ncells = t->is_voxel ? (int64_t)t->gd.nx * t->gd.ny * t->gd.nz : (int64_t)t->gf.nx * t->gf.ny * t->gf.nz;
    const uint32_t mask = t->is_voxel ? t->gd.cs_mask : t->gf.cs_mask;
    DevBuf<unsigned long long> d;
    const int bins = 1024 + 32 + 1;
    HIP_TRY(d.alloc((size_t)bins));
    HIP_TRY(hipMemsetAsync(d.p, 0, sizeof(unsigned long long) * bins, ctx->stream));
    hipLaunchKernelGGL(k_cell_pop, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t *)t->cell_start, mask,
                       ncells, d.p, d.p + (bins - 1));
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> h((size_t)bins);
    HIP_TRY(hipMemcpyAsync(h.data(), d.p, sizeof(unsigned long long) * bins, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    t->pop_max = (int64_t)h[(size_t)bins - 1];
    unsigned long long total = 0, run = 0;
    for (int b = 0; b < bins - 1; ++b) total += h[(size_t)b];
    t->pop_p99 = t->pop_max;
    for (int b = 0; b < bins - 1; ++b) {
        run += h[(size_t)b];
        if ((double)run >= 0.99 * (double)total) { t->pop_p99 = b < 1024 ? b : (int64_t)1 << (b - 1024 + 1); break; }   // (upper edge of a log bin)
    }
    if (t->pop_p99 > t->pop_max) t->pop_p99 = t->pop_max;
    return PCR_OK;
}

pcr_status pcr_count_nonfinite(pcr_context *ctx, const void *d_xyz, int is_f64, int64_t n, int64_t *count, float *lo_out, float *hi_out) {
    float lo[3], hi[3];
    pcr_status s = is_f64 ? device_bbox<double>(ctx, (const double *)d_xyz, n, lo, hi, count)
                          : device_bbox<float>(ctx, (const float *)d_xyz, n, lo, hi, count);
    for (int a = 0; a < 3; ++a) {
        if (lo_out) lo_out[a] = lo[a];
        if (hi_out) hi_out[a] = hi[a];
    }
    return s;
}

pcr_status pcr_build_point_grid(pcr_context *ctx, const float *d_xyz, int64_t n, float cell_hint, pcr_target *t, bool use_env, double halo_default) {
    double h = cell_hint > 0 ? (double)cell_hint : 0.5;
    const char *env = use_env ? getenv("PCR_GRID_CELL") : nullptr;
    bool auto_h = !(cell_hint > 0);
    if (env && atof(env) > 0) { h = atof(env); auto_h = false; }
    // halo margin as a fraction of the cell edge (PCR_HALO; 0 = no extended lists).  0.1: ~1.7 copies per
    // point, ring 0 certifies every query whose match is closer than 0.1 h + its distance to the cell wall
    // Measured (MI355X): 1.06 M points, converged poses 70 -> 57 us and 84 -> 60 us, first poses +1 %; at 1e8
    // points (+2.8 GB, nothing cache-resident) +3 %: on by default up to 2^24 points.
    double halo = n <= ((int64_t)1 << 24) ? halo_default : 0.0;
    const char *he = getenv("PCR_HALO");
    if (he && *he) halo = atof(he);
    bool heavy = false;
    PCR_TRY((build_grid<float, float, PtF>(ctx, d_xyz, n, h, auto_h, &t->gf, &t->cell_start, &t->cell_seed, &t->pts, &t->occupied,
                                           halo, &t->cs_h, &t->pts_h, &t->j_h, &t->n_h, use_env ? &heavy : nullptr)));
    t->heavy = heavy;
    if (heavy) {                  // leaf / group boxes over the cell-sorted points and over the extended lists
        PCR_TRY(make_leaf_boxes(ctx, t->pts, n, t->gf.h, t->gf.slack, &t->lbox, &t->gbox));
        t->gf.lbox = t->lbox; t->gf.gbox = t->gbox;
        if (t->pts_h) {
            PCR_TRY(make_leaf_boxes(ctx, t->pts_h, t->n_h, t->gf.h, t->gf.slack, &t->lbox_h, &t->gbox_h));
            t->gf.lbox_h = t->lbox_h; t->gf.gbox_h = t->gbox_h;
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return PCR_OK;       // (no row-occupancy bitmap for point targets: measured slower, nn_device.h)
}

// The DEEPER sets of extended lists of a point target (mid: halo PCR_HALO2_FRAC x cell, far: PCR_HALO3_FRAC), built by the first
// pass that gets their cost back (pass.hip: pass_setup); a pass picks one of the sets by how far the scan moved.
pcr_status pcr_build_deep_lists(pcr_context *ctx, pcr_target *t) {
    if (t->is_voxel || !t->cs_h || t->n <= 0 || t->deep[0].cs) return PCR_OK;
    // (an opt-out and a size cap.  PCR_DEEP_LISTS=0 never builds a set; the estimate -- copies per point scale
    // with (1 + 2 margin)^2 on a surface: 2.3 at 0.25 cell and 3.2 at 0.35 where the first set holds n_h / n at 0.1 -- of a set
    // and the sets before it must fit PCR_DEEP_LISTS_MB, default 1/16 of the device's free memory, or the target does without it)
    const char *de = getenv("PCR_DEEP_LISTS");
    if (de && atoi(de) == 0) return PCR_OK;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
    const char *mb = getenv("PCR_DEEP_LISTS_MB");
    const double budget = mb && *mb ? atof(mb) * 1048576.0 : (double)free_b / 16.0;
    const double frac[PCR_DEEP_SETS] = {PCR_HALO2_FRAC, PCR_HALO3_FRAC};
    double used = 0.0;
    // (a heavy target gets the mid set only: the far set's depth was measured on clouds of even density, and on a LiDAR sweep
    // it lost -- plane_lidar 0.243 -> 0.248 ms per step)
    for (int k = 0; k < (t->heavy ? 1 : PCR_DEEP_SETS); ++k) {
        const double grow = (1.0 + 2.0 * frac[k]) * (1.0 + 2.0 * frac[k]) / (1.2 * 1.2);
        used += (double)(t->n_h > 0 ? t->n_h : t->n) * grow * 20.0 + 4.0 * ((double)t->gf.nx * t->gf.ny * t->gf.nz);
        if (used > budget) break;
        DevBuf<uint32_t> cs_h, j_h;
        DevBuf<PtF> pts_h;
        int64_t n_h = 0;
        PCR_TRY(build_halo_lists(ctx, t->gf, t->pts, t->n, t->cell_start, frac[k], &cs_h, &pts_h, &j_h, &n_h));
        if (n_h <= 0) break;          // (the copies do not fit the 28-bit offsets: nor would a deeper set's)
        pcr_target::ListSet &d = t->deep[k];
        d.halo = (float)(frac[k] * (double)t->gf.h);
        d.n = n_h;
        d.cs = cs_h.release(); d.pts = pts_h.release(); d.j = j_h.release();
        if (t->heavy) {
            PCR_TRY(make_leaf_boxes(ctx, d.pts, n_h, t->gf.h, t->gf.slack, &d.lbox, &d.gbox));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
    }
    return PCR_OK;
}

pcr_status pcr_build_centroid_grid(pcr_context *ctx, const double *d_mean, int64_t n, double cell, pcr_target *t) {
    uint32_t *cs_h = nullptr, *j_h = nullptr; PtF *pts_h = nullptr; int64_t n_h = 0;
    PCR_TRY((build_grid<double, double, PtD>(ctx, d_mean, n, cell, false, &t->gd, &t->cell_start, &t->cell_seed, &t->means, &t->occupied,
                                             0.0, &cs_h, &pts_h, &j_h, &n_h)));
    const char *oe = getenv("PCR_ROW_OCC");
    if (n > 0 && !(oe && atoi(oe) == 0)) PCR_TRY(make_row_occ<double>(ctx, t->cell_start, &t->gd, &t->rowocc));
    return PCR_OK;
}

// ---- float32 filter of a centroid search (pass_device.h: nn_point_filter) ----------------------
__global__ void __launch_bounds__(256) k_means_to_f32(const PtD *__restrict__ means, int64_t n, float *__restrict__ xyz) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const PtD m = means[j];
    xyz[3 * j] = (float)m.x; xyz[3 * j + 1] = (float)m.y; xyz[3 * j + 2] = (float)m.z;     // round to nearest
}

// A point index over the float32-rounded centroids, built from the CELL-SORTED array `means`: the "original index" a
// float32 search returns is then the index the reduce kernels gather with.  Only when rounding moves a centroid by
// less than 1 % of a cell (coordinates below ~1e5 m for 1 m cells): beyond that the filter would rarely certify.
pcr_status pcr_build_centroid_filter(pcr_context *ctx, pcr_target *t) {
    if (t->n <= 0 || !ctx->vox_filter) return PCR_OK;
    const Geom<double> &g = t->gd;
    double maxabs = 0;
    const double lo[3] = {g.ox, g.oy, g.oz}, ext[3] = {g.nx * g.h, g.ny * g.h, g.nz * g.h};
    for (int i = 0; i < 3; ++i) {
        maxabs = fmax(maxabs, fabs(lo[i]));
        maxabs = fmax(maxabs, fabs(lo[i] + ext[i]));
    }
    const double band = gn_filter_band(maxabs);
    if (!(band <= 0.01 * g.h)) return PCR_OK;
    DevBuf<float> xyz;
    HIP_TRY(xyz.alloc((size_t)t->n * 3));
    hipLaunchKernelGGL(k_means_to_f32, dim3((unsigned)((t->n + 255) / 256)), dim3(256), 0, ctx->stream, t->means, t->n, xyz.p);
    HIP_TRY(hipGetLastError());
    pcr_target *f = new pcr_target();
    f->ctx = ctx; f->n = t->n;
    t->filter = f;                                   // (owned by t from here on: freed with it, also on the error path)
    // The filter index takes DEEPER extended lists than a point target (0.4 cell against 0.1): a query sits 0.2-0.5 voxel from its
    // centroid, i.e. a good part of a (two-voxel) cell, at EVERY pose, and the lists of a few hundred thousand centroids stay in
    // the caches whatever their depth.  Search us per 6-pose trajectory, margin 0.1 / 0.25 / 0.4 / 0.5 / 0.6 / 0.8 / 1.0 cell:
    // vplane_10m 3699 / 3643 / 3382 / 3473 / 3397 / 3683 / 3466, ndt_10m 2559 / 2434 / 2252 / 2244 / 2207 / 2590 / 2649.
    static const double halo_env = getenv("PCR_FILTER_HALO") ? atof(getenv("PCR_FILTER_HALO")) : 0.0;     // (developer: sweep)
    PCR_TRY(pcr_build_point_grid(ctx, xyz.p, t->n, (float)g.h, f, false, halo_env > 0.0 ? halo_env : 0.4));
    t->filter_band = band;
    return PCR_OK;
}

// ---- row permutations into cell-sorted order -------------------------------------------------
__global__ void __launch_bounds__(256) k_perm_normals(const float *__restrict__ in, int64_t n,
                                                      const PtF *__restrict__ pts, PtN *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const PtF p = pts[j];
    const size_t i = __float_as_uint(p.w);
    PtN r;
    r.x = p.x; r.y = p.y; r.z = p.z; r.orig = (uint32_t)i;
    r.nx = in[3 * i]; r.ny = in[3 * i + 1]; r.nz = in[3 * i + 2]; r.pad = 0;
    out[j] = r;
}

// caller-order (N,3) normals -> cell-sorted {point, normal} records
pcr_status pcr_permute_normals(pcr_context *ctx, const float *d_in, int64_t n, const PtF *pts, PtN *out) {
    if (n == 0) return PCR_OK;
    hipLaunchKernelGGL(k_perm_normals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, pts, out);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

// ---- quirk Q6: the float64 coordinates of a point target, in the index's order --------------------------------
// out[j] = float64 coordinates of the point stored at cell-sorted position j (w = its original index, as in the centroid
// arrays); dev = the largest distance between a point's float64 position and the float32 record the index was built on
// (positive doubles order like their bit patterns: one 64-bit atomicMax)
__global__ void __launch_bounds__(256) k_perm_pts64(const double *__restrict__ xyz64, int64_t n, const PtF *__restrict__ pts,
                                                    PtD *out, unsigned long long *dev) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double d = 0.0;
    if (j < n) {
        const PtF p = pts[j];
        const size_t i = __float_as_uint(p.w);
        const double x = xyz64[3 * i], y = xyz64[3 * i + 1], z = xyz64[3 * i + 2];
        out[j] = make_double4(x, y, z, __longlong_as_double((long long)i));
        const double ex = x - (double)p.x, ey = y - (double)p.y, ez = z - (double)p.z;
        d = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
        if (!(d >= 0.0)) d = __longlong_as_double(0x7ff0000000000000LL);      // NaN: refuse (the caller checks for inf)
    }
    for (int off = 32; off >= 1; off >>= 1) d = fmax(d, __shfl_xor(d, off, 64));
    // (a wave only adds to the queue on one word when it can raise it: the maximum is monotone, a stale read costs an atomic)
    if ((threadIdx.x & 63) == 0 && d > 0.0 &&
        (unsigned long long)__double_as_longlong(d) > __hip_atomic_load(dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(dev, (unsigned long long)__double_as_longlong(d));
}

pcr_status pcr_attach_points_f64(pcr_context *ctx, pcr_target *t, const double *d_xyz64) {
    const int64_t n = t->n;
    DevBuf<PtD> out;
    HIP_TRY(out.alloc_exact((size_t)(n > 0 ? n : 1) + PCR_PTS_PAD));
    {   // sentinel records behind the last point (nn_scan_range over-reads a batch): +inf coordinates, index ~0
        PtD pad[PCR_PTS_PAD];
        for (int i = 0; i < PCR_PTS_PAD; ++i) {
            pad[i].x = pad[i].y = pad[i].z = INFINITY;
            const long long m = 0xffffffffLL; memcpy(&pad[i].w, &m, 8);
        }
        HIP_TRY(hipMemcpyAsync(out.p + (size_t)n, pad, sizeof pad, hipMemcpyHostToDevice, ctx->stream));
    }
    DevBuf<unsigned long long> dev;
    HIP_TRY(dev.alloc(1));
    HIP_TRY(hipMemsetAsync(dev.p, 0, sizeof(unsigned long long), ctx->stream));
    if (n > 0) {
        hipLaunchKernelGGL(k_perm_pts64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_xyz64, n,
                           (const PtF *)t->pts, out.p, dev.p);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, dev.p, sizeof bits, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double band;
    memcpy(&band, &bits, 8);
    const Geom<float> &gf = t->gf;
    if (!(band <= 0.25 * (double)gf.h)) {
        // (not an argument error.  Coordinates of UTM magnitude have a float32 ulp of 0.03-0.5 m: rounding moves the
        // points by more than the float32 index can bound with a usable band.  The target keeps its float32 index -- the
        // caller may go on with the float32 search, as the previous revision did -- and says so.)
        pcr_set_error("float64 search coordinates not attached: rounding to float32 moves a point by %g m (cell %g m); "
                      "the target keeps its float32 search", band, (double)gf.h);
        return PCR_ERR_UNSUPPORTED;
    }
    pcr_persist_free(ctx, t->pts64);
    t->pts64 = out.release();
    t->band64 = band * 1.01 + 1e-30;
    Geom<double> &g = t->gq;
    g.ox = (double)gf.ox; g.oy = (double)gf.oy; g.oz = (double)gf.oz;
    g.h = (double)gf.h; g.inv_h = (double)gf.inv_h;
    g.nx = gf.nx; g.ny = gf.ny; g.nz = gf.nz;
    // the cells were assigned to the float32 records in float32 arithmetic (gf.slack covers that); a point's float64
    // position lies within band64 of its record
    g.slack = (double)gf.slack * 2.0 + t->band64;
    g.cs_mask = gf.cs_mask;
    g.seed = nullptr; g.halo = 0; g.cs_h = nullptr; g.pts_h = nullptr; g.j_h = nullptr; g.rowocc = nullptr; g.nyw = 0; g.nxb = 0;
    g.lbox = nullptr; g.gbox = nullptr; g.lbox_h = nullptr; g.gbox_h = nullptr;
    g.xq = 0;                      // (the float64 side is searched by nn_scan_range: correct on any order inside a cell)
    return PCR_OK;
}

struct ColSel { int c[9]; int n; };
__global__ void __launch_bounds__(256) k_perm_f64(const double *__restrict__ in, int64_t n, int stride, ColSel sel,
                                                  const PtD *__restrict__ means, double *out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t i = key_index(means[j]);
    for (int k = 0; k < sel.n; ++k) out[(size_t)j * sel.n + k] = in[i * stride + sel.c[k]];
}

pcr_status pcr_permute_rows_f64(pcr_context *ctx, const double *d_in, int64_t n, int in_stride, const int *cols,
                                int ncols, const PtD *means, double *out) {
    if (n == 0) return PCR_OK;
    ColSel sel;
    sel.n = ncols;
    for (int k = 0; k < ncols; ++k) sel.c[k] = cols[k];
    hipLaunchKernelGGL(k_perm_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_in, n, in_stride, sel,
                       means, out);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

// ---- scan: Morton order, SoA ------------------------------------------------------------------
__device__ __forceinline__ unsigned long long spread21(unsigned long long v) {
    v &= 0x1fffffULL;
    v = (v | (v << 32)) & 0x1f00000000ffffULL;
    v = (v | (v << 16)) & 0x1f0000ff0000ffULL;
    v = (v | (v << 8)) & 0x100f00f00f00f00fULL;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ULL;
    v = (v | (v << 2)) & 0x1249249249249249ULL;
    return v;
}

// Morton keys of `bits` bits per axis over the scan's box, which k_bbox left ON THE DEVICE (round 5: the scan set-up used to
// synchronise for it before this kernel could be launched).
__global__ void __launch_bounds__(256) k_morton(const float *__restrict__ xyz, int64_t n, const unsigned *__restrict__ box, int bits,
                                                unsigned long long *keys, uint32_t *idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool any = (int64_t)box[6] < n;
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned ul = box[a], uh = box[3 + a];
        lo[a] = any ? __uint_as_float((ul & 0x80000000u) ? (ul & 0x7fffffffu) : ~ul) : 0.f;
        hi[a] = any ? __uint_as_float((uh & 0x80000000u) ? (uh & 0x7fffffffu) : ~uh) : 0.f;
    }
    float ext = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    if (!(ext > 0)) ext = 1.f;
    const float lim = (float)((1u << bits) - 1u);
    const float scale = lim / ext;
    const unsigned long long qx = (unsigned long long)fminf(fmaxf((xyz[3 * i] - lo[0]) * scale, 0.f), lim);
    const unsigned long long qy = (unsigned long long)fminf(fmaxf((xyz[3 * i + 1] - lo[1]) * scale, 0.f), lim);
    const unsigned long long qz = (unsigned long long)fminf(fmaxf((xyz[3 * i + 2] - lo[2]) * scale, 0.f), lim);
    keys[i] = spread21(qx) | (spread21(qy) << 1) | (spread21(qz) << 2);
    idx[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_to_soa(const float *__restrict__ xyz, const uint32_t *__restrict__ order, int64_t n,
                                                float *x, float *y, float *z) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t i = order ? order[j] : (size_t)j;
    x[j] = xyz[3 * i]; y[j] = xyz[3 * i + 1]; z[j] = xyz[3 * i + 2];
}

pcr_status pcr_sort_scan(pcr_context *ctx, const float *d_xyz, int64_t n, unsigned flags, pcr_scan *s) {
    PCR_REQUIRE(n < ((int64_t)1 << 31), "at most 2^31-1 points per scan shard");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t nn = (size_t)(n > 0 ? n : 1);
    s->ctx = ctx;
    HIP_TRY(pcr_scan_alloc(s, (void **)&s->x, 4 * nn)); HIP_TRY(pcr_scan_alloc(s, (void **)&s->y, 4 * nn)); HIP_TRY(pcr_scan_alloc(s, (void **)&s->z, 4 * nn));
    s->n = n;
    if (n == 0) return PCR_OK;
    const unsigned nb = (unsigned)((n + 255) / 256);
    DevBuf<unsigned> d_box;
    HIP_TRY(d_box.alloc(BBOX_WORDS));
    PCR_TRY(device_bbox_launch<float>(ctx, d_xyz, n, d_box.p));
    DevBuf<unsigned long long> k1, k2;
    DevBuf<uint32_t> i1, i2;
    if (flags & PCR_FLAG_NO_SCAN_SORT) {
        hipLaunchKernelGGL(k_to_soa, dim3(nb), dim3(256), 0, ctx->stream, d_xyz, (const uint32_t *)nullptr, n, s->x, s->y, s->z);
    } else {
        // Key width: a Morton cell 8x finer than the point spacing of a SURFACE filling the box (ext / sqrt(n); any real cloud is
        // sparser) already holds one point at most, and points of one cell keep their order (stable sort): 13 bits per axis
        // at 1.06 M points, 16 at 1e8 -- 5 / 6 radix passes instead of the 8 that 21 bits per axis take (25 us each per 1 M).
        int bits = (int)ceil(2.5 + 0.5 * log2((double)n));
        bits = bits < 10 ? 10 : (bits > 21 ? 21 : bits);
        const char *be = getenv("PCR_MORTON_BITS");
        if (be && atoi(be) >= 1 && atoi(be) <= 21) bits = atoi(be);
        HIP_TRY(k1.alloc(nn)); HIP_TRY(k2.alloc(nn));
        HIP_TRY(i1.alloc(nn));
        // PCR_FLAG_KEEP_ORDER: the sorted permutation lands in a block the scan keeps instead of a temporary
        uint32_t *perm = nullptr;
        if (flags & PCR_FLAG_KEEP_ORDER) { HIP_TRY(pcr_scan_alloc(s, (void **)&s->order, 4 * nn)); perm = s->order; }
        else { HIP_TRY(i2.alloc(nn)); perm = i2.p; }
        hipLaunchKernelGGL(k_morton, dim3(nb), dim3(256), 0, ctx->stream, d_xyz, n, (const unsigned *)d_box.p, bits, k1.p, i1.p);
        PCR_TRY(sort_pairs<unsigned long long>(ctx, k1, k2, i1, perm, n, 3 * bits));
        hipLaunchKernelGGL(k_to_soa, dim3(nb), dim3(256), 0, ctx->stream, d_xyz, (const uint32_t *)perm, n, s->x, s->y, s->z);
        s->sorted = true;
    }
    HIP_TRY(hipGetLastError());
    unsigned hb[7];
    HIP_TRY(hipMemcpyAsync(hb, d_box.p, sizeof hb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));             // (the one synchronisation of a scan set-up)
    float lo[3], hi[3];
    bbox_decode(hb, n, lo, hi);
    for (int i = 0; i < 3; ++i) {          // (certified reuse: where the scan is, to judge how far a pose change moves it)
        s->bb_c[i] = 0.5f * (lo[i] + hi[i]); s->bb_e[i] = 0.5f * (hi[i] - lo[i]);
        if (!(fabsf(s->bb_c[i]) < 1e30f) || !(s->bb_e[i] < 1e30f)) { s->bb_c[i] = 0.f; s->bb_e[i] = 1e30f; }
    }
    return PCR_OK;
}
