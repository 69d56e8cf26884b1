/*
 * pcr.h -- C ABI of the MI355X-native point-cloud registration core (libpcr_hip.so).
 *
 * The reference (scomup/point-cloud-registration) is pure Python/NumPy and has no FFI of
 * its own; its seams are Python duck types.  This header is the
 * drop-in boundary a maintainer would bind with ctypes from inside the reference's classes
 * (INTEGRATION.md shows the stub).  Every entry point names the reference interface it
 * replaces (paths relative to /root/reference/point_cloud_registration/).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, opaque handles; no C++/torch types.
 *   - every function returns a pcr_status (0 = PCR_OK); pcr_last_error() gives the message
 *     of the last failure on the calling thread.
 *   - host buffers are caller-owned, read (or written) during the call and never retained;
 *     *_device variants take device pointers valid on the context's GPU.
 *   - one context = one GPU = one HIP stream; handles are not thread-safe; calls that
 *     return data to the host are synchronous on return.
 *   - one process drives one GPU; multi-GPU = one process per GPU joined with
 *     pcr_comm_init (RCCL over xGMI), the scan sharded across ranks.
 *   - point clouds are float32 (N,3) row-major unless stated.  4x4 transforms are float64
 *     row-major.  The normal equations come back as out[29]:
 *       out[0..20]  upper triangle of H (6x6) row-major: 00 01 02 03 04 05 11 12 .. 55
 *       out[21..26] g,  out[27] e2,  out[28] number of correspondences that passed the gate
 */
#ifndef PCR_H
#define PCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_API __attribute__((visibility("default")))

/* Bumped whenever an existing entry point changes its argument layout or the size of an array it writes
 * (4: PCR_K_COUNT 5 -> 6, i.e. pcr_profile_read writes six entries).  A binding compares it with
 * pcr_abi_version() of the library it loaded before calling anything else.                                   */
#define PCR_ABI_VERSION 5

typedef int pcr_status;
enum {
    PCR_OK = 0,
    PCR_ERR_INVALID = -1,     /* bad argument */
    PCR_ERR_HIP = -2,         /* HIP runtime failure (message has the HIP error string) */
    PCR_ERR_NO_TARGET = -3,   /* target lacks what the requested kind needs (normals / icov) */
    PCR_ERR_COMM = -4,        /* RCCL failure or communicator misuse */
    PCR_ERR_SINGULAR = -5,    /* pcr_align: H singular (zero correspondences); quirk Q7 */
    PCR_ERR_NOMEM = -6,
    PCR_ERR_UNSUPPORTED = -7  /* an optional fast path is not available for this input (the target stays usable as it was):
                                 pcr_target_points_set_f64 on coordinates float32 cannot resolve */
};

/* registration kinds: which reference class's calc_H_g_e2 is evaluated */
enum {
    PCR_ICP = 0,      /* icp.py:24-57 */
    PCR_PLANE = 1,    /* plane_icp.py:30-69 */
    PCR_VPLANE = 2,   /* voxelized_plane_icp.py:23-64 */
    PCR_NDT = 3       /* ndt.py:24-57 */
};

/* compat flags */
enum {
    PCR_FLAG_ICP_RR_QUIRK = 1u,   /* reproduce icp.py:53-54: g[3:] = sum p x (R r) (quirk Q1); default */
    PCR_FLAG_NO_SCAN_SORT = 2u,   /* pcr_scan_create: keep the caller's point order on the device */
    PCR_FLAG_LOCAL_ONLY = 4u,     /* pcr_linearize / pcr_align: this rank's sums only, no all-reduce even when a
                                     communicator is attached to the context (the collective is a per-call decision) */
    PCR_FLAG_HOST_LOOP = 8u,      /* pcr_align: host-driven loop (one pcr_linearize + host solve per iteration)
                                     instead of the device-resident one; same arithmetic, same bits */
    PCR_FLAG_DEVICE_LOOP = 16u,   /* pcr_align: device-resident loop even where the library would pick the host-driven
                                     one (small scans on one GPU, where it is ~8 % faster: 37.6 vs 41.0 us per iteration
                                     on a 100 k-point scan) */
    PCR_FLAG_KEEP_ORDER = 32u     /* pcr_scan_create: a Morton-sorted scan remembers the caller's point order (4 bytes per
                                     point), which pcr_linearize_rows / _weighted / pcr_scan_coreset need */
};

typedef struct pcr_context pcr_context;
typedef struct pcr_target pcr_target;
typedef struct pcr_scan pcr_scan;
typedef struct pcr_group pcr_group;                 /* single-process multi-device: one context + host thread per member */
typedef struct pcr_group_target pcr_group_target;   /* the same target index on every member */
typedef struct pcr_group_scan pcr_group_scan;       /* a scan cut into one contiguous shard per member */

/* ---- library / context ------------------------------------------------------------ */
PCR_API const char *pcr_last_error(void);
PCR_API const char *pcr_version(void);
PCR_API int pcr_abi_version(void);
PCR_API pcr_status pcr_device_count(int *count);
PCR_API pcr_status pcr_context_create(int device, pcr_context **out);
PCR_API pcr_status pcr_context_destroy(pcr_context *ctx);
/* the context's HIP stream (hipStream_t as void*), for callers that order their own work */
PCR_API pcr_status pcr_context_stream(pcr_context *ctx, void **stream);
PCR_API pcr_status pcr_context_synchronize(pcr_context *ctx);
/* Destroying targets and scans does not return their device memory to the HIP allocator: the blocks go to a
 * per-context cache (hipFree synchronises the device, ~60 us each) and are handed out again to later targets /
 * scans of a similar size.  At most PCR_CACHE_LIMIT_MB (default 1024) of idle blocks are kept; they are invisible to
 * other allocators of the process (torch) until pcr_context_trim, which synchronises the stream and hipFree()s all
 * of them (released_bytes may be NULL), or an allocation failure inside the library, which does the same.        */
PCR_API pcr_status pcr_context_trim(pcr_context *ctx, uint64_t *released_bytes);

/* ---- multi-GPU: one process per GPU, RCCL all-reduce of the 29 doubles per iteration ----
 * No reference counterpart (the reference is single-process).  Rank 0 obtains an id with
 * pcr_comm_unique_id and distributes the 128 bytes out of band (bench.py uses
 * torch.distributed); every rank then calls pcr_comm_init.  After that pcr_linearize /
 * pcr_align return the SUM over all ranks' scan shards, unless the call carries
 * PCR_FLAG_LOCAL_ONLY (no collective is issued then; every rank of the communicator must
 * make the same choice for a given call).                                                */
PCR_API pcr_status pcr_comm_unique_id(void *id128);
PCR_API pcr_status pcr_comm_init(pcr_context *ctx, const void *id128, int nranks, int rank);
PCR_API pcr_status pcr_comm_destroy(pcr_context *ctx);
/* The same exchange WITHOUT a collective library in the loop (opt-in; RCCL stays the default): every rank exports a block of
 * slots (pcr_comm_p2p_export -> 64 bytes = a hipIpcMemHandle_t, distributed out of band like the RCCL id), maps its peers'
 * (pcr_comm_p2p_attach: handles = nranks x 64 bytes in rank order, at most 8 ranks), and a one-wave kernel between fold and
 * hand-off stores the 29 doubles + a sequence word into every rank's block, waits for everybody's words in its own and sums
 * the slots in rank order (bit-identical sums on every rank).  Exercised with two processes on one GPU; not yet on xGMI.
 * pcr_comm_p2p_failed reports whether an exchange gave up waiting for a peer (its sums are NaN then).                   */
PCR_API pcr_status pcr_comm_p2p_export(pcr_context *ctx, void *handle64);
PCR_API pcr_status pcr_comm_p2p_attach(pcr_context *ctx, const void *handles, int nranks, int rank);
PCR_API pcr_status pcr_comm_p2p_failed(pcr_context *ctx, int *failed);
/* 1: this context's slots are fine-grained device memory (coherent across devices while a kernel runs); 0: the coarse-grained
 * fallback, sound only between ranks that share ONE device -- ranks on different devices must agree on another transport
 * (distributed.py does).  PCR_P2P_ALLOW_COARSE=0 makes pcr_comm_p2p_export fail instead of falling back.
 * Since round 6 a timed-out exchange makes pcr_linearize / pcr_align of THAT rank return PCR_ERR_COMM (the device-resident
 * loop stops on it) instead of NaN sums with PCR_OK.                                                                    */
PCR_API pcr_status pcr_comm_p2p_finegrained(pcr_context *ctx, int *finegrained);

/* ---- single-process multi-device groups ("pcr_init(device_ids, n_dev)"; the reference is one process:
 * registration.py:28,71) ----
 * pcr_group_create: one context + one host thread per entry of device_ids (1..8 entries; an id may repeat -- [0, 0] are two
 * contexts on one GPU, which is how a one-GPU box exercises N > 1).  Targets are built once per member (the index is
 * replicated), pcr_group_scan_create cuts the scan into contiguous, balanced shards (member i: points [lo_i, hi_i), the
 * bounds of distributed.shard_bounds), and pcr_group_linearize / pcr_group_align run pcr_linearize / pcr_align on every
 * member at once with the members' 29 sums exchanged through the peer-to-peer kernel above on in-process peer pointers
 * (hipDeviceEnablePeerAccess; no IPC, no RCCL, no torch): every member takes the same Gauss-Newton step on bit-identical
 * sums, and the call returns member 0's copy -- what the SPMD run with the same sharding returns, bit for bit.
 * Calls on one group are serialised by the caller (like every other handle); errors: the first failing member's status,
 * pcr_last_error() names the member.  PCR_FLAG_LOCAL_ONLY is ignored (a group call is the sum over its members).
 * Members must agree: pcr_group_linearize compares every member's 29 sums with member 0's, pcr_group_align every member's
 * status, iteration count, pose and (with a trace wanted) every row of its trace; on any difference the call returns
 * PCR_ERR_COMM and pcr_last_error() names the first member that disagrees.
 * pcr_group_scan_member: member i's shard (borrowed, like pcr_group_target_member): pcr_scan_read_matches / reuse stats of
 * one member; a plain pcr_linearize over it needs PCR_FLAG_LOCAL_ONLY (the member's context is attached to the exchange). */
PCR_API pcr_status pcr_group_create(const int *device_ids, int n, pcr_group **out);
PCR_API pcr_status pcr_group_destroy(pcr_group *g);
PCR_API pcr_status pcr_group_size(pcr_group *g, int *n);
PCR_API pcr_status pcr_group_context(pcr_group *g, int i, pcr_context **ctx);            /* borrowed */
PCR_API pcr_status pcr_group_target_points_create(pcr_group *g, const float *xyz, int64_t n, const float *normals_or_null,
                                                  float cell_hint, pcr_group_target **out);
PCR_API pcr_status pcr_group_target_voxels_create(pcr_group *g, const void *xyz, int xyz_is_f64, int64_t n, double voxel_size,
                                                  int min_points, pcr_group_target **out);
PCR_API pcr_status pcr_group_target_estimate_normals(pcr_group_target *gt, int k, int compat, float *normals_out_or_null);
PCR_API pcr_status pcr_group_target_set_normals(pcr_group_target *gt, const float *normals);
PCR_API pcr_status pcr_group_target_points_set_f64(pcr_group_target *gt, const double *xyz64);
PCR_API pcr_status pcr_group_target_member(pcr_group_target *gt, int i, pcr_target **t);  /* borrowed */
PCR_API pcr_status pcr_group_target_destroy(pcr_group_target *gt);
PCR_API pcr_status pcr_group_scan_create(pcr_group *g, const float *xyz, int64_t n, unsigned flags, pcr_group_scan **out);
PCR_API pcr_status pcr_group_scan_size(pcr_group_scan *gs, int64_t *n);
PCR_API pcr_status pcr_group_scan_member(pcr_group_scan *gs, int i, pcr_scan **s);        /* borrowed */
PCR_API pcr_status pcr_group_scan_destroy(pcr_group_scan *gs);
PCR_API pcr_status pcr_group_linearize(pcr_group_target *gt, pcr_group_scan *gs, int kind, const double T[16], double max_dist,
                                       unsigned flags, double out[29]);
PCR_API pcr_status pcr_group_align(pcr_group_target *gt, pcr_group_scan *gs, int kind, const double T_init[16], int max_iter,
                                   double tol, double max_dist, unsigned flags, double T_out[16], int *iterations,
                                   double *trace_or_null);

/* ---- targets ------------------------------------------------------------------------
 * pcr_target_points_create replaces ICP.set_target (icp.py:17-22) and the KD-tree half of
 * PlaneICP.set_target (plane_icp.py:19-22): float32 copy of the cloud + an exact-NN index
 * (a dense cell grid in HBM instead of pykdtree's KD-tree, kdtree.py:18-21).
 * normals (N,3) float32 may be NULL; cell_hint = 0 picks the cell size automatically.     */
PCR_API pcr_status pcr_target_points_create(pcr_context *ctx, const float *xyz, int64_t n,
                                            const float *normals_or_null, float cell_hint,
                                            pcr_target **out);
PCR_API pcr_status pcr_target_points_create_device(pcr_context *ctx, const float *d_xyz, int64_t n,
                                                   const float *d_normals_or_null, float cell_hint,
                                                   pcr_target **out);
/* caller-supplied normals, PlaneICP.set_target(target, kdree, norm) (plane_icp.py:25-27)  */
PCR_API pcr_status pcr_target_set_normals(pcr_target *t, const float *normals);
/* Quirk Q6 -- PlaneICP.set_target builds its KD-tree on the ORIGINAL array (plane_icp.py:22) and gathers from the float32
 * copy (plane_icp.py:20,44): a float64 target is SEARCHED in float64 (queries up-cast, float64 distances, float64 gate,
 * plane_icp.py:40-41); so is KDTree(float64 data).query (kdtree.py:18-21).  xyz64 = the (N,3) float64 array whose
 * float32 rounding the target was created from; PCR_PLANE passes and pcr_nn_query_f64 then return the float64 search's
 * neighbour (float32 filter search over the index + float64 check, float64 box search for what that cannot separate);
 * PCR_ICP keeps the float32 search (icp.py:19-20 builds its tree on the float32 copy).  +32 bytes per point.          */
PCR_API pcr_status pcr_target_points_set_f64(pcr_target *t, const double *xyz64);
/* k-NN PCA normals, estimate_norm_with_tree (estimate_normals.py:27-87).  compat != 0 keeps
 * the reference's float32 single-pass covariance; normals_out (N,3) may be NULL.           */
PCR_API pcr_status pcr_target_estimate_normals(pcr_target *t, int k, int compat, float *normals_out);
PCR_API pcr_status pcr_target_get_normals(pcr_target *t, float *normals_out);

/* Voxel targets, VPlaneICP.set_target / NDT.set_target (voxelized_plane_icp.py:18-21,
 * ndt.py:18-22) = VoxelGrid.set_points + calc_icov (voxel.py:104-165, 69-102) built on the
 * GPU: hash keys (voxel.py:12-21), group, mean, two-pass covariance, min_points filter,
 * smallest-eigenvector normal, closed-form inverse covariance, and an exact
 * nearest-CENTROID index (voxel.py:165,171-179).  xyz_is_f64 selects the dtype the keys
 * are computed in (float32 clouds divide in float32, as NumPy does).                      */
PCR_API pcr_status pcr_target_voxels_create(pcr_context *ctx, const void *xyz, int xyz_is_f64, int64_t n,
                                            double voxel_size, int min_points, pcr_target **out);
/* the same from precomputed statistics (mean, norm: (n_v,3) float64; icov: (n_v,3,3) float64,
 * norm / icov may be NULL): lets tests inject the oracle's voxels for kernel-only parity.   */
PCR_API pcr_status pcr_target_voxels_create_from_stats(pcr_context *ctx, const double *mean,
                                                       const double *norm_or_null, const double *icov_or_null,
                                                       int64_t n_v, double voxel_size, pcr_target **out);
/* read the voxel statistics back (any pointer may be NULL); *n_v is always written          */
PCR_API pcr_status pcr_target_voxels_get(pcr_target *t, int64_t *n_v, double *mean, double *cov,
                                         double *norm, double *icov, int64_t *counts, int64_t *keys);
PCR_API pcr_status pcr_target_size(pcr_target *t, int64_t *n);
PCR_API pcr_status pcr_target_destroy(pcr_target *t);

/* ---- scan ---------------------------------------------------------------------------
 * Registration.align casts the scan to float32 once (registration.py:83) and reuses it for
 * every iteration: uploaded once, Morton-sorted on the device for gather coherence (the
 * sums do not depend on point order beyond rounding).                                      */
PCR_API pcr_status pcr_scan_create(pcr_context *ctx, const float *xyz, int64_t n, unsigned flags, pcr_scan **out);
PCR_API pcr_status pcr_scan_create_device(pcr_context *ctx, const float *d_xyz, int64_t n, unsigned flags,
                                          pcr_scan **out);
PCR_API pcr_status pcr_scan_size(pcr_scan *s, int64_t *n);
PCR_API pcr_status pcr_scan_destroy(pcr_scan *s);
/* Test / diagnostic seam: the correspondences the last search + reduce pass over this scan left in HBM -- one
 * word per scan point IN THE SCAN'S DEVICE ORDER (Morton-sorted unless PCR_FLAG_NO_SCAN_SORT): the index of the
 * matched record in the target's cell-sorted arrays, 0xffffffff = no correspondence.  Lets a test compare two
 * search kernels match by match (KDTree.query's idx, kdtree.py:18-21 / voxel.py:171-179); fails when the scan
 * has only run the fused small-scan kernel, which keeps its matches in registers.                            */
PCR_API pcr_status pcr_scan_read_matches(pcr_scan *s, uint32_t *out);

/* calc_H_g_e2(cur_T, source) takes the scan as an array on every call and is pure in it (registration.py:55-68):
 * the drop-in class keeps the device copy of the last scan and re-uploads when the CONTENT of the caller's array
 * changed.  pcr_hash64 is the content hash it uses: 64-bit, non-cryptographic, multi-threaded (12.7 MB in ~0.1 ms
 * on the GPU box's host; the value does not depend on the number of threads).                               */
PCR_API pcr_status pcr_hash64(const void *data, uint64_t nbytes, uint64_t *out);
/* LZF, the codec of PCD "DATA binary_compressed" (the real data/B-01.pcd of benchmark/test_data.py:11,24 may be stored that
 * way): decompress in_len bytes into out (capacity out_len; *written = bytes produced; PCR_ERR_INVALID on a corrupt or
 * oversized stream), and a greedy compressor for writers and tests (out_cap >= in_len + in_len / 32 + 8 always suffices).  Host
 * only, no GPU involved.                                                                                                  */
PCR_API pcr_status pcr_lzf_decompress(const void *in, uint64_t in_len, void *out, uint64_t out_len, uint64_t *written);
PCR_API pcr_status pcr_lzf_compress(const void *in, uint64_t in_len, void *out, uint64_t out_cap, uint64_t *written);
/* CPUs the process may actually use: affinity mask capped by the cgroup CPU-bandwidth quota (cpu.max).  The hash
 * pool above is sized from it; a host application should size ITS thread pools (OpenMP, BLAS) the same way -- on a
 * 256-CPU box inside a 16-CPU container, pools sized by the visible CPUs get every thread of the process parked for
 * the rest of a 100 ms scheduler period, the calling thread of pcr_linearize included.          */
PCR_API int pcr_usable_cpus(void);

/* ---- Gauss-Newton coresets (caratheodory.py:62-138; K. Koide, arXiv 2307.02948) ----------------
 * pcr_gn_set = create_gn_set(J, r) (caratheodory.py:118-138): J (n, d) row-major and r (n), each float32 or float64
 * (*_is_f64), 1 <= d <= 12 -> P_out (m, n) float64 row-major, m = d (d + 1) / 2 + d + 1: the rows J[:, a] J[:, b] for
 * (a, b) in np.triu_indices(d) order, then J[:, a] r, then r^2.  Every product is rounded once in the type NumPy's
 * promotion gives it (float32 x float32 in float32, then widened): the reference's values bit for bit.
 * pcr_coreset = fast_caratheodory(P, u, k, n_target) (caratheodory.py:62-116): P (m, n) float64 row-major, u (n) finite
 * and > 0, k > m + 1, n_target >= m + 1 (the reference does not finish below those: its caratheodory() returns the
 * same chunk again, caratheodory.py:42-43).  Writes *n_out <= n_target points: idx_out ascending, w_out > 0 with
 * sum w P[:, idx] = sum u P up to rounding, P_sel_out = P[:, idx] as (m, *n_out) row-major.  The chunk bounds are the
 * reference's np.linspace ones; the Caratheodory elimination of each level runs on the host in float64 with its null
 * vector from a pivoted QR (the reference: the last right-singular vector of an SVD), so the points chosen differ from
 * the reference's -- only the properties above are the contract.  n <= n_target: the inputs and 0..n-1, no GPU work.
 * P is uploaded once and stays in HBM; the O(n m) sums of every level run on the GPU, bit-reproducible.              */
PCR_API pcr_status pcr_gn_set(pcr_context *ctx, const void *J, int J_is_f64, const void *r, int r_is_f64, int64_t n, int d,
                              double *P_out);
PCR_API pcr_status pcr_coreset(pcr_context *ctx, const double *P, int m, int64_t n, const double *u, int k, int64_t n_target,
                               int64_t *n_out, double *w_out, int64_t *idx_out, double *P_sel_out);

/* ---- the hot path ---------------------------------------------------------------------
 * One calc_H_g_e2: transform (math_tools.py:111-113) -> exact 1-NN (kdtree.py:18-21 /
 * voxel.py:171-179) -> gate dist < max_dist -> residual + Jacobian -> 6x6 normal equations
 * (icp.py:24-57, plane_icp.py:30-69, voxelized_plane_icp.py:23-64, ndt.py:24-57), summed
 * over all ranks when a communicator is attached.  The search is bounded by max_dist, which
 * is exact for these sums (anything farther is gated out anyway).                          */
PCR_API pcr_status pcr_linearize(pcr_target *t, pcr_scan *s, int kind, const double T[16],
                                 double max_dist, unsigned flags, double out[29]);

/* ---- per-correspondence rows, weighted sums, scan coresets ---------------------------------
 * What pcr_linearize accumulates, written out per scan point IN THE CALLER'S ORDER.  The scan must know that order: created
 * with PCR_FLAG_KEEP_ORDER (Morton-sorted, 4 more bytes per point) or with PCR_FLAG_NO_SCAN_SORT; any other scan gives
 * PCR_ERR_INVALID.  Each call runs an ordinary full search into a match buffer of its own at pose T and the same transform and
 * gate as pcr_linearize, so a point is in or out exactly as there; the scan's reuse state is left alone (a following
 * pcr_linearize / pcr_align returns the bits it would have returned without the call).  n = points of the scan,
 * m = 1 (PCR_PLANE, PCR_VPLANE) or 3 (PCR_ICP, PCR_NDT).
 * pcr_linearize_rows: J (n, m, 6), r (n, m), w (n) = 1 where the point is gated in, else 0 with zero rows;
 *   PLANE / VPLANE: J = [n, p x (R^T n)], r = n . (R p + t - q); ICP / NDT: J = [I, -R skew(p)], r = R p + t - q;
 *   W_or_null (NDT: n x 9) = the matched voxel's inverse covariance, symmetric; idx_or_null (n) = the matched target point
 *   (the caller's index) or voxel (its position in pcr_target_voxels_get's order), -1 where gated out.
 * pcr_linearize_weighted: out[0..27] = sum_i weights[i] x (the 28 sums' terms of point i: triu(H) 21, g 6, e2) over the gated-in
 *   points, out[28] = sum of their weights; weights (n, caller order) finite and >= 0.  ICP terms come from J = [I, -R skew(p)],
 *   g[3:] = p x (R r) under PCR_FLAG_ICP_RR_QUIRK, p x (R^T r) without.  Fixed summation order: bit-reproducible.
 * pcr_scan_coreset: fast_caratheodory (pcr_coreset) over those terms with unit weights, the terms never leaving HBM: at most
 *   n_target gated-in points (idx_out: ascending caller indices) with weights w_out > 0 whose weighted sums equal the full
 *   ones up to rounding; *n_out of them.  At most n_target gated-in points: all of them, weight 1.  k > 29, n_target >= 29.
 * Device memory: pcr_linearize_weighted and pcr_scan_coreset hold the terms as 28 x n doubles whatever the gated-in count --
 *   224 bytes per SCAN point plus ~50 of bookkeeping (237 MB at 1.06 M points, 2.2 GB at 10 M) -- and pcr_linearize_rows a device
 *   copy of its outputs; all of it is taken for the length of the call and kept in the context's block cache afterwards.
 * PCR_ERR_UNSUPPORTED: a context with a communicator attached (pcr_comm_*, members of a pcr_group); PCR_PLANE over a target
 * with float64 coordinates (quirk Q6).                                                                                   */
PCR_API pcr_status pcr_linearize_rows(pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist, unsigned flags,
                                      double *J, double *r, double *w, double *W_or_null, int64_t *idx_or_null);
PCR_API pcr_status pcr_linearize_weighted(pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist, unsigned flags,
                                          const double *weights, double out[29]);
PCR_API pcr_status pcr_scan_coreset(pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist, unsigned flags,
                                    int k, int64_t n_target, int64_t *idx_out, double *w_out, int64_t *n_out);

/* Registration.align (registration.py:71-113) run entirely behind the boundary: up to
 * max_iter x { pcr_linearize, dx = -solve(H, g), stop if |dx| < tol (before the update,
 * quirk Q4), T <- plus(T, dx) (math_tools.py:101-108, first-order expSO3 branch, quirk Q3) }.
 * The loop is device-resident (large scans, and always with a communicator): the pose stays in HBM, the 6x6 solve and the update run in a one-wave
 * kernel (k_gn_update) behind the reduce kernel, iterations are enqueued back to back and the host reads one
 * result (PCR_FLAG_HOST_LOOP selects the host-driven form of the same arithmetic).
 * trace_or_null receives up to max_iter rows of 16 (T before the step) + 29 doubles.
 * Returns PCR_ERR_SINGULAR where numpy.linalg.solve would raise LinAlgError (quirk Q7).     */
PCR_API pcr_status pcr_align(pcr_target *t, pcr_scan *s, int kind, const double T_init[16],
                             int max_iter, double tol, double max_dist, unsigned flags,
                             double T_out[16], int *iterations, double *trace_or_null);

/* ---- Generalized ICP: distribution to distribution ------------------------------------------
 * No reference counterpart (the reference only borrows small_gicp's tree, kdtree.py:26-57).  Every point of the target AND of
 * the scan carries a covariance, float32 (N, 6) = xx xy xz yy yz zz, supplied by the caller or estimated on the GPU; a
 * correspondence (p, Cp) -> (q, Cq) at pose T = (R, t) is weighed with M = (Cq + R Cp R^T)^-1:
 *   H = sum J^T M J,  g = sum J^T M d,  e2 = sum d^T M d,  J = [I, -R skew(p)],  d = R p + t - q,  count = matches kept.
 * Correspondence and gate are exactly PCR_ICP's: float32 transform, exact 1-NN over the float32 target, kept iff the float32
 * distance is < max_dist; d is formed in float32, then widened.  M is float64: R the float64 rotation of T, the inverse by
 * the closed form of the voxel targets (adjugate / determinant, voxel.py:69-102) INCLUDING its rule for det == 0 -- the
 * adjugate is divided by 1e6 instead, so a degenerate pair (e.g. two PCR_COV_RAW covariances of one-point neighbourhoods)
 * contributes (almost) nothing where a plain inverse would give Inf / NaN.  Conventions are PCR_NDT's: translation Jacobian I
 * with a right-multiplicative update (quirk Q2), dM/dT ignored (as every GICP implementation does), so the Gauss-Newton step
 * of pcr_align drives the loop unchanged (quirks Q3, Q4, Q7).
 * pcr_*_estimate_covariances: the k nearest neighbours of every point within its OWN cloud, the point itself included
 *   (1 <= k <= 64, else PCR_ERR_INVALID; a cloud of fewer than k points uses the neighbours found), two-pass float64
 *   covariance with divisor = neighbours found, then
 *     PCR_COV_PLANE  C = I - (1 - eps) n n^T, n = eigenvector of the smallest eigenvalue: the usual "eigenvalues -> (eps, 1, 1)"
 *                    regularisation, which depends on the normal only; 0 < eps <= 1
 *     PCR_COV_RAW    the covariance itself (eps ignored).
 *   A scan builds a temporary index over its own device points for this and releases it before returning.
 * Arrays that cross the boundary (set, get, cov_out) are in the CALLER's order; a scan must know that order for them
 *   (PCR_FLAG_KEEP_ORDER or PCR_FLAG_NO_SCAN_SORT, else PCR_ERR_INVALID).  Estimating without cov_out works on any scan.
 *   set: non-finite values give PCR_ERR_INVALID.  get: PCR_ERR_NO_TARGET when there are none.
 * pcr_gicp_linearize: out[29] as pcr_linearize; PCR_ERR_NO_TARGET when either side has no covariances.  A full search into a
 *   match buffer of the call (the scan's reuse state is left alone, as for pcr_linearize_rows), then a reduce launch that
 *   writes one row of sums per block and a one-block fold that adds the rows in order: no atomics, and the grid depends on
 *   the scan size and the device only -- two calls return the same bits.  An empty scan gives zeros without a launch.
 * pcr_gicp_align: the host-driven loop of pcr_align(PCR_FLAG_HOST_LOOP) over pcr_gicp_linearize: same step, same trace rows
 *   (16 + 29 doubles), PCR_ERR_SINGULAR as there.
 * PCR_ERR_UNSUPPORTED: a context with a communicator attached (pcr_comm_*, members of a pcr_group).                        */
enum { PCR_COV_PLANE = 0, PCR_COV_RAW = 1 };
PCR_API pcr_status pcr_target_estimate_covariances(pcr_target *t, int k, int mode, double eps, float *cov_out_or_null);
PCR_API pcr_status pcr_target_set_covariances(pcr_target *t, const float *cov6);
PCR_API pcr_status pcr_target_get_covariances(pcr_target *t, float *cov6);
PCR_API pcr_status pcr_scan_estimate_covariances(pcr_scan *s, int k, int mode, double eps, float *cov_out_or_null);
PCR_API pcr_status pcr_scan_set_covariances(pcr_scan *s, const float *cov6);
PCR_API pcr_status pcr_scan_get_covariances(pcr_scan *s, float *cov6);
PCR_API pcr_status pcr_gicp_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags,
                                      double out[29]);
PCR_API pcr_status pcr_gicp_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                  unsigned flags, double T_out[16], int *iterations, double *trace_or_null);

/* ---- Voxelized GICP: distribution to voxel ---------------------------------------------------
 * No reference counterpart (Koide, Yokozuka, Oishi, Banno: "Voxelized GICP", ICRA 2021; small_gicp / fast_gicp).  GICP's
 * weighting on a VOXEL target: a scan point p (float32, untransformed) with covariance Cp (float32, six values xx xy xz yy yz
 * zz: exactly GICP's scan covariances, pcr_scan_*_covariances) at pose T = (R, t) is matched to the nearest kept centroid mu
 * and weighed with M = (Cv + R Cp R^T)^-1, Cv the float64 covariance of that voxel:
 *   H = sum J^T M J,  g = sum J^T M d,  e2 = sum d^T M d,  J = [I, -R skew(p)],  d = R p + t - mu,  count = matches kept.
 * Correspondence and gate are exactly PCR_NDT's / PCR_VPLANE's: float32 transform, exact nearest kept centroid in float64,
 * d = (double)xform(p) - mu formed in float64, kept iff sqrt(d . d) < max_dist (strict, float64).  M is float64: Cp widened,
 * R Cp R^T evaluated in the order GICP evaluates it, the inverse by the closed form of the voxel targets INCLUDING its rule
 * for det == 0 (the adjugate is divided by 1e6 instead).  Unlike PCR_NDT's bare voxel covariance, the summed matrix is well
 * conditioned as soon as either side is regularised.  Conventions and the Gauss-Newton step are PCR_NDT's.
 * pcr_target_voxels_set_covariances: one Cv per kept voxel, (n, 6) float64 xx xy xz yy yz zz, from
 *     PCR_COV_RAW    the voxel's own covariance (the bits pcr_target_voxels_get returns as cov; eps ignored)
 *     PCR_COV_PLANE  I - (1 - eps) n n^T with n the voxel's normal, evaluated in float64: eigenvalues (eps, 1, 1), the sign
 *                    of n does not matter; 0 < eps <= 1
 *     cov6_or_null   non-NULL overrides mode: the caller's own, n x 6 in the order of pcr_target_voxels_get (ascending key)
 *                    -- e.g. the mean of the point covariances in the voxel.  A non-finite entry gives PCR_ERR_INVALID and
 *                    leaves the old covariances in place.
 *   A point target, or a voxel target that does not hold what the mode needs, gives PCR_ERR_NO_TARGET.  The inverse
 *   covariances pcr_linearize(PCR_NDT) reads are not touched.
 * pcr_target_voxels_get_covariances: the same rows back, key order; PCR_ERR_NO_TARGET when there are none.
 * pcr_vgicp_linearize: out[29] as pcr_linearize.  PCR_ERR_NO_TARGET for a point target, a voxel target without covariances or
 *   a scan without covariances.  A full centroid search into a match buffer of the call (the scan's reuse state is left
 *   alone), then a reduce launch that writes one row of sums per block with plain stores and a one-block fold that adds the
 *   rows in block order: no atomics, the grid depends on the scan size and the device only -- two calls return the same bits.
 *   An empty scan gives zeros.
 * pcr_vgicp_align: the host-driven loop of pcr_align(PCR_FLAG_HOST_LOOP) over pcr_vgicp_linearize: same step, same trace rows
 *   (16 + 29 doubles), PCR_ERR_SINGULAR as there.
 * PCR_ERR_UNSUPPORTED: a context with a communicator attached (pcr_comm_*, members of a pcr_group).                        */
PCR_API pcr_status pcr_target_voxels_set_covariances(pcr_target *t, int mode, double eps, const double *cov6_or_null);
PCR_API pcr_status pcr_target_voxels_get_covariances(pcr_target *t, double *cov6);
PCR_API pcr_status pcr_vgicp_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags,
                                       double out[29]);
PCR_API pcr_status pcr_vgicp_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                   unsigned flags, double T_out[16], int *iterations, double *trace_or_null);

/* ---- Symmetric point-to-plane ICP: the normals of BOTH clouds ---------------------------------
 * No reference counterpart (Rusinkiewicz: "A Symmetric Objective Function for ICP", SIGGRAPH 2019; the fixed-normal-sum form
 * of PCL).  A point target with normals (the PtN records PCR_PLANE gathers) and a scan that carries one float32 normal per
 * point.  Every correspondence pulls along the mean of the two normals, so the error vanishes for any pair of points on the
 * same second-order patch, not only on the same plane.  Everything is float64 from widened float32 inputs and nothing is
 * contracted but the explicit fma()s of the accumulation.  For scan point p (untransformed) with normal n_p, matched target
 * record (q, n_q) and pose T = (R, t), in this order of operations:
 *   tp = xform(T, p)                                    float32, ((R_i0 x + R_i1 y) + R_i2 z) + t_i, exactly PCR_ICP's
 *   d  = tp - q                                         float32; kept iff sqrt(d . d) < (float)max_dist (strict, float32):
 *                                                       correspondence and gate are exactly PCR_ICP's
 *   v_i = (R[3i] n_p.x + R[3i+1] n_p.y) + R[3i+2] n_p.z   the rotated scan normal, R the float64 rotation of T
 *   c  = (n_q.x v_0 + n_q.y v_1) + n_q.z v_2
 *   normal gate: skipped unless |c| >= min_cos (a NaN c is skipped); min_cos = 0 keeps every finite pair
 *   s  = c < 0 ? -1 : +1                                PCA normals carry no sign: the objective does not depend on it -- negating
 *                                                       any n_p or n_q returns the same bits wherever c != 0.  At c == 0 (-0
 *                                                       included) there is no sign to follow: s = +1, and negating ONE of the
 *                                                       two normals turns m into 0.5 (n_q - v); such a pair passes min_cos = 0 only
 *   m  = 0.5 (n_q + s v)                                componentwise; the products with s and 0.5 are exact
 *   r  = (m_0 d_0 + m_1 d_1) + m_2 d_2,  J = [m, p x (R^T m)]      PCR_PLANE's row with m in the place of the normal
 *   H += J^T J, g += J^T r, e2 += r r (fma), count += 1            PCR_PLANE's accumulation; out[29] as pcr_linearize
 * m is held fixed within a pass: its dependence on the pose is ignored, as GICP ignores its weight's.  Where R n_p = +-n_q the
 * pass is PCR_PLANE's.  The Gauss-Newton step of pcr_align drives the loop unchanged (quirks Q2, Q3, Q4, Q7).
 * pcr_scan_estimate_normals: what pcr_target_estimate_normals(compat = 0) computes, for every scan point within the scan: the
 *   k nearest neighbours, the point itself included (1 <= k <= 64, else PCR_ERR_INVALID; fewer points than k: the neighbours
 *   found), centred float64 covariance, the unit eigenvector of its smallest eigenvalue (a one-point neighbourhood: (1, 0, 0)).
 *   The scan builds a temporary index over its own device points and releases it before returning.  A failure never leaves a
 *   scan holding uninitialised normals.
 * Arrays that cross the boundary (set, get, normals_out) are (n, 3) float32 in the CALLER's order; the scan must know that
 *   order (PCR_FLAG_KEEP_ORDER or PCR_FLAG_NO_SCAN_SORT, else PCR_ERR_INVALID).  Estimating without normals_out works on any
 *   scan.  set: a non-finite entry gives PCR_ERR_INVALID and leaves the old normals.  get: PCR_ERR_NO_TARGET when there are none.
 *   Normals and GICP covariances coexist on a scan.
 * pcr_symm_linearize: PCR_ERR_NO_TARGET for a voxel target, a point target without normals or a scan without normals;
 *   PCR_ERR_INVALID for min_cos outside [0, 1] or NaN.  A full search into a match buffer of the call (the scan's reuse state is
 *   left alone), then a reduce launch that writes one row of sums per block with plain stores and a one-block fold that adds
 *   the rows in block order: no atomics, the grid depends on the scan size and the device only -- two calls return the same
 *   bits.  An empty scan gives zeros.
 * pcr_symm_align: the host-driven loop of pcr_align(PCR_FLAG_HOST_LOOP) over pcr_symm_linearize: same step, same trace rows
 *   (16 + 29 doubles), PCR_ERR_SINGULAR as there.
 * PCR_ERR_UNSUPPORTED: a context with a communicator attached (pcr_comm_*, members of a pcr_group).                        */
PCR_API pcr_status pcr_scan_estimate_normals(pcr_scan *s, int k, float *normals_out_or_null);
PCR_API pcr_status pcr_scan_set_normals(pcr_scan *s, const float *normals);
PCR_API pcr_status pcr_scan_get_normals(pcr_scan *s, float *normals);
PCR_API pcr_status pcr_symm_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos,
                                      unsigned flags, double out[29]);
PCR_API pcr_status pcr_symm_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                  double min_cos, unsigned flags, double T_out[16], int *iterations, double *trace_or_null);

/* ---- Colored ICP: geometry plus intensity on the target's tangent planes -----------------------
 * No reference counterpart (Park, Zhou, Koltun: "Colored Point Cloud Registration Revisited", ICCV 2017; the form Open3D
 * offers).  "Intensity" is one float32 per point: a LiDAR return strength, or a colour reduced to one channel; its scale is the
 * caller's business (Open3D: values in [0, 1] with coordinates in metres).  A point target with normals (the PtN records
 * PCR_PLANE gathers) carries an intensity I_q and a gradient g_q (three floats) per point; a scan carries an intensity I_p per
 * point.  Everything is float64 from widened float32 inputs and nothing is contracted but the explicit fma()s of the
 * accumulation.
 * The gradient of target point q with unit normal n (pcr_target_estimate_color_gradients): over its k nearest neighbours q_i
 *   within the target, nearest first (1 <= k <= 64; the point itself is found as always and left out here with every other
 *   neighbour whose float32 squared distance is not > 0; w = the number that remain), in this order of operations:
 *   e  = q_i - q                                        per component, float64
 *   en = (e_0 n_0 + e_1 n_1) + e_2 n_2,  u = e - en n   the neighbour's offset within the tangent plane
 *   M += u u^T (xx xy xz yy yz zz),  b += u (I_i - I_q) neighbour by neighbour, a product and an addition each
 *   M_ab += (double)(w w) (n_a n_b)                     Open3D's constraint row: the component along n is pinned to zero
 *   det = a bc + 2 de f - a f^2 - b e^2 - c d^2         (a b c = M_xx M_yy M_zz, d e f = M_xy M_xz M_yz; left to right)
 *   s  = M^-1 b                                         the adjugate over det, the expressions of the GICP weight's inverse;
 *                                                       s_i = (o_i0 b_0 + o_i1 b_1) + o_i2 b_2
 *   sn = (s_0 n_0 + s_1 n_1) + s_2 n_2,  g = s - sn n   one projection, so g is tangent to rounding; rounded to float32
 *   g is EXACTLY zero when w < 3, when det is not > 0, or when a component of the float32 result is not finite.  There is no
 *   conditioning guard beyond det > 0: near-collinear neighbourhoods give large gradients, as they do in Open3D.  The result
 *   does not depend on the sign of n; doubling every intensity doubles it bit for bit.
 * One correspondence: found and gated exactly as PCR_ICP's.  For scan point p (untransformed) with intensity I_p, matched
 *   target record (q, n, I_q, g) and pose T = (R, t):
 *   tp = xform(T, p),  d = tp - q                       float32, kept iff sqrt(d . d) < (float)max_dist (strict, float32)
 *   r_G = (n_0 d_0 + n_1 d_1) + n_2 d_2,  J_G = [n, p x (R^T n)]          PCR_PLANE's row
 *   gn  = (g_0 n_0 + g_1 n_1) + g_2 n_2,  m = g - gn n                    the gradient's tangent part (given gradients need not
 *                                                                         be tangent)
 *   r_C = (I_q - I_p) + ((m_0 d_0 + m_1 d_1) + m_2 d_2),  J_C = [m, p x (R^T m)]   PCR_PLANE's row with m in the place of n:
 *                                                       Open3D's I_q + g . (s' - q) - I_p, s' = tp projected onto the tangent
 *                                                       plane of q, and its exact derivative
 *   with a_G = sqrt(lambda), a_C = sqrt(1 - lambda), taken once on the host in double:
 *   J = a_G J_G, r = a_G r_G:   H += J^T J, g += J^T r, e2 += r r (fma)   PCR_PLANE's accumulation
 *   J = a_C J_C, r = a_C r_C:   the same                                  count += 1 once per CORRESPONDENCE: out[28]
 *   A pair whose target gradient is zero adds (a_C (I_q - I_p))^2 to e2 and nothing else on the colour side.  lambda = 1 returns
 *   the bits of the same call with zero gradients and any intensities.  Negating any target normal returns the same bits.
 * pcr_target_set_intensity: (n,) intensities and optionally (n, 3) gradients, float32, in the CALLER's order.  Needs a point
 *   target with normals, else PCR_ERR_NO_TARGET.  A non-finite entry gives PCR_ERR_INVALID and leaves the old payload.  Given
 *   gradients are stored as they are; without them the gradients are zero until estimated.
 * pcr_target_estimate_color_gradients: needs intensities (PCR_ERR_NO_TARGET); k outside [1, 64]: PCR_ERR_INVALID.
 * pcr_target_get_color: caller's order; either array may be NULL.  PCR_ERR_NO_TARGET when there is no colour payload.
 * pcr_target_set_normals / pcr_target_estimate_normals FREE a target's colour payload: the gradients lie in the tangent planes
 *   of the normals they were estimated with, and a later coloured pass is refused instead of reading stale ones.
 * pcr_scan_set_intensity / _get_intensity: (n,) float32 in the CALLER's order; the scan must know that order
 *   (PCR_FLAG_KEEP_ORDER or PCR_FLAG_NO_SCAN_SORT, else PCR_ERR_INVALID).  set: a non-finite entry gives PCR_ERR_INVALID and
 *   leaves the old intensities.  get: PCR_ERR_NO_TARGET when there are none.  Intensities, normals and GICP covariances coexist
 *   on a scan.
 * pcr_color_linearize: PCR_ERR_NO_TARGET for a voxel target, a point target without normals or without colour records, or a
 *   scan without intensities; PCR_ERR_INVALID for lambda_geometric outside [0, 1] or NaN.  Search, reduce and fold as
 *   pcr_symm_linearize: no atomics, two calls return the same bits.  An empty scan gives zeros.
 * pcr_color_align: the host-driven loop of pcr_align(PCR_FLAG_HOST_LOOP) over pcr_color_linearize: same step, same trace rows
 *   (16 + 29 doubles), PCR_ERR_SINGULAR as there.
 * PCR_ERR_UNSUPPORTED: a context with a communicator attached (pcr_comm_*, members of a pcr_group).                        */
PCR_API pcr_status pcr_target_set_intensity(pcr_target *t, const float *intensity, const float *gradient_or_null);
PCR_API pcr_status pcr_target_estimate_color_gradients(pcr_target *t, int k, float *gradient_out_or_null);
PCR_API pcr_status pcr_target_get_color(pcr_target *t, float *intensity_or_null, float *gradient_or_null);
PCR_API pcr_status pcr_scan_set_intensity(pcr_scan *s, const float *intensity);
PCR_API pcr_status pcr_scan_get_intensity(pcr_scan *s, float *intensity);
PCR_API pcr_status pcr_color_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric,
                                       unsigned flags, double out[29]);
PCR_API pcr_status pcr_color_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                   double lambda_geometric, unsigned flags, double T_out[16], int *iterations,
                                   double *trace_or_null);

/* ---- robust kernels inside the pass of GICP, VGICP, SymmetricICP and ColoredICP ----------------
 * No reference counterpart (what Open3D's RobustKernel, PCL and small_gicp offer): a correspondence inside the gate is weighed
 * by w(s), s its squared residual, so that wrong ones -- moving objects, vegetation, partial overlap -- pull less.  New entry
 * points only; the plain ones above keep their kernels and their bits.
 * A kernel is a function of s and a scale c > 0, with c2 = c * c taken ONCE on the host.  Float64, nothing contracted, each a
 * fixed sequence of compare, +, -, x, / and sqrt:
 *   PCR_ROBUST_HUBER    w = s <= c2 ? 1 : c / sqrt(s)
 *   PCR_ROBUST_CAUCHY   w = 1 / (1 + s / c2)
 *   PCR_ROBUST_TUKEY    u = 1 - s / c2;  w = s <= c2 ? u u : 0
 *   PCR_ROBUST_GM       l = c2 / (c2 + s);  w = l l            (Geman-McClure: pcr_fgr_linearize's line process with mu = c2)
 *   PCR_ROBUST_NONE     the plain pass: rb == NULL or this kind run the plain kernel and return its bits; the scale is not read
 * Every w lies in [0, 1]; w(0) = 1; every kernel is continuous at s = c2.
 * What s is:
 *   pcr_symm_*    s = r r of the one row
 *   pcr_color_*   each of the two rows has its own s and its own weight (Open3D's convention): s_G = (a_G r_G)(a_G r_G),
 *                 s_C = (a_C r_C)(a_C r_C), the row's residual after the sqrt(lambda) / sqrt(1 - lambda) factor
 *   pcr_gicp_*, pcr_vgicp_*   s = d^T M d with M the 3 x 3 weight the plain pass forms and d the residual, widened:
 *                 Md_i = (M_i0 d_0 + M_i1 d_1) + M_i2 d_2,  s = (d_0 Md_0 + d_1 Md_1) + d_2 Md_2
 * The sums are the IRLS ones, H = sum w J^T J, g = sum w J^T r, e2 = sum w r r:
 *   rows (symm, color):  Jw = w J and rw = w r, one product each, then the plain accumulation with them on the left:
 *                 H_ij = fma(Jw_i, J_j, H_ij), g_i = fma(Jw_i, r, g_i), e2 = fma(rw, r, e2)
 *   gicp, vgicp:  every entry of M times w, one product each, then the plain accumulation with w M in the place of M
 * out[28] stays the NUMBER of correspondences inside the gate (for symm: through the normal gate too), whatever their weights.
 * Search, distance gate, normal gate and the det == 0 rule are the plain pass's; so are the reduce's three phases, its fold
 * (plain stores, no atomics) and its grid, which depends on the scan size and the device only: two calls return the same bits.
 * pcr_*_linearize_robust: the refusals of the plain call, and PCR_ERR_INVALID for a kind that is none of the above, or (kind
 *   not NONE) a scale that is not finite, not > 0, or whose square is not finite or not > 0 (1e200; 1e-200).  The outputs
 *   are then untouched.
 * pcr_*_align_robust: the host-driven loop of the plain *_align over the robust pass: same step, same stop rule, same trace
 *   rows (16 + 29 doubles: the sums of pcr_*_linearize_robust at the row's pose), PCR_ERR_SINGULAR as there -- which a Tukey
 *   scale below every residual returns, every weight being 0.  A refusal leaves T_out untouched.
 * pcr_*_residuals: s of every scan point at pose T -- what a caller picks a scale from (a median, say) -- as (n) doubles, for
 *   pcr_color_residuals (n, 2) = s_G, s_C, in the CALLER's order: the scan must know that order (PCR_FLAG_KEEP_ORDER or
 *   PCR_FLAG_NO_SCAN_SORT, else PCR_ERR_INVALID).  +inf (every value of the point) where the point has no correspondence or
 *   a gate drops it.  Refusals of the plain linearize otherwise; s_out is untouched then.                              */
#define PCR_ROBUST_NONE 0
#define PCR_ROBUST_HUBER 1
#define PCR_ROBUST_CAUCHY 2
#define PCR_ROBUST_TUKEY 3
#define PCR_ROBUST_GM 4
typedef struct {
    int kind;      /* PCR_ROBUST_* */
    double scale;  /* c */
} pcr_robust;
PCR_API pcr_status pcr_gicp_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_robust *rb,
                                             unsigned flags, double out[29]);
PCR_API pcr_status pcr_gicp_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                         const pcr_robust *rb, unsigned flags, double T_out[16], int *iterations,
                                         double *trace_or_null);
PCR_API pcr_status pcr_gicp_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double *s_out);
PCR_API pcr_status pcr_vgicp_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_robust *rb,
                                              unsigned flags, double out[29]);
PCR_API pcr_status pcr_vgicp_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                          const pcr_robust *rb, unsigned flags, double T_out[16], int *iterations,
                                          double *trace_or_null);
PCR_API pcr_status pcr_vgicp_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, unsigned flags, double *s_out);
PCR_API pcr_status pcr_symm_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos,
                                             const pcr_robust *rb, unsigned flags, double out[29]);
PCR_API pcr_status pcr_symm_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                         double min_cos, const pcr_robust *rb, unsigned flags, double T_out[16], int *iterations,
                                         double *trace_or_null);
PCR_API pcr_status pcr_symm_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos, unsigned flags,
                                      double *s_out);
PCR_API pcr_status pcr_color_linearize_robust(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric,
                                              const pcr_robust *rb, unsigned flags, double out[29]);
PCR_API pcr_status pcr_color_align_robust(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                          double lambda_geometric, const pcr_robust *rb, unsigned flags, double T_out[16],
                                          int *iterations, double *trace_or_null);
PCR_API pcr_status pcr_color_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric,
                                       unsigned flags, double *s_out);

/* ---- Voxelized GICP with direct voxel neighbourhoods: 1, 7 or 27 voxels, no search ------------
 * The association of the VGICP paper and of fast_gicp / small_gicp (DIRECT1 / DIRECT7 / DIRECT27): a scan point is paired
 * with the kept voxel that CONTAINS its transformed position and with that voxel's neighbours, one distribution-to-
 * distribution term per voxel found; the voxels are found by integer lookup in the target's hash keys.  The rule:
 *   t        the float32 transform of scan point p as every pass computes it: ((R0 x + R1 y) + R2 z) + t, nothing contracted
 *   cell     c = floor((double)t / voxel_size) per axis: voxel_size the double the target was built with, IEEE float64
 *            division (no reciprocal).  A point with a non-finite coordinate, or with |c| > 2^40 on an axis, has no voxel.
 *            (A float32 cloud is BUILT with the division in float32.  The two agree exactly for power-of-two voxel sizes;
 *            otherwise they agree except for coordinates within rounding of a voxel face.)
 *   offsets  neighbors = 1: (0,0,0)
 *            neighbors = 7: (0,0,0), (-1,0,0), (+1,0,0), (0,-1,0), (0,+1,0), (0,0,-1), (0,0,+1)
 *            neighbors = 27: dz outer, dy middle, dx inner, each -1, 0, +1: the own voxel is column 13
 *   voxel    of cell c + o: the kept voxel whose key equals the build's hash of c + o,
 *            ((((z P) mod M) + y) P) mod M + x with P = 116101, M = 10^10 and the non-negative modulo -- the keys
 *            pcr_target_voxels_get returns.  The hash is the build's own identity of a voxel: the lookup inherits its
 *            collisions and adds none.
 *   pair     (point, found voxel v) is kept iff sqrt((dx^2 + dy^2) + dz^2) < max_dist with d = (double)t - mean_v (strict,
 *            float64: the gate of pcr_vgicp_linearize)
 *   term     every kept pair contributes exactly what a correspondence of pcr_vgicp_linearize contributes: M = (Cv + R Cp
 *            R^T)^-1 with its det == 0 rule, the same accumulation; under a robust kernel the weight w(d^T M d) of
 *            pcr_vgicp_linearize_robust.  The pairs of a point are added in offset order.  No weighting by point counts.
 *   out[28]  the number of kept pairs
 * pcr_target_voxels_lookup: the key-order indices (rows of pcr_target_voxels_get) of the voxels of m float32 points, taken as
 *   already transformed: idx is m x neighbors int64, -1 where there is no kept voxel.  The lookup data are built by the first
 *   call that needs them and freed with the target; keys that do not ascend strictly give PCR_ERR_INVALID then.
 * pcr_target_voxels_set_keys: the keys of a target made by pcr_target_voxels_create_from_stats, n int64 in the order of its
 *   means (such a target has none, and every call of this section gives PCR_ERR_NO_TARGET until it does).  PCR_ERR_INVALID
 *   on a target built from points: its keys are the build's.  Only the ORDER of the keys is ever checked (strictly ascending,
 *   by the first lookup).  That key i is the hash of the cell mean i lies in is the caller's responsibility and is NOT
 *   verified: with keys that do not belong to the means a point is paired with whatever voxel its cell's key names, the gate
 *   on the distance to that voxel's mean being the only thing that still drops such a pair.
 * pcr_vgicp_direct_linearize: out[29] as pcr_vgicp_linearize; rb NULL or PCR_ROBUST_NONE: the plain pass.  One launch, one
 *   lane per scan point, and the fold of pcr_vgicp_linearize: no atomics, the grid depends on the scan size and the device
 *   only -- two calls return the same bits.  Refused, in this order: NULL arguments; neighbors not 1, 7 or 27
 *   (PCR_ERR_INVALID); the robust kernel; a point target, a target without covariances or keys, a scan without covariances
 *   (PCR_ERR_NO_TARGET); different contexts; max_dist <= 0; a context with a communicator (PCR_ERR_UNSUPPORTED).  A target
 *   with no kept voxel and an empty scan give zeros.  A refused call writes nothing.
 * pcr_vgicp_direct_align: the host-driven loop of pcr_vgicp_align over that pass: same step, same trace rows.
 * pcr_vgicp_direct_residuals: d^T M d of every (point, offset), n x neighbors float64 in the caller's order (the scan must
 *   know it), +inf where there is no kept pair.                                                                            */
PCR_API pcr_status pcr_target_voxels_lookup(pcr_target *t, const float *xyz, int64_t m, int neighbors, int64_t *idx);
PCR_API pcr_status pcr_target_voxels_set_keys(pcr_target *t, const int64_t *keys);
PCR_API pcr_status pcr_vgicp_direct_linearize(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, int neighbors,
                                              const pcr_robust *rb_or_null, unsigned flags, double out[29]);
PCR_API pcr_status pcr_vgicp_direct_align(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                          int neighbors, const pcr_robust *rb_or_null, unsigned flags, double T_out[16], int *iterations,
                                          double *trace_or_null);
PCR_API pcr_status pcr_vgicp_direct_residuals(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, int neighbors,
                                              unsigned flags, double *s_out);

/* ---- adaptive pass: trimmed ICP and robust scales taken from each pass's own residuals ---------
 * No reference counterpart (Chetverikov et al.: "The Trimmed Iterative Closest Point Algorithm", ICPR 2002; what PCL offers as
 * CorrespondenceRejectorTrimmed / CorrespondenceRejectorMedianDistance and libpointmatcher as TrimmedDistOutlierFilter /
 * MedianDistOutlierFilter): the threshold of a trim, or the scale c of a robust kernel, is an order statistic of the pass's OWN
 * squared residuals, found on the device between the search and the reduce -- no host round trip, the one stream
 * synchronisation of a pass.  New entry points only; the plain and the robust ones above keep their kernels and their bits.
 * One pass at pose T:
 *   search and gates   the search, the distance gate, the unit's own gate and the det == 0 rule are the plain pass's
 *   key     every scan point gets a key in device order (no caller order is needed: PCR_FLAG_KEEP_ORDER is not required): the
 *           squared residual s that pcr_*_residuals defines; for pcr_color_* s_G + s_C, one addition, geometric row first;
 *           +inf where the point has no correspondence or a gate drops it
 *   rank    m = the number of keys < +inf = the plain pass's out[28], and out[28] here;  k = max(1, floor(quantile * m)), the
 *           product taken once in float64.  m = 0: all 29 sums are zero and stats = (+inf, 0, 0, 0)
 *   tau     the k-th smallest key (1-based), exact, by pcr_order_statistic's selection on the device
 *   PCR_ROBUST_TRIM    a correspondence is kept iff its STORED key <= tau (not a recomputation: the kept count is n_le by
 *           construction); ties at tau are all kept, so there is no index tie-break and n_le >= k.  Kept terms enter with weight
 *           exactly 1 through the robust pass's weighted accumulation (a product with 1 is exact), a dropped one with weight 0.
 *           factor is not read
 *   PCR_ROBUST_HUBER .. PCR_ROBUST_GM    c = factor * sqrt(tau) and c2 = c * c, both taken once on the device, in float64, by
 *           the selection's last kernel; the robust reduce of the unit then runs with that kernel read from device memory: the
 *           same points per lane, the same order of operations, a weight per row for pcr_color_*, exactly as
 *           pcr_*_linearize_robust with scale = c -- whose 29 values it returns bit for bit.  If c2 is not > 0 (tau = 0: a scan
 *           that is a subset of the target at the true pose; underflow) every kernel takes its limit for c -> 0:
 *           w = (s == 0 ? 1 : 0)
 *   stats   (tau, c, n_le, k): n_le the number of keys <= tau; c = 0 under PCR_ROBUST_TRIM
 * The selection never rounds, orders keys as float64 `<` does and does not depend on its grid: two calls return the same bits.
 * pcr_*_linearize_adaptive: the refusals of the plain call in their order (NULL arguments, the unit's own parameter first),
 *   then PCR_ERR_INVALID for a kind outside 1 .. 5, a quantile outside (0, 1] or NaN, or (M-estimators only) a factor that is
 *   not finite and > 0.  out and stats are then untouched.  pcr_*_linearize_robust / _align_robust keep refusing kind 5.
 * pcr_*_align_adaptive: the host-driven loop of *_align over this pass: same step, same stop rule, same trace rows (16 + 29
 *   doubles), PCR_ERR_SINGULAR as there; stats_or_null takes 4 doubles per iteration.  A refusal leaves every output untouched.
 * pcr_order_statistic: the selection on its own, over n host keys: *value = the k-th smallest (1-based) of the keys < +inf,
 *   *n_le = the number of keys <= *value.  Exact; the order is that of float64 `<` (negative keys, -0.0 == +0.0 -- returned as
 *   +0.0 --, denormals); a NaN key counts as outside, as +inf does.  PCR_ERR_INVALID with untouched outputs for NULL arguments,
 *   n < 1, k < 1 or k above the number of keys < +inf.                                                                      */
#define PCR_ROBUST_TRIM 5 /* valid in pcr_adaptive only */
typedef struct {
    int kind;        /* PCR_ROBUST_HUBER .. PCR_ROBUST_GM, or PCR_ROBUST_TRIM */
    double quantile; /* in (0, 1] */
    double factor;   /* c = factor * sqrt(tau); not read under PCR_ROBUST_TRIM */
} pcr_adaptive;
PCR_API pcr_status pcr_order_statistic(pcr_context *ctx, const double *keys, int64_t n, int64_t k, double *value, int64_t *n_le);
PCR_API pcr_status pcr_gicp_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_adaptive *ad,
                                               unsigned flags, double out[29], double stats[4]);
PCR_API pcr_status pcr_gicp_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                           const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations,
                                           double *trace_or_null, double *stats_or_null);
PCR_API pcr_status pcr_vgicp_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, const pcr_adaptive *ad,
                                                unsigned flags, double out[29], double stats[4]);
PCR_API pcr_status pcr_vgicp_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                            const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations,
                                            double *trace_or_null, double *stats_or_null);
PCR_API pcr_status pcr_symm_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double min_cos,
                                               const pcr_adaptive *ad, unsigned flags, double out[29], double stats[4]);
PCR_API pcr_status pcr_symm_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                           double min_cos, const pcr_adaptive *ad, unsigned flags, double T_out[16], int *iterations,
                                           double *trace_or_null, double *stats_or_null);
PCR_API pcr_status pcr_color_linearize_adaptive(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double lambda_geometric,
                                                const pcr_adaptive *ad, unsigned flags, double out[29], double stats[4]);
PCR_API pcr_status pcr_color_align_adaptive(pcr_target *t, pcr_scan *s, const double T_init[16], int max_iter, double tol, double max_dist,
                                            double lambda_geometric, const pcr_adaptive *ad, unsigned flags, double T_out[16],
                                            int *iterations, double *trace_or_null, double *stats_or_null);

/* ---- batches: many scans and / or start poses against ONE target in one launch -----------
 * No reference counterpart (Registration.align takes one scan, registration.py:71).  A scan of the sizes people register
 * (up to ~260 k points) runs as ONE fused kernel per Gauss-Newton iteration and is latency-bound: it fills a fraction of the
 * chip with waves that wait on dependent misses.  A caller with K scans (a LiDAR sequence against a map, several robots,
 * loop-closure candidates) or K start poses for one scan (multi-start) gets one launch per iteration for the WHOLE batch: a
 * second grid dimension over the items, each item with its own partial sums, tickets, pose and trace rows.
 * pcr_scan_batch_create: S scans in one upload -- xyz = all points concatenated, offsets[S + 1] ascending from 0 (empty scans
 * allowed); every scan is Morton-sorted exactly as pcr_scan_create sorts it.  Device blocks come from and return to the
 * context's block cache, like a scan's.  "One upload" is one host-to-device copy only: each scan is then sorted by its own
 * pcr_scan_create_device -- its own x / y / z blocks, its own sort temporaries, one stream synchronisation each -- so creating a
 * batch costs about what S pcr_scan_create calls cost minus S - 1 copies; create it once and reuse it across calls.
 * An ITEM of a call = scan item_scan[i] of the batch at pose T[16 i ..]; several items may name the same scan (the points are
 * held once).  item_scan == NULL: item i = scan i and n_items must be the number of scans.  At most 65535 items per call.
 * pcr_linearize_batch: out[29 i ..] = what pcr_linearize gives for item i alone.
 * pcr_align_batch: per item T_out[16 i ..], iterations[i], item_status[i] (PCR_OK, or PCR_ERR_SINGULAR with T_out = the pose
 * of the failed solve, as pcr_align leaves it), and with trace_or_null != NULL max_iter rows of 45 doubles per item (row r of
 * item i at 45 (max_iter i + r); rows past iterations[i] are zero).  iterations / item_status may be NULL.  A singular item
 * neither fails the call nor disturbs the others: the call itself fails only for bad arguments, unsupported configurations
 * or HIP errors.  The loop is always the device-resident one (PCR_FLAG_HOST_LOOP / PCR_FLAG_DEVICE_LOOP are ignored).
 * Every item runs the fused small-scan kernel with the block count, work split, fold order and Gauss-Newton step of a single
 * launch over that scan, so its sums, trace rows, iteration count and pose are BIT-IDENTICAL to pcr_linearize /
 * pcr_align(PCR_FLAG_DEVICE_LOOP) of that scan alone under pcr_set_variant(ctx, 0) -- which is also what the default variant
 * runs for scans of up to num_cu x 1024 points.  Larger items are accepted and correct (sums equal to the default path's up
 * to the order of summation) but are not what this is for: above that size search + reduce is the faster pipeline.
 * PCR_ERR_UNSUPPORTED: a context with a communicator attached (pcr_comm_*, members of a pcr_group); PCR_PLANE over a target
 * with float64 coordinates (pcr_target_points_set_f64: quirk Q6 always runs search + reduce).  Certified reuse
 * (pcr_set_reuse) does not apply to batches.                                                                             */
typedef struct pcr_scan_batch pcr_scan_batch;
PCR_API pcr_status pcr_scan_batch_create(pcr_context *ctx, const float *xyz, const int64_t *offsets, int n_scans, unsigned flags,
                                         pcr_scan_batch **out);
PCR_API pcr_status pcr_scan_batch_size(pcr_scan_batch *b, int *n_scans, int64_t *n_points);
PCR_API pcr_status pcr_scan_batch_destroy(pcr_scan_batch *b);
PCR_API pcr_status pcr_linearize_batch(pcr_target *t, pcr_scan_batch *b, int kind, int n_items, const int *item_scan,
                                       const double *T, double max_dist, unsigned flags, double *out);
PCR_API pcr_status pcr_align_batch(pcr_target *t, pcr_scan_batch *b, int kind, int n_items, const int *item_scan,
                                   const double *T_init, int max_iter, double tol, double max_dist, unsigned flags,
                                   double *T_out, int *iterations, pcr_status *item_status, double *trace_or_null);

/* ---- fine seam: KDTree(data).query(points, k) (kdtree.py:18-65) ------------------------
 * dist is Euclidean (not squared).  For point targets dist is float32 and idx indexes the
 * array given to pcr_target_points_create; for voxel targets use the f64 variant (idx =
 * kept-voxel index).  r_max <= 0 or inf = unbounded (as the reference); with a bound,
 * queries with no neighbour inside r_max get idx = -1, dist = inf.                         */
PCR_API pcr_status pcr_nn_query(pcr_target *t, const float *q, int64_t m, float r_max, float *dist, int64_t *idx);
PCR_API pcr_status pcr_nn_query_f64(pcr_target *t, const float *q, int64_t m, double r_max, double *dist, int64_t *idx);
PCR_API pcr_status pcr_knn_query(pcr_target *t, const float *q, int64_t m, int k, float *dist, int64_t *idx);
/* float64 QUERIES: a voxel target, or a point target with float64 coordinates (pcr_target_points_set_f64).  The query is
 * never rounded: the result is the (float64 distance, index) minimum over the float64 coordinates, what a tree built on
 * the float64 array returns -- also for queries far outside the data.  pcr_knn_query_f64: 1 <= k <= 64, rows nearest first,
 * padded with dist = inf, idx = n when the target holds fewer than k.  PCR_ERR_INVALID for a float32-only point target. */
PCR_API pcr_status pcr_nn_query_dd(pcr_target *t, const double *q, int64_t m, double r_max, double *dist, int64_t *idx);
PCR_API pcr_status pcr_knn_query_f64(pcr_target *t, const double *q, int64_t m, int k, double *dist, int64_t *idx);

/* ---- fixed-radius search over a point target (no reference counterpart) -----------------
 * Everything within r of a query, exactly: a point is a neighbour iff the distance pcr_knn_query (pcr_knn_query_f64 for the
 * _dd pair) would report for the pair is <= r -- sqrtf of the float32 squared distance against r in float32, sqrt of
 * (dx*dx + dy*dy) + dz*dz against r in float64 -- so r = 0 finds coincident points.  A query with a NaN or infinite
 * coordinate has no neighbours.  Two calls, CSR layout: pcr_radius_count writes count[m]; the caller forms
 * offsets[m + 1] = 0 and the running sums of count; pcr_radius_query fills dist / idx [offsets[i], offsets[i + 1]) with the
 * neighbours of query i ordered by (squared distance, index) ascending, the k-NN's order; idx indexes the array given to
 * pcr_target_points_create.  The same call twice returns the same bits.
 * PCR_ERR_INVALID: r negative, NaN or infinite; a voxel target; the _dd pair on a point target without float64 coordinates
 * (pcr_target_points_set_f64); offsets that do not start at 0, decrease, or give a segment a length other than what the
 * search finds -- dist and idx are then left untouched.  m = 0 returns PCR_OK; an empty target counts zero everywhere.
 * A call holds at most PCR_RADIUS_CHUNK entries (environment, default 2^26) on the device at a time: queries are taken in
 * chunks of consecutive queries whose segments fit, a larger query alone; the results do not depend on the chunking.     */
PCR_API pcr_status pcr_radius_count(pcr_target *t, const float *q, int64_t m, float r, int64_t *count);
PCR_API pcr_status pcr_radius_query(pcr_target *t, const float *q, int64_t m, float r, const int64_t *offsets, float *dist, int64_t *idx);
PCR_API pcr_status pcr_radius_count_dd(pcr_target *t, const double *q, int64_t m, double r, int64_t *count);
PCR_API pcr_status pcr_radius_query_dd(pcr_target *t, const double *q, int64_t m, double r, const int64_t *offsets, double *dist,
                                       int64_t *idx);
/* The mean distance from every point of a point target to its k nearest neighbours within the target (1 <= k <= 64; the
 * point itself included, as for normals and covariances): the float32 distances pcr_knn_query reports, summed in float64
 * nearest first and divided by the number found.  mean_out: n doubles in the order of the array the target was created
 * from.  Always searches the float32 copy of the points.                                                              */
PCR_API pcr_status pcr_knn_mean_distance(pcr_target *t, int k, double *mean_out);

/* ---- FPFH descriptors and exact feature matching (no reference counterpart) ---------------
 * Fast Point Feature Histograms (Rusu, Blodow, Beetz, ICRA 2009) in the Open3D form, of a point target that has normals
 * (pcr_target_points_create(..., normals), pcr_target_set_normals or pcr_target_estimate_normals), at a radius r (float32,
 * finite, >= 0).
 * Neighbourhood of point i: every point j of the target that pcr_radius_query returns for the query p_i at r -- the float32
 *   rule sqrtf(dist2_f32) <= r -- except the pairs with d2 == 0, d2 = (dx*dx + dy*dy) + dz*dz in float64 over the widened
 *   float32 coordinates: the point itself and its exact duplicates are dropped, on both passes.  k_i = neighbours left.
 * Pair feature of (p = point i, q = neighbour j), normals np, nq, all in float64 from the widened float32 inputs, no
 *   contraction, every dot product (ax*bx + ay*by) + az*bz:
 *     d = q - p, L = sqrt(d2), a1 = np . d, a2 = nq . d
 *     |a1| < |a2| (strict): n1 = nq, n2 = np, d = -d; otherwise n1 = np, n2 = nq
 *     phi = (n1 . d) / L, v = d x n1
 *     v . v == 0 (d parallel to n1, or a zero normal): alpha = theta = 0; otherwise v = v / sqrt(v . v), w = n1 x v,
 *     alpha = v . n2, theta = atan2(w . n2, n1 . n2)
 *     bin coordinates 11 (alpha + 1) / 2, 11 (phi + 1) / 2, 11 (theta + pi) / (2 pi); bin = clamp(floor(coordinate), 0, 10);
 *     the three features fill three blocks of 11 bins: 33 bins, alpha first.
 * SPFH: unsigned counts per bin over the neighbourhood, and k_i; S_i[b] = 100 count[b] / k_i in float64, 0 when k_i == 0.
 * FPFH: A_i[b] = sum over the neighbourhood of S_j[b] / d2_ij in float64; per 11-bin block F_i[b] = S_i[b] + 100 A_i[b] /
 *   sum_block(A_i) (the second term 0 when the block sum is not > 0), rounded to float32: every block of a point that has
 *   neighbours sums to 200.  The counts are exact; the float64 sums are taken in the order the index is walked, ~1e-14
 *   relative.  No atomics: the same call twice returns the same bits.
 * pcr_target_spfh: counts (n x 33) and k (n); pcr_target_fpfh: fpfh (n x 33) and, when not NULL, k (n); rows in the order of
 *   the array the target was created from.  Always over the float32 copy of the points.
 * PCR_ERR_NO_TARGET: a point target without normals.  PCR_ERR_INVALID: a voxel target; r negative, NaN or infinite.  An
 *   empty target returns PCR_OK without a launch.
 *
 * pcr_feature_match: for every row i of A (na x dim) its nearest row of B (nb x dim), float32, 1 <= dim <= 64 (else
 *   PCR_ERR_INVALID), host arrays.  d2(i, j) = the float32 sum over c = 0 .. dim - 1, in that order, of (A[i,c] - B[j,c])^2,
 *   every step a separate subtract, multiply and add.  idx[i] = the j that minimises the key (d2, j), d2_first[i] that
 *   distance, d2_second[i] the distance of the second smallest key over all j (equal to d2_first for duplicate rows of B, inf
 *   when nb == 1).  A NaN distance never wins; a row with no other distance gets idx = -1, d2_first = inf.  The result
 *   does not depend on how the work is tiled or split.  na == 0 returns PCR_OK; nb == 0 fills idx = -1 and both distances
 *   with inf; neither launches anything.                                                                                */
PCR_API pcr_status pcr_target_spfh(pcr_target *t, float r, uint32_t *counts, int64_t *k);
PCR_API pcr_status pcr_target_fpfh(pcr_target *t, float r, float *fpfh, int64_t *k_or_null);
PCR_API pcr_status pcr_feature_match(pcr_context *ctx, const float *A, int64_t na, const float *B, int64_t nb, int dim,
                                     int64_t *idx, float *d2_first, float *d2_second);
/* pcr_target_fpfh_rows: the descriptors of m chosen points only -- fpfh (m x 33) and, when not NULL, k (m); row s belongs to
 *   point rows[s] (an index into the array the target was created from) and equals row rows[s] of pcr_target_fpfh bit for
 *   bit: the SPFH pass still runs over the whole target (the neighbours' histograms are needed), the second pass and the
 *   copy-back cover the m rows.  rows must be strictly ascending and inside [0, n), else PCR_ERR_INVALID with the outputs left
 *   untouched; the other refusals are pcr_target_fpfh's.  m == 0 returns PCR_OK without a launch.                        */
PCR_API pcr_status pcr_target_fpfh_rows(pcr_target *t, float r, const int64_t *rows, int64_t m, float *fpfh, int64_t *k_or_null);

/* ---- ISS keypoints (no reference counterpart) ----------------------------------------------
 * Intrinsic Shape Signatures (Zhong, ICCV workshops 2009) in the Open3D form, of a point target, over the float32 copy of the
 * points; no normals are needed.
 * Support set N_r(i): exactly what pcr_radius_query finds for the query p_i at r -- the float32 rule sqrtf(dist2_f32) <= r --
 *   the point itself and its exact duplicates included.  k_i = |N_r(i)|.
 * Scatter matrix of i at the salient radius, all in float64 from the widened float32 inputs, no contraction, every sum a plain
 *   +: the members are taken in ascending order of the index's cell-sorted position (the order in which the radius search
 *   walks them for ANY query); the anchor a is the first member; for every member d = q - a, s1 += d (3 sums),
 *   s2 += d d^T (6 sums); m = s1 / k, C = s2 / k - m m^T, stored xx xy xz yy yz zz.  The anchor and the order are functions of
 *   the member set, not of the query: two points with the same support set get bit-identical sums and eigenvalues.
 * Eigenvalues l1 >= l2 >= l3 of C: cyclic Jacobi in float64 (the sweep rule of the normal estimation), the sorted diagonal.
 * Saliency: i is salient iff k_i >= min_neighbors, l1 > 0, l2 < gamma21 * l1, l3 < gamma32 * l2 and l3 > 0 (products, no
 *   division); s_i = l3 when salient, else 0.
 * Keypoint at the non-maximum radius rn: s_i > 0, |N_rn(i)| >= min_neighbors (the point itself included), and for every other
 *   j in N_rn(i): s_j < s_i, or s_j == s_i and orig_j > orig_i (orig = the index in the caller's array): a tie goes to the
 *   smaller original index, a cluster of exact duplicates yields at most one keypoint.
 * Defaults of the Python layer, as Open3D's: gamma21 = gamma32 = 0.975, min_neighbors = 5; radii of 6 x and 4 x the cloud's
 *   resolution, resolution = 2 * mean(pcr_knn_mean_distance(t, 2)) in float64 (that call counts the point itself at distance
 *   0), both rounded to float32.
 * pcr_target_iss_saliency: eig (n x 3, l1 l2 l3), saliency (n) and k (n); pcr_target_iss_keypoints: is_keypoint (n bytes,
 *   0 / 1) and, when not NULL, saliency (n); everything in the order of the array the target was created from.  No atomics:
 *   the same call twice returns the same bits.
 * PCR_ERR_INVALID: a voxel target; a radius negative, NaN or infinite; a gamma that is not finite and > 0;
 *   min_neighbors < 1 -- the outputs are then left untouched.  An empty target returns PCR_OK without a launch.           */
PCR_API pcr_status pcr_target_iss_saliency(pcr_target *t, float r, double gamma21, double gamma32, int min_neighbors,
                                           double *eig /* n x 3 */, double *saliency, int64_t *k);
PCR_API pcr_status pcr_target_iss_keypoints(pcr_target *t, float r_salient, float r_nonmax, double gamma21, double gamma32,
                                            int min_neighbors, uint8_t *is_keypoint, double *saliency_or_null);

/* ---- radius and hybrid neighbourhoods for normals and covariances (no reference counterpart) ----
 * The k nearest neighbours of a LiDAR return lie on its own ring line; a ball (Open3D's KDTreeSearchParamRadius, PCL's
 * setRadiusSearch) or a ball capped at its nearest max_nn (KDTreeSearchParamHybrid) does not.  For a point p of a cloud, a
 * radius r (float32, finite, >= 0) and 0 <= max_nn <= 64, always over the float32 copy of the points:
 * Radius set (max_nn == 0): exactly what pcr_radius_query returns for the query p against its own cloud -- the float32 rule
 *   sqrtf(dist2_f32) <= r, p itself and its exact duplicates included; a point with a NaN or infinite coordinate has the
 *   empty set.
 * Hybrid set (1 <= max_nn <= 64): the first min(max_nn, count) entries of that segment in its order, (squared distance, index)
 *   ascending: the nearest max_nn OF THE BALL, with the radius search's <= r -- not the bounded k-NN's strict <.
 * Moments, all in float64 from the widened float32 inputs, no contraction, every sum a plain +: count = the members of the
 *   set; the anchor a = the first member in summation order; for every member d = q - a, s1 += d (3 sums), s2 += d d^T (6
 *   sums); mean = a + s1 / count; raw covariance C = s2 / count - (s1 / count)(s1 / count)^T, stored xx xy xz yy yz zz -- the
 *   arithmetic of the ISS scatter matrix above.  The empty set has count 0, mean 0 and C = 0.
 * Summation order: the radius set in ascending order of the index's cell-sorted position (the order in which the radius
 *   search walks the members for ANY query), so two points with the same set get the same bits; the hybrid set in list order,
 *   nearest first.
 * Normal: the unit eigenvector of the smallest eigenvalue of C (cyclic Jacobi in float64, as pcr_target_estimate_normals),
 *   rounded to float32; exactly (0, 0, 0) when count < 3.  A zero normal makes PlaneICP's row vanish (J = 0, r = 0) instead of
 *   pulling along an arbitrary direction: a target point whose ball holds fewer than three points takes no part in its pose.
 *   (SymmetricICP averages it with the scan's normal; its min_cos > 0 gates such a pair out.)
 * Covariance: C through the mode / eps finish of pcr_target_estimate_covariances (PCR_COV_PLANE: I - (1 - eps) n n^T with n the
 *   eigenvector above; PCR_COV_RAW: C itself), rounded to float32.  A set of one member (or none) has C = 0: that call's k = 1.
 * pcr_target_ball_moments: count (n), mean3 (n x 3), cov6 (n x 6, the raw covariance) in the order of the array the target
 *   was created from.  pcr_target_estimate_normals_radius fills the target's normals exactly as pcr_target_estimate_normals
 *   does (pcr_target_get_normals, PlaneICP, SymmetricICP, ColoredICP and FPFH then read them; a colour payload is freed),
 *   pcr_target_estimate_covariances_radius its covariances as pcr_target_estimate_covariances does; the _scan_ pair estimates
 *   every scan point within the scan, as pcr_scan_estimate_normals / _covariances do.  The _out_or_null arrays receive the
 *   estimate and the counts in the caller's order.  No atomics: the same call twice returns the same bits.
 * PCR_ERR_INVALID, checked in this order, nothing written: a NULL argument; r negative, NaN or infinite; max_nn outside
 *   [0, 64]; (covariances) a bad mode / eps; a voxel target; a scan that does not know the caller's order where an output is
 *   asked for.  An empty cloud returns PCR_OK without a launch.
 * PCR_BALL_TIMES=1 (environment, read once): every call reports its kernel's milliseconds on stderr.                     */
PCR_API pcr_status pcr_target_ball_moments(pcr_target *t, float r, int max_nn, int64_t *count, double *mean3, double *cov6);
PCR_API pcr_status pcr_target_estimate_normals_radius(pcr_target *t, float r, int max_nn, float *normals_out_or_null,
                                                      int64_t *count_out_or_null);
PCR_API pcr_status pcr_scan_estimate_normals_radius(pcr_scan *s, float r, int max_nn, float *normals_out_or_null,
                                                    int64_t *count_out_or_null);
PCR_API pcr_status pcr_target_estimate_covariances_radius(pcr_target *t, float r, int max_nn, int mode, double eps,
                                                          float *cov_out_or_null, int64_t *count_out_or_null);
PCR_API pcr_status pcr_scan_estimate_covariances_radius(pcr_scan *s, float r, int max_nn, int mode, double eps,
                                                        float *cov_out_or_null, int64_t *count_out_or_null);

/* ---- pose hypotheses from correspondences: RANSAC (no reference counterpart) ---------------
 * The last third of a global registration: from matches (pcr_feature_match) to a pose that an aligner can start from.
 * src, dst: m x 3 float32 host arrays, finite; row j is one correspondence, scan point -> map point.  A pose is 12 float32:
 *   R row-major (9), then t (3); it maps src into the frame of dst (the init_T convention of pcr_align).
 * Inlier rule, float32, no fma, exactly this order:
 *     x = ((R00*px + R01*py) + R02*pz) + tx, likewise y and z;  d = x - q;  d2 = (dx*dx + dy*dy) + dz*dz
 *   row j is an inlier iff d2 <= thr, thr = max_dist * max_dist in float32; a NaN anywhere is not an inlier.  count = the
 *   number of inliers, an integer: independent of tiling, splitting and order.
 * Sampling, counter-based: hypothesis h depends on (seed, h, m) only.  mix = SplitMix64's step,
 *     z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31
 *   (mix(0) = 0xE220A8397B1DCDAF, mix(1) = 0x910A2DEC89025CC1).  s = mix(seed), u_k = mix(s ^ (4h + k)) for k = 0, 1, 2,
 *     c0 = mulhi64(u_0, m), c1 = mulhi64(u_1, m - 1), c2 = mulhi64(u_2, m - 2)
 *     c1 += (c1 >= c0);  a = min(c0, c1), b = max(c0, c1):  c2 += (c2 >= a), then c2 += (c2 >= b)
 *   -- uniform over the ordered triples of distinct rows.  m < 3 gives no hypotheses.
 * Validity, float64 over the widened float32 points, no contraction, every dot product (ax*bx + ay*by) + az*bz: for the
 *   edges (i, j) = (0,1), (1,2), (2,0): a2 = |p_i - p_j|^2, b2 = |q_i - q_j|^2; valid iff every edge has a2 >= s^2 b2,
 *   b2 >= s^2 a2, a2 >= e^2 and b2 >= e^2 (s = edge_similarity, e = min_edge, widened to float64: Open3D's edge-length checker
 *   plus a minimum edge length), and both triangles are non-degenerate: |e1|^2 > 0 and |e1 x e2|^2 > 0 on each side.
 * Fit, the triad construction in float64 with +, -, x, / and sqrt only: on the source side e1 = p1 - p0, e2 = p2 - p0,
 *   w = e1 x e2, u1 = e1 / sqrt(e1 . e1), u3 = w / sqrt(w . w), u2 = u3 x u1; the same on the destination side gives v1, v2,
 *   v3 (a x b = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx));
 *     R[r][c] = (v1[r]*u1[c] + v2[r]*u2[c]) + v3[r]*u3[c];  cp = ((p0 + p1) + p2) / 3, cq likewise;
 *     t[r] = cq[r] - ((R[r][0]*cp[0] + R[r][1]*cp[1]) + R[r][2]*cp[2]);  R and t rounded to float32.
 *   An invalid hypothesis has an all-NaN pose and count = -1.  (The 3-point least-squares fit is deliberately not used: it
 *   needs an eigen or singular value solver that no restatement matches bit for bit; least squares belongs to the refinement
 *   over all inliers, on the host.)
 * Selection: the largest count, ties to the smallest h -- a maximum over a key, so it does not depend on the grid or on the
 *   chunks (PCR_RANSAC_CHUNK hypotheses at a time, default 2^20, read once per process: device memory is bounded by about
 *   48 bytes x chunk).  Residual sums take no part; there is no early termination: two calls return the same bits.  No valid
 *   hypothesis: best = -1, the identity pose, count = 0, PCR_OK.
 * pcr_pose_score: count[i] (and, when not NULL, mask[i * m + j] = 0 / 1 bytes) of poses[i] over all m rows.  With few poses the
 *   rows are split over blocks and the integer partial counts added; pcr_pose_score_splits(m, b) is the host-side rule (needs
 *   no device): the number of row splits a call with these sizes uses.  Rows pass through tiles of PCR_RANSAC_TILE.
 * pcr_ransac_poses: n_hyp hypotheses of `seed`; *best, best_pose, *best_count, *n_valid (the number of valid hypotheses) and,
 *   when not NULL, per hypothesis the three sampled rows, the pose and the count.  With m < 3 (and n_hyp > 0) those arrays
 *   read as invalid hypotheses: rows -1, NaN poses, counts -1.
 * PCR_ERR_INVALID: max_dist or min_edge negative or non-finite; edge_similarity outside [0, 1]; m > 2^24; n_hyp (or b) < 0 or
 *   > 2^26; src or dst non-finite.  m == 0, b == 0, n_hyp == 0 and m < 3 return PCR_OK without a launch: counts 0, best -1.
 *   One GPU of one process.  A refused call leaves the context usable.                                                    */
#define PCR_RANSAC_TILE 256
PCR_API pcr_status pcr_pose_score(pcr_context *ctx, const float *src, const float *dst, int64_t m, const float *poses /* b x 12 */,
                                  int64_t b, float max_dist, int32_t *count /* b */, uint8_t *mask_or_null /* b x m */);
PCR_API pcr_status pcr_ransac_poses(pcr_context *ctx, const float *src, const float *dst, int64_t m, int64_t n_hyp, uint64_t seed,
                                    float max_dist, float edge_similarity, float min_edge, int64_t *best, float best_pose[12],
                                    int32_t *best_count, int64_t *n_valid, int32_t *samples_or_null /* n_hyp x 3 */,
                                    float *poses_or_null /* n_hyp x 12 */, int32_t *counts_or_null /* n_hyp */);
PCR_API int pcr_pose_score_splits(int64_t m, int64_t b);

/* ---- a pose from correspondences without hypotheses: fast global registration (no reference counterpart) ---------------
 * Zhou, Park, Koltun (ECCV 2016), what Open3D's registration_fgr_based_on_feature_matching does after the matching: a few
 * dozen Gauss-Newton steps over the matches themselves under a Geman-McClure line process whose scale mu is annealed from
 * "everything is an inlier" down to the inlier distance.  Cost: iterations x matches; deterministic by construction.
 * src, dst: m x 3 float32 host arrays, finite; row j is one match p -> q.  mult: m int32 >= 0, the multiplicity c_j of a
 *   match (NULL: all 1).  The pose T is 16 doubles, row-major, and maps src into the frame of dst.
 * One pass at (T, mu): float64 over the widened float32 points, no fma, every dot product (a*b + c*d) + e*f:
 *     x = ((R00*px + R01*py) + R02*pz) + tx, likewise y and z;  r = x - q;  r2 = (r0*r0 + r1*r1) + r2*r2
 *     l = mu / (mu + r2);  w = c_j * (l*l)
 *     J = [I, -skew(x)]:  row 0 = [1 0 0  0  x2 -x1],  row 1 = [0 1 0  -x2 0 x0],  row 2 = [0 0 1  x1 -x0 0]
 *     out[0..20] += w * triu(J^T J), out[21..26] += w * J^T r, out[27] += w * r2, out[28] += w
 *   with the terms written out (each is w times the bracket; a leading minus negates the product, which is exact):
 *     triu(J^T J), row by row:  1 0 0 0 x2 -x1 | 1 0 -x2 0 x0 | 1 x1 -x0 0 | (x1*x1 + x2*x2) -(x0*x1) -(x0*x2) |
 *                               (x0*x0 + x2*x2) -(x1*x2) | (x0*x0 + x1*x1)
 *     J^T r:  r0, r1, r2, (x1*r2 - x2*r1), (x2*r0 - x0*r2), (x0*r1 - x1*r0)
 *   The weight handed out per match is l*l (without c_j): a fixed sequence of +, x and / in float64.
 * Summation: the unit is the tile of PCR_FGR_TILE consecutive matches.  The terms of a tile are folded in a fixed order (wave
 *   shuffles, then the four waves in wave order) into ONE row of sums, and the rows are added in ascending tile order.  Which
 *   block folds which tile does not enter (a block takes PCR_FGR_WIDTH consecutive tiles per trip; pcr_fgr_blocks(m) is the
 *   host-side rule for the grid, PCR_FGR_BLOCKS in the environment caps it): the sums do not depend on the grid, there are
 *   no atomics, and the same call twice returns the same bits.
 * Step: dx = -solve(H, g) (LU with partial pivoting, an exactly zero pivot = singular), |dx| = sqrt of the six squares added
 *   in index order.  The update is LEFT-multiplied: T <- [exp(dx[3:]), dx[:3]; 0 1] * T (exp: first order below |w|^2 <= 1e-5,
 *   Rodrigues above; every entry of the product the sum over k = 0 .. 3 in order).  The local aligners' J = [I, -R skew(p)]
 *   with T <- T * dT is NOT used here: its translation block is right near R = I only, and this loop starts anywhere.
 * Schedule: after iteration it (from 0), if (it + 1) % period == 0 and mu > mu_min: mu = max(mu / division, mu_min).
 * Loop (pcr_fgr_pose), for it = 0 .. max_iter - 1: pass at (T, mu); trace row it = T (16), the 29 sums, mu (PCR_FGR_TRACE
 *   doubles); a singular system ends it with status 2, T staying at the last good pose; when tol > 0, mu == mu_min and
 *   |dx| < tol it ends with status 1 (the test precedes the update: T stays); else the update and the schedule.  Status 0:
 *   max_iter passes were made.  *iterations = the passes made (trace rows written; the rest of the trace is 0), *mu_final =
 *   mu after the last schedule step, weight = l*l of every match at (T_out, *mu_final).  The default form keeps pose, mu
 *   and counter on the device and enqueues all passes back to back; PCR_FLAG_HOST_LOOP reads the 29 sums back and steps on
 *   the host, per iteration: the same arithmetic, the same bits.
 * pcr_fgr_tuples: Open3D's tuple test with RANSAC's sampler and validity rule above.  Tuple h = the three rows of hypothesis
 *   h of `seed`; it is valid iff its three edges pass the edge-length rule with s = tuple_scale and e = min_edge and both
 *   triangles are non-degenerate.  mult[j] = the number of valid tuples row j is in (an integer count: independent of order
 *   and of the chunks, PCR_FGR_CHUNK tuples per launch, default 2^20), *n_valid = the valid tuples.  m < 3: all 0.
 * PCR_ERR_INVALID: src or dst non-finite; mu, mu0 or mu_min not finite or not > 0; division <= 1; period < 1; max_iter < 0;
 *   a negative mult; m > 2^24; n_tuples < 0 or > 2^26; tuple_scale outside [0, 1]; min_edge negative or non-finite -- the
 *   outputs are then left untouched and the context stays usable.  m == 0 or max_iter == 0 return PCR_OK without a launch:
 *   T_out = T_init, zero sums, 0 iterations, status 0, mu_final = mu0, weights 1.  One GPU of one process.               */
#define PCR_FGR_TILE 256
#define PCR_FGR_WIDTH 4
#define PCR_FGR_TRACE 46
PCR_API pcr_status pcr_fgr_linearize(pcr_context *ctx, const float *src, const float *dst, int64_t m, const int32_t *mult_or_null,
                                     const double T[16], double mu, double out[29], double *weight_or_null /* m */);
PCR_API pcr_status pcr_fgr_pose(pcr_context *ctx, const float *src, const float *dst, int64_t m, const int32_t *mult_or_null,
                                const double T_init[16], double mu0, double mu_min, double division, int period, int max_iter,
                                double tol, unsigned flags, double T_out[16], int *iterations,
                                int *status /* 0 ran out, 1 converged, 2 singular */, double *mu_final,
                                double *weight_or_null /* m */, double *trace_or_null /* max_iter x PCR_FGR_TRACE */);
PCR_API pcr_status pcr_fgr_tuples(pcr_context *ctx, const float *src, const float *dst, int64_t m, int64_t n_tuples, uint64_t seed,
                                  float tuple_scale, float min_edge, int32_t *mult /* m */, int64_t *n_valid);
PCR_API int pcr_fgr_blocks(int64_t m);
/* developer builds carry a single-block form of the loop for match lists that fit into the LDS of one workgroup (the same
 * bits, measured slower; PCR_FGR_SOLO=1 in the environment selects it for every list that fits): *m_max = the largest list
 * it serves on this device, 0 in a library without it                                                                   */
PCR_API pcr_status pcr_fgr_solo_max(pcr_context *ctx, int64_t *m_max);

/* ---- consensus sets from the compatibility graph of the matches: SC2 (no reference counterpart) ---------------
 * Where 1-3 % of the matches are right, a triple of matches is clean once in 10^6 (RANSAC) and the right ones do not dominate
 * the first Gauss-Newton steps (FGR).  The length of a pair of matches is invariant under a rigid motion, so the right ones
 * can be told apart before any pose exists: the compatibility graph of TEASER and of SC2-PCR (Chen et al., CVPR 2022), and
 * its second-order measure, the number of compatible neighbours that two compatible matches share.  Everything below is an
 * integer: two calls, any grid and a restatement agree bit for bit.
 * src, dst: m x 3 float32 host arrays; row i is one match p_i -> q_i.  Non-finite values are allowed (see below).
 * 1. Compatibility, float64 over the widened float32 points, no fma, every dot product (x*x + y*y) + z*z:
 *      a2 = |p_i - p_j|^2, b2 = |q_i - q_j|^2;  C_ij = 1 iff i != j and fabs(sqrt(a2) - sqrt(b2)) <= d
 *    (the float64 sqrt is correctly rounded).  Negating a difference is exact, so C is symmetric by construction; a NaN
 *    anywhere makes the comparison false: a match with a non-finite coordinate is compatible with nothing.  C is a bit matrix
 *    of m rows of W = ceil(m / 64) 64-bit words: bit (j & 63) of word (j >> 6) of row i is C_ij; the diagonal and the padding
 *    bits of the last word are 0.
 * 2. Degrees: deg1_i = popcount(row_i);  deg2_i = the sum over j with C_ij = 1 of popcount(row_i & row_j) -- the row sum of
 *    C o (C C), twice the number of triangles of the graph through i.
 * 3. Seeds: the n_seeds rows with the largest deg2, ties to the smaller row, in that order; n_seeds is clipped to m
 *    (*n_seeds_out = min(n_seeds, m), so many rows of seeds / members / scores are written).
 * 4. The consensus set of seed s, k slots: s itself comes first, its score = popcount(row_s) = deg1_s; then up to k - 1 rows j
 *    with C_sj = 1 by score_sj = popcount(row_s & row_j) descending, ties to the smaller j -- the maximum of the 64-bit key
 *    (score << 32) | (0xffffffff - j), k - 1 times; rows with score 0 are included, last.  Slots beyond the set: member -1,
 *    score -1.
 * The pose from these sets (a least-squares fit per seed, scored with pcr_pose_score, the winner refined) is the host's:
 *   global_registration.py: sc2_pose.  The two-stage selection and the spectral weights of the paper are left out.
 * pcr_compat_consensus builds the bits once, computes the degrees, picks the seeds on the host and runs the consensus kernel.
 * PCR_ERR_INVALID: m < 0 or m > PCR_COMPAT_M_MAX; d not finite or not > 0; k < 2 or k > PCR_COMPAT_K_MAX; n_seeds < 1 -- the
 *   outputs are then left untouched and the context stays usable.  m == 0 returns PCR_OK without a launch and writes nothing
 *   but *n_seeds_out = 0.  PCR_COMPAT_TIMES=1 in the environment (read once per process) reports the kernels' milliseconds on
 *   stderr.  One GPU of one process.                                                                                      */
#define PCR_COMPAT_M_MAX 32768        /* bit matrix <= 128 MiB */
#define PCR_COMPAT_K_MAX 64
PCR_API pcr_status pcr_compat_bits(pcr_context *ctx, const float *src, const float *dst, int64_t m, double d,
                                   uint64_t *bits /* m x ceil(m / 64) */);
PCR_API pcr_status pcr_compat_degrees(pcr_context *ctx, const float *src, const float *dst, int64_t m, double d, int64_t *deg1 /* m */,
                                      int64_t *deg2 /* m */);
PCR_API pcr_status pcr_compat_consensus(pcr_context *ctx, const float *src, const float *dst, int64_t m, double d, int n_seeds, int k,
                                        int64_t *deg1_or_null /* m */, int64_t *deg2_or_null /* m */, int32_t *seeds /* n_seeds */,
                                        int32_t *members /* n_seeds x k */, int32_t *scores /* n_seeds x k */, int *n_seeds_out);

/* ---- instrumentation ------------------------------------------------------------------
 * With profiling on, every launch of a hot-path kernel is bracketed by HIP events on the
 * context's stream; pcr_profile_read drains them (synchronises) and reports per-kernel
 * launch count and total milliseconds since the last reset.  on = n > 1 brackets only every
 * n-th pass (an event pair costs a few microseconds of stream time: sampling keeps a timed
 * region honest); on = 1 every pass; 0 off.  pcr_align's device-resident loop keeps up to two
 * iterations queued beyond the one that converges: those launches return at once but are
 * bracketed like the others, so per-kernel averages taken over an align include them.        */
enum { PCR_K_LINEARIZE = 0, PCR_K_FINALIZE = 1, PCR_K_NN = 2, PCR_K_REDUCE = 3, PCR_K_ALLREDUCE = 4, PCR_K_CERTIFY = 5, PCR_K_COUNT = 6 };
PCR_API pcr_status pcr_profile_enable(pcr_context *ctx, int on);
PCR_API pcr_status pcr_profile_reset(pcr_context *ctx);
PCR_API pcr_status pcr_profile_read(pcr_context *ctx, int64_t launches[PCR_K_COUNT], double total_ms[PCR_K_COUNT]);
/* the same with the caller's array capacity stated (at most `capacity` entries are written; *count = PCR_K_COUNT of
 * the library): what a binding compiled against an older header should call                                       */
PCR_API pcr_status pcr_profile_read_n(pcr_context *ctx, int capacity, int64_t *launches, double *total_ms, int *count);
/* grid geometry of a target's NN index: cell size, dims, occupied cells, points (or voxels) */
PCR_API pcr_status pcr_target_index_info(pcr_target *t, double *cell, int64_t dims[3], int64_t *occupied, int64_t *n);
/* How unevenly the points fill the index (round 6): the largest and the 99th-percentile population of an OCCUPIED cell, and
 * whether the target was built as "heavy" (some cells hold far more points than the average -- a LiDAR sweep's ring lines,
 * density ~ 1/r^2): its cell edge then stops at PCR_CELLS_PER_POINT (default 8) grid cells per point instead of shrinking to
 * ~5 points per occupied cell, the points of a cell are Morton-sorted, and every range of more than 24 records is searched
 * through boxes over 64 and 8 consecutive records (csrc/nn_device.h: nn_scan_range_lb).  Any pointer may be NULL.         */
PCR_API pcr_status pcr_target_index_population(pcr_target *t, int64_t *pop_max, int64_t *pop_p99, int *heavy);
/* point targets: *xq = the x quantum (metres, cell / 65536) when the records of every cell and of every extended list are
 * stored in ascending x, so that the plain search scans a row of cells from the query's x outward; 0 when they are not
 * (heavy targets, voxel targets, PCR_XORDER=0 in the environment when the target was built).
 * pcr_x_order_rule: the host-side rule behind it (needs no device): 1 when a target of `n` points whose cell ids take
 * `cell_bits` bits gets the x order -- float32 point targets without heavy cells, unless PCR_XORDER=0                       */
PCR_API pcr_status pcr_target_index_x_order(pcr_target *t, double *xq);
PCR_API int pcr_x_order_rule(int f32_point_target, int heavy, int64_t n, int cell_bits);
/* point targets: margin (metres) and total records of the extended per-cell lists ring 0 searches (a cell's
 * own points plus the neighbours' points within the margin of the shared face; PCR_HALO sets the margin as a
 * fraction of the cell edge, default 0.1, 0 = none).  Voxel targets: the same of the float32 filter index over
 * the rounded centroids (both 0: the target has no filter -- coordinates too large -- and searches in float64) */
PCR_API pcr_status pcr_target_index_halo(pcr_target *t, double *halo, int64_t *records);
/* point targets: the same of the second, deeper set of lists (margin 0.25 x cell), which the library builds once a target
 * has served a dozen search + reduce passes and which serves the passes of a Gauss-Newton run whose scan still moves by
 * 0.12 to 0.4 cell per pass (the mid set); both 0 while it does not exist                                              */
PCR_API pcr_status pcr_target_index_halo2(pcr_target *t, double *halo, int64_t *records);
/* point targets: margin and records of list set `set`: 0 near (= pcr_target_index_halo), 1 mid (= pcr_target_index_halo2),
 * 2 far (margin 0.35 x cell, built with the mid set except on heavy targets, serves the passes whose scan moves by 0.4 to
 * 1.5 cell; beyond that the near set, no list reaching across such a step); both 0 while
 * the set does not exist                                                                                               */
PCR_API pcr_status pcr_target_index_list_set(pcr_target *t, int set, double *halo, int64_t *records);
/* voxel targets: the bound (metres) on how far rounding to float32 moved any centroid of the filter index -- what the
 * float32 filter search of the centroid search (voxel.py:171-179) subtracts from its lower bounds before the float64
 * check; 1.75 x 2^-24 x the largest coordinate magnitude of the centroid grid.  0 = no filter index (not built yet:
 * the first search + reduce pass builds it; or refused: band > 1 % of the index cell)                               */
PCR_API pcr_status pcr_target_filter_band(pcr_target *t, double *band);
/* work counters of the NN search for one pose (point targets): out[0..3] = rings entered, row
 * segments loaded, rows pruned by arithmetic, candidates tested, summed over queries; out[4..7] = the
 * same with each wave's maximum charged to all 64 lanes (the cost under divergence); out[8..10] =
 * wave wall-clock cycles summed over waves: prologue (load, transform, cell), ring 0, outer rings.
 * pcr_nn_counters_x: the same traversal on a target in the OLD order inside a cell (built under
 * PCR_XORDER=0, no heavy cells; zeros otherwise): out[0] = candidates tested, out[1..2] = those of them
 * whose bound (p.x - q.x)^2 + (slab distance of the row)^2 was within the best distance at the time of
 * the test / within the final best -- what a scan that knew the order of x inside a row could not have
 * skipped, summed over queries.
 * pcr_nn_counters_edge: the queries OUTSIDE the target's grid box on their own: out[0] = how many, out[1..2] = their
 * candidates and row segments, out[3..4] = the wave maxima of candidates and of row segments charged to them, out[5..6] =
 * waves of 64 queries that hold at least one / all waves, out[7..8] = queries inside the box whose own cell is empty and
 * has no list (they start from the cell's seed) and their candidates                                 */
PCR_API pcr_status pcr_nn_counters(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double out[11]);
PCR_API pcr_status pcr_nn_counters_x(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double out[3]);
PCR_API pcr_status pcr_nn_counters_edge(pcr_target *t, pcr_scan *s, const double T[16], double max_dist, double out[9]);
/* select the hot-path variant: 2 (default) = chosen per launch by the size of the scan: 1 = NN kernel
 * writing correspondences to HBM followed by a reduce kernel (faster for large scans: twice the
 * occupancy), 0 = one fused transform+NN+reduce kernel (faster for small, latency-bound scans: 100 k
 * points 49 vs 59 us per pass); either way the last blocks fold the partial sums inside the kernel   */
PCR_API pcr_status pcr_set_variant(pcr_context *ctx, int variant);
PCR_API pcr_status pcr_get_variant(pcr_context *ctx, int *variant);
/* NN search kernel of variant 1: 0 = per-lane ring search (shipped; plain passes over a voxel target run a float32 filter
 * search over the rounded centroids and check its winner in float64 -- results identical to the float64 search),
 * 2 = wave-cooperative LDS-staged search, 3 = as 0 with the centroid search in float64 throughout (A/B, tests),
 * 4 = wave-cooperative search with an MFMA distance filter (round 5); 2 and 4: developer build only                */
PCR_API pcr_status pcr_set_nn_mode(pcr_context *ctx, int mode);
/* Certified reuse of the previous pass' matches (no reference counterpart: Registration.align,
 * registration.py:89-111, searches afresh every iteration).  When consecutive passes over one scan and target
 * differ by a small pose change, a pass first proves -- per point, by the triangle inequality on a bound the
 * previous search recorded -- that the old match is still the exact nearest neighbour, and searches only the
 * points where the proof fails.  The correspondences, and therefore all 29 sums, are bit-identical to a full
 * search; only the time changes.  mode: 0 = off (the DEFAULT since round 5: at the reference's tol = 1e-3 a Gauss-Newton
 * run stops as soon as its steps reach millimetres, the automatic policy never engaged on a BASELINE config, and the state
 * costs 4 bytes per scan point -- opt in for tight tolerances / re-evaluation in place, where it pays 1.2-2.6x), 1 =
 * automatic (tried when the scan's typical displacement since the last pass is below tau x cell size of the target's
 * index), 2 = always.  mu = how far beyond its match a tracking search looks, x cell size.  tau / mu <= 0 keep the
 * current value.  PCR_REUSE in the environment sets the mode of new contexts.                                          */
PCR_API pcr_status pcr_set_reuse(pcr_context *ctx, int mode, double tau, double mu);
PCR_API pcr_status pcr_get_reuse(pcr_context *ctx, int *mode, double *tau, double *mu);
/* out[0..2] = passes over this scan by search mode (full, tracking, certify + list); out[3] / out[4] = points
 * the list passes had to search / points they covered; out[5..7] = mode, searched points (-1 = not read
 * back) and typical displacement (m) of the last pass                                                      */
PCR_API pcr_status pcr_scan_reuse_stats(pcr_scan *s, double out[8]);
/* How many pcr_linearize passes of this context had the last level of their fold taken by the host: a host-driven pass on
 * one GPU (no communicator) that is neither ICP nor a certify + list pass hands the host 8 partial rows in pinned memory
 * instead of folding them on the device; the host adds them in the device's order, so the sums are bit-identical.
 * PCR_HOST_FOLD=0 in the environment of a new context keeps every pass on the device path (the count stays 0).       */
PCR_API pcr_status pcr_context_host_fold_passes(pcr_context *ctx, uint64_t *passes);
/* variant 1: 1 (default) = the reduce kernel folds the per-block partial sums itself
 * (k_reduce_finalize); 0 = separate fold kernel                                             */
PCR_API pcr_status pcr_set_fuse_finalize(pcr_context *ctx, int on);
/* 1 when the library carries the developer / A-B kernels (unfused folds, the wave-cooperative LDS-staged search, the work
 * counters: csrc/kernels_dev.hip) -- libpcr_hip_dev.so, built by `make DEV=1`; the shipped libpcr_hip.so returns 0 and
 * refuses pcr_set_nn_mode(2), pcr_set_fuse_finalize(0) and pcr_nn_counters with PCR_ERR_INVALID.                      */
PCR_API int pcr_has_dev_kernels(void);
PCR_API pcr_status pcr_get_pipeline(pcr_context *ctx, int *variant, int *fuse_finalize, int *nn_mode);

#ifdef __cplusplus
}
#endif
#endif /* PCR_H */
