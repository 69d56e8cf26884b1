"""Gauss-Newton driver with the reference's ``Registration`` interface.

Same names, arguments and error behaviour as ``point_cloud_registration/registration.py:10-113``:
``set_target`` / ``is_target_set`` / ``align(source, init_T, verbose)`` /
``calc_H_g_e2(cur_T, source) -> (H 6x6, g 6, e2)``.  The O(N) body of ``calc_H_g_e2`` is one
call into libpcr_hip.so (transform + exact NN + gate + residual/Jacobian + 6x6 reduction on the
MI355X); the 6x6 solve, the boxplus and the tolerance test stay on the host, as in the
reference.

Additions (none changes a default):
* ``device=`` -- which GPU this process drives (default ``LOCAL_RANK``);
* ``comm=`` -- a :class:`distributed.Communicator`; the scan passed to ``align`` is then this
  rank's SHARD and every ``calc_H_g_e2`` returns the sum over all ranks;
* ``devices=`` -- a list of GPU ids for ONE process (``PlaneICP(devices=[0, 1, 2, 3, 4, 5, 6, 7])``): ``set_target`` builds
  the target on every listed GPU, ``align`` / ``calc_H_g_e2`` take the WHOLE scan, shard it across them behind the C ABI
  (``pcr_group_*``) and exchange the 29 sums GPU to GPU -- the reference's single-process call order
  (registration.py:28,71; demo_matching.py:147-152) on a whole node, no torchrun (SURVEY.md sections 5 and 8b);
* ``upload(source)`` -- returns a handle to the device copy of a scan; ``calc_H_g_e2(cur_T, handle)`` and
  ``align(handle)`` then skip the upload and the per-call content hash of the array form;
* ``native_loop`` (default True) -- ``align`` runs the whole loop behind the C ABI (``pcr_align``):
  pose in HBM, solve + boxplus in a one-wave kernel behind the reduce kernel, iterations enqueued back to
  back, one result read by the host.  ``native_loop=False`` keeps the Python loop of the reference
  (one ``calc_H_g_e2`` + ``numpy.linalg.solve`` per iteration), which ``verbose=True`` also uses
  (it prints the reference's line before every solve).
"""

import numpy as np

from . import _capi
from .math_tools import plus


class UploadedScan:
    """A scan that already lives on the GPU (``Registration.upload``): pass it wherever ``source`` is expected
    to skip the per-call content hash of the array form."""

    def __init__(self, scan, shape):
        self._scan = scan
        self.shape = shape

    def close(self):
        self._scan.close()


def normalize_batch_inputs(sources, poses=None):
    """Input forms of ``align_batch`` / ``calc_H_g_e2_batch`` -> ``(arrays, offsets, item_scan, Ts)``.  Pure (no GPU).

    ``sources``: a sequence of (N_i, 3) arrays -- one item each; the same array OBJECT appearing several times is listed
    once -- or ONE (N, 3) array, which every pose of ``poses`` is applied to (multi-start).  ``poses``: (B, 4, 4), or (4, 4)
    broadcast over the items, default identity.
    Returns the distinct scans as float32 arrays (registration.py:83), their offsets in the concatenated upload
    (len(arrays) + 1, int64), the scan index of every item (B, intc) and the poses as (B, 4, 4) float64."""
    if poses is not None:
        poses = np.asarray(poses, dtype=np.float64)
        if poses.shape[-2:] != (4, 4) or poses.ndim not in (2, 3):
            raise ValueError("poses must have shape (B, 4, 4) or (4, 4)")
    single = isinstance(sources, np.ndarray) and sources.ndim == 2
    if single:
        B = poses.shape[0] if poses is not None and poses.ndim == 3 else 1
        items = [sources] * B
    else:
        try:
            items = list(sources)
        except TypeError:
            raise ValueError("sources must be a sequence of (N, 3) arrays or one (N, 3) array") from None
        B = len(items)
    if B == 0:
        raise ValueError("an empty batch: no sources / no poses")
    arrays, index, item_scan = [], {}, np.zeros(B, np.intc)
    for i, src in enumerate(items):
        k = index.get(id(src))
        if k is None:
            a = np.asarray(src)
            if a.ndim != 2 or a.shape[1] != 3:
                raise ValueError(f"source {i} must have shape (N, 3)")
            k = index[id(src)] = len(arrays)
            arrays.append(a.astype(np.float32, copy=False))
        item_scan[i] = k
    if poses is None:
        Ts = np.broadcast_to(np.eye(4), (B, 4, 4)).copy()
    elif poses.ndim == 2:
        Ts = np.broadcast_to(poses, (B, 4, 4)).copy()
    elif poses.shape[0] == B:
        Ts = np.ascontiguousarray(poses)
    else:
        raise ValueError(f"{poses.shape[0]} poses for {B} sources")
    offsets = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([a.shape[0] for a in arrays], out=offsets[1:])
    return arrays, offsets, item_scan, Ts


def ball_neighbourhood(obj, radius, max_nn, kw, name="radius"):
    """The ``radius`` / ``max_nn`` keywords of a class that estimates normals or covariances -> None (the k nearest
    neighbours) or ``(radius, max_nn)`` as ``_capi.check_ball`` returns them.  The ball estimates run on one GPU of one
    process: with ``devices=`` or ``comm=`` among the keywords ``kw`` they are refused."""
    if radius is None and max_nn is None:
        return None
    ball = _capi.check_ball(radius, max_nn)
    if kw.get("devices") is not None or kw.get("comm") is not None:
        raise NotImplementedError(f"{type(obj).__name__} does not support {name}= with devices= or comm=")
    return ball


class Registration:
    KIND = None           # _capi.ICP / PLANE / VPLANE / NDT in the subclasses

    def __init__(self, max_iter=30, tol=1e-3, device=None, comm=None, native_loop=True,
                 compat_flags=_capi.FLAG_ICP_RR_QUIRK, devices=None):
        self.max_iter = max_iter
        self.tol = tol
        self._is_target_set = False
        self._device = device
        self._comm = comm
        if devices is not None and (comm is not None or device is not None):
            raise ValueError("devices= (one process, several GPUs) excludes device= and comm= (one process per GPU)")
        self._group = _capi.get_group(devices) if devices is not None else None
        self._native_loop = native_loop
        self._flags = compat_flags
        self._target = None            # _capi.Target
        self._scan = None              # (_capi.Scan, key) cache for calc_H_g_e2(cur_T, source)
        self._scan_key = None
        self.last_iterations = 0
        self.last_correspondences = 0

    # -- reference interface -------------------------------------------------------------------
    def is_target_set(self):
        return self._is_target_set

    def set_target(self, target):
        self._is_target_set = True
        raise NotImplementedError("set_target is not implemented.")

    def update_target(self, target):
        # registration.py:36-43: an unimplemented stub in the reference as well
        raise NotImplementedError("update_target is not implemented.")

    def linearize(self, cur_T, source, return_index=False):
        """Per-point Jacobians, residuals and weights at ``cur_T`` (registration.py:45-53, which no class of the reference
        implements) -> ``(Js (N, m, 6), rs (N, m), ws)``, in the order of ``source``; m = 1 (PlaneICP, VPlaneICP) or 3 (ICP, NDT).

        ``ws`` is (N,): 1.0 where the point has a correspondence inside ``max_dist``, else 0.0 with zero rows.  For NDT ``ws``
        is (N, 3, 3) = mask x the matched voxel's inverse covariance, and the sums are
        ``H = einsum("nij,nik,nkl->jl", Js, ws, Js)``, ``g = einsum("nij,nik,nk->j", Js, ws, rs)``,
        ``e2 = einsum("ni,nij,nj->", rs, ws, rs)``.  For the other classes the reference's generic ``calc_H_g_e2``
        (registration.py:62-67: ``H = sum w J^T J``, ``g = sum w J^T r``, ``e2 = sum w r^T r``) applied to the result reproduces
        the class's own sums up to rounding -- except ICP under the default compat flag (quirk Q1), whose own ``g[3:]`` is
        ``sum p x (R r)`` where the rows give ``sum p x (R^T r)``.
        PlaneICP / VPlaneICP: ``J = [n, p x (R^T n)]``, ``r = n . (R p + t - q)``; ICP / NDT: ``J = [I, -R skew(p)]``,
        ``r = R p + t - q``.  ``return_index=True`` appends ``idx`` (N,) int64: the matched target point / voxel (its position
        in ``pcr_target_voxels_get``'s order), -1 where there is none."""
        scan = self._rows_scan(source)
        J, r, w, W, idx = _capi.linearize_rows(self._target, scan, self.KIND, np.asarray(cur_T, dtype=np.float64), self._max_dist(),
                                               self._flags, want_index=return_index)
        ws = w[:, None, None] * W if W is not None else w
        return (J, r, ws, idx) if return_index else (J, r, ws)

    def calc_H_g_e2(self, cur_T, source, weights=None):
        """Hessian (6x6), gradient (6) and squared error at ``cur_T`` for ``source`` (N,3).  ``weights`` (N,), finite and
        >= 0, in the order of ``source``: every point's terms are multiplied by its weight (a caller's own robust kernel is
        ``linearize`` -> weights -> this); ``last_weight_sum`` then holds the sum of the gated-in weights."""
        if weights is None:
            if not self._is_target_set:
                raise ValueError("Target is not set.")
            scan = self._scan_for(source)
            return self._linearize(np.asarray(cur_T, dtype=np.float64), scan)
        n = source.shape[0] if isinstance(source, UploadedScan) else np.asarray(source).shape[0]
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError(f"weights must have shape ({n},)")
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("weights must be finite and >= 0")
        scan = self._rows_scan(source)
        out = _capi.linearize_weighted(self._target, scan, self.KIND, np.asarray(cur_T, dtype=np.float64), self._max_dist(), w, self._flags)
        H, g, e2, _ = _capi.unpack29(out)
        self.last_weight_sum = float(out[28])
        return H, g, e2

    def coreset(self, cur_T, source, N_target=1024, k=64):
        """Exact downsampling of ``source`` at ``cur_T`` (K. Koide, arXiv 2307.02948; the reference's
        fast_voxelized_plane_icp.py) -> ``(indices, weights)``: at most ``N_target`` of the points that have a correspondence,
        ``indices`` ascending, ``weights > 0``, such that ``calc_H_g_e2(cur_T, source[indices], weights=weights)`` equals
        ``calc_H_g_e2(cur_T, source)`` up to rounding.  The per-point terms are computed and reduced on the GPU; only the
        selection crosses PCIe.  ``N_target >= 29`` and ``k > 29`` (28 sums + 1)."""
        if int(N_target) < 29:
            raise ValueError("N_target must be at least 29")
        if int(k) <= 29:
            raise ValueError("k must exceed 29")
        scan = self._rows_scan(source)
        return _capi.scan_coreset(self._target, scan, self.KIND, np.asarray(cur_T, dtype=np.float64), self._max_dist(), int(k),
                                  int(N_target), self._flags)

    def _rows_scan(self, source):
        """The scan of ``linearize`` / weighted ``calc_H_g_e2`` / ``coreset``: uploaded with the caller's order kept."""
        if self._comm is not None or self._group is not None:
            raise ValueError("per-point rows, weights and coresets run on one GPU of one process: not with comm= or devices=")
        if not self._is_target_set:
            raise ValueError("Target is not set.")
        if isinstance(source, UploadedScan) and not (source._scan.flags & (_capi.FLAG_KEEP_ORDER | _capi.FLAG_NO_SCAN_SORT)):
            raise ValueError("this UploadedScan does not remember the caller's order: upload(source, keep_order=True)")
        return self._scan_for(source, flags=_capi.FLAG_KEEP_ORDER)

    def upload(self, source, keep_order=False):
        """Upload (and Morton-sort) ``source`` once; the returned handle can stand in for the array in
        ``calc_H_g_e2`` / ``align`` (the caller then owns the "has it changed?" question).  ``keep_order=True``: the device
        copy remembers the order of ``source`` (4 bytes per point), which ``linearize`` / ``coreset`` / weights need."""
        src = np.asarray(source)
        if src.ndim != 2 or src.shape[1] != 3:
            raise ValueError("source must have shape (N, 3)")
        flags = _capi.FLAG_KEEP_ORDER if keep_order else 0
        return UploadedScan(_capi.Scan(self._ctx(), src.astype(np.float32, copy=False), flags=flags), src.shape)

    def align(self, source, init_T=np.eye(4), verbose=False):
        """Gauss-Newton alignment of ``source`` onto the target; returns the 4x4 float64 pose."""
        if self.is_target_set() is False:
            raise ValueError("Target is not set.")
        scan = self._scan_for(source, fresh=True)     # the reference copies the scan per call
        return self._align(scan, init_T, verbose)

    def _align(self, scan, init_T, verbose):
        """``align`` once the scan is on the device: the native loop, or the reference's Python loop over ``_linearize``."""
        cur_T = np.array(init_T, dtype=np.float64)
        if self._native_loop and not verbose and not self._needs_host_reduce():
            T, iters, trace = self._native_align(scan, cur_T)
            self.last_iterations = iters
            if iters:
                self.last_correspondences = int(round(trace[iters - 1, 16 + 28]))
            return T
        it = 0
        for it in range(self.max_iter):
            H, g, e2 = self._linearize(cur_T, scan)
            if verbose:
                print(f"iter {it}, error {e2}")
            dx = -np.linalg.solve(H, g)          # LinAlgError when H is singular (quirk Q7)
            if np.linalg.norm(dx) < self.tol:    # the test precedes the update (quirk Q4)
                break
            cur_T = plus(cur_T, dx)
        self.last_iterations = it + 1 if self.max_iter > 0 else 0
        return cur_T

    # -- batches: many scans and / or start poses against the target in one launch --------------
    def align_batch(self, sources, init_Ts=None, return_info=False):
        """``align`` of B items at once (``pcr_align_batch``): ``sources`` is a sequence of (N_i, 3) arrays, or ONE (N, 3)
        array with ``init_Ts`` of shape (B, 4, 4) (multi-start); ``init_Ts``: (B, 4, 4), or (4, 4) for all, default identity.
        Returns the (B, 4, 4) float64 poses, each bit-identical to ``align`` of that item alone through the fused kernel;
        sets ``last_batch_iterations`` / ``last_batch_correspondences`` / ``last_batch_status``.  Items whose normal equations
        are singular (quirk Q7) raise ``numpy.linalg.LinAlgError`` naming them, unless ``return_info=True``, which returns
        ``(Ts, info)`` instead (``info["singular"]`` lists them; their pose is the one of the failed solve)."""
        arrays, item_scan, Ts = self._batch_inputs(sources, init_Ts)
        batch = _capi.ScanBatch(self._ctx(), arrays)
        try:
            T, iters, status, trace = _capi.align_batch(self._target, batch, self.KIND, Ts, self.max_iter, self.tol,
                                                        self._max_dist(), self._call_flags(), item_scan=item_scan,
                                                        want_trace=True)
        finally:
            batch.close()
        B = T.shape[0]
        cnt = np.zeros(B, np.int64)
        for i in range(B):
            if iters[i] > 0:
                cnt[i] = int(round(trace[i, iters[i] - 1, 16 + 28]))
        self.last_batch_iterations = iters.astype(np.int64)
        self.last_batch_correspondences = cnt
        self.last_batch_status = status.astype(np.int64)
        singular = [int(i) for i in np.flatnonzero(status == _capi.PCR_ERR_SINGULAR)]
        if return_info:
            return T, {"iterations": self.last_batch_iterations, "correspondences": cnt, "status": self.last_batch_status,
                       "singular": singular}
        if singular:
            raise np.linalg.LinAlgError(f"Singular matrix (batch items {singular})")
        return T

    def calc_H_g_e2_batch(self, cur_Ts, sources):
        """``calc_H_g_e2`` of B items in one launch -> ``(H (B, 6, 6), g (B, 6), e2 (B,))``; input forms as ``align_batch``."""
        arrays, item_scan, Ts = self._batch_inputs(sources, cur_Ts)
        batch = _capi.ScanBatch(self._ctx(), arrays)
        try:
            out = _capi.linearize_batch(self._target, batch, self.KIND, Ts, self._max_dist(), self._call_flags(),
                                        item_scan=item_scan)
        finally:
            batch.close()
        B = out.shape[0]
        H, g, e2, cnt = np.zeros((B, 6, 6)), np.zeros((B, 6)), np.zeros(B), np.zeros(B, np.int64)
        for i in range(B):
            H[i], g[i], e2[i], cnt[i] = _capi.unpack29(out[i])
        self.last_batch_correspondences = cnt
        return H, g, e2

    def _batch_inputs(self, sources, poses):
        if not self._is_target_set:
            raise ValueError("Target is not set.")
        if self._comm is not None or self._group is not None:
            raise ValueError("batched alignment runs on one GPU of one process: not with comm= or devices=")
        arrays, _, item_scan, Ts = normalize_batch_inputs(sources, poses)
        return arrays, item_scan, Ts

    # -- internals -----------------------------------------------------------------------------
    def _ctx(self):
        if self._group is not None:
            return self._group
        if self._comm is not None and getattr(self._comm, "ctx", None) is not None:
            return self._comm.ctx
        return _capi.get_context(self._device)

    def _max_dist(self):
        return float(getattr(self, "max_dist", 2.0))

    def _needs_host_reduce(self):
        return self._comm is not None and not self._comm.in_library

    def _call_flags(self):
        """The collective is a per-call decision: only a Registration that was given ``comm=`` joins the
        all-reduce, whatever else shares the (process-wide) context."""
        if self._group is not None or (self._comm is not None and self._comm.in_library):
            return self._flags
        return self._flags | _capi.FLAG_LOCAL_ONLY

    @staticmethod
    def _digest(src):
        """64-bit hash of the WHOLE scan buffer (``pcr_hash64`` inside libpcr_hip.so: multi-threaded, ~0.1 ms per
        1e6 float32 points on the GPU box's host; no optional Python dependency)."""
        if src.size == 0:
            return 0
        if src.flags.c_contiguous:
            return _capi.hash64(src)
        if src.flags.f_contiguous:                # (a transposed result, e.g. (R @ P.T).T: hash its buffer as it lies)
            return _capi.hash64(src.T) ^ 0x5bd1e995
        return _capi.hash64(np.ascontiguousarray(src))

    def _scan_for(self, source, fresh=False, flags=0):
        """Upload (and Morton-sort) the scan; ``calc_H_g_e2`` called repeatedly with the same array
        (the Gauss-Newton pattern) reuses the device copy.  "Same" = same shape, dtype and content:
        the whole buffer is hashed on every call, so an in-place edit is always seen
        (``calc_H_g_e2`` stays pure in its inputs, as in the reference); ``align`` always uploads
        afresh.  ``flags``: what the caller needs of the scan (``FLAG_KEEP_ORDER`` for rows, weights and coresets).  One
        scan is cached; it is reused when its flags INCLUDE the requested ones, so an order-keeping scan also serves
        plain calls.  The other way round it cannot: a plain scan cached first is closed and the array uploaded again,
        with its order kept, on the first rows call (once; later calls of either sort reuse that copy)."""
        if isinstance(source, UploadedScan):
            return source._scan
        src = np.asarray(source)
        if src.ndim != 2 or src.shape[1] != 3:
            raise ValueError("source must have shape (N, 3)")
        key = None if fresh else (src.shape, src.dtype.str, self._digest(src))
        # (a cached scan that remembers the caller's order is the same device copy plus the permutation: it serves a plain
        # request too, so linearize / weights / coreset alternating with plain calc_H_g_e2 upload and sort once)
        if key is not None and self._scan is not None and self._scan_key == key and (self._scan.flags & flags) == flags:
            return self._scan
        if self._scan is not None:
            self._scan.close()
        self._scan = _capi.Scan(self._ctx(), src.astype(np.float32, copy=False), flags=flags)   # registration.py:83
        self._scan_key = key
        return self._scan

    # the two entry points of a pass: its 29 sums at cur_T, and its whole Gauss-Newton loop -> (T, iterations, trace)
    def _native_linearize(self, scan, cur_T):
        return _capi.linearize(self._target, scan, self.KIND, cur_T, self._max_dist(), self._call_flags())

    def _native_align(self, scan, cur_T):
        return _capi.align(self._target, scan, self.KIND, cur_T, self.max_iter, self.tol, self._max_dist(), self._call_flags(),
                           want_trace=True)

    def _linearize(self, cur_T, scan):
        out = self._native_linearize(scan, cur_T)
        if self._needs_host_reduce():
            out = self._comm.allreduce(out)
        H, g, e2, cnt = _capi.unpack29(out)
        self.last_correspondences = cnt
        return H, g, e2

    def _set_target_handle(self, handle):
        if self._target is not None:
            self._target.close()
        self._target = handle
        self._is_target_set = True


class MatchPass(Registration):
    """The driver of the aligners whose pass has entry points of its own (``GICP``, ``VGICP``, ``SymmetricICP``,
    ``ColoredICP``): one GPU of one process, ``k`` neighbours for what they estimate.  A subclass names its unit (``_UNIT``,
    a row of ``_capi.MATCH_UNITS``) and supplies ``_pass_params``, what the unit's entry points take between ``max_dist`` and
    the flags; it keeps its own ``set_target``, scan preparation (``_pass_scan``) and ``calc_H_g_e2_no_parallel_ver``.

    ``robust`` (``None``, ``"huber"``, ``"cauchy"``, ``"tukey"``, ``"gm"``) with ``robust_scale`` = c weighs every
    correspondence inside the gate by a robust kernel of its squared residual (``math_tools.robust_weight``; ``include/pcr.h``
    says what the squared residual of each class is), inside the pass: ``calc_H_g_e2`` and ``align`` then return the IRLS sums
    and pose.  ``None`` passes no kernel, which the library defines as the plain pass: the bits the class returned before
    there were kernels.  ``residuals`` returns the squared residuals a scale can be chosen from.

    The adaptive pass (``include/pcr.h``) takes the threshold or the scale from each pass's own squared residuals, on the device:
    ``trim=ratio`` in (0, 1] keeps the ``max(1, floor(ratio m))`` best of the m correspondences of every pass, ties at the
    threshold included (trimmed ICP; exclusive with ``robust``); ``robust_scale=("quantile", q, factor)`` runs the kernel with
    c = factor sqrt(the q-quantile of the squared residuals), recomputed every pass (``math_tools.trim_threshold`` is the rule of
    both).  After a call ``last_adaptive`` = ``{"tau", "scale", "kept", "k"}`` of its last pass, after ``align`` also
    ``last_adaptive_trace``, (iterations, 4) in that order.  With neither, the calls are what they were."""
    KIND = None           # no kind of pcr_linearize
    _UNIT = None          # "gicp", "vgicp", "symm", "color"

    def __init__(self, max_iter=30, max_dist=2, tol=1e-3, k=10, robust=None, robust_scale=1.0, trim=None, radius=None, max_nn=None, **kw):
        # what the class estimates -- target and scan payloads -- comes from the ball when there is one (include/pcr.h: radius
        # and hybrid neighbourhoods), else from the k nearest neighbours
        self._ball = ball_neighbourhood(self, radius, max_nn, kw)
        self.radius, self.max_nn = radius, max_nn
        if kw.get("devices") is not None or kw.get("comm") is not None:
            raise ValueError(f"{type(self).__name__} runs on one GPU of one process: not with comm= or devices=")
        if not 1 <= int(k) <= 64:
            raise ValueError("k must be in [1, 64]")
        adaptive = None
        if trim is not None:
            if robust is not None:
                raise ValueError("trim and robust exclude each other")
            adaptive = _capi.check_adaptive("trim", trim)
        if isinstance(robust_scale, (tuple, list)):
            if robust is None or len(robust_scale) != 3 or robust_scale[0] != "quantile":
                raise ValueError('robust_scale must be a float, or ("quantile", q, factor) beside a robust kernel')
            try:
                q, factor = float(robust_scale[1]), float(robust_scale[2])
            except (TypeError, ValueError) as exc:
                raise ValueError('robust_scale must be a float, or ("quantile", q, factor) beside a robust kernel') from exc
            kind, scale = _capi.check_robust(robust, 1.0)[0], tuple(robust_scale)      # ("robust must be ..." first)
            adaptive = _capi.check_adaptive(robust, q, factor)
        else:
            kind, scale = _capi.check_robust(robust, robust_scale)
        super().__init__(max_iter=max_iter, tol=tol, **kw)
        self.max_dist = max_dist
        self.k = int(k)
        self.robust, self.robust_scale = robust, scale
        self.trim = None if trim is None else adaptive[1]
        self._robust = None if robust is None or adaptive is not None else (kind, scale)
        self._adaptive = adaptive                     # (kind, quantile, factor) of pcr_adaptive, or None
        self.last_adaptive = None
        self.last_adaptive_trace = None

    def _pass_params(self):
        return ()

    # -- what the class estimates, on a ``_capi.Target`` or a ``_capi.Scan`` alike
    def _neighbourhood(self):
        """What a payload cache remembers of the neighbourhood an estimate came from: a scan that served a ``k = 10`` aligner
        is estimated again for one with a ball, and the other way round."""
        return ("k", self.k) if self._ball is None else ("ball",) + self._ball

    def _estimate_normals(self, cloud, **target_only):
        if self._ball is not None:
            return cloud.estimate_normals_radius(*self._ball, want=False)
        return cloud.estimate_normals(self.k, want=False, **target_only)

    def _estimate_covariances(self, cloud, mode, eps):
        if self._ball is not None:
            return cloud.estimate_covariances_radius(*self._ball, mode=mode, eps=eps, want=False)
        return cloud.estimate_covariances(self.k, mode, eps, want=False)

    def _pass_scan(self, source, *extras, **kw):
        """The device copy of ``source`` with what the class's pass needs on it (``source_cov``, ``source_normals``, ...)."""
        raise NotImplementedError

    def _payload_scan(self, source, fresh, attr, given, set_payload, estimated=None, estimate=None):
        """The device copy of ``source`` with a per-point payload of the class on it (covariances, normals, intensities).  It
        belongs to the ``_capi.Scan``: uploaded or estimated once per uploaded scan, gone with it.  ``given(n)``: the caller's
        array, checked for ``n`` points, put there by ``set_payload(scan, array)``; ``None``: ``estimate(scan)``, whose
        parameters are ``estimated``.  What the scan carries is remembered on it as ``attr``: ``("given", digest)`` or
        ``estimated``."""
        if not self._is_target_set:
            raise ValueError("Target is not set.")
        # the caller's order is kept (4 bytes per point): payloads cross the boundary in it
        scan = self._scan_for(source, fresh=fresh, flags=_capi.FLAG_KEEP_ORDER)
        if given is not None:
            array = given(scan.n)
            tag, put = ("given", self._digest(array)), lambda: set_payload(scan, array)
        else:
            tag, put = estimated, lambda: estimate(scan)
        if getattr(scan, attr, None) != tag:
            put()
            setattr(scan, attr, tag)
        return scan

    # (the kernel is an argument of the call, as min_cos and lambda are: nothing of it stays on the scan, which aligners share)
    def _entry(self, what):
        return getattr(_capi, f"{self._UNIT}_{what}")

    _STATS = ("tau", "scale", "kept", "k")

    def _native_linearize(self, scan, cur_T):
        if self._adaptive is not None:
            out, stats = self._entry("linearize_adaptive")(self._target, scan, cur_T, self._max_dist(), *self._pass_params(),
                                                           adaptive=self._adaptive, flags=self._flags)
            self.last_adaptive = dict(zip(self._STATS, stats.tolist()))
            return out
        return self._entry("linearize_robust")(self._target, scan, cur_T, self._max_dist(), *self._pass_params(), robust=self._robust,
                                               flags=self._flags)

    def _native_align(self, scan, cur_T):
        if self._adaptive is not None:
            T, iters, stats, trace = self._entry("align_adaptive")(self._target, scan, cur_T, self.max_iter, self.tol, self._max_dist(),
                                                                   *self._pass_params(), adaptive=self._adaptive, flags=self._flags,
                                                                   want_trace=True)
            self.last_adaptive_trace = stats
            self.last_adaptive = dict(zip(self._STATS, stats[-1].tolist())) if iters else None
            return T, iters, trace
        return self._entry("align_robust")(self._target, scan, cur_T, self.max_iter, self.tol, self._max_dist(), *self._pass_params(),
                                           robust=self._robust, flags=self._flags, want_trace=True)

    def residuals(self, cur_T, source, *extras, **kw):
        """The squared residual of every point of ``source`` at ``cur_T``, in its order, ``inf`` where the point has no
        correspondence inside the gates: (N,) float64 -- ``ColoredICP``: (N, 2), the geometric and the colour row.  What
        ``robust`` weighs, whatever this object's own kernel; a scale can be chosen from it (its median, say).  The per-class
        extras (``source_cov``, ``source_normals``, ``source_intensity``) are taken exactly as ``calc_H_g_e2`` takes them."""
        scan = self._pass_scan(source, *extras, **kw)
        return self._entry("residuals")(self._target, scan, np.asarray(cur_T, dtype=np.float64), self._max_dist(), *self._pass_params(),
                                        flags=self._flags)

    # -- out of scope ----------------------------------------------------------------------------
    def _unsupported(self, what):
        raise NotImplementedError(f"{type(self).__name__} does not support {what}")

    def linearize(self, *a, **kw):
        self._unsupported("linearize()")

    def coreset(self, *a, **kw):
        self._unsupported("coreset()")

    def align_batch(self, *a, **kw):
        self._unsupported("align_batch()")

    def calc_H_g_e2_batch(self, *a, **kw):
        self._unsupported("calc_H_g_e2_batch()")
