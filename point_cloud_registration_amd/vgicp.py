"""Voxelized GICP (Koide, Yokozuka, Oishi, Banno: "Voxelized GICP", ICRA 2021) behind the ``Registration`` interface.

``GICP``'s weighting on the voxel targets of ``NDT`` / ``VPlaneICP``: every scan point -- matched to the nearest kept centroid
and gated exactly as ``NDT`` matches and gates it -- is weighed with ``M = (Cv + R Cp R^T)^-1``.  ``Cv`` is one float64
covariance per kept voxel, ``(Nv, 6)`` = xx xy xz yy yz zz in the order of ``voxels.mean``: ``regularization="plane"``
(``I - (1 - eps) n n^T`` from the voxel's normal, eigenvalues ``(eps, 1, 1)``), ``"raw"`` (``voxels.cov`` itself) or the
caller's own through ``set_covariance``.  ``Cp`` is the scan point's float32 covariance, exactly ``GICP``'s: given by the
caller or estimated on the GPU from the ``k`` nearest neighbours with the same ``regularization`` / ``eps``.  Where ``NDT``
inverts the bare voxel covariance, the sum inverted here is well conditioned as soon as either side is regularised; a
determinant of exactly 0 is replaced by 1e6, the rule of ``calc_icov``.
"""

import numpy as np

from . import _capi
from .gicp import _MODES, ScanCovariances, _full, _xform32
from .math_tools import plus, skew
from .registration import Registration
from .voxel import VoxelGrid


class VGICP(ScanCovariances, Registration):
    KIND = None           # no kind of pcr_linearize: the pass has entry points of its own (pcr_vgicp_*)

    def __init__(self, voxel_size=1.0, max_iter=30, max_dist=2, tol=1e-3, k=10, eps=1e-3, regularization="plane", **kw):
        if kw.get("devices") is not None or kw.get("comm") is not None:
            raise ValueError("VGICP runs on one GPU of one process: not with comm= or devices=")
        if regularization not in _MODES:
            raise ValueError(f"regularization must be one of {sorted(_MODES)}, not {regularization!r}")
        if not 1 <= int(k) <= 64:
            raise ValueError("k must be in [1, 64]")
        super().__init__(max_iter=max_iter, tol=tol, **kw)
        self.voxel_size = voxel_size
        self.max_dist = max_dist
        self.k = int(k)
        self.eps = float(eps)
        self.regularization = regularization
        self._covariance = None

    # -- target ----------------------------------------------------------------------------------
    def set_target(self, target):
        """The voxel build of ``NDT.set_target`` (``self.voxels``), then one covariance per kept voxel by ``regularization``."""
        self.voxels = VoxelGrid(self.voxel_size, device=self._device, _ctx=self._ctx())
        self.voxels.set_points(target)
        self.voxels._target.set_voxel_covariances(_MODES[self.regularization], self.eps)
        self._covariance = None                     # read back the first time somebody asks
        self._target = self.voxels._target
        self._is_target_set = True

    @property
    def covariance(self):
        """The voxels' covariances, float64 (Nv, 6) = xx xy xz yy yz zz, in the order of ``voxels.mean``."""
        if self._covariance is None and self._target is not None:
            self._covariance = self._target.get_voxel_covariances()
        return self._covariance

    def set_covariance(self, cov):
        """The caller's own voxel covariances, (Nv, 6) or (Nv, 3, 3) float64 in the order of ``voxels.mean`` -- e.g. the mean of
        the point covariances in every voxel.  A non-finite entry raises ``ValueError`` and leaves the old ones."""
        if not self._is_target_set:
            raise ValueError("Target is not set.")
        self._target.set_voxel_covariances(cov=cov)
        self._covariance = None

    # -- passes ----------------------------------------------------------------------------------
    def calc_H_g_e2(self, cur_T, source, source_cov=None, weights=None):
        """Hessian (6x6), gradient (6) and squared (Mahalanobis) error at ``cur_T``.  ``source_cov``: (N, 6) or (N, 3, 3) in
        the order of ``source``; default: estimated once per uploaded scan with this object's ``k`` / ``regularization``."""
        if weights is not None:
            raise NotImplementedError("VGICP does not support weights=")
        scan = self._gicp_scan(source, source_cov)
        return self._vgicp_linearize(np.asarray(cur_T, dtype=np.float64), scan)

    def align(self, source, init_T=np.eye(4), verbose=False, source_cov=None):
        if self.is_target_set() is False:
            raise ValueError("Target is not set.")
        scan = self._gicp_scan(source, source_cov, fresh=True)
        cur_T = np.array(init_T, dtype=np.float64)
        if self._native_loop and not verbose:
            T, iters, trace = _capi.vgicp_align(self._target, scan, cur_T, self.max_iter, self.tol, self._max_dist(),
                                                self._flags, want_trace=True)
            self.last_iterations = iters
            if iters:
                self.last_correspondences = int(round(trace[iters - 1, 16 + 28]))
            return T
        it = 0
        for it in range(self.max_iter):
            H, g, e2 = self._vgicp_linearize(cur_T, scan)
            if verbose:
                print(f"iter {it}, error {e2}")
            dx = -np.linalg.solve(H, g)
            if np.linalg.norm(dx) < self.tol:
                break
            cur_T = plus(cur_T, dx)
        self.last_iterations = it + 1 if self.max_iter > 0 else 0
        return cur_T

    def calc_H_g_e2_no_parallel_ver(self, cur_T, source, source_cov=None):
        """Per-point loop of the same sums, for reading and for tests: host Python over the GPU's correspondences
        (``self.voxels.kdtree.query``) and covariances, the inverse by ``numpy.linalg.inv``."""
        cur_T = np.asarray(cur_T, dtype=np.float64)
        R = cur_T[:3, :3]
        source = np.asarray(source)
        Cp = self.source_covariance(source) if source_cov is None else _capi.cov6(source_cov)
        Cv = self.covariance
        src_trans = _xform32(cur_T, source.astype(np.float32))
        dist, idx = self.voxels.kdtree.query(src_trans)
        H, g, e2 = np.zeros((6, 6)), np.zeros(6), 0.0
        for i in np.nonzero(dist < self.max_dist)[0]:
            M = np.linalg.inv(_full(Cv[idx[i]]) + R @ _full(Cp[i]) @ R.T)
            J = np.hstack([np.eye(3), -R @ skew(np.asarray(source[i], dtype=np.float64))])
            d = src_trans[i].astype(np.float64) - self.voxels.mean[idx[i]]
            H += J.T @ M @ J
            g += J.T @ M @ d
            e2 += d @ M @ d
        return H, g, e2

    # -- out of scope ----------------------------------------------------------------------------
    def linearize(self, *a, **kw):
        raise NotImplementedError("VGICP does not support linearize()")

    def coreset(self, *a, **kw):
        raise NotImplementedError("VGICP does not support coreset()")

    def align_batch(self, *a, **kw):
        raise NotImplementedError("VGICP does not support align_batch()")

    def calc_H_g_e2_batch(self, *a, **kw):
        raise NotImplementedError("VGICP does not support calc_H_g_e2_batch()")

    # -- internals -------------------------------------------------------------------------------
    def _vgicp_linearize(self, cur_T, scan):
        out = _capi.vgicp_linearize(self._target, scan, cur_T, self._max_dist(), self._flags)
        H, g, e2, cnt = _capi.unpack29(out)
        self.last_correspondences = cnt
        return H, g, e2
