"""Voxelized GICP (Koide, Yokozuka, Oishi, Banno: "Voxelized GICP", ICRA 2021) behind the ``Registration`` interface.

``GICP``'s weighting on the voxel targets of ``NDT`` / ``VPlaneICP``: every scan point -- matched to the nearest kept centroid
and gated exactly as ``NDT`` matches and gates it -- is weighed with ``M = (Cv + R Cp R^T)^-1``.  ``Cv`` is one float64
covariance per kept voxel, ``(Nv, 6)`` = xx xy xz yy yz zz in the order of ``voxels.mean``: ``regularization="plane"``
(``I - (1 - eps) n n^T`` from the voxel's normal, eigenvalues ``(eps, 1, 1)``), ``"raw"`` (``voxels.cov`` itself) or the
caller's own through ``set_covariance``.  ``Cp`` is the scan point's float32 covariance, exactly ``GICP``'s: given by the
caller or estimated on the GPU from the ``k`` nearest neighbours with the same ``regularization`` / ``eps``.  Where ``NDT``
inverts the bare voxel covariance, the sum inverted here is well conditioned as soon as either side is regularised; a
determinant of exactly 0 is replaced by 1e6, the rule of ``calc_icov``.

``neighbors=1``, ``7`` or ``27`` selects the association of the paper (fast_gicp's / small_gicp's DIRECT1 / DIRECT7 / DIRECT27)
instead: every scan point is paired with the kept voxel that CONTAINS its transformed position and with that voxel's neighbours
(``VoxelGrid.lookup``), one term of the same form per voxel found inside ``max_dist``, found by integer lookup with no search
(``include/pcr.h``: direct voxel neighbourhoods).  ``last_correspondences`` then counts the kept (point, voxel) pairs and
``residuals`` returns (N, neighbors).  ``None``, the default, is the nearest-centroid pass.
"""

import numpy as np

from . import _capi
from .gicp import _MODES, DistributionPass
from .voxel import VoxelGrid


class VGICP(DistributionPass):
    _UNIT = "vgicp"

    def __init__(self, voxel_size=1.0, max_iter=30, max_dist=2, tol=1e-3, k=10, eps=1e-3, regularization="plane", neighbors=None,
                 **kw):
        super().__init__(max_iter, max_dist, tol, k, eps, regularization, **kw)
        self.voxel_size = voxel_size
        if neighbors is not None:
            if neighbors not in _capi.NEIGHBORS:
                raise ValueError("neighbors must be None, 1, 7 or 27")
            if self._adaptive is not None:
                raise ValueError("trim= and a quantile robust_scale select over one key per scan point: not with neighbors=")
        self.neighbors = neighbors

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

    # -- direct voxel neighbourhoods: the same calls through the pcr_vgicp_direct_* entry points ----
    def _native_linearize(self, scan, cur_T):
        if self.neighbors is None:
            return super()._native_linearize(scan, cur_T)
        return _capi.vgicp_direct_linearize(self._target, scan, cur_T, self._max_dist(), self.neighbors, robust=self._robust,
                                            flags=self._flags)

    def _native_align(self, scan, cur_T):
        if self.neighbors is None:
            return super()._native_align(scan, cur_T)
        return _capi.vgicp_direct_align(self._target, scan, cur_T, self.max_iter, self.tol, self._max_dist(), self.neighbors,
                                        robust=self._robust, flags=self._flags, want_trace=True)

    def residuals(self, cur_T, source, *extras, **kw):
        if self.neighbors is None:
            return super().residuals(cur_T, source, *extras, **kw)
        scan = self._pass_scan(source, *extras, **kw)
        return _capi.vgicp_direct_residuals(self._target, scan, np.asarray(cur_T, dtype=np.float64), self._max_dist(), self.neighbors,
                                            flags=self._flags)

    def _match(self, src_trans):
        if self.neighbors is not None:
            # every voxel found for a point, in offset order: scan rows repeat
            found = self.voxels.lookup(src_trans, self.neighbors)
            rows, cols = np.nonzero(found >= 0)
            idx = found[rows, cols]
            d = src_trans[rows].astype(np.float64) - self.voxels.mean[idx]
            keep = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < self.max_dist
            return rows[keep], idx[keep], d[keep]
        # NDT's: float64 residual against the voxel mean, float64 gate (``self.voxels.kdtree.query``)
        dist, idx = self.voxels.kdtree.query(src_trans)
        keep = np.nonzero(dist < self.max_dist)[0]
        return keep, idx[keep], src_trans[keep].astype(np.float64) - self.voxels.mean[idx[keep]]
