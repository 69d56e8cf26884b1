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

from .gicp import _MODES, DistributionPass
from .voxel import VoxelGrid


class VGICP(DistributionPass):
    _UNIT = "vgicp"

    def __init__(self, voxel_size=1.0, max_iter=30, max_dist=2, tol=1e-3, k=10, eps=1e-3, regularization="plane", **kw):
        super().__init__(max_iter, max_dist, tol, k, eps, regularization, **kw)
        self.voxel_size = voxel_size

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

    def _match(self, src_trans):
        # NDT's: float64 residual against the voxel mean, float64 gate (``self.voxels.kdtree.query``)
        dist, idx = self.voxels.kdtree.query(src_trans)
        keep = np.nonzero(dist < self.max_dist)[0]
        return keep, idx[keep], src_trans[keep].astype(np.float64) - self.voxels.mean[idx[keep]]
