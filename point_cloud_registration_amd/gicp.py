"""Generalized ICP (Segal, Haehnel, Thrun: "Generalized-ICP", RSS 2009) behind the ``Registration`` interface.

The reference has no GICP class (it only borrows small_gicp's tree as a KD-tree back end, ``kdtree.py:26-57``); this one follows
the conventions of its ``NDT``: ``J = [I, -R skew(p)]`` with the right-multiplicative update of ``plus``, and the dependence of
the weight matrix on the pose ignored, as every GICP implementation does.  Every correspondence -- found and gated exactly as
``ICP`` finds and gates it -- is weighed with ``M = (Cq + R Cp R^T)^-1``, ``Cq`` / ``Cp`` the covariances of the matched target
point and of the scan point: float32 ``(N, 6)`` = xx xy xz yy yz zz, given by the caller or estimated on the GPU from the ``k``
nearest neighbours (``regularization="plane"``: ``I - (1 - eps) n n^T``, eigenvalues ``(eps, 1, 1)``; ``"raw"``: the k-NN
covariance itself).  A singular ``Cq + R Cp R^T`` (determinant exactly 0) is divided by 1e6 instead of its determinant, the
rule of the voxel targets' ``calc_icov``: such a pair contributes next to nothing instead of Inf / NaN.

``DistributionPass`` is what ``GICP`` and ``VGICP`` (``vgicp.py``) share: everything but the target side.
"""

import numpy as np

from . import _capi
from .kdtree import KDTree
from .math_tools import skew
from .registration import MatchPass

_MODES = {"plane": _capi.COV_PLANE, "raw": _capi.COV_RAW}


class ScanCovariances:
    """The scan side of GICP and VGICP: covariances on the device copy of a scan.  The host class provides ``k``, ``eps``,
    ``regularization`` and ``Registration``'s scan cache."""

    def source_covariance(self, source):
        """The covariances ``calc_H_g_e2`` / ``align`` use for ``source`` (estimated now if they have not been), in its order."""
        return self._gicp_scan(source, None).get_covariances()

    def _gicp_scan(self, source, source_cov, fresh=False):
        """The device copy of ``source`` with covariances on it (``MatchPass._payload_scan``)."""
        def given(n):
            c = _capi.cov6(source_cov)
            if c.shape != (n, 6):
                raise ValueError("source_cov must have shape (N, 6) or (N, 3, 3)")
            return c
        return self._payload_scan(source, fresh, "_gicp_cov", given if source_cov is not None else None, _capi.Scan.set_covariances,
                                  ("estimated", self._neighbourhood(), self.regularization, self.eps),
                                  lambda scan: self._estimate_covariances(scan, _MODES[self.regularization], self.eps))


class DistributionPass(ScanCovariances, MatchPass):
    """The distribution-to-distribution pass behind ``GICP`` and ``VGICP``.  A subclass supplies the target side:
    ``set_target``, ``covariance``, its ``_UNIT`` and ``_match`` for the per-point loop."""

    def __init__(self, max_iter=30, max_dist=2, tol=1e-3, k=10, eps=1e-3, regularization="plane", **kw):
        super().__init__(max_iter, max_dist, tol, k, **kw)
        if regularization not in _MODES:
            raise ValueError(f"regularization must be one of {sorted(_MODES)}, not {regularization!r}")
        self.eps = float(eps)
        self.regularization = regularization
        self._covariance = None

    def _pass_scan(self, source, source_cov=None):
        return self._gicp_scan(source, source_cov)

    # -- passes ----------------------------------------------------------------------------------
    def calc_H_g_e2(self, cur_T, source, source_cov=None, weights=None):
        """Hessian (6x6), gradient (6) and squared (Mahalanobis) error at ``cur_T``.  ``source_cov``: (N, 6) or (N, 3, 3) in
        the order of ``source``; default: estimated once per uploaded scan with this object's ``k`` / ``regularization``."""
        if weights is not None:
            self._unsupported("weights=")
        scan = self._gicp_scan(source, source_cov)
        return self._linearize(np.asarray(cur_T, dtype=np.float64), scan)

    def align(self, source, init_T=np.eye(4), verbose=False, source_cov=None):
        return self._align(self._gicp_scan(source, source_cov, fresh=True), init_T, verbose)

    def calc_H_g_e2_no_parallel_ver(self, cur_T, source, source_cov=None):
        """Per-point loop of the same sums, for reading and for tests: host Python over the GPU's correspondences
        (``_match``) and covariances, the inverse by ``numpy.linalg.inv``."""
        cur_T = np.asarray(cur_T, dtype=np.float64)
        R = cur_T[:3, :3]
        source = np.asarray(source)
        Cp = self.source_covariance(source) if source_cov is None else _capi.cov6(source_cov)
        Cq = self.covariance
        keep, idx, res = self._match(_xform32(cur_T, source.astype(np.float32)))
        H, g, e2 = np.zeros((6, 6)), np.zeros(6), 0.0
        for i, j, d in zip(keep, idx, res):
            M = np.linalg.inv(_full(Cq[j]) + R @ _full(Cp[i]) @ R.T)
            J = np.hstack([np.eye(3), -R @ skew(np.asarray(source[i], dtype=np.float64))])
            H += J.T @ M @ J
            g += J.T @ M @ d
            e2 += d @ M @ d
        return H, g, e2

    def _match(self, src_trans):
        """(scan points that pass the gate, the target element each is matched to, its float64 residual) for the
        transformed float32 scan."""
        raise NotImplementedError


class GICP(DistributionPass):
    _UNIT = "gicp"

    # -- target ----------------------------------------------------------------------------------
    def set_target(self, target, kdree=None, cov=None):
        """float32 copy of the target, an exact-NN index on the GPU and one covariance per point: ``cov`` (N, 6) or
        (N, 3, 3) when given, else estimated from the ``k`` nearest neighbours.  ``kdree`` keeps the keyword of
        ``PlaneICP.set_target``; as there, a foreign tree is never searched."""
        target = np.asarray(target).astype(np.float32)
        c = None
        if cov is not None:                         # (checked before anything of the previous target is replaced)
            c = _capi.cov6(cov)
            if c.shape != (target.shape[0], 6):
                raise ValueError("cov must have shape (N, 6) or (N, 3, 3)")
        tree = KDTree(target, device=self._device, _ctx=self._ctx())
        if c is None:
            self._estimate_covariances(tree._target, _MODES[self.regularization], self.eps)
        else:
            tree._target.set_covariances(c)
        self.kdtree, self.target = tree, target
        self._covariance = c                        # None: read back the first time somebody asks, as PlaneICP.normal is
        self._target = self.kdtree._target
        self._is_target_set = True

    @property
    def covariance(self):
        """The target's covariances, float32 (N, 6) = xx xy xz yy yz zz, in the order of the target."""
        if self._covariance is None and self._target is not None:
            self._covariance = self._target.get_covariances()
        return self._covariance

    def _match(self, src_trans):
        # ICP's: float32 residual against the matched point, float32 gate (``self.kdtree.query``)
        dist, idx = self.kdtree.query(src_trans)
        keep = np.nonzero(dist < np.float32(self.max_dist))[0]
        return keep, idx[keep], (src_trans[keep] - self.target[idx[keep]]).astype(np.float64)


def _xform32(T, p):
    """The kernels' float32 transform, in their order of operations: ((R0 x + R1 y) + R2 z) + t (BLAS may fuse or reorder)."""
    T = np.asarray(T, dtype=np.float64).astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1)


def _full(c6):
    c = np.asarray(c6, dtype=np.float64)
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
