"""Symmetric point-to-plane ICP (Rusinkiewicz: "A Symmetric Objective Function for ICP", SIGGRAPH 2019; the fixed-normal-sum
form PCL offers) behind the ``Registration`` interface.

The reference has no such class; this one follows the conventions of its ``PlaneICP``: ``J = [m, p x (R^T m)]``,
``r = m . (R p + t - q)`` with the right-multiplicative update of ``plus``.  Every correspondence -- found and gated exactly
as ``ICP`` finds and gates it -- pulls along ``m = (n_q + s R n_p) / 2``, the mean of the matched target normal and the
rotated scan normal, ``s = sign(n_q . R n_p)``: PCA normals carry no sign, and with this rule neither does the objective.
``m`` is held fixed within a pass.  A pair whose normals disagree (``|n_q . R n_p| < min_normal_cos``) is left out.  Normals
are float32 ``(N, 3)``, given by the caller or estimated on the GPU from the ``k`` nearest neighbours -- on BOTH clouds: the
scan's live on its device copy, estimated once per uploaded scan.  ``include/pcr.h`` states the arithmetic, order included.
"""

import numpy as np

from . import _capi
from .gicp import _xform32
from .kdtree import KDTree
from .math_tools import skew
from .registration import MatchPass


class SymmetricICP(MatchPass):
    _UNIT = "symm"

    def __init__(self, max_iter=30, max_dist=2, tol=1e-3, k=10, min_normal_cos=0.0, **kw):
        super().__init__(max_iter, max_dist, tol, k, **kw)
        if not 0.0 <= float(min_normal_cos) <= 1.0:             # (false for NaN)
            raise ValueError("min_normal_cos must be in [0, 1]")
        self.min_normal_cos = float(min_normal_cos)
        self._normal = None

    def _pass_params(self):
        return (self.min_normal_cos,)

    # -- target ----------------------------------------------------------------------------------
    def set_target(self, target, norm=None):
        """float32 copy of the target (a float64 array is cast: no quirk Q6 here), an exact-NN index on the GPU and one
        normal per point: ``norm`` (N, 3) when given, else the k-NN PCA normal (centred float64 covariance)."""
        target = np.asarray(target).astype(np.float32)
        n = None
        if norm is not None:                        # (checked before anything of the previous target is replaced)
            n = np.ascontiguousarray(norm, dtype=np.float32)
            if n.shape != target.shape:
                raise ValueError("norm must have the shape of the target")
        tree = KDTree(target, device=self._device, _ctx=self._ctx())
        if n is None:
            self._estimate_normals(tree._target, compat=False)
        else:
            tree._target.set_normals(n)
        self.kdtree, self.target = tree, target
        self._normal = n                            # None: read back the first time somebody asks, as PlaneICP.normal is
        self._target = self.kdtree._target
        self._is_target_set = True

    @property
    def normal(self):
        """The target's normals, float32 (N, 3), in the order of the target."""
        if self._normal is None and self._target is not None:
            self._normal = self._target.get_normals()
        return self._normal

    # -- scan ------------------------------------------------------------------------------------
    def source_normals(self, source):
        """The normals the pass used for ``source``, in its order: what its device copy carries -- the ``source_normals=`` of
        the last ``calc_H_g_e2`` over it, or the estimate -- estimated now if it carries none."""
        if not self._is_target_set:
            raise ValueError("Target is not set.")
        scan = self._scan_for(source, flags=_capi.FLAG_KEEP_ORDER)
        if getattr(scan, "_symm_nrm", None) is None:
            scan = self._symm_scan(source, None)
        return scan.get_normals()

    def _symm_scan(self, source, source_normals, fresh=False):
        """The device copy of ``source`` with normals on it (``MatchPass._payload_scan``)."""
        def given(n):
            nrm = np.ascontiguousarray(source_normals, dtype=np.float32)
            if nrm.shape != (n, 3):
                raise ValueError("source_normals must have shape (N, 3)")
            return nrm
        return self._payload_scan(source, fresh, "_symm_nrm", given if source_normals is not None else None, _capi.Scan.set_normals,
                                  ("estimated", self._neighbourhood()), self._estimate_normals)

    def _pass_scan(self, source, source_normals=None):
        return self._symm_scan(source, source_normals)

    # -- passes ----------------------------------------------------------------------------------
    def calc_H_g_e2(self, cur_T, source, source_normals=None, weights=None):
        """Hessian (6x6), gradient (6) and squared error at ``cur_T``.  ``source_normals``: (N, 3) in the order of ``source``;
        default: estimated once per uploaded scan with this object's ``k``."""
        if weights is not None:
            self._unsupported("weights=")
        scan = self._symm_scan(source, source_normals)
        return self._linearize(np.asarray(cur_T, dtype=np.float64), scan)

    def align(self, source, init_T=np.eye(4), verbose=False, source_normals=None):
        return self._align(self._symm_scan(source, source_normals, fresh=True), init_T, verbose)

    def calc_H_g_e2_no_parallel_ver(self, cur_T, source, source_normals=None):
        """Per-point loop of the same sums, for reading and for tests: host Python over the GPU's correspondences
        (``self.kdtree.query``) and normals."""
        cur_T = np.asarray(cur_T, dtype=np.float64)
        R = cur_T[:3, :3]
        source = np.asarray(source)
        Np = self.source_normals(source) if source_normals is None else np.asarray(source_normals, dtype=np.float32)
        Nq = self.normal
        src_trans = _xform32(cur_T, source.astype(np.float32))
        dist, idx = self.kdtree.query(src_trans)
        H, g, e2 = np.zeros((6, 6)), np.zeros(6), 0.0
        for i in np.nonzero(dist < np.float32(self.max_dist))[0]:
            d = (src_trans[i] - self.target[idx[i]]).astype(np.float64)          # float32 subtraction, then widened
            nq = np.asarray(Nq[idx[i]], dtype=np.float64)
            v = R @ np.asarray(Np[i], dtype=np.float64)
            c = float(nq @ v)
            if not abs(c) >= self.min_normal_cos:
                continue
            m = 0.5 * (nq + (-v if c < 0 else v))
            r = float(m @ d)
            J = np.concatenate([m, skew(np.asarray(source[i], dtype=np.float64)) @ (R.T @ m)])
            H += np.outer(J, J)
            g += J * r
            e2 += r * r
        return H, g, e2
