"""Colored ICP (Park, Zhou, Koltun: "Colored Point Cloud Registration Revisited", ICCV 2017; the form Open3D offers) behind
the ``Registration`` interface.

The reference has no such class; this one follows the conventions of its ``PlaneICP``: ``J = [n, p x (R^T n)]`` with the
right-multiplicative update of ``plus``.  Every correspondence -- found and gated exactly as ``ICP`` finds and gates it --
contributes two rows: ``PlaneICP``'s, ``r_G = n . d``, and a colour row ``r_C = (I_q - I_p) + m . d`` with ``d = R p + t - q``
and ``m`` the tangent part of the target's intensity gradient at ``q``: the target's intensity carried along its tangent plane
to the foot of the transformed point, minus the scan point's.  The rows are weighted ``lambda_geometric`` and
``1 - lambda_geometric``.  "Intensity" is one float32 per point, a LiDAR return strength or a colour reduced to one channel; its
scale is the caller's (Open3D: values in [0, 1], coordinates in metres).  Normals and gradients are float32 ``(N, 3)``, given by
the caller or estimated on the GPU from the ``k`` nearest neighbours.  ``include/pcr.h`` states the arithmetic, order included.
"""

import numpy as np

from . import _capi
from .gicp import _xform32
from .kdtree import KDTree
from .math_tools import skew
from .registration import MatchPass


def as_intensity(values, n, name):
    """(N,) intensities, or (N, 3) colours reduced to (r + g + b) / 3 in float64 -- then float32."""
    a = np.asarray(values)
    if a.shape == (n, 3):
        a = a.astype(np.float64)
        a = (a[:, 0] + a[:, 1] + a[:, 2]) / 3.0
    elif a.shape != (n,):
        raise ValueError(f"{name} must have shape (N,) or (N, 3)")
    return np.ascontiguousarray(a, dtype=np.float32)


class ColoredICP(MatchPass):
    _UNIT = "color"

    def __init__(self, max_iter=30, max_dist=2, tol=1e-3, k=10, lambda_geometric=0.968, **kw):
        super().__init__(max_iter, max_dist, tol, k, **kw)
        if not 0.0 <= float(lambda_geometric) <= 1.0:             # (false for NaN)
            raise ValueError("lambda_geometric must be in [0, 1]")
        self.lambda_geometric = float(lambda_geometric)
        self._normal = self._intensity = self._gradient = None

    def _pass_params(self):
        return (self.lambda_geometric,)

    # -- target ----------------------------------------------------------------------------------
    def set_target(self, target, intensity, norm=None, gradient=None):
        """float32 copy of the target (a float64 array is cast: no quirk Q6 here), an exact-NN index on the GPU, one normal
        per point -- ``norm`` (N, 3) when given, else the k-NN PCA normal -- its ``intensity`` ((N,), or (N, 3) colours ->
        (r + g + b) / 3) and the intensity's gradient along the tangent plane: ``gradient`` (N, 3) when given, stored as it is,
        else estimated from the same ``k`` neighbours."""
        target = np.asarray(target).astype(np.float32)
        if target.ndim != 2 or target.shape[1] != 3:
            raise ValueError("target must have shape (N, 3)")
        # (everything is checked before anything of the previous target is replaced)
        inten = as_intensity(intensity, len(target), "intensity")
        if not np.all(np.isfinite(inten)):
            raise ValueError("intensity must be finite")
        n = g = None
        if norm is not None:
            n = np.ascontiguousarray(norm, dtype=np.float32)
            if n.shape != target.shape:
                raise ValueError("norm must have the shape of the target")
        if gradient is not None:
            g = np.ascontiguousarray(gradient, dtype=np.float32)
            if g.shape != target.shape:
                raise ValueError("gradient must have the shape of the target")
            if not np.all(np.isfinite(g)):
                raise ValueError("gradient must be finite")
        tree = KDTree(target, device=self._device, _ctx=self._ctx())
        if n is None:
            self._estimate_normals(tree._target, compat=False)      # (the gradient below stays with the k nearest neighbours)
        else:
            tree._target.set_normals(n)
        tree._target.set_intensity(inten, g)
        if g is None:
            tree._target.estimate_color_gradients(self.k, want=False)
        self.kdtree, self.target = tree, target
        self._normal, self._intensity, self._gradient = n, inten, g      # None: read back the first time somebody asks
        self._target = self.kdtree._target
        self._is_target_set = True

    @property
    def normal(self):
        """The target's normals, float32 (N, 3), in the order of the target."""
        if self._normal is None and self._target is not None:
            self._normal = self._target.get_normals()
        return self._normal

    @property
    def intensity(self):
        """The target's intensities, float32 (N,), in the order of the target."""
        return self._intensity

    @property
    def gradient(self):
        """The target's intensity gradients, float32 (N, 3), in the order of the target."""
        if self._gradient is None and self._target is not None:
            self._gradient = self._target.get_color()[1]
        return self._gradient

    # -- scan ------------------------------------------------------------------------------------
    def _color_scan(self, source, source_intensity, fresh=False):
        """The device copy of ``source`` with its intensities on it (``MatchPass._payload_scan``; nothing to estimate)."""
        if not self._is_target_set:
            raise ValueError("Target is not set.")
        if source_intensity is None:
            raise ValueError("ColoredICP needs the scan's intensities")
        return self._payload_scan(source, fresh, "_color_int", lambda n: as_intensity(source_intensity, n, "source_intensity"),
                                  _capi.Scan.set_intensity)

    def _pass_scan(self, source, source_intensity=None):
        return self._color_scan(source, source_intensity)

    # -- passes ----------------------------------------------------------------------------------
    def calc_H_g_e2(self, cur_T, source, source_intensity=None, weights=None):
        """Hessian (6x6), gradient (6) and squared error at ``cur_T``.  ``source_intensity``: (N,) or (N, 3) colours, in the
        order of ``source``."""
        if weights is not None:
            self._unsupported("weights=")
        scan = self._color_scan(source, source_intensity)
        return self._linearize(np.asarray(cur_T, dtype=np.float64), scan)

    def align(self, source, source_intensity=None, init_T=np.eye(4), verbose=False):
        return self._align(self._color_scan(source, source_intensity, fresh=True), init_T, verbose)

    def calc_H_g_e2_no_parallel_ver(self, cur_T, source, source_intensity=None):
        """Per-point loop of the same sums, for reading and for tests: host Python over the GPU's correspondences
        (``self.kdtree.query``), normals and gradients."""
        cur_T = np.asarray(cur_T, dtype=np.float64)
        R = cur_T[:3, :3]
        source = np.asarray(source)
        Ip = as_intensity(source_intensity, len(source), "source_intensity").astype(np.float64)
        Nq, Iq, Gq = self.normal, self.intensity, self.gradient
        lam = self.lambda_geometric
        src_trans = _xform32(cur_T, source.astype(np.float32))
        dist, idx = self.kdtree.query(src_trans)
        H, g, e2 = np.zeros((6, 6)), np.zeros(6), 0.0
        for i in np.nonzero(dist < np.float32(self.max_dist))[0]:
            d = (src_trans[i] - self.target[idx[i]]).astype(np.float64)          # float32 subtraction, then widened
            n = np.asarray(Nq[idx[i]], dtype=np.float64)
            gq = np.asarray(Gq[idx[i]], dtype=np.float64)
            m = gq - float(gq @ n) * n
            S = skew(np.asarray(source[i], dtype=np.float64))
            for wgt, v, r in ((lam, n, float(n @ d)), (1.0 - lam, m, float(Iq[idx[i]]) - Ip[i] + float(m @ d))):
                J = np.concatenate([v, S @ (R.T @ v)])
                H += wgt * np.outer(J, J)
                g += wgt * J * r
                e2 += wgt * r * r
        return H, g, e2
