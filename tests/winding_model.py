"""Test oracle of the winding-number calls (include/m2s.h m2s_winding_numbers & co.): the header's definitions restated in numpy, f64.

* `exact_winding`: w(p) = (1 / 4 pi) sum_t Omega_t(p) with the Van Oosterom-Strackee solid angle and the header's zero-contribution rules
  (a triangle whose raw normal is zero, or whose numerator is exactly 0, contributes 0; a NaN point gives NaN).
* `Tree` / `tree_winding`: the same order-1 expansion with the same acceptance rule |c~ - p| > beta r, over a tree of its own (median
  split of the centroids along their widest axis, leaves of at most 8 triangles).  It does not reproduce the library's LBVH and need
  not: E_model(beta) = max |tree - exact| is the yardstick the GPU's error is measured against.
"""
import numpy as np

LEAF = 8


def triangles_of(vertices, indices, topology=0):
    """[T, 3, 3] f64 corner positions in Topology order (0 = TriangleList, 1 = TriangleStrip as lib.rs:175-193 walks it)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    if indices is None:
        idx = np.arange(v.shape[0], dtype=np.int64)
    else:
        idx = np.asarray(indices).astype(np.int64).reshape(-1)
    if topology == 0:
        idx = idx[: idx.size // 3 * 3].reshape(-1, 3)
    else:
        n = max(idx.size - 2, 0)
        idx = np.stack([idx[0:n], idx[1:n + 1], idx[2:n + 2]], -1) if n else np.zeros((0, 3), np.int64)
    return v[idx]


def exact_winding(tris, points, chunk=256):
    """w of every point: f64[P].  tris [T, 3, 3] f64, points [P, 3] (taken as f32 values)."""
    tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.zeros(pts.shape[0])
    if tris.shape[0] == 0:
        return out
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    flat = (n == 0).all(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(0, pts.shape[0], chunk):
            p = pts[s:s + chunk, None, :]
            a, b, c = tris[None, :, 0] - p, tris[None, :, 1] - p, tris[None, :, 2] - p
            la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
            num = (a * np.cross(b, c)).sum(-1)
            den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
            om = 2.0 * np.arctan2(num, den)
            om = np.where(flat[None, :] | (num == 0), 0.0, om)
            out[s:s + chunk] = om.sum(-1) / (4.0 * np.pi)
    return out


class Tree:
    """Median-split tree over triangle centroids with the per-node records of the header: centre, radius, S, M."""

    def __init__(self, tris):
        self.tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
        self.area_vec = 0.5 * np.cross(self.tris[:, 1] - self.tris[:, 0], self.tris[:, 2] - self.tris[:, 0])
        self.area = np.sqrt((self.area_vec ** 2).sum(-1))
        self.cen = self.tris.mean(1)
        self.nodes = []   # (centre, r, S, M, ids, left, right)
        self.root = self._build(np.arange(self.tris.shape[0])) if self.tris.shape[0] else None

    def _build(self, ids):
        a, c, w = self.area_vec[ids], self.cen[ids], self.area[ids]
        centre = (w[:, None] * c).sum(0) / w.sum() if w.sum() > 0 else c.mean(0)
        r = np.sqrt(((self.tris[ids].reshape(-1, 3) - centre) ** 2).sum(-1).max())
        S = a.sum(0)
        M = (a[:, :, None] * (c - centre)[:, None, :]).sum(0)
        me = len(self.nodes)
        self.nodes.append(None)
        left = right = -1
        if ids.size > LEAF:
            axis = int(np.argmax(c.max(0) - c.min(0)))
            order = ids[np.argsort(c[:, axis], kind="stable")]
            left, right = self._build(order[: ids.size // 2]), self._build(order[ids.size // 2:])
        self.nodes[me] = (centre, r, S, M, ids, left, right)
        return me


def tree_winding(tree, points, beta):
    """The order-1 Barnes-Hut sum of every point: f64[P]."""
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.zeros(pts.shape[0])
    if tree.root is None:
        return out

    def visit(node, sel):
        centre, r, S, M, ids, left, right = tree.nodes[node]
        x = centre - pts[sel]
        d2 = (x * x).sum(-1)
        with np.errstate(invalid="ignore"):
            accept = d2 > (beta * r) ** 2 if np.isfinite(beta) else np.zeros(sel.size, bool)
        if accept.any():
            xa, da = x[accept], np.sqrt(d2[accept])
            dip = xa @ S
            quad = np.einsum("pi,ij,pj->p", xa, M, xa)
            out[sel[accept]] += (dip + np.trace(M) - 3.0 * quad / da ** 2) / (4.0 * np.pi * da ** 3)
        rest = sel[~accept]
        if rest.size == 0:
            return
        if left < 0:
            out[rest] += exact_winding(tree.tris[ids], pts[rest].astype(np.float32))
        else:
            visit(left, rest)
            visit(right, rest)

    visit(tree.root, np.arange(pts.shape[0]))
    return out


def model_error(tris, points, betas):
    """E_model(beta) = max |tree - exact| over the points, and the exact values: ({beta: E}, w_exact)."""
    w = exact_winding(tris, points)
    tree = Tree(tris)
    return {float(b): float(np.abs(tree_winding(tree, points, b) - w).max()) for b in betas}, w


def single_triangle_on_axis(radius, height):
    """Closed form: w of an equilateral triangle with circumradius `radius` in the plane z = 0 (normal +z), seen from (0, 0, -height)
    on its axis; the normal points away from the point, so w > 0.  The corners project to an equilateral spherical triangle with
    cos(side) = (h^2 - R^2 / 2) / (h^2 + R^2); the spherical law of cosines gives its angles, cos A = cos s / (1 + cos s), and the
    solid angle is the spherical excess 3 A - pi."""
    h, R = float(height), float(radius)
    cos_s = (h * h - 0.5 * R * R) / (h * h + R * R)
    A = np.arccos(cos_s / (1.0 + cos_s))
    return (3.0 * A - np.pi) / (4.0 * np.pi)


def holed(vertices, indices, z_above=0.8):
    """The triangle list without the triangles whose centroid lies above z = z_above."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    idx = np.asarray(indices).reshape(-1, 3)
    keep = v[idx].astype(np.float64).mean(1)[:, 2] <= z_above
    return np.ascontiguousarray(idx[keep].reshape(-1))
