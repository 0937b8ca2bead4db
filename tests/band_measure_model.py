"""The definition of m2s_band_measure (include/m2s.h) in numpy, to the bit of every integer field.

The measured surface is the mesh m2s_band_isosurface would extract (tests/band_isosurface_model.py): the cells whose 8 corners are all
active, the case from d < iso, the table of isosurface_table.h, the same float32 t = (iso - d0) / (d1 - d0) per crossing edge.  Per
triangle, with u the local coordinate of a vertex in its cell (the edge's corner offset, u[axis] = t) and U = (double)(i, j, k) + (double)u:

  area     q = u * cell_size (float32, per axis), A2 = |(q1 - q0) x (q2 - q0)| in float32 (sum of squares left to right, sqrt; a
           non-finite A2 counts as 0), w = floor((double)A2 * 2^(24 - E)), E = floor(log2(cmax * cmax)) with the product in float32
  volume   a = U1 - U0, b = U2 - U0, nz = a.x * b.y - a.y * b.x, sz = (U0.z + U1.z) + U2.z, llrint((nz * sz) * 2^20)
  moments  n = a x b, s = ((x0*x0 + x1*x1) + x2*x2) + ((x0*x1 + x1*x2) + x2*x0) over the vertices' U[c], llrint((n[c] * s) * 2^8)

in float64 without fused operations; a float64 term that is not finite counts as 0.  The sums are 64-bit integers (two's complement), per
group: the group of a cell is the label of its base corner's list place, the group of a vertex the label of the point that owns its edge.

Everything is dense on a box of the grid, so this is for small grids and for small boxes of large ones: `box` = (lo, shape) must hold
every active cell, with no active point on a high side of the box that is not a face of the grid (no cell is cut off by the box)."""
from typing import NamedTuple

import numpy as np

import isosurface_model as im

F = np.float32
D = np.float64
LABEL_NONE = 0xffffffff
INT_FIELDS = ("n_triangles", "n_vertices", "n_open", "n_border", "area_q", "volume_q", "moment_q")


class Raw(NamedTuple):
    """The integer fields of the groups' records, (n_groups,) each and moment_q (n_groups, 3), with the call's area exponent and n_skipped."""
    n_triangles: np.ndarray
    n_vertices: np.ndarray
    n_open: np.ndarray
    n_border: np.ndarray
    area_q: np.ndarray
    volume_q: np.ndarray
    moment_q: np.ndarray
    area_exponent: int
    n_skipped: int


def exponent_of(x):
    """sample.hip.h's sample_exponent: floor(log2(x)) of a positive finite float32 from its bits, subnormals included."""
    b = int(np.array(x, F).view(np.uint32))
    e, m = (b >> 23) & 0xff, b & 0x7fffff
    if e:
        return e - 127
    top = 22
    while top > 0 and not (m >> top) & 1:
        top -= 1
    return top - 149


def area_exponent(cell_size):
    cs = np.asarray(cell_size, F)
    cmax = cs.max()
    with np.errstate(over="ignore", under="ignore"):
        return exponent_of(F(cmax * cmax))


def moment_limit_ok(cell_count):
    n = [int(v) for v in cell_count]
    return n[0] * n[1] * n[2] * max(n) < 2 ** 50


def _llrint(x):
    """Round to nearest even -> int64; a term that is not finite (or, which no grid within the limits produces, not below 2^62) is 0."""
    ok = np.abs(x) < 2.0 ** 62     # a NaN fails the comparison
    return np.where(ok, np.rint(np.where(ok, x, 0.0)), 0.0).astype(np.int64)


def _sum(groups, values, n_groups, dtype):
    out = np.zeros(n_groups, dtype)
    np.add.at(out, groups, values.astype(dtype))
    return out


def measure(cell_count, cell_size, cells, distances, iso=0.0, labels=None, n_groups=1, box=None):
    """-> Raw.  cells: the grid's L = k + j*nz + i*ny*nz, ascending; labels: uint32 per list place, or None for one group."""
    count = tuple(int(v) for v in cell_count)
    cs = np.asarray(cell_size, F)
    lo, shape = ((0, 0, 0), count) if box is None else (tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1]))
    n_groups = 1 if labels is None else int(n_groups)
    L = np.asarray(cells).astype(np.int64).reshape(-1)
    assert (np.diff(L) > 0).all(), "cells must ascend strictly"
    ny, nz = count[1], count[2]
    idx = (L // (ny * nz) - lo[0], (L // nz) % ny - lo[1], L % nz - lo[2])
    assert all((0 <= c).all() and (c < n).all() for c, n in zip(idx, shape)), "a cell outside the box"
    act = np.zeros(shape, bool)
    d = np.zeros(shape, F)
    grp = np.full(shape, -1, np.int64)     # -1: not active, or skipped
    act[idx] = True
    d[idx] = np.asarray(distances, F).reshape(-1)
    lab = np.zeros(L.size, np.int64) if labels is None else np.asarray(labels).astype(np.int64).reshape(-1)
    assert lab.size == L.size
    valid = lab < n_groups
    grp[idx] = np.where(valid, lab, -1)
    for axis in range(3):
        assert lo[axis] + shape[axis] == count[axis] or not np.take(act, -1, axis).any(), "an active point on a face where the box cuts the grid"
    iso = F(iso)
    inside = d < iso
    E = area_exponent(cs)

    # ---- vertices: by the point that owns the edge ----
    n_vertices = np.zeros(n_groups, np.uint64)
    n_border = np.zeros(n_groups, np.uint64)
    gi = np.indices(shape)
    for a in range(3):
        if shape[a] < 2:
            continue
        near = tuple(slice(0, -1) if x == a else slice(None) for x in range(3))
        far = tuple(slice(1, None) if x == a else slice(None) for x in range(3))
        flag = act[near] & act[far] & (inside[near] != inside[far]) & (grp[near] >= 0)
        border = np.zeros(flag.shape, bool)
        for b in range(3):
            if b != a:
                ib = gi[b][near] + lo[b]
                border |= (ib == 0) | (ib == count[b] - 1)
        g = grp[near][flag]
        n_vertices += _sum(g, np.ones(g.size), n_groups, np.uint64)
        n_border += _sum(g, border[flag], n_groups, np.uint64)

    zero_u, zero_i = np.zeros(n_groups, np.uint64), np.zeros(n_groups, np.int64)
    if min(shape) < 2:
        return Raw(zero_u, n_vertices, zero_u.copy(), n_border, zero_u.copy(), zero_i, np.zeros((n_groups, 3), np.int64), E, int((~valid).sum()))

    # ---- cells: by the base corner ----
    sx, sy, sz_ = (n - 1 for n in shape)
    corner = lambda x, c: x[(c >> 2) & 1:((c >> 2) & 1) + sx, (c >> 1) & 1:((c >> 1) & 1) + sy, (c & 1):(c & 1) + sz_]   # noqa: E731
    n_act = sum(corner(act, c).astype(np.int64) for c in range(8))
    n_in = sum(corner(act & inside, c).astype(np.int64) for c in range(8))
    case = sum(corner(inside, c).astype(np.int64) << c for c in range(8))
    base_grp = corner(grp, 0)
    counted = base_grp >= 0
    is_open = counted & (n_act < 8) & (n_in > 0) & (n_in < n_act)
    n_open = _sum(base_grp[is_open], np.ones(int(is_open.sum())), n_groups, np.uint64)
    ci, cj, ck = np.nonzero(counted & (n_act == 8) & (im.TRI_COUNT[case] > 0))
    cc = case[ci, cj, ck]
    cnt = im.TRI_COUNT[cc]
    rep = np.repeat(np.arange(cc.size), cnt)
    tri = np.arange(rep.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    e = im.TRIS[cc[rep], tri]                                        # (m, 3) local edges
    g = base_grp[ci, cj, ck][rep]
    n_triangles = _sum(g, np.ones(g.size), n_groups, np.uint64)

    d8 = np.stack([corner(d, c)[ci, cj, ck] for c in range(8)], 1)   # (cells, 8)
    off = im.EDGE_OFF                                                # (12, 3)
    ax = im.EDGE_AXIS
    c0 = 4 * off[:, 0] + 2 * off[:, 1] + off[:, 2]
    c1 = c0 + (4 >> ax)
    with np.errstate(all="ignore"):
        t12 = ((iso - d8[:, c0]) / (d8[:, c1] - d8[:, c0])).astype(F)   # (cells, 12); used only where the edge crosses
    u = off[e].astype(F)                                             # (m, 3 vertices, 3 axes)
    tv = t12[rep[:, None], e]
    for a in range(3):
        u[:, :, a] = np.where(ax[e] == a, tv, u[:, :, a])

    with np.errstate(all="ignore"):
        # area, float32 in world scale
        q = (u * cs[None, None, :]).astype(F)
        p, r = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        nx_, ny_, nz_ = p[:, 1] * r[:, 2] - p[:, 2] * r[:, 1], p[:, 2] * r[:, 0] - p[:, 0] * r[:, 2], p[:, 0] * r[:, 1] - p[:, 1] * r[:, 0]
        A2 = np.sqrt(((nx_ * nx_ + ny_ * ny_) + nz_ * nz_).astype(F)).astype(F)
        A2 = np.where(A2 < np.inf, A2, F(0)).astype(F)
        w = np.floor(np.ldexp(A2.astype(D), 24 - E))
        assert (w < 2.0 ** 63).all()
        area_q = _sum(g, w, n_groups, np.uint64)
        # volume and first moments, float64 in index space
        base = np.stack([ci + lo[0], cj + lo[1], ck + lo[2]], 1)[rep].astype(D)    # (m, 3)
        U = base[:, None, :] + u.astype(D)
        a_, b_ = U[:, 1] - U[:, 0], U[:, 2] - U[:, 0]
        n = np.stack([a_[:, 1] * b_[:, 2] - a_[:, 2] * b_[:, 1], a_[:, 2] * b_[:, 0] - a_[:, 0] * b_[:, 2], a_[:, 0] * b_[:, 1] - a_[:, 1] * b_[:, 0]], 1)
        sz = (U[:, 0, 2] + U[:, 1, 2]) + U[:, 2, 2]
        volume_q = _sum(g, _llrint((n[:, 2] * sz) * 2.0 ** 20), n_groups, np.int64)
        moment_q = np.zeros((n_groups, 3), np.int64)
        for c in range(3):
            x0, x1, x2 = U[:, 0, c], U[:, 1, c], U[:, 2, c]
            s = ((x0 * x0 + x1 * x1) + x2 * x2) + ((x0 * x1 + x1 * x2) + x2 * x0)
            moment_q[:, c] = _sum(g, _llrint((n[:, c] * s) * 2.0 ** 8), n_groups, np.int64)
    return Raw(n_triangles, n_vertices, n_open, n_border, area_q, volume_q, moment_q, E, int((~valid).sum()))


def derived(raw, first_cell, cell_size, group=0):
    """(area, volume, centroid[3]) of one group in world units, as the header derives them from the raw sums on the host."""
    first, cs = np.asarray(first_cell, F).astype(D), np.asarray(cell_size, F).astype(D)
    area = float(np.ldexp(D(int(raw.area_q[group])), raw.area_exponent - 25))
    v6 = D(int(raw.volume_q[group])) * 2.0 ** -20 / 6.0
    volume = float(v6 * cs[0] * cs[1] * cs[2])
    with np.errstate(all="ignore"):
        centroid = [float(first[c] + (D(int(raw.moment_q[group, c])) * 2.0 ** -8 / 24.0) / v6 * cs[c]) if raw.volume_q[group] != 0 else float("nan")
                    for c in range(3)]
    return area, volume, centroid


def closed(raw, group=0):
    return int(raw.n_open[group]) == 0 and int(raw.n_border[group]) == 0


def euler(raw, group=0):
    return int(raw.n_vertices[group]) - int(raw.n_triangles[group]) // 2


# ---- independent float64 measures of an extracted mesh ------------------------------------------------------------------------------------
def mesh_area(v, tris):
    n = im.normals(v, tris)
    return float(0.5 * np.sqrt((n * n).sum(1)).sum())


def mesh_centroid(v, tris):
    """The centre of mass of the solid a closed mesh bounds: signed tetrahedra from the origin."""
    v = np.asarray(v, D)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    six_v = np.einsum("ij,ij->i", a, np.cross(b, c))
    return ((a + b + c) / 4.0 * six_v[:, None]).sum(0) / six_v.sum()


# ---- fields the tests share ---------------------------------------------------------------------------------------------------------------
def sphere_distance(shape, centre, radius, cell=(1.0, 1.0, 1.0)):
    """The signed distance to a sphere (centre and radius in world units of a grid at the origin with cells `cell`), float32."""
    i, j, k = np.meshgrid(*(np.arange(n, dtype=D) * c for n, c in zip(shape, cell)), indexing="ij")
    return (np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius).astype(F)


def torus_distance(shape, centre, major, minor):
    i, j, k = np.meshgrid(*(np.arange(n, dtype=D) for n in shape), indexing="ij")
    ring = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2) - major
    return (np.sqrt(ring ** 2 + (k - centre[2]) ** 2) - minor).astype(F)


def band_of(d_dense, width):
    """(cells uint64 ascending, distances) of the points with |d| <= width."""
    d = np.asarray(d_dense, F).reshape(-1)
    active = np.abs(d) <= F(width)
    return np.flatnonzero(active).astype(np.uint64), d[active]
