"""Test oracle of m2s_grid_isosurface (include/m2s.h): the header's contract restated in numpy, vectorised over points and cells.
The table comes from tools/gen_isosurface_table.py, the generator of the committed header.  Every position is computed with
correctly rounded float32 operations in the header's order (numpy never fuses), so the GPU output must equal this bit for bit.

Grids are (nx, ny, nz) float32 arrays in the library's layout (L = k + j*nz + i*ny*nz, C order), or, for slabs, a function
layers(a, b) -> d[a:b] that lets a large grid be read a few layers at a time."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_isosurface_table as gen  # noqa: E402

F = np.float32
MAX_TRIS = gen.MAX_TRIS
TRI_COUNT = np.array([len(t) for t in gen.TABLE], np.int64)
TRIS = np.full((256, MAX_TRIS, 3), -1, np.int64)
for _c, _t in enumerate(gen.TABLE):
    if _t:
        TRIS[_c, :len(_t)] = _t
EDGE_OFF = np.array([o for o, _ in gen.EDGES], np.int64)    # (12, 3)
EDGE_AXIS = np.array([a for _, a in gen.EDGES], np.int64)   # (12,)


class GridI:
    """first_cell, cell_size, cell_count of an m2s_grid, as float32 / int64."""

    def __init__(self, first_cell, cell_size, cell_count):
        self.first = np.array(first_cell, F)
        self.cs = np.array(cell_size, F)
        self.n = tuple(int(v) for v in cell_count)

    @classmethod
    def of(cls, grid):
        return cls(grid.get_first_cell(), grid.get_cell_size(), grid.get_cell_count())

    def coord(self, axis, i):
        """m2s_grid_cell_center along one axis: first_cell + (float)i * cell_size, float32."""
        return (self.first[axis] + np.asarray(i, np.int64).astype(F) * self.cs[axis]).astype(F)


def _crossings(inside, n_own, nx_left):
    """Crossing flags (n_own, ny, nz, 3) of the points in the first n_own layers of `inside`; nx_left = layers that exist from the
    first one on (so the x-edge of the grid's last layer has no far end)."""
    n_own = min(n_own, inside.shape[0])
    _, ny, nz = inside.shape
    c = np.zeros((n_own, ny, nz, 3), bool)
    nxe = min(n_own, nx_left - 1, inside.shape[0] - 1)
    if nxe > 0:
        c[:nxe, :, :, 0] = inside[:nxe] != inside[1:nxe + 1]
    c[:, :-1, :, 1] = inside[:n_own, :-1] != inside[:n_own, 1:]
    c[:, :, :-1, 2] = inside[:n_own, :, :-1] != inside[:n_own, :, 1:]
    return c


def _cases(inside, n_cells_x):
    """Cases (n_cells_x, ny-1, nz-1) of the cells whose lowest corner is in the first n_cells_x layers of `inside`."""
    case = np.zeros((n_cells_x, inside.shape[1] - 1, inside.shape[2] - 1), np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                s = inside[dx:dx + n_cells_x, dy:dy + inside.shape[1] - 1, dz:dz + inside.shape[2] - 1]
                case |= s.astype(np.int64) << (4 * dx + 2 * dy + dz)
    return case


def _vertices(g, d, cross, i0, iso):
    """Positions of the crossing edges `cross` (layers from i0), in ascending 3*L + a, and their keys."""
    ny, nz = g.n[1], g.n[2]
    ii, jj, kk, aa = np.nonzero(cross)   # C order = ascending (L, a)
    gi = ii + i0
    d0 = d[ii, jj, kk]
    d1 = d[ii + (aa == 0), jj + (aa == 1), kk + (aa == 2)]
    iso = F(iso)
    t = (iso - d0) / (d1 - d0)
    idx = [gi, jj, kk]
    pos = np.empty((ii.size, 3), F)
    for ax in range(3):
        p = g.coord(ax, idx[ax])
        p1 = g.coord(ax, idx[ax] + 1)
        on = aa == ax
        pos[:, ax] = np.where(on, p + t * (p1 - p), p)
    keys = 3 * (kk + jj * nz + gi * ny * nz) + aa
    return pos.astype(F), keys.astype(np.int64)


def _triangles(g, case, i0, keys, v_base):
    """Triangles (global vertex ids) of the cells `case` (lowest corner layers from i0), cell L order then table order."""
    ny, nz = g.n[1], g.n[2]
    ci, cj, ck = np.nonzero(TRI_COUNT[case] > 0)
    cc = case[ci, cj, ck]
    cnt = TRI_COUNT[cc]
    rep = np.repeat(np.arange(cc.size), cnt)
    tri = np.arange(rep.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    e = TRIS[cc[rep], tri]                                     # (m, 3) local edges
    oi = (ci + i0)[rep][:, None] + EDGE_OFF[e, 0]
    oj = cj[rep][:, None] + EDGE_OFF[e, 1]
    ok = ck[rep][:, None] + EDGE_OFF[e, 2]
    key = 3 * (ok + oj * nz + oi * ny * nz) + EDGE_AXIS[e]
    pos = np.searchsorted(keys, key)
    assert np.all(keys[np.minimum(pos, keys.size - 1)] == key), "a triangle uses an edge that does not cross"
    return (pos + v_base).astype(np.int64)


def extract(g, d, iso=0.0):
    """The whole m2s_grid_isosurface output: (vertices f32 (n, 3), indices u32 (m, 3))."""
    d = np.asarray(d, F).reshape(g.n)
    inside = d < F(iso)
    cross = _crossings(inside, g.n[0], g.n[0])
    pos, keys = _vertices(g, d, cross, 0, iso)
    if min(g.n) < 2:
        return pos, np.zeros((0, 3), np.uint32)
    tris = _triangles(g, _cases(inside, g.n[0] - 1), 0, keys, 0)
    return pos, tris.astype(np.uint32)


def counts(g, layers, iso, x0, x1, chunk=16):
    """(crossing edges owned by points in layers [x0, x1), triangles of cells in layers [x0, x1)), read `chunk` layers at a time."""
    nv = nt = 0
    nx = g.n[0]
    for a in range(x0, x1, chunk):
        b = min(a + chunk, x1)
        inside = layers(a, min(b + 1, nx)) < F(iso)
        nv += int(_crossings(inside, b - a, nx - a).sum())
        ncx = min(b, nx - 1) - a
        if ncx > 0 and g.n[1] > 1 and g.n[2] > 1:
            nt += int(TRI_COUNT[_cases(inside, ncx)].sum())
    return nv, nt


def extract_slab(g, layers, iso, x0, x1, chunk=16):
    """The part of the output that belongs to the cell layers [x0, x1), with global indices:
    v_base, vertices (those of the points in layers [x0, min(x1 + 1, nx)), a contiguous range of the output from v_base),
    t_base, triangles (those of the cells in layers [x0, x1), a contiguous range from t_base)."""
    nx = g.n[0]
    v_base, t_base = counts(g, layers, iso, 0, x0, chunk)
    xe = min(x1 + 1, nx)
    d = np.asarray(layers(x0, min(xe + 1, nx)), F)
    inside = d < F(iso)
    pos, keys = _vertices(g, d, _crossings(inside, xe - x0, nx - x0), x0, iso)
    ncx = min(x1, nx - 1) - x0
    if ncx > 0 and g.n[1] > 1 and g.n[2] > 1:
        tris = _triangles(g, _cases(inside, ncx), x0, keys, v_base)
    else:
        tris = np.zeros((0, 3), np.int64)
    return v_base, pos, t_base, tris.astype(np.uint32)


# ---- checks on meshes -------------------------------------------------------------------------------------------------------------
def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def open_edges(tris):
    """Directed edges (a, b) whose opposite (b, a) no triangle has, and whether some directed edge appears more than once."""
    e = directed_edges(tris)
    n = int(e.max()) + 1 if e.size else 1
    k = e[:, 0] * n + e[:, 1]
    uk, cnt = np.unique(k, return_counts=True)
    rev = e[:, 1] * n + e[:, 0]
    missing = ~np.isin(rev, uk)
    return e[missing], bool((cnt > 1).any())


def euler(n_vertices, tris):
    e = directed_edges(tris)
    und = np.unique(np.sort(e, 1), axis=0)
    return n_vertices - und.shape[0] + len(tris)


def volume(v, tris):
    v = np.asarray(v, np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def normals(v, tris):
    v = np.asarray(v, np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return np.cross(b - a, c - a)
