"""Host-side mirror of the reference's public interface for the hot path, over the C ABI.

Same names, argument meaning and error behaviour as mesh_to_sdf 0.4.0
(/root/reference/mesh_to_sdf/src/lib.rs:151-311, generate/grid.rs:265-274, grid.rs:30-170), so
the parity tests read like the reference's own tests:

    sdf = generate_sdf(vertices, Topology.TriangleList(indices), query_points, AccelerationMethod.RtreeBvh)
    grid = Grid.from_bounding_box(bbox_min, bbox_max, [nx, ny, nz])
    sdf = generate_grid_sdf(vertices, Topology.TriangleList(indices), grid, SignMethod.Raycast)

numpy in -> numpy out (host pointers through the ABI: the drop-in case, H2D/D2H inside the call);
torch CUDA tensors in -> torch CUDA tensor out (device pointers, enqueued on torch's current
stream, nothing crosses PCIe).  Where the reference panics this raises M2SPanic.
"""
import ctypes as C
import enum
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import M2SGrid, M2SOpts, M2STimings


class M2SError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"m2s error {code}: {msg}")
        self.code = code


class M2SPanic(M2SError):
    """The reference would have panicked here (index out of range, NaN distance, empty R-tree)."""


class SignMethod(enum.IntEnum):
    """lib.rs:204-216 (default Raycast)."""
    Raycast = 0
    Normal = 1


@dataclass(frozen=True)
class AccelerationMethod:
    """lib.rs:224-239: None(SignMethod) | Bvh(SignMethod) | Rtree | RtreeBvh (default)."""
    kind: int
    sign: SignMethod = SignMethod.Raycast

    @staticmethod
    def None_(sign: SignMethod = SignMethod.Raycast):
        return AccelerationMethod(0, SignMethod(sign))

    @staticmethod
    def Bvh(sign: SignMethod = SignMethod.Raycast):
        return AccelerationMethod(1, SignMethod(sign))


AccelerationMethod.Rtree = AccelerationMethod(2, SignMethod.Normal)
AccelerationMethod.RtreeBvh = AccelerationMethod(3, SignMethod.Raycast)


@dataclass(frozen=True)
class Topology:
    """lib.rs:151-167.  indices=None means 0..len(vertices)."""
    kind: int
    indices: Optional[object] = None

    @staticmethod
    def TriangleList(indices=None):
        return Topology(0, indices)

    @staticmethod
    def TriangleStrip(indices=None):
        return Topology(1, indices)


class Grid:
    """grid.rs:30-170.  All arithmetic is the reference's f32 arithmetic (through the C ABI helpers)."""

    def __init__(self, first_cell, cell_size, cell_count):  # Grid::new, grid.rs:43-49
        self._g = M2SGrid()
        for k in range(3):
            self._g.first_cell[k] = float(np.float32(first_cell[k]))
            self._g.cell_size[k] = float(np.float32(cell_size[k]))
            self._g.cell_count[k] = int(cell_count[k])

    new = classmethod(lambda cls, first_cell, cell_size, cell_count: cls(first_cell, cell_size, cell_count))

    @classmethod
    def from_bounding_box(cls, bbox_min, bbox_max, cell_count):  # grid.rs:59-74
        g = cls.__new__(cls)
        g._g = M2SGrid()
        mn = (C.c_float * 3)(*[float(np.float32(v)) for v in bbox_min])
        mx = (C.c_float * 3)(*[float(np.float32(v)) for v in bbox_max])
        cnt = (C.c_uint64 * 3)(*[int(v) for v in cell_count])
        _lib.lib().m2s_grid_from_bounding_box(mn, mx, cnt, C.byref(g._g))
        return g

    def __eq__(self, other):  # #[derive(PartialEq)], grid.rs:27
        return isinstance(other, Grid) and bytes(self._g) == bytes(other._g)

    def __repr__(self):
        return f"Grid(first_cell={list(self._g.first_cell)}, cell_size={list(self._g.cell_size)}, cell_count={list(self._g.cell_count)})"

    def get_first_cell(self):
        return np.array(list(self._g.first_cell), np.float32)

    def get_cell_size(self):
        return np.array(list(self._g.cell_size), np.float32)

    def get_cell_count(self):
        return [int(v) for v in self._g.cell_count]

    def get_total_cell_count(self):
        c = self.get_cell_count()
        return c[0] * c[1] * c[2]

    def get_last_cell(self):  # grid.rs:82-88 (first + count * size, as written in the reference)
        f, s, c = self.get_first_cell(), self.get_cell_size(), self.get_cell_count()
        return (f + np.array(c, np.float32) * s).astype(np.float32)

    def get_bounding_box(self):  # grid.rs:110-119
        f, s, c = self.get_first_cell(), self.get_cell_size(), self.get_cell_count()
        mn = (f - s * np.float32(0.5)).astype(np.float32)
        mx = (mn + np.array(c, np.float32) * s).astype(np.float32)
        return mn, mx

    def get_cell_idx(self, cell):  # grid.rs:122-124
        return int(_lib.lib().m2s_grid_cell_idx(C.byref(self._g), (C.c_uint64 * 3)(*[int(v) for v in cell])))

    def get_cell_integer_coordinates(self, cell_idx):  # grid.rs:127-132
        c = self.get_cell_count()
        return [cell_idx // (c[1] * c[2]), (cell_idx // c[2]) % c[1], cell_idx % c[2]]

    def get_cell_center(self, cell):  # grid.rs:135-141
        out = (C.c_float * 3)()
        _lib.lib().m2s_grid_cell_center(C.byref(self._g), (C.c_uint64 * 3)(*[int(v) for v in cell]), out)
        return np.array(list(out), np.float32)

    def snap_point_to_grid(self, point):  # grid.rs:145-170 -> ("Inside"|"Outside", [x, y, z])
        mn, _ = self.get_bounding_box()
        s, c = self.get_cell_size(), self.get_cell_count()
        with np.errstate(all="ignore"):
            cell = np.floor((np.asarray(point, np.float32) - mn) / s)
        cell = [0 if not np.isfinite(v) and np.isnan(v) else int(np.clip(v, -2.0**62, 2.0**62)) for v in cell]
        res = [min(max(cell[k], 0), c[k] - 1) for k in range(3)]
        return ("Inside" if res == cell else "Outside"), res

    def __eq__(self, other):
        return isinstance(other, Grid) and bytes(self._g) == bytes(other._g)


def _raise(rc):
    msg = _lib.last_error()
    if rc in (_lib.ERR_BAD_ARG, _lib.ERR_NAN, _lib.ERR_EMPTY_MESH):
        raise M2SPanic(rc, msg)
    raise M2SError(rc, msg)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class _Args:
    """Normalises (vertices, topology[, queries]) to raw pointers for one call."""

    def __init__(self, vertices, topology: Topology, queries=None):
        self.keep = []
        self.device = _is_torch(vertices) and vertices.is_cuda
        if self.device:
            import torch

            self.torch = torch
            self.dev = vertices.device
            v = vertices.detach().to(torch.float32).contiguous().reshape(-1, 3)
            self.n_verts = v.shape[0]
            self.p_verts = v.data_ptr() if v.numel() else None
            self.keep.append(v)
            idx = topology.indices
            self.index_bytes = 4
            if idx is None:
                self.p_idx, self.n_idx = None, 0
            else:
                if not _is_torch(idx):
                    idx = torch.as_tensor(np.ascontiguousarray(idx).astype(np.int64), device=self.dev)
                idx = idx.to(device=self.dev, dtype=torch.int32).contiguous().reshape(-1)  # bit pattern == u32
                self.n_idx = idx.numel()
                self.p_idx = idx.data_ptr() if idx.numel() else _dummy_device_ptr(torch, self.dev, self.keep)
                self.keep.append(idx)
            if queries is not None:
                q = queries if _is_torch(queries) else torch.as_tensor(np.asarray(queries, np.float32), device=self.dev)
                q = q.detach().to(device=self.dev, dtype=torch.float32).contiguous().reshape(-1, 3)
                self.n_q = q.shape[0]
                self.p_q = q.data_ptr() if q.numel() else None
                self.keep.append(q)
        else:
            v = np.ascontiguousarray(np.asarray(vertices, np.float32)).reshape(-1, 3)
            self.n_verts = v.shape[0]
            self.p_verts = v.ctypes.data if v.size else None
            self.keep.append(v)
            idx = topology.indices
            if idx is None:
                self.p_idx, self.n_idx, self.index_bytes = None, 0, 4
            else:
                idx = np.asarray(idx)
                if idx.dtype == np.uint16:
                    idx = np.ascontiguousarray(idx).reshape(-1)
                    self.index_bytes = 2
                else:
                    if idx.size and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
                        raise M2SPanic(_lib.ERR_BAD_ARG, "index does not fit u32")
                    idx = np.ascontiguousarray(idx.astype(np.uint32)).reshape(-1)
                    self.index_bytes = 4
                self.n_idx = idx.size
                self._empty = np.zeros(4, np.uint32)
                self.p_idx = idx.ctypes.data if idx.size else self._empty.ctypes.data
                self.keep.append(idx)
            if queries is not None:
                q = np.ascontiguousarray(np.asarray(queries, np.float32)).reshape(-1, 3)
                self.n_q = q.shape[0]
                self.p_q = q.ctypes.data if q.size else None
                self.keep.append(q)
        self.topology = topology.kind

    def opts(self, timings=None, algorithm=0, x_begin=0, x_end=0, synchronous=True, peer_out=None, peer_mode=0, lane=0, x_period=0):
        o = M2SOpts()
        o.struct_size = C.sizeof(M2SOpts)
        o.algorithm = int(algorithm)
        o.x_begin, o.x_end = int(x_begin), int(x_end)
        o.x_period = int(x_period)
        o.synchronous = 1 if synchronous else 0
        o.lane = int(lane)
        if peer_out:
            ptrs = [int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p) for p in peer_out]
            arr = (C.c_void_p * len(ptrs))(*ptrs)
            self.keep.append(arr)
            o.n_peer_out = len(ptrs)
            o.peer_out = C.cast(arr, C.POINTER(C.c_void_p))
            o.peer_mode = int(peer_mode)
        if timings is not None:
            o.timings = C.pointer(timings)
        if self.device:
            o.device = self.dev.index if self.dev.index is not None else self.torch.cuda.current_device()
            # torch's current stream, exactly: its default stream has handle 0, which must NOT be read as
            # "pick your own stream" or work torch orders after this call (collectives!) would race with it
            o.stream = self.torch.cuda.current_stream(self.dev).cuda_stream
            o.stream_mode = 1
            o.mem_kind = _lib.MEM_DEVICE
        else:
            o.device = -1
            o.mem_kind = _lib.MEM_HOST
        return o


def _dummy_device_ptr(torch, dev, keep):
    t = torch.zeros(4, dtype=torch.int32, device=dev)
    keep.append(t)
    return t.data_ptr()


def generate_sdf(vertices, indices: Topology, query_points, acceleration_method: AccelerationMethod = None, *,
                 timings: M2STimings = None, algorithm: int = 0):
    """lib.rs:291-311."""
    am = acceleration_method if acceleration_method is not None else AccelerationMethod.RtreeBvh
    a = _Args(vertices, indices, query_points)
    n_out = C.c_size_t(0)
    if a.device:
        out = a.torch.empty(a.n_q, dtype=a.torch.float32, device=a.dev)
        p_out = out.data_ptr() if a.n_q else None
    else:
        out = np.empty(a.n_q, np.float32)
        p_out = out.ctypes.data if a.n_q else None
    o = a.opts(timings, algorithm)
    rc = _lib.lib().m2s_generate_sdf(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, a.p_q, a.n_q,
                                     int(am.kind), int(am.sign), p_out, C.byref(n_out), C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return out[: n_out.value]


def _closest_buffers(a, n):
    """(triangles uint32[n], points f32[n, 3], distances f32[n]) on the call's side, and their raw pointers."""
    if a.device:
        t = a.torch
        tri = t.empty(n, dtype=t.int32, device=a.dev)   # bit pattern == u32; handed out as uint32 where torch has it
        pts = t.empty((n, 3), dtype=t.float32, device=a.dev)
        dist = t.empty(n, dtype=t.float32, device=a.dev)
        ptrs = [x.data_ptr() if n else None for x in (tri, pts, dist)]
    else:
        tri, pts, dist = np.empty(n, np.uint32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
        ptrs = [x.ctypes.data if n else None for x in (tri, pts, dist)]
    return (tri, pts, dist), ptrs


def _closest_result(a, bufs):
    tri, pts, dist = bufs
    if a.device and hasattr(a.torch, "uint32"):
        tri = tri.view(a.torch.uint32)
    return tri, pts, dist


def closest_points(vertices, indices: Topology, query_points, *, timings: M2STimings = None, algorithm: int = 0):
    """Nearest triangle, closest point on it and unsigned distance of every query (include/m2s.h m2s_closest_points): returns
    (triangles uint32[n], points f32[n, 3], distances f32[n]).  The triangle index is in Topology order (lowest index on ties,
    0xFFFFFFFF where no distance is comparable); distances are bit-equal to |generate_sdf(.., RtreeBvh)|."""
    a = _Args(vertices, indices, query_points)
    bufs, (pt, pp, pd) = _closest_buffers(a, a.n_q)
    o = a.opts(timings, algorithm)
    rc = _lib.lib().m2s_closest_points(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, a.p_q, a.n_q, pt, pp, pd,
                                       C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return _closest_result(a, bufs)


def grid_closest_points(vertices, indices: Topology, grid: "Grid", *, timings: M2STimings = None, algorithm: int = 0,
                        x_slab: Sequence[int] = None, out=None):
    """closest_points for the cell centres of `grid`, flattened in grid order (z + y * nz + x * ny * nz).  `x_slab=(x0, x1)`
    computes only the cells with x0 <= x < x1; `out` = (triangles, points, distances) of the whole grid to write into (the rest is
    left untouched)."""
    a = _Args(vertices, indices)
    total = grid.get_total_cell_count()
    if out is None:
        bufs, ptrs = _closest_buffers(a, total)
    else:
        bufs = tuple(out)
        ptrs = [(x.data_ptr() if a.device else x.ctypes.data) if total else None for x in bufs]
    xb, xe = (0, 0) if x_slab is None else (int(x_slab[0]), int(x_slab[1]))
    if x_slab is not None and xb == xe:
        return _closest_result(a, bufs)
    o = a.opts(timings, algorithm, xb, xe)
    rc = _lib.lib().m2s_grid_closest_points(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, C.byref(grid._g),
                                            *ptrs, C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return _closest_result(a, bufs)


WINDING_BETA_DEFAULT = _lib.WINDING_BETA_DEFAULT


def _queries_of(a, query_points):
    """(array kept alive, count, raw pointer) of a query set on the side of `a` (device tensor or numpy)."""
    if a.device:
        q = query_points if _is_torch(query_points) else a.torch.as_tensor(np.asarray(query_points, np.float32), device=a.dev)
        q = q.detach().to(device=a.dev, dtype=a.torch.float32).contiguous().reshape(-1, 3)
        return q, q.shape[0], (q.data_ptr() if q.numel() else None)
    q = np.ascontiguousarray(np.asarray(query_points, np.float32)).reshape(-1, 3)
    return q, q.shape[0], (q.ctypes.data if q.size else None)


def _f32_buffer(a, n, out=None):
    """f32[n] on the call's side (or `out`), and its raw pointer."""
    if out is None:
        out = a.torch.empty(n, dtype=a.torch.float32, device=a.dev) if a.device else np.empty(n, np.float32)
    return out, ((out.data_ptr() if a.device else out.ctypes.data) if n else None)


def _winding_queries(call, a, n_q, p_q, beta, threshold, signed, timings, algorithm, synchronous=True):
    """One point-form winding call: `call(p_q, n_q, beta, threshold, p_w, p_sdf, opts)`; returns w, or signed distances."""
    out, p_out = _f32_buffer(a, n_q)
    o = a.opts(timings, algorithm, synchronous=synchronous or not a.device)
    rc = call(p_q, n_q, float(beta), float(threshold), None if signed else p_out, p_out if signed else None, C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return out


def _winding_grid(call, a, grid, beta, threshold, signed, timings, algorithm, x_slab, out, synchronous=True):
    """One grid-form winding call: `call(grid, beta, threshold, p_w, p_sdf, opts)`."""
    out, p_out = _f32_buffer(a, grid.get_total_cell_count(), out)
    xb, xe = (0, 0) if x_slab is None else (int(x_slab[0]), int(x_slab[1]))
    if x_slab is not None and xb == xe:
        return out
    o = a.opts(timings, algorithm, xb, xe, synchronous or not a.device)
    rc = call(C.byref(grid._g), float(beta), float(threshold), None if signed else p_out, p_out if signed else None, C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return out


def _one_shot_winding_queries(vertices, indices, query_points, beta, threshold, signed, timings, algorithm):
    a = _Args(vertices, indices, query_points)
    L = _lib.lib()
    return _winding_queries(lambda *r: L.m2s_winding_numbers(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, *r),
                            a, a.n_q, a.p_q, beta, threshold, signed, timings, algorithm)


def _one_shot_winding_grid(vertices, indices, grid, beta, threshold, signed, timings, algorithm, x_slab, out):
    a = _Args(vertices, indices)
    L = _lib.lib()
    return _winding_grid(lambda *r: L.m2s_grid_winding_numbers(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, *r),
                         a, grid, beta, threshold, signed, timings, algorithm, x_slab, out)


def winding_numbers(vertices, indices: Topology, query_points, *, beta: float = WINDING_BETA_DEFAULT, algorithm: int = 0,
                    timings: M2STimings = None):
    """Generalized winding number of every query (include/m2s.h m2s_winding_numbers): f32[n], 1 inside and 0 outside a closed mesh whose
    right-hand normals point outward, smooth across holes; `w >= 0.5` is the robust inside test.  `beta` is the Barnes-Hut opening
    parameter (>= 1; `float('inf')`: the exact sum through the tree); `algorithm=1`: all pairs, no tree."""
    return _one_shot_winding_queries(vertices, indices, query_points, beta, 0.5, False, timings, algorithm)


def grid_winding_numbers(vertices, indices: Topology, grid: "Grid", *, beta: float = WINDING_BETA_DEFAULT, algorithm: int = 0,
                         timings: M2STimings = None, x_slab: Sequence[int] = None, out=None):
    """winding_numbers for the cell centres of `grid`, flattened in grid order; `x_slab` / `out` as for grid_closest_points."""
    return _one_shot_winding_grid(vertices, indices, grid, beta, 0.5, False, timings, algorithm, x_slab, out)


def generate_sdf_winding(vertices, indices: Topology, query_points, *, beta: float = WINDING_BETA_DEFAULT, threshold: float = 0.5,
                         algorithm: int = 0, timings: M2STimings = None):
    """Signed distances whose sign is the winding number's: -d where w >= threshold, else +d; |result| is bit-equal to the distance of
    closest_points.  For meshes with holes, open borders or self-intersections, where neither SignMethod gives a usable sign."""
    return _one_shot_winding_queries(vertices, indices, query_points, beta, threshold, True, timings, algorithm)


def generate_grid_sdf_winding(vertices, indices: Topology, grid: "Grid", *, beta: float = WINDING_BETA_DEFAULT, threshold: float = 0.5,
                              algorithm: int = 0, timings: M2STimings = None, x_slab: Sequence[int] = None, out=None):
    """generate_sdf_winding for the cell centres of `grid`."""
    return _one_shot_winding_grid(vertices, indices, grid, beta, threshold, True, timings, algorithm, x_slab, out)


class RayHits(NamedTuple):
    """First hit of every ray: t f32[n] (+inf: none), triangle uint32[n] (0xFFFFFFFF: none), uv f32[n, 2] (NaN: none)."""
    t: object
    triangle: object
    uv: object


def _ray_call(call, a, origins, directions, t_min, t_max, want, timings, algorithm, synchronous=True):
    """One ray call, `call(p_org, p_dir, n, ropts, p_t, p_tri, p_uv, p_count, p_occ, opts)`; `want` names the outputs: "hits" (t, triangle,
    uv), "count" or "occluded".  Returns the arrays asked for, on the side of `a`."""
    org, n, p_org = _queries_of(a, origins)
    dirs, n_d, p_dir = _queries_of(a, directions)
    if n != n_d:
        raise M2SPanic(_lib.ERR_BAD_ARG, "origins and directions differ in length (%d, %d)" % (n, n_d))
    ro = _lib.M2SRayOpts(C.sizeof(_lib.M2SRayOpts), float(t_min), float(t_max))

    def buf(shape, np_dtype, torch_dtype):
        x = a.torch.empty(shape, dtype=getattr(a.torch, torch_dtype), device=a.dev) if a.device else np.empty(shape, np_dtype)
        return x, ((x.data_ptr() if a.device else x.ctypes.data) if n else None)

    ptrs = [None] * 5
    if want == "hits":
        (t, ptrs[0]), (tri, ptrs[1]), (uv, ptrs[2]) = buf(n, np.float32, "float32"), buf(n, np.uint32, "int32"), buf((n, 2), np.float32, "float32")
        if a.device and hasattr(a.torch, "uint32"):
            tri = tri.view(a.torch.uint32)
        res = RayHits(t, tri, uv)
    elif want == "count":
        res, ptrs[3] = buf(n, np.uint32, "int32")
    else:
        res, ptrs[4] = buf(n, np.uint8, "uint8")
    o = a.opts(timings, algorithm, synchronous=synchronous or not a.device)
    rc = call(p_org, p_dir, n, C.byref(ro), *ptrs, C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    if want == "occluded":
        return res.bool() if a.device else res.astype(bool)
    return res


def _one_shot_rays(vertices, indices, origins, directions, t_min, t_max, want, timings, algorithm):
    a = _Args(vertices, indices)
    L = _lib.lib()
    return _ray_call(lambda *r: L.m2s_cast_rays(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, *r), a, origins, directions,
                     t_min, t_max, want, timings, algorithm)


def cast_rays(vertices, indices: Topology, origins, directions, t_min: float = 0.0, t_max: float = float("inf"), algorithm: int = 0, *,
              timings: M2STimings = None) -> RayHits:
    """First hit of every ray o + t d, t_min <= t <= t_max, on the mesh (include/m2s.h m2s_cast_rays): RayHits(t, triangle, uv) with the
    watertight test of Woop, Benthin and Wald, defined to the bit.  `directions` are used as given, so t is in units of |d|; the triangle
    index is in Topology order (the lowest index on exact ties of t); hit = a + u (b - a) + v (c - a).  `algorithm=1`: every triangle for
    every ray, no tree.  Host arrays or device tensors, as the other calls take them."""
    return _one_shot_rays(vertices, indices, origins, directions, t_min, t_max, "hits", timings, algorithm)


def count_intersections(vertices, indices: Topology, origins, directions, t_min: float = 0.0, t_max: float = float("inf"), algorithm: int = 0,
                        *, timings: M2STimings = None):
    """Number of triangles every ray hits in range, uint32[n].  A ray through a shared edge or vertex counts every triangle that includes it."""
    return _one_shot_rays(vertices, indices, origins, directions, t_min, t_max, "count", timings, algorithm)


def test_occlusions(vertices, indices: Topology, origins, directions, t_min: float = 0.0, t_max: float = float("inf"), algorithm: int = 0, *,
                    timings: M2STimings = None):
    """bool[n]: is anything in the way of the ray within [t_min, t_max].  The walk stops at a ray's first hit."""
    return _one_shot_rays(vertices, indices, origins, directions, t_min, t_max, "occluded", timings, algorithm)


test_occlusions.__test__ = False   # (a public name that starts with "test": not a test for pytest to collect)


class SurfaceSamples(NamedTuple):
    """Area-weighted surface samples: points f32[n, 3], triangle uint32[n] (Topology order), uv f32[n, 2] (weights of b and c),
    normal f32[n, 3] (unit right-hand normal; None unless asked for), area (float: the total area of the triangles with area)."""
    points: object
    triangle: object
    uv: object
    normal: object
    area: float


def _sample_call(call, a, n, seed, first_sample, normals, timings, algorithm, synchronous=True, points_only=False):
    """One sampling call, `call(n, sopts, p_point, p_tri, p_uv, p_normal, p_area, opts)`; the arrays are made on the side of `a`."""
    n = int(n)
    if n < 0:
        raise M2SPanic(_lib.ERR_BAD_ARG, "negative sample count")
    so = _lib.M2SSurfaceSampleOpts(C.sizeof(_lib.M2SSurfaceSampleOpts), 0, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_sample))

    def buf(shape, np_dtype, torch_dtype):
        x = a.torch.empty(shape, dtype=getattr(a.torch, torch_dtype), device=a.dev) if a.device else np.empty(shape, np_dtype)
        return x, ((x.data_ptr() if a.device else x.ctypes.data) if n else None)

    pts, p_pts = buf((n, 3), np.float32, "float32")
    tri = uv = nrm = None
    p_tri = p_uv = p_nrm = None
    if not points_only:
        (tri, p_tri), (uv, p_uv) = buf(n, np.uint32, "int32"), buf((n, 2), np.float32, "float32")
        if a.device and hasattr(a.torch, "uint32"):
            tri = tri.view(a.torch.uint32)
    if normals:
        nrm, p_nrm = buf((n, 3), np.float32, "float32")
    area = C.c_double(0.0)
    o = a.opts(timings, algorithm, synchronous=synchronous or not a.device)
    rc = call(n, C.byref(so), p_pts, p_tri, p_uv, p_nrm, C.byref(area), C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return SurfaceSamples(pts, tri, uv, nrm, float(area.value))


def sample_surface(vertices, indices: Topology, n: int, seed: int = 0, first_sample: int = 0, normals: bool = False, *, algorithm: int = 0,
                   timings: M2STimings = None) -> SurfaceSamples:
    """`n` points distributed uniformly over the surface (include/m2s.h m2s_sample_surface), defined to the bit: sample i is global sample
    first_sample + i, and its value depends only on the triangles in Topology order, `seed` and that number — so ranks of a job take
    disjoint ranges of one seed, and two half calls equal one whole call.  Triangles without area are never chosen; a mesh with none
    raises.  Host arrays or device tensors, as the other calls take them; tests/sample_model.py is the definition in numpy."""
    a = _Args(vertices, indices)
    L = _lib.lib()
    return _sample_call(lambda *r: L.m2s_sample_surface(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, *r), a, n, seed,
                        first_sample, normals, timings, algorithm)


def surface_area(vertices, indices: Topology) -> float:
    """Total area of the mesh's triangles as the sampler weighs them (non-finite areas count as 0); 0.0 for a mesh without area."""
    a = _Args(vertices, indices)
    area = C.c_double(0.0)
    o = a.opts()
    rc = _lib.lib().m2s_sample_surface(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, 0, None, None, None, None, None,
                                       C.byref(area), C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return float(area.value)


class Voxels(NamedTuple):
    """Occupancy of a grid: occupancy uint8[nx, ny, nz] (0 / 1), bits uint32[nx, ny, ceil(nz / 32)] (cell k of a row is bit k & 31 of
    word k >> 5; None unless asked for), cells (grid-order indices of the set cells, ascending; uint64 on the host, int64 on the device;
    None unless asked for), count (set cells; None for an asynchronous call)."""
    occupancy: object
    bits: object
    cells: object
    count: Optional[int]


def _voxel_call(call, a, grid, solid, bits, cells, timings, algorithm, synchronous=True, occupancy=True, count=True):
    """One voxelization, `call(grid, vopts, p_bits, p_occ, p_cells, capacity, p_count, opts)`; the arrays are made on the side of `a`.
    `cells` takes a counting call first: its capacity is the count."""
    nx, ny, nz = (int(v) for v in grid.get_cell_count())
    nzw = (nz + 31) // 32
    vo = _lib.M2SVoxelizeOpts(C.sizeof(_lib.M2SVoxelizeOpts), 1 if solid else 0)
    synchronous = synchronous or not a.device
    if cells and not synchronous:
        raise M2SPanic(_lib.ERR_BAD_ARG, "cells needs a synchronous call")

    def buf(shape, np_dtype, torch_dtype):
        x = a.torch.empty(shape, dtype=getattr(a.torch, torch_dtype), device=a.dev) if a.device else np.empty(shape, np_dtype)
        filled = x.numel() if a.device else x.size
        return x, ((x.data_ptr() if a.device else x.ctypes.data) if filled else None)

    want_count = synchronous and (count or cells)
    count = C.c_uint64(0)
    cell_arr, p_cells, capacity = None, None, 0
    if cells:
        o = a.opts(None, algorithm)
        rc = call(C.byref(grid._g), C.byref(vo), None, None, None, 0, C.byref(count), C.byref(o))
        if rc != _lib.M2S_OK:
            _raise(rc)
        capacity = int(count.value)
        cell_arr, p_cells = buf(capacity, np.uint64, "int64")
    occ, p_occ = buf((nx, ny, nz), np.uint8, "uint8") if occupancy else (None, None)
    bit_arr, p_bits = buf((nx, ny, nzw), np.uint32, "int32") if bits else (None, None)
    if bits and a.device and hasattr(a.torch, "uint32"):
        bit_arr = bit_arr.view(a.torch.uint32)
    o = a.opts(timings, algorithm, synchronous=synchronous)
    rc = call(C.byref(grid._g), C.byref(vo), p_bits, p_occ, p_cells, capacity, C.byref(count) if want_count else None, C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return Voxels(occ, bit_arr, cell_arr, int(count.value) if want_count else None)


def voxelize(vertices, indices: Topology, grid: "Grid", solid: bool = False, *, bits: bool = False, cells: bool = False, algorithm: int = 0,
             timings: M2STimings = None, occupancy: bool = True, count: bool = True) -> Voxels:
    """Which cells of `grid` the mesh occupies (include/m2s.h m2s_voxelize), defined to the bit: a cell is set when its closed box touches
    a triangle (the separating-axis test of Akenine-Moller with its operations fixed), and with `solid` also when its centre is inside by
    the Raycast sign of generate_grid_sdf.  `algorithm=1` tests every cell against every triangle (the definition; the same bits).  Host
    arrays or device tensors, as the other calls take them; tests/voxel_model.py is the definition in numpy.  `occupancy=False` /
    `count=False` leave those outputs out (None): the count costs one synchronisation of the stream."""
    a = _Args(vertices, indices)
    L = _lib.lib()
    return _voxel_call(lambda *r: L.m2s_voxelize(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, *r), a, grid, solid, bits,
                       cells, timings, algorithm, True, occupancy, count)


class NarrowBand(NamedTuple):
    """The cells of a grid within a band of the surface (include/m2s.h m2s_narrow_band_sdf): cells (their grid-order indices L, ascending;
    uint64 on the host, int64 on the device), distances (float32, distances[n] = the dense generate_grid_sdf value at cells[n], bit for bit),
    bits (uint32[nx, ny, ceil(nz / 32)], the layout of Voxels.bits; None unless asked for), count, grid."""
    cells: object
    distances: object
    bits: object
    count: int
    grid: "Grid"

    def ijk(self):
        """(count, 3) cell coordinates: L = k + j*nz + i*ny*nz undone."""
        _, ny, nz = (int(v) for v in self.grid.get_cell_count())
        if _is_torch(self.cells):
            L = self.cells
            out = L.new_empty((L.numel(), 3))
        else:
            L = np.asarray(self.cells).astype(np.int64)
            out = np.empty((L.size, 3), np.int64)
        out[:, 0], out[:, 1], out[:, 2] = L // (ny * nz), (L // nz) % ny, L % nz
        return out

    def to_dense(self, fill=float("nan")):
        """float32[nx, ny, nz] with `fill` outside the band: for small grids (it is the array the band exists to avoid)."""
        shape = tuple(int(v) for v in self.grid.get_cell_count())
        if _is_torch(self.cells):
            out = self.distances.new_full((shape[0] * shape[1] * shape[2],), fill)
            out[self.cells] = self.distances
        else:
            out = np.full(shape[0] * shape[1] * shape[2], fill, np.float32)
            out[np.asarray(self.cells).astype(np.int64)] = self.distances
        return out.reshape(shape)

    def isosurface(self, iso: float = 0.0, *, timings: M2STimings = None):
        """band_isosurface on this band's own cells, distances and grid: (vertices, indices, n_open), and no dense array on the way."""
        return band_isosurface(self.grid, self.cells, self.distances, iso=iso, timings=timings)

    def field(self, background=None, inside=None) -> "BandField":
        """A BandField of this band's own cells, distances and grid: sample and ray-march it with no dense array on the way.  inside: a
        sign mask in the layout of `bits` (or the Voxels of voxelize(solid=True, bits=True) on the same grid); Mesh.narrow_band_field
        makes one itself."""
        return BandField(self.grid, self.cells, self.distances, background=background, inside=inside)


def _band_widths(band):
    """band: one width for both sides, or (interior, exterior)."""
    interior, exterior = (band, band) if np.isscalar(band) else band
    return float(interior), float(exterior)


def _band_call(call, a, grid, band, sign_method, bits, algorithm, timings, capacity, synchronous=True):
    """One narrow-band call, `call(grid, sign, bopts, p_cells, p_dist, capacity, p_bits, p_count, opts)`; the arrays are made on the side of
    `a`.  Without `capacity` the call runs twice: a counting call (no cells, no distances), then the fill with the count as capacity."""
    nx, ny, nz = (int(v) for v in grid.get_cell_count())
    interior, exterior = _band_widths(band)
    bo = _lib.M2SBandOpts(C.sizeof(_lib.M2SBandOpts), exterior, interior)
    synchronous = synchronous or not a.device

    def buf(shape, np_dtype, torch_dtype):
        x = a.torch.empty(shape, dtype=getattr(a.torch, torch_dtype), device=a.dev) if a.device else np.empty(shape, np_dtype)
        filled = x.numel() if a.device else x.size
        return x, ((x.data_ptr() if a.device else x.ctypes.data) if filled else None)

    count = C.c_uint64(0)
    if capacity is None:
        o = a.opts(None, algorithm)
        rc = call(C.byref(grid._g), int(sign_method), C.byref(bo), None, None, 0, None, C.byref(count), C.byref(o))
        if rc != _lib.M2S_OK:
            _raise(rc)
        capacity = int(count.value)
    cell_arr, p_cells = buf(int(capacity), np.uint64, "int64")
    dist_arr, p_dist = buf(int(capacity), np.float32, "float32")
    bit_arr, p_bits = buf((nx, ny, (nz + 31) // 32), np.uint32, "int32") if bits else (None, None)
    if bits and a.device and hasattr(a.torch, "uint32"):
        bit_arr = bit_arr.view(a.torch.uint32)
    o = a.opts(timings, algorithm, synchronous=synchronous)
    rc = call(C.byref(grid._g), int(sign_method), C.byref(bo), p_cells, p_dist, int(capacity), p_bits, C.byref(count), C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    n = int(count.value)
    return NarrowBand(cell_arr[:n], dist_arr[:n], bit_arr, n, grid)


def narrow_band_sdf(vertices, indices: Topology, grid: "Grid", band, sign_method: SignMethod = SignMethod.Raycast, *, bits: bool = False,
                    algorithm: int = 0, timings: M2STimings = None, capacity: Optional[int] = None) -> NarrowBand:
    """The cells of `grid` whose generate_grid_sdf value D lies in the band -interior <= D <= exterior, and those values bit for bit
    (include/m2s.h m2s_narrow_band_sdf): what a level-set or sparse-brick pipeline reads of a grid, at the cost of the cells near the surface
    instead of all of them.  `band` is one width in world units or (interior, exterior); either may be inf.  `algorithm=1` runs the dense
    call and filters it (the definition; the same bits).  Host arrays or device tensors, as the other calls take them.  Without `capacity`
    the call runs twice (count, then fill); with one (an upper bound of the active cells) it runs once and raises when it is short."""
    a = _Args(vertices, indices)
    L = _lib.lib()
    return _band_call(lambda *r: L.m2s_narrow_band_sdf(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, *r), a, grid, band,
                      sign_method, bits, algorithm, timings, capacity)


# DeepSDF's near-surface noise (Park et al. 2019: variances 0.0025 and 0.00025 in a unit sphere), as fractions of half the bounding-box diagonal
NEAR_SURFACE_SIGMAS = (0.05, 0.0158)


def _near_surface_points(a, surf, lo, hi, n, sigmas, uniform_fraction, seed):
    """The query points of sample_sdf_near_surface on the side of `a`: `surf` displaced by equal shares of Gaussian noise of every sigma,
    then uniform points in the 1.1x bounding box [lo, hi]."""
    n_uniform = n - surf.shape[0]
    if a.device:
        t = a.torch
        gen = t.Generator(device=a.dev)
        gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
        noise = t.randn(surf.shape, generator=gen, device=a.dev, dtype=t.float32)
        share = t.as_tensor(np.asarray(sigmas, np.float32), device=a.dev)[t.arange(surf.shape[0], device=a.dev) % len(sigmas)]
        near = surf + noise * share[:, None]
        box_lo, box_hi = t.as_tensor(lo, device=a.dev), t.as_tensor(hi, device=a.dev)
        uni = box_lo + t.rand((n_uniform, 3), generator=gen, device=a.dev, dtype=t.float32) * (box_hi - box_lo)
        return t.cat([near, uni]).contiguous()
    rng = np.random.default_rng(int(seed) & 0xFFFFFFFFFFFFFFFF)
    noise = rng.standard_normal(surf.shape, dtype=np.float32)
    share = np.asarray(sigmas, np.float32)[np.arange(surf.shape[0]) % len(sigmas)]
    near = (surf + noise * share[:, None]).astype(np.float32)
    uni = (lo + rng.random((n_uniform, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([near, uni]))


def _sample_sdf_near_surface(mesh, n, sigmas, uniform_fraction, sign, seed):
    a = mesh._a
    n = int(n)
    if not 0.0 <= uniform_fraction <= 1.0:
        raise M2SPanic(_lib.ERR_BAD_ARG, "uniform_fraction must lie in [0, 1]")
    if sign not in ("winding", "raycast", "normal"):
        raise M2SPanic(_lib.ERR_BAD_ARG, "sign must be 'winding', 'raycast' or 'normal'")
    v = a.keep[0]
    if a.device:
        lo, hi = v.min(0).values.cpu().numpy(), v.max(0).values.cpu().numpy()
    else:
        lo, hi = v.min(0), v.max(0)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    half_diagonal = 0.5 * float(np.linalg.norm(hi - lo))
    if sigmas is None:
        sigmas = [s * half_diagonal for s in NEAR_SURFACE_SIGMAS]
    sigmas = [float(s) for s in sigmas]
    n_uniform = int(round(n * uniform_fraction)) if sigmas else n
    centre, half = 0.5 * (lo + hi), 0.55 * (hi - lo)
    surf = mesh.sample_surface(n - n_uniform, seed=seed).points
    pts = _near_surface_points(a, surf, (centre - half).astype(np.float32), (centre + half).astype(np.float32), n, sigmas, uniform_fraction, seed)
    if sign == "winding":
        sdf = mesh.generate_sdf_winding(pts)
    elif sign == "raycast":
        sdf = mesh.generate_sdf(pts, AccelerationMethod.RtreeBvh)
    else:
        sdf = mesh.generate_sdf(pts, AccelerationMethod.Bvh(SignMethod.Normal))
    return pts, sdf


def sample_sdf_near_surface(vertices, indices: Topology, n: int, sigmas=None, uniform_fraction: float = 0.05, sign: str = "winding",
                            seed: int = 0):
    """Training samples for a neural SDF, as DeepSDF and the `mesh_to_sdf` package draw them: (points f32[n, 3], sdf f32[n]).  All but
    `uniform_fraction` of the points are surface samples (sample_surface under `seed`) displaced by isotropic Gaussian noise — equal shares
    for every entry of `sigmas`, row i taking sigmas[i % len(sigmas)]; default: 0.05 and 0.0158 of half the bounding-box diagonal — and the
    rest, the last rows, lie uniformly in the bounding box scaled by 1.1.  The noise comes from torch.randn under a seeded generator on the
    data's device (numpy for host arrays) and is not part of any bit contract; `sdf` is: it is bit-equal to the named distance call on the
    returned points — "winding": Mesh.generate_sdf_winding, "raycast": Mesh.generate_sdf with RtreeBvh, "normal": Mesh.generate_sdf with
    Bvh(Normal).  One persistent mesh serves the whole call."""
    with Mesh(vertices, indices) as mesh:
        return _sample_sdf_near_surface(mesh, n, sigmas, uniform_fraction, sign, seed)


class SampleMode(enum.IntEnum):
    """How a grid is read between cell centres (include/m2s.h m2s_sample_mode = the client shader's MODE_*)."""
    Snap = 0
    Trilinear = 1
    Tetrahedral = 2


class _GridQuery:
    """The grid's distances and the per-point arrays of one grid query, on the side of `distances`: a CUDA tensor keeps everything on
    its device (torch's current stream), anything else goes through host memory."""

    def __init__(self, distances, timings=None, synchronous=True):
        self.keep = []
        self.device = _is_torch(distances) and distances.is_cuda
        if self.device:
            import torch

            self.torch = torch
            self.dev = distances.device
            d = distances.detach().to(torch.float32).contiguous().reshape(-1)
        else:
            d = np.ascontiguousarray(np.asarray(distances, np.float32)).reshape(-1)
        self.n_cells = d.numel() if self.device else d.size
        self.p_d = self.ptr(d)
        o = M2SOpts()
        o.struct_size = C.sizeof(M2SOpts)
        o.synchronous = 1 if synchronous else 0
        if timings is not None:
            o.timings = C.pointer(timings)
        if self.device:
            o.device = self.dev.index if self.dev.index is not None else self.torch.cuda.current_device()
            o.stream = self.torch.cuda.current_stream(self.dev).cuda_stream
            o.stream_mode = 1
            o.mem_kind = _lib.MEM_DEVICE
        else:
            o.device = -1
            o.mem_kind = _lib.MEM_HOST
        self.opts = o

    def ptr(self, x):
        self.keep.append(x)
        n = x.numel() if self.device else x.size
        return (x.data_ptr() if self.device else x.ctypes.data) if n else None

    def points(self, x):
        """(n, 3) float32 on this call's side -> (pointer, n)."""
        if self.device:
            t = x if _is_torch(x) else self.torch.as_tensor(np.asarray(x, np.float32))
            t = t.detach().to(device=self.dev, dtype=self.torch.float32).contiguous().reshape(-1, 3)
            return self.ptr(t), t.shape[0]
        if _is_torch(x):
            x = x.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(x, np.float32)).reshape(-1, 3)
        return self.ptr(a), a.shape[0]

    def empty(self, shape, dtype=np.float32):
        if self.device:
            kind = {np.uint32: self.torch.int32, np.uint8: self.torch.uint8, np.uint64: self.torch.int64}.get(dtype, self.torch.float32)
            t = self.torch.empty(shape, dtype=kind, device=self.dev)
            return t, self.ptr(t)
        a = np.empty(shape, dtype)
        return a, self.ptr(a)

    def check_cells(self, grid):
        if self.n_cells != grid.get_total_cell_count():
            raise M2SPanic(_lib.ERR_BAD_ARG, f"distances hold {self.n_cells} values, the grid has {grid.get_total_cell_count()} cells")


def _sample_opts(mode, iso, outside, max_steps):
    so = _lib.M2SSampleOpts()
    so.struct_size = C.sizeof(_lib.M2SSampleOpts)
    so.mode, so.iso, so.outside, so.max_steps = int(mode), float(np.float32(iso)), float(np.float32(outside)), int(max_steps)
    return so


def sample_grid(grid: Grid, distances, points, *, mode: SampleMode = SampleMode.Trilinear, iso: float = 0.0, outside: float = 100.0,
                normals: bool = False, timings: M2STimings = None):
    """Samples a grid SDF at arbitrary points as the reference client's shader does (sdf_grid / estimate_normal of
    draw_raymarching.wgsl; include/m2s.h m2s_sample_grid): `outside` beyond the grid box, else the snapped, trilinear or tetrahedral
    value minus `iso`.  distances: the grid's cells in grid order (generate_grid_sdf's output).  Returns values f32[n], or
    (values, normals f32[n, 3]) with normals=True.  A CUDA tensor `distances` keeps the call on its device."""
    q = _GridQuery(distances, timings)
    q.check_cells(grid)
    p_pts, n = q.points(points)
    values, p_v = q.empty(n)
    nrm, p_n = q.empty((n, 3)) if normals else (None, None)
    so = _sample_opts(mode, iso, outside, 100)
    rc = _lib.lib().m2s_sample_grid(C.byref(grid._g), q.p_d, p_pts, n, C.byref(so), p_v, p_n, C.byref(q.opts))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return (values, nrm) if normals else values


def raymarch_grid(grid: Grid, distances, origins, directions, *, mode: SampleMode = SampleMode.Trilinear, iso: float = 0.0,
                  outside: float = 100.0, max_steps: int = 100, normals: bool = False, timings: M2STimings = None):
    """Sphere-traces rays through a grid SDF as the reference client's shader does (sdf_3d of draw_raymarching.wgsl; include/m2s.h
    m2s_raymarch_grid).  Directions are used as given (not normalised).  Returns (positions f32[n, 3], dist f32[n], steps u32[n],
    hit bool[n][, normals f32[n, 3]]): a hit is a ray that entered the grid box and ended closer than 0.01 * the largest cell size."""
    q = _GridQuery(distances, timings)
    q.check_cells(grid)
    p_o, n = q.points(origins)
    p_d, n_d = q.points(directions)
    if n != n_d:
        raise M2SPanic(_lib.ERR_BAD_ARG, f"{n} origins but {n_d} directions")
    out, p_out = q.empty((n, 4))
    steps, p_s = q.empty(n, np.uint32)
    nrm, p_n = q.empty((n, 3)) if normals else (None, None)
    so = _sample_opts(mode, iso, outside, max_steps)
    rc = _lib.lib().m2s_raymarch_grid(C.byref(grid._g), q.p_d, p_o, p_d, n, C.byref(so), p_out, p_s, p_n, C.byref(q.opts))
    if rc != _lib.M2S_OK:
        _raise(rc)
    eps = np.float32(0.01) * np.float32(max(grid.get_cell_size()))
    pos, dist = out[:, :3], out[:, 3]
    # the miss output (0, 0, 0, 1) with no step is not a hit even where 1 < eps (cells larger than 100)
    miss = (steps == 0) & (dist == 1.0) & (pos == 0).all(1)
    hit = (dist < float(eps)) & ~miss
    if q.device and hasattr(q.torch, "uint32"):
        steps = steps.view(q.torch.uint32)
    res = (pos, dist, steps, hit)
    return res + (nrm,) if normals else res


def grid_isosurface(grid: Grid, distances, *, iso: float = 0.0, timings: M2STimings = None):
    """Extracts the level set d = iso of a grid SDF as a welded, indexed triangle mesh (marching cubes over the cell centres;
    include/m2s.h m2s_grid_isosurface states the exact contract).  Triangles wind outwards (towards increasing d).  Returns
    (vertices f32[n, 3], indices u32[m, 3]).  A CUDA tensor `distances` keeps the call on its device and returns tensors."""
    q = _GridQuery(distances, timings)
    q.check_cells(grid)
    L = _lib.lib()
    counts = (C.c_uint64 * 2)()
    it = float(np.float32(iso))
    rc = L.m2s_grid_isosurface(C.byref(grid._g), q.p_d, it, None, 0, None, 0, counts, C.byref(q.opts))
    if rc != _lib.M2S_OK:
        _raise(rc)
    nv, nt = int(counts[0]), int(counts[1])
    verts, p_v = q.empty((max(nv, 1), 3))          # never NULL: NULL for both outputs means "count only"
    idx, p_i = q.empty((max(nt, 1), 3), np.uint32)
    rc = L.m2s_grid_isosurface(C.byref(grid._g), q.p_d, it, p_v, nv, p_i, nt, counts, C.byref(q.opts))
    if rc != _lib.M2S_OK:
        _raise(rc)
    verts, idx = verts[:nv], idx[:nt]
    if q.device and hasattr(q.torch, "uint32"):
        idx = idx.view(q.torch.uint32)
    return verts, idx


def _band_cells(q: "_GridQuery", cells):
    """A band's `cells` on the side of `q` (made from its distances) -> (pointer, n): int64 on the device, uint64 on the host."""
    if q.device:
        t = q.torch
        c = cells
        if not _is_torch(c):
            h = np.ascontiguousarray(np.asarray(c).reshape(-1))
            c = t.as_tensor(h.view(np.int64) if h.dtype == np.uint64 else h.astype(np.int64))
        c = c.detach().reshape(-1)
        if c.dtype != t.int64:
            c = c.view(t.int64) if c.dtype == getattr(t, "uint64", None) else c.to(t.int64)
        c = c.to(device=q.dev).contiguous()
        n = c.numel()
    else:
        c = cells.detach().cpu().numpy() if _is_torch(cells) else np.asarray(cells)
        c = np.ascontiguousarray(c.reshape(-1))
        c = c.view(np.uint64) if c.dtype in (np.uint64, np.int64) else c.astype(np.uint64)   # a negative int64 is out of range either way
        n = c.size
    if n != q.n_cells:
        raise M2SPanic(_lib.ERR_BAD_ARG, f"{n} cells but {q.n_cells} distances")
    return q.ptr(c), n


def band_isosurface(grid: Grid, cells, distances, *, iso: float = 0.0, timings: M2STimings = None):
    """Extracts the level set d = iso from a narrow band (include/m2s.h m2s_band_isosurface): `cells` are strictly ascending grid-order
    indices L (uint64 or int64), `distances` their values.  The result is grid_isosurface of any dense grid that agrees with the band,
    kept where the band decides it alone: the vertices whose edge has both ends in the band and the triangles whose cell has all 8 corners
    in it, bit for bit and in the same order.  The work is proportional to the band; no array of distances sized by the grid exists.
    Returns (vertices f32[n, 3], indices u32[m, 3], n_open).  n_open is the number of active points P that own a cell
    (i < nx-1, j < ny-1, k < nz-1) with two properties: the cell's 8 corners are not all active; among its active corners at least one
    is inside and at least one is outside.  A non-zero value proves the band was too narrow for this iso.  Zero does not prove the
    opposite, because cells whose lowest corner is inactive are not visited.  CUDA tensors keep the call on their device and return
    tensors; the call runs twice, count then fill."""
    q = _GridQuery(distances, timings)
    p_c, n = _band_cells(q, cells)
    L = _lib.lib()
    counts = (C.c_uint64 * 3)()
    it = float(np.float32(iso))
    rc = L.m2s_band_isosurface(C.byref(grid._g), p_c, q.p_d, n, it, None, 0, None, 0, counts, C.byref(q.opts))
    if rc != _lib.M2S_OK:
        _raise(rc)
    nv, nt = int(counts[0]), int(counts[1])
    verts, p_v = q.empty((max(nv, 1), 3))          # never NULL: NULL for both outputs means "count only"
    idx, p_i = q.empty((max(nt, 1), 3), np.uint32)
    rc = L.m2s_band_isosurface(C.byref(grid._g), p_c, q.p_d, n, it, p_v, nv, p_i, nt, counts, C.byref(q.opts))
    if rc != _lib.M2S_OK:
        _raise(rc)
    verts, idx = verts[:nv], idx[:nt]
    if q.device and hasattr(q.torch, "uint32"):
        idx = idx.view(q.torch.uint32)
    return verts, idx, int(counts[2])


def _f32_up(x: float) -> float:
    """The smallest float32 that is not below x."""
    y = np.float32(x)
    if float(y) < x:
        y = np.nextafter(y, np.float32(np.inf))
    return float(y)


def isosurface_band(grid: Grid, iso: float = 0.0):
    """The (interior, exterior) widths narrow_band_sdf needs so that band_isosurface at `iso` equals grid_isosurface of the dense grid:
    the band contains [iso - w, iso + w] with w = 1.001 x the cell diagonal sqrt(sx^2 + sy^2 + sz^2), computed in float64 and rounded up
    to float32; interior = max(0, w - iso) and exterior = max(0, iso + w), each rounded up to float32.  For an exact distance field every
    cell the level set cuts then has all 8 corners in the band."""
    sx, sy, sz = (float(v) for v in grid.get_cell_size())
    w = _f32_up(1.001 * float(np.sqrt(sx * sx + sy * sy + sz * sz)))
    iso = float(np.float32(iso))
    return _f32_up(max(0.0, w - iso)), _f32_up(max(0.0, iso + w))


def _remesh(band: "NarrowBand", iso, keep_largest: int = 0):
    if keep_largest > 0:
        with band.field() as whole, whole.keep_largest(keep_largest) as kept:
            verts, idx, n_open = kept.isosurface(iso)
    else:
        verts, idx, n_open = band.isosurface(iso)
    if n_open != 0:
        raise M2SError(_lib.ERR_BAD_ARG, f"remesh: the band is too narrow for iso = {iso}: {n_open} cells are cut but incomplete")
    return verts, idx


def remesh(vertices, indices: Topology, grid: Grid, *, iso: float = 0.0, sign_method: SignMethod = SignMethod.Raycast, keep_largest: int = 0):
    """Mesh -> level set -> mesh without a dense grid: narrow_band_sdf with the band of isosurface_band(grid, iso), then its isosurface at
    `iso`.  The sparse voxel remesh (iso = 0) / offset surface (iso != 0) of the mesh on `grid`; where the distance field is exact the
    result is grid_isosurface(grid, generate_grid_sdf(...), iso) bit for bit.  Returns (vertices, indices); raises M2SError if the band
    turns out too narrow (n_open != 0).  keep_largest = k > 0 erases all but the band's k largest connected components first
    (BandField.keep_largest): loose parts and debris do not reach the mesh."""
    return _remesh(narrow_band_sdf(vertices, indices, grid, isosurface_band(grid, iso), sign_method), iso, int(keep_largest))


def _boolean(mesh_a: "Mesh", mesh_b: "Mesh", op, grid: Grid, sign_method, keep_largest: int = 0):
    op = _csg_op(op)
    w = isosurface_band(grid, 0.0)                    # (interior, exterior): the same width w on both sides at iso = 0
    with mesh_a.narrow_band_field(grid, w, sign_method, True, background=w) as fa, \
            mesh_b.narrow_band_field(grid, w, sign_method, True, background=w) as fb, fa.csg(fb, op) as fr:
        if keep_largest > 0:
            with fr.keep_largest(keep_largest) as kept:
                verts, idx, n_open = kept.isosurface(0.0)
        else:
            verts, idx, n_open = fr.isosurface(0.0)
    if n_open != 0:
        raise M2SError(_lib.ERR_BAD_ARG, f"boolean: the bands are too narrow: {n_open} cells are cut but incomplete")
    return verts, idx


def boolean(vertices_a, indices_a: Topology, vertices_b, indices_b: Topology, op, grid: Grid, *, sign_method: SignMethod = SignMethod.Raycast,
            keep_largest: int = 0):
    """A mesh boolean through level sets, without a dense grid: both meshes to narrow band fields on `grid` (the widths of
    isosurface_band(grid, 0), both backgrounds that width, the Raycast sign beyond the band), BandField.csg with `op` (a CsgOp or its
    name: union, intersection, difference = a minus b), then the isosurface at 0.  Where the distance fields are exact the result is
    grid_isosurface of min / max of the two dense grids clamped to the band width, bit for bit.  Returns (vertices, indices); raises
    M2SError if a band turns out too narrow (n_open != 0).  The surface is that of the grid's resolution: features below a cell are lost.
    keep_largest = k > 0 erases all but the result's k largest connected components before meshing (BandField.keep_largest): the
    slivers and floating debris a boolean leaves where two surfaces nearly coincide."""
    with Mesh(vertices_a, indices_a) as ma, Mesh(vertices_b, indices_b) as mb:
        return _boolean(ma, mb, op, grid, sign_method, int(keep_largest))


def default_background(distances):
    """(inside, outside) backgrounds of a band field made from `distances` alone: outside = max(distances.max(), 0) and
    inside = max(-distances.min(), 0), the largest values known to be lower bounds of |D| beyond the band (a band holds every cell with
    -interior <= D <= exterior, so a cell it lacks is farther than its largest value on that side).  (0, 0) for an empty band."""
    n = distances.numel() if _is_torch(distances) else np.asarray(distances).size
    if n == 0:
        return 0.0, 0.0
    hi, lo = float(distances.max()), float(distances.min())
    return max(-lo, 0.0), max(hi, 0.0)


def _inside_bits(inside):
    """The sign mask of a band field: a Voxels or NarrowBand (its bits) or the bits array itself."""
    if isinstance(inside, (Voxels, NarrowBand)):
        if inside.bits is None:
            raise M2SPanic(_lib.ERR_BAD_ARG, "inside: the voxelization / band was made without bits=True")
        return inside.bits
    if inside is True:
        raise M2SPanic(_lib.ERR_BAD_ARG, "inside=True needs the mesh: use Mesh.narrow_band_field")
    return inside


class CsgOp(enum.IntEnum):
    """include/m2s.h `m2s_csg_op`: how BandField.csg combines two bands."""
    Union = 0
    Intersection = 1
    Difference = 2


def _csg_op(op) -> CsgOp:
    """A CsgOp, its number or its name in any case."""
    try:
        return CsgOp[op.capitalize()] if isinstance(op, str) else CsgOp(int(op))
    except (KeyError, ValueError, TypeError):
        raise M2SPanic(_lib.ERR_BAD_ARG, f"op = {op!r} is not a CsgOp (union, intersection, difference)") from None


def _backgrounds(background):
    """background: a scalar for both sides, or (inside, outside) -> (inside, outside)."""
    if np.isscalar(background):
        return float(background), float(background)
    bg_in, bg_out = (float(v) for v in background)
    return bg_in, bg_out


class RedistanceInfo(NamedTuple):
    """include/m2s.h `m2s_band_redistance_info`: the sweeps that changed a value, whether the last one run changed none, the frozen
    cells next to the zero set, the sign changes towards an inactive cell (> 0: the band does not bracket its own zero set there), the
    candidate cells the sweeps ran over."""
    sweeps: int
    converged: bool
    n_frozen: int
    n_open: int
    n_candidates: int


class FilterKind(enum.IntEnum):
    """include/m2s.h `m2s_filter_kind`: what BandField.filter runs.  Mean is the separable 3 x 3 x 3 box (four iterations approximate a
    Gaussian), Laplacian one explicit step of the heat equation, MeanCurvature one explicit step of the mean-curvature flow."""
    Mean = 0
    Laplacian = 1
    MeanCurvature = 2


_FILTER_NAMES = {"mean": FilterKind.Mean, "laplacian": FilterKind.Laplacian, "meancurvature": FilterKind.MeanCurvature}


def _filter_kind(kind) -> FilterKind:
    """A FilterKind, its number or its name in any case (mean, laplacian, mean_curvature)."""
    try:
        return _FILTER_NAMES[kind.replace("_", "").replace(" ", "").lower()] if isinstance(kind, str) else FilterKind(int(kind))
    except (KeyError, ValueError, TypeError):
        raise M2SPanic(_lib.ERR_BAD_ARG, f"kind = {kind!r} is not a FilterKind (mean, laplacian, mean_curvature)") from None


class FilterInfo(NamedTuple):
    """include/m2s.h `m2s_band_filter_info`: the passes run, the largest |result - input| over the cells, the cells whose bits changed,
    the cells whose sign changed, and the candidates that were not finite and were therefore dropped (per cell and pass)."""
    passes: int
    max_change: float
    n_changed: int
    n_sign_flips: int
    n_nonfinite: int


class AdvectKind(enum.IntEnum):
    """include/m2s.h `m2s_advect_kind`: what BandField.advect steps.  Velocity carries the field along a velocity per cell
    (phi_t + u . grad phi = 0), Normal moves the surface along its normal by a speed per cell (phi_t + F |grad phi| = 0)."""
    Velocity = 0
    Normal = 1


class AdvectInfo(NamedTuple):
    """include/m2s.h `m2s_band_advect_info`: the steps run, the largest |result - input| over the cells, the largest CFL number of a
    cell (stable up to 1; reported, not enforced), the cells with a field entry other than zero, the cells whose bits changed, the
    cells whose sign changed, and the candidates that were not finite and were therefore dropped (per cell and step)."""
    steps: int
    max_change: float
    max_cfl: float
    n_moving: int
    n_changed: int
    n_sign_flips: int
    n_nonfinite: int


class FlowInfo(NamedTuple):
    """What BandField.flow ran: the rounds (each an advect followed by a redistance), the steps over all rounds, and the time reached."""
    rounds: int
    steps: int
    time: float


def flow_round(field, kind, cell_size, left: float, cfl: float = 0.5, reach: float = 1.0):
    """The schedule of one round of BandField.flow -> (steps, dt, time taken).  field: the round's float32[n, 3] velocities or
    float32[n] speeds (a device tensor or a host array); left: the time that remains.  In float64, from the binary32 entries:
    rate = the largest |u_i| r_i + |u_j| r_j + |u_k| r_k (or |F| (r_i + r_j + r_k)) with r_a = 1 / h_a in binary32, fastest = the
    largest |u| (or |F|).  The round lasts reach * min(h) / fastest, or `left` where that is no more than it (to a millionth), in steps = ceil(that * rate / cfl) steps (65 536 at the
    most, a shorter round then) of dt = the round's time / steps rounded to binary32, one float down where the rounding would lift
    dt * rate above cfl.  (0, 0.0, left) when nothing moves; raises on a non-finite field."""
    h = np.asarray(cell_size, np.float32)
    r = (np.float32(1) / h).astype(np.float64)
    velocity = int(kind) == int(AdvectKind.Velocity)
    if _is_torch(field):
        import torch as t

        a = field.detach().to(t.float64).abs()
        if a.numel() == 0:
            return 0, 0.0, float(left)
        if velocity:
            a = a.reshape(-1, 3)
            rate = float(((a[:, 0] * float(r[0]) + a[:, 1] * float(r[1])) + a[:, 2] * float(r[2])).max())
            fastest = math.sqrt(float(((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).max()))
        else:
            fastest = float(a.max())
            rate = fastest * float((r[0] + r[1]) + r[2])
    else:
        a = np.abs(np.asarray(field, np.float32).astype(np.float64))
        if a.size == 0:
            return 0, 0.0, float(left)
        if velocity:
            a = a.reshape(-1, 3)
            rate = float(((a[:, 0] * r[0] + a[:, 1] * r[1]) + a[:, 2] * r[2]).max())
            fastest = math.sqrt(float(((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).max()))
        else:
            fastest = float(a.max())
            rate = fastest * float((r[0] + r[1]) + r[2])
    if not (np.isfinite(rate) and np.isfinite(fastest)):
        raise M2SPanic(_lib.ERR_BAD_ARG, "flow: the velocity or speed is not finite")
    if rate == 0.0:
        return 0, 0.0, float(left)
    took = float(reach) * float(h.min()) / fastest
    if left <= took * (1 + 1e-6):                                    # no round for a remainder of rounding's size
        took = float(left)
    steps = max(1, int(np.ceil(took * rate / float(cfl))))
    if steps > 65536:
        steps = 65536
        took = steps * float(cfl) / rate
    dt = np.float32(took / steps)
    if float(dt) * rate > float(cfl):
        dt = np.nextafter(dt, np.float32(0))
    return steps, float(dt), took


class ResampleInfo(NamedTuple):
    """include/m2s.h `m2s_band_resample_info`: the result's cells, the points on the source box that had some but not all of their
    reads in the band (the rim the interpolation loses), the points whose value came out non-finite and were dropped, and the sign
    changes towards an inactive cell (> 0: the result does not bracket its own zero set there; the target cells outgrew the band)."""
    n_cells: int
    n_partial: int
    n_nonfinite: int
    n_open: int


class Connectivity(enum.IntEnum):
    """include/m2s.h `m2s_connectivity`: which cells of a band count as joined.  Faces (6), faces and edges (18), faces, edges and
    corners (26)."""
    Faces = 6
    Edges = 18
    Corners = 26


def _connectivity(c) -> Connectivity:
    try:
        return Connectivity(int(c))
    except (ValueError, TypeError):
        raise M2SPanic(_lib.ERR_BAD_ARG, f"connectivity = {c!r} is not 6, 18 or 26") from None


class SelectInfo(NamedTuple):
    """include/m2s.h `m2s_band_select_info`: the result's cells, the cells erased, and the inactive points whose inside bit was
    cleared because the erased cells bracketed them."""
    n_cells: int
    n_dropped: int
    n_sign_cleared: int


class Components:
    """The connected components of a BandField's cells (include/m2s.h m2s_band_components), numbered 0 .. count - 1 in ascending order of
    their smallest cell index, the raster numbering of scipy.ndimage.label.  labels: one uint32 per cell in list order (the order of
    `to_band().cells`), a device tensor for a field made from device tensors, a host array otherwise.  Per component, as host arrays:
    first_cell (its smallest L), n_cells, n_negative (cells with a value < 0: a volume proxy), box_lo / box_hi (the inclusive
    (i, j, k) bounding box, uint32[count, 3])."""

    def __init__(self, labels, connectivity, first_cell, n_cells, n_negative, box_lo, box_hi):
        self.labels, self.connectivity = labels, connectivity
        self.first_cell, self.n_cells, self.n_negative, self.box_lo, self.box_hi = first_cell, n_cells, n_negative, box_lo, box_hi
        self.count = int(n_cells.size)

    def largest(self, k: int = 1):
        """The numbers of the k components with the most cells, largest first; a tie goes to the lower number."""
        order = np.argsort(-self.n_cells.astype(np.int64), kind="stable")
        return order[:max(int(k), 0)].astype(np.int64)

    def at_least(self, min_cells: int):
        """The numbers of the components with min_cells cells or more, ascending."""
        return np.flatnonzero(self.n_cells >= int(min_cells)).astype(np.int64)

    def measure(self, field: "BandField", iso: float = 0.0):
        """`field.measure(iso, self)`: one Measure per component of the level set d = iso of `field`, whose labelling this is."""
        return field.measure(iso, self)


class Measure(NamedTuple):
    """include/m2s.h `m2s_band_measure_record`: the level set d = iso of a BandField, or of one group of its cells, measured as
    `isosurface` would mesh it.  n_triangles, n_vertices, n_open (cells cut inside the band but incomplete) and n_border (vertices on a
    boundary face of the grid) are counts; area_q, volume_q and moment_q are the raw integer sums the header defines to the bit; area,
    volume and centroid are world units.  closed: n_open == 0 and n_border == 0; only then are volume and centroid a volume and a
    centre of mass.  euler: n_vertices - n_triangles / 2, the Euler characteristic of a closed surface."""
    n_triangles: int
    n_vertices: int
    n_open: int
    n_border: int
    area_q: int
    volume_q: int
    moment_q: tuple
    area: float
    volume: float
    centroid: tuple
    closed: bool
    euler: int


class ShapesInfo(NamedTuple):
    """include/m2s.h `m2s_band_shapes_info`: the result's cells, the grid points inside the union (the set bits of its sign mask), the
    shapes left out because a coordinate was not finite or the radius negative or not finite, and the sound shapes that reach no
    grid point within the exterior width."""
    n_cells: int
    n_inside: int
    n_skipped: int
    n_off_grid: int


def _similarity(transform):
    """A 3 x 4 or 4 x 4 map p = A q + t from source space to target space -> (to_source float32[12], value_scale float32): checked in
    float64 to be a similarity (A^T A = s^2 I to a relative 1e-5; reflections pass), inverted as [A^T / s^2, -A^T t / s^2]."""
    M = np.asarray(transform.detach().cpu().numpy() if _is_torch(transform) else transform, np.float64)
    if M.shape == (4, 4):
        if not np.array_equal(M[3], (0.0, 0.0, 0.0, 1.0)):
            raise ValueError("resample: the last row of a 4 x 4 transform must be (0, 0, 0, 1)")
        M = M[:3]
    if M.shape != (3, 4) or not np.isfinite(M).all():
        raise ValueError("resample: the transform must be a finite 3 x 4 or 4 x 4 array")
    A, t = M[:, :3], M[:, 3]
    G = A.T @ A
    s2 = np.trace(G) / 3.0
    if not s2 > 0 or np.abs(G - s2 * np.eye(3)).max() > 1e-5 * s2:
        raise ValueError("resample: the transform is not a similarity (rotation, uniform scale, reflection, translation)")
    inv = A.T / s2
    return np.concatenate([inv, (-inv @ t)[:, None]], 1).astype(np.float32).reshape(12), np.float32(np.sqrt(s2))


class BandField:
    """A narrow band made queryable (include/m2s.h `m2s_band`): the index of the band's cells, its distances and an optional sign mask,
    resident on the device, built once and sampled or ray-marched many times with no dense grid anywhere.  It stands for the dense grid D'
    that holds distances[n] at cells[n], -background_inside on the other cells whose `inside` bit is set and +background_outside on the
    rest; `sample` and `raymarch` equal sample_grid / raymarch_grid on D' bit for bit.

    cells: strictly ascending grid-order indices L (uint64 or int64); distances: their float32 values; host arrays or device tensors
    (a CUDA tensor `distances` builds the handle on its device).  inside: uint32[nx, ny, ceil(nz / 32)] in the layout of Voxels.bits
    (or a Voxels / NarrowBand carrying one); None: every cell beyond the band is outside.  background: a scalar or (inside, outside);
    None means default_background(distances).  A zero background stalls a march: a ray that enters the region it fills stops there
    (dist < eps), so give a band that has cells on one side only an explicit background for the other.
    Two fields on the same grid combine on the device into a third (`csg`, `union`, `intersection`, `difference`, or `a | b`, `a & b`,
    `a - b`); `redistance` turns a combined field back into distances at any width and `offset` grows or shrinks the solid;
    `filter` and `smooth` fair it (mean, Laplacian, mean-curvature flow), everywhere or inside a region;
    `resample` takes it to another grid, moved, turned or scaled on the way, so that fields born on different grids can be combined;
    `to_band` hands a field's lists back as a NarrowBand and `isosurface` meshes it.  `background` is (inside, outside) and
    `count` the number of cells, for a combined field as the library reports them.
    A context manager; `close` frees the device memory."""

    def __init__(self, grid: Grid, cells, distances, *, background=None, inside=None, timings: M2STimings = None):
        self._h = C.c_void_p()
        q = _GridQuery(distances, timings)
        self._dev = q.dev if q.device else None     # the side the lists came from: where to_band puts them again
        p_c, n = _band_cells(q, cells)
        if background is None:
            bg_in, bg_out = default_background(distances)
        else:
            bg_in, bg_out = _backgrounds(background)
        p_bits = None
        bits = _inside_bits(inside)
        if bits is not None:
            nx, ny, nz = (int(v) for v in grid.get_cell_count())
            words = nx * ny * ((nz + 31) // 32)
            if q.device:
                t = q.torch
                b = bits if _is_torch(bits) else t.as_tensor(np.ascontiguousarray(np.asarray(bits)).astype(np.uint32).view(np.int32))
                b = b.detach()
                if b.dtype != t.int32:
                    b = b.view(t.int32) if b.dtype == getattr(t, "uint32", None) else b.to(t.int32)
                b = b.to(device=q.dev).contiguous().reshape(-1)
                have = b.numel()
            else:
                b = bits.detach().cpu().numpy() if _is_torch(bits) else np.asarray(bits)
                b = np.ascontiguousarray(b.reshape(-1))
                b = b.view(np.uint32) if b.dtype in (np.uint32, np.int32) else b.astype(np.uint32)
                have = b.size
            if have != words:
                raise M2SPanic(_lib.ERR_BAD_ARG, f"inside holds {have} words, the grid needs {words}")
            p_bits = q.ptr(b)
        fo = _lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in)))
        rc = _lib.lib().m2s_band_create(C.byref(grid._g), p_c, q.p_d, n, p_bits, C.byref(fo), C.byref(q.opts), C.byref(self._h))
        if rc != _lib.M2S_OK:
            self._h = C.c_void_p()
            _raise(rc)
        self.grid = grid
        self.count = n
        self.background = (float(np.float32(bg_in)), float(np.float32(bg_out)))
        nbytes = C.c_uint64(0)
        rc = _lib.lib().m2s_band_info(self._h, None, None, C.byref(nbytes))
        if rc != _lib.M2S_OK:
            _raise(rc)
        self.device_bytes = int(nbytes.value)

    def _handle(self):
        if not getattr(self, "_h", None) or not self._h.value:
            raise M2SError(_lib.ERR_BAD_ARG, "the BandField is closed")
        return self._h

    def sample(self, points, *, mode: SampleMode = SampleMode.Trilinear, iso: float = 0.0, outside: float = 100.0, normals: bool = False,
               support: bool = False, timings: M2STimings = None, synchronous: bool = True):
        """sample_grid on the grid the band stands for: values f32[n], then normals f32[n, 3] with normals=True, then support u8[n] with
        support=True (how many of the sample's 1 / 8 / 4 cell reads hit a band cell; the full number means band values only).  CUDA tensor
        points keep the call on their device (the handle's), anything else goes through host memory."""
        h = self._handle()
        q = _GridQuery(points if _is_torch(points) and points.is_cuda else np.zeros(0, np.float32), timings, synchronous)
        p_pts, n = q.points(points)
        values, p_v = q.empty(n)
        nrm, p_n = q.empty((n, 3)) if normals else (None, None)
        sup, p_s = q.empty(n, np.uint8) if support else (None, None)
        so = _sample_opts(mode, iso, outside, 100)
        if n:                                                                # no points: the empty arrays, and no NULL outputs to explain
            rc = _lib.lib().m2s_band_sample(h, p_pts, n, C.byref(so), p_v, p_n, p_s, C.byref(q.opts))
            if rc != _lib.M2S_OK:
                _raise(rc)
        res = (values,) + ((nrm,) if normals else ()) + ((sup,) if support else ())
        return res if len(res) > 1 else values

    def raymarch(self, origins, directions, *, mode: SampleMode = SampleMode.Trilinear, iso: float = 0.0, outside: float = 100.0,
                 max_steps: int = 100, normals: bool = False, support: bool = False, timings: M2STimings = None, synchronous: bool = True):
        """raymarch_grid on the grid the band stands for: (positions f32[n, 3], dist f32[n], steps u32[n], hit bool[n][, normals f32[n, 3]]
        [, support u8[n]]); support is that of the last sample the march evaluated."""
        h = self._handle()
        q = _GridQuery(origins if _is_torch(origins) and origins.is_cuda else np.zeros(0, np.float32), timings, synchronous)
        p_o, n = q.points(origins)
        p_d, n_d = q.points(directions)
        if n != n_d:
            raise M2SPanic(_lib.ERR_BAD_ARG, f"{n} origins but {n_d} directions")
        out, p_out = q.empty((n, 4))
        steps, p_s = q.empty(n, np.uint32)
        nrm, p_n = q.empty((n, 3)) if normals else (None, None)
        sup, p_u = q.empty(n, np.uint8) if support else (None, None)
        so = _sample_opts(mode, iso, outside, max_steps)
        if n:
            rc = _lib.lib().m2s_band_raymarch(h, p_o, p_d, n, C.byref(so), p_out, p_s, p_n, p_u, C.byref(q.opts))
            if rc != _lib.M2S_OK:
                _raise(rc)
        eps = np.float32(0.01) * np.float32(max(self.grid.get_cell_size()))
        pos, dist = out[:, :3], out[:, 3]
        miss = (steps == 0) & (dist == 1.0) & (pos == 0).all(1)   # as raymarch_grid
        hit = (dist < float(eps)) & ~miss
        if q.device and hasattr(q.torch, "uint32"):
            steps = steps.view(q.torch.uint32)
        return (pos, dist, steps, hit) + ((nrm,) if normals else ()) + ((sup,) if support else ())

    @classmethod
    def _adopt(cls, h, grid: Grid, dev):
        """A BandField around a handle the library made (a CSG result): count, background and device_bytes as it reports them."""
        self = cls.__new__(cls)
        self._h, self.grid, self._dev = h, grid, dev
        L = _lib.lib()
        n, nbytes, fo = C.c_uint64(0), C.c_uint64(0), _lib.M2SBandFieldOpts()
        for rc in (L.m2s_band_info(h, None, C.byref(n), C.byref(nbytes)), L.m2s_band_field_info(h, C.byref(fo), None)):
            if rc != _lib.M2S_OK:
                _raise(rc)
        self.count, self.device_bytes = int(n.value), int(nbytes.value)
        self.background = (float(fo.background_inside), float(fo.background_outside))
        return self

    @classmethod
    def from_capsules(cls, grid: Grid, a, b, radius, band, *, background=None, timings: M2STimings = None) -> "BandField":
        """The union of the capsules a[n]-b[n] with the radii `radius` as a resident BandField, with no mesh on the way (include/m2s.h
        m2s_band_from_capsules states the result per grid point, to the bit): the value is the smallest distance to a capsule's
        surface, active where it lies within the half-widths `band` (a scalar or (interior, exterior)), with a sign mask on every
        point.  a, b: float32[n, 3], numpy arrays or device tensors (a CUDA tensor `a` keeps the call on its device); b None: spheres.
        radius: a scalar or an array of n.  background: a scalar or (inside, outside); None is the two widths.  Shapes with a
        non-finite coordinate or radius, or a negative radius, are left out and counted.  Inside the union the values are a lower
        bound of the depth: follow with `redistance` before reading them as distances.  The result carries `.shapes_info` (a
        ShapesInfo)."""
        interior, exterior = _band_widths(band)
        q = _GridQuery(a if _is_torch(a) and a.is_cuda else np.zeros(0, np.float32), timings)
        p_a, n = q.points(a)
        p_b = None
        if b is not None:
            p_b, n_b = q.points(b)
            if n_b != n:
                raise M2SPanic(_lib.ERR_BAD_ARG, f"{n} first ends but {n_b} second ends")
        so = _lib.M2SBandShapesOpts(C.sizeof(_lib.M2SBandShapesOpts), float(np.float32(exterior)), float(np.float32(interior)), 0.0)
        p_r = None
        if np.isscalar(radius):
            so.radius = float(np.float32(radius))
        else:
            if q.device:
                r = radius if _is_torch(radius) else q.torch.as_tensor(np.asarray(radius, np.float32))
                r = r.detach().to(device=q.dev, dtype=q.torch.float32).contiguous().reshape(-1)
                n_r = r.numel()
            else:
                r = radius.detach().cpu().numpy() if _is_torch(radius) else radius
                r = np.ascontiguousarray(np.asarray(r, np.float32)).reshape(-1)
                n_r = r.size
            if n_r != n:
                raise M2SPanic(_lib.ERR_BAD_ARG, f"{n} shapes but {n_r} radii")
            p_r = q.ptr(r)
        fo = None
        if background is not None:
            bg_in, bg_out = _backgrounds(background)
            fo = C.byref(_lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in))))
        info = _lib.M2SBandShapesInfo()
        h = C.c_void_p()
        rc = _lib.lib().m2s_band_from_capsules(C.byref(grid._g), p_a, p_b, p_r, n, C.byref(so), fo, C.byref(q.opts), C.byref(h), C.byref(info), None)
        if rc != _lib.M2S_OK:
            _raise(rc)
        out = cls._adopt(h, grid, q.dev if q.device else None)
        out.shapes_info = ShapesInfo(int(info.n_cells), int(info.n_inside), int(info.n_skipped), int(info.n_off_grid))
        return out

    @classmethod
    def from_spheres(cls, grid: Grid, centers, radius, band, *, background=None, timings: M2STimings = None) -> "BandField":
        """The union of the balls around centers[n] with the radii `radius` (a scalar or an array): `from_capsules` with b = a.  A
        particle set becomes a surface with `from_spheres(...).smooth(...).isosurface()`."""
        return cls.from_capsules(grid, centers, None, radius, band, background=background, timings=timings)

    @classmethod
    def from_points(cls, grid: Grid, points, radius: float, band, *, background=None, timings: M2STimings = None) -> "BandField":
        """`from_spheres` with one radius for every point: a point cloud dilated by `radius`."""
        return cls.from_spheres(grid, points, float(radius), band, background=background, timings=timings)

    @classmethod
    def from_edges(cls, grid: Grid, vertices, edges, radius, band, *, background=None, timings: M2STimings = None) -> "BandField":
        """The union of the capsules along the edges[m] = (i, j) of the graph on vertices[n]: a strut lattice, a dilated wireframe.
        radius: a scalar, or one per edge.  The two ends are gathered on the side of `vertices` and go to `from_capsules`."""
        if _is_torch(vertices) and vertices.is_cuda:
            import torch

            v = vertices.detach().to(torch.float32).reshape(-1, 3)
            e = edges if _is_torch(edges) else torch.as_tensor(np.asarray(edges).astype(np.int64))
            e = e.detach().to(device=v.device, dtype=torch.int64).reshape(-1, 2)
            if e.numel() and (int(e.min()) < 0 or int(e.max()) >= v.shape[0]):
                raise M2SPanic(_lib.ERR_BAD_ARG, f"edges name a vertex outside [0, {v.shape[0]})")
            a, b = v[e[:, 0]].contiguous(), v[e[:, 1]].contiguous()
        else:
            v = vertices.detach().cpu().numpy() if _is_torch(vertices) else vertices
            v = np.asarray(v, np.float32).reshape(-1, 3)
            e = edges.detach().cpu().numpy() if _is_torch(edges) else edges
            e = np.asarray(e).astype(np.int64).reshape(-1, 2)
            if e.size and (int(e.min()) < 0 or int(e.max()) >= v.shape[0]):
                raise M2SPanic(_lib.ERR_BAD_ARG, f"edges name a vertex outside [0, {v.shape[0]})")
            a, b = v[e[:, 0]], v[e[:, 1]]
        return cls.from_capsules(grid, a, b, radius, band, background=background, timings=timings)

    def _side(self, timings=None) -> "_GridQuery":
        """The options and buffers of a call with no input array, on the side this field's lists came from."""
        if self._dev is None:
            return _GridQuery(np.zeros(0, np.float32), timings)
        import torch

        return _GridQuery(torch.empty(0, dtype=torch.float32, device=self._dev), timings)

    def csg(self, other: "BandField", op, background=None, *, timings: M2STimings = None) -> "BandField":
        """The union, intersection or difference (self minus other) of two fields on the same grid as a new resident BandField
        (include/m2s.h m2s_band_csg states the result per grid point, to the bit): min / max of the two grids the bands stand for, active
        where an active operand supplies the value, with a sign mask on every point.  No dense grid exists on the way and nothing
        leaves the device.  background: a scalar or (inside, outside); None takes the smaller of the operands' on each side, which keeps
        sphere tracing safe.  The zero set is the combined solid's; away from it the values are a lower bound of its distance, not
        the exact distance (the usual level-set CSG)."""
        op = _csg_op(op)
        if not isinstance(other, BandField):
            raise M2SPanic(_lib.ERR_BAD_ARG, "csg: the other operand is not a BandField")
        q = self._side(timings)
        fo = None
        if background is not None:
            bg_in, bg_out = _backgrounds(background)
            fo = C.byref(_lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in))))
        h = C.c_void_p()
        rc = _lib.lib().m2s_band_csg(self._handle(), other._handle(), int(op), fo, C.byref(q.opts), C.byref(h))
        if rc != _lib.M2S_OK:
            _raise(rc)
        return BandField._adopt(h, self.grid, self._dev)

    def union(self, other: "BandField", background=None) -> "BandField":
        return self.csg(other, CsgOp.Union, background)

    def intersection(self, other: "BandField", background=None) -> "BandField":
        return self.csg(other, CsgOp.Intersection, background)

    def difference(self, other: "BandField", background=None) -> "BandField":
        return self.csg(other, CsgOp.Difference, background)

    def __or__(self, other):
        return self.csg(other, CsgOp.Union) if isinstance(other, BandField) else NotImplemented

    def __and__(self, other):
        return self.csg(other, CsgOp.Intersection) if isinstance(other, BandField) else NotImplemented

    def __sub__(self, other):
        return self.csg(other, CsgOp.Difference) if isinstance(other, BandField) else NotImplemented

    def redistance(self, band, background=None, max_sweeps: int = 0, *, timings: M2STimings = None) -> "BandField":
        """A new resident BandField with the same zero set, values that are distances again and the half-widths `band` (a scalar or
        (interior, exterior)), narrower or wider than this one (include/m2s.h m2s_band_redistance states the result per grid point, to
        the bit).  The cells next to the zero set keep their values in every bit; from them Jacobi sweeps of the first-order update
        run over the cells within reach, and what they do not reach within the widths is dropped.  Use it after `csg`, whose values
        are only a lower bound of the distance, and before anything that reads the band as a distance: isosurface(iso != 0), a march,
        a second csg after an offset.  background: a scalar or (inside, outside); None is the two widths.  max_sweeps 0 is the
        library's cap.  The result carries `.redistance_info` (a RedistanceInfo)."""
        interior, exterior = _band_widths(band)
        q = self._side(timings)
        ro = _lib.M2SBandRedistanceOpts(C.sizeof(_lib.M2SBandRedistanceOpts), float(np.float32(exterior)), float(np.float32(interior)), int(max_sweeps))
        fo = None
        if background is not None:
            bg_in, bg_out = _backgrounds(background)
            fo = C.byref(_lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in))))
        info = _lib.M2SBandRedistanceInfo(C.sizeof(_lib.M2SBandRedistanceInfo))
        h = C.c_void_p()
        rc = _lib.lib().m2s_band_redistance(self._handle(), C.byref(ro), fo, C.byref(q.opts), C.byref(h), C.byref(info))
        if rc != _lib.M2S_OK:
            _raise(rc)
        out = BandField._adopt(h, self.grid, self._dev)
        out.redistance_info = RedistanceInfo(int(info.sweeps), bool(info.converged), int(info.n_frozen), int(info.n_open), int(info.n_candidates))
        return out

    def filter(self, kind, iterations: int = 1, *, where: "BandField" = None, background=None, timings: M2STimings = None) -> "BandField":
        """A new resident BandField on the same cells whose values have been smoothed by `iterations` iterations of `kind` (a
        FilterKind, its number or its name; include/m2s.h m2s_band_filter states the result per grid point, to the bit).  where: a
        BandField on the same grid whose inside is the region to smooth; the cells outside it keep every bit, which is how a
        union's seam becomes a fillet while the rest of the surface stays put.  background: a scalar or (inside, outside); None
        keeps this field's.  The result is not a distance field: follow it with `redistance`, or call `smooth`.  It carries
        `.filter_info` (a FilterInfo)."""
        kind = _filter_kind(kind)
        if where is not None and not isinstance(where, BandField):
            raise M2SPanic(_lib.ERR_BAD_ARG, "filter: where is not a BandField")
        q = self._side(timings)
        fl = _lib.M2SBandFilterOpts(C.sizeof(_lib.M2SBandFilterOpts), int(kind), int(iterations), 1)
        fo = None
        if background is not None:
            bg_in, bg_out = _backgrounds(background)
            fo = C.byref(_lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in))))
        info = _lib.M2SBandFilterInfo(C.sizeof(_lib.M2SBandFilterInfo))
        h = C.c_void_p()
        rc = _lib.lib().m2s_band_filter(self._handle(), where._handle() if where is not None else None, C.byref(fl), fo, C.byref(q.opts),
                                        C.byref(h), C.byref(info))
        if rc != _lib.M2S_OK:
            _raise(rc)
        out = BandField._adopt(h, self.grid, self._dev)
        out.filter_info = FilterInfo(int(info.passes), float(info.max_change), int(info.n_changed), int(info.n_sign_flips), int(info.n_nonfinite))
        return out

    def centers(self):
        """The centres of the field's cells, float32[n, 3] in list order, as m2s_grid_cell_center gives them (first_cell +
        (float)idx * cell_size per axis): where a velocity or a speed for `advect` is evaluated.  A device tensor for a field made from
        device tensors, a host array otherwise, like `to_band`."""
        cells = self.to_band().cells
        first, size = self.grid.get_first_cell(), self.grid.get_cell_size()
        _, ny, nz = self.grid.get_cell_count()
        if _is_torch(cells):
            import torch as t

            L = cells.to(t.int64)
            idx = (L // (ny * nz), (L // nz) % ny, L % nz)
            return t.stack([idx[a].to(t.float32) * float(size[a]) + float(first[a]) for a in range(3)], 1)
        L = np.asarray(cells).astype(np.int64)
        idx = (L // (ny * nz), (L // nz) % ny, L % nz)
        return np.stack([first[a] + idx[a].astype(np.float32) * size[a] for a in range(3)], 1).astype(np.float32)

    def _cell_field(self, q, value, width, what):
        """`value` (an array with one entry per cell, or a scalar / a vector of `width` broadcast to the cells) as the float32 array
        [n, width] or [n] a call on q's side reads."""
        shape = (self.count, width) if width > 1 else (self.count,)
        if q.device:
            t = q.torch
            f = value if _is_torch(value) else t.as_tensor(np.asarray(value, np.float32))
            f = f.detach().to(device=q.dev, dtype=t.float32)
            if f.numel() == (width if width > 1 else 1):
                f = f.reshape(-1).expand(shape) if width > 1 else f.reshape(()).expand(shape)
            have = f.numel()
            f = f.contiguous()
        else:
            f = np.asarray(value.detach().cpu().numpy() if _is_torch(value) else value, np.float32)
            if f.size == (width if width > 1 else 1):
                f = np.broadcast_to(f.reshape(-1) if width > 1 else f.reshape(()), shape)
            have = f.size
            f = np.ascontiguousarray(f)
        if have != self.count * width:
            raise M2SPanic(_lib.ERR_BAD_ARG, f"{what} holds {have} values, the field's {self.count} cells need {self.count * width}")
        return f.reshape(shape)

    def advect(self, dt: float, steps: int = 1, *, velocity=None, speed=None, background=None, timings: M2STimings = None) -> "BandField":
        """A new resident BandField on the same cells whose values have taken `steps` first-order upwind steps of `dt` (include/m2s.h
        m2s_band_advect states the result per grid point, to the bit).  Exactly one of velocity (phi_t + u . grad phi = 0: the field
        is carried along u) and speed (phi_t + F |grad phi| = 0: the surface moves outward along its normal by F) is given: an array
        with one entry per cell in list order (float32[n, 3] / float32[n], as `centers` orders them; a device tensor or a host
        array), or a 3-vector / a scalar for every cell.  A cell whose entry is zero keeps every bit.  background: a scalar or
        (inside, outside); None keeps this field's.  The result is not a distance field and the band does not follow the surface:
        move it by less than the half-width minus two cells, then `redistance`, or call `flow`.  It carries `.advect_info` (an
        AdvectInfo), whose max_cfl should stay at or below 1."""
        if (velocity is None) == (speed is None):
            raise M2SPanic(_lib.ERR_BAD_ARG, "advect: give exactly one of velocity and speed")
        kind = AdvectKind.Velocity if speed is None else AdvectKind.Normal
        q = self._side(timings)
        h = self._handle()
        f = self._cell_field(q, velocity if speed is None else speed, 3 if speed is None else 1, "velocity" if speed is None else "speed")
        ao = _lib.M2SBandAdvectOpts(C.sizeof(_lib.M2SBandAdvectOpts), int(kind), int(steps), 0, float(np.float32(dt)))
        fo = None
        if background is not None:
            bg_in, bg_out = _backgrounds(background)
            fo = C.byref(_lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in))))
        info = _lib.M2SBandAdvectInfo(C.sizeof(_lib.M2SBandAdvectInfo))
        out = C.c_void_p()
        rc = _lib.lib().m2s_band_advect(h, q.ptr(f), C.byref(ao), fo, C.byref(q.opts), C.byref(out), C.byref(info))
        if rc != _lib.M2S_OK:
            _raise(rc)
        res = BandField._adopt(out, self.grid, self._dev)
        res.advect_info = AdvectInfo(int(info.steps), float(info.max_change), float(info.max_cfl), int(info.n_moving), int(info.n_changed),
                                     int(info.n_sign_flips), int(info.n_nonfinite))
        return res

    def flow(self, time: float, band, *, velocity=None, speed=None, cfl: float = 0.5, reach: float = 1.0) -> "BandField":
        """The field moved over `time` by a velocity or a normal speed, as a new BandField of half-widths `band` that is a distance
        field again: the tracker around `advect`.  velocity / speed: as for `advect`, or a callable f(centers) that is evaluated on
        the cells' centres at the start of every round.  A round takes the largest steps with max_cfl <= cfl until the fastest cell
        has moved `reach` of the smallest cell edge or `time` is used up (`flow_round` is the schedule), then `redistance(band)`
        re-grows the band around the moved zero set.  Raises if a round's zero set leaves what the band brackets (n_open > 0):
        lower `reach` or widen `band`.  The result carries `.flow_info` (a FlowInfo), and the last round's `.advect_info` and
        `.redistance_info`."""
        if (velocity is None) == (speed is None):
            raise M2SPanic(_lib.ERR_BAD_ARG, "flow: give exactly one of velocity and speed")
        given, kind = (velocity, AdvectKind.Velocity) if speed is None else (speed, AdvectKind.Normal)
        if not (np.isfinite(time) and time >= 0 and cfl > 0 and reach > 0):
            raise M2SPanic(_lib.ERR_BAD_ARG, f"flow: time = {time}, cfl = {cfl}, reach = {reach}")
        width = 3 if kind == AdvectKind.Velocity else 1
        cur, left, rounds, steps, reached, last = self, float(time), 0, 0, 0.0, None
        try:
            while left > 0 and cur.count:
                f = cur._cell_field(cur._side(), given(cur.centers()) if callable(given) else given, width, "the field")
                n_steps, dt, took = flow_round(f, kind, self.grid.get_cell_size(), left, cfl, reach)
                if n_steps == 0:                                     # nothing moves any more
                    break
                with cur.advect(dt, n_steps, **{"velocity" if kind == AdvectKind.Velocity else "speed": f}) as moved:
                    nxt = moved.redistance(band)
                    nxt.advect_info = last = moved.advect_info
                if cur is not self:
                    cur.close()
                cur = nxt
                if cur.redistance_info.n_open:
                    raise M2SError(_lib.ERR_BAD_ARG, f"flow: round {rounds + 1} leaves the band at {cur.redistance_info.n_open} cell faces; "
                                                     "lower reach or widen the band")
                rounds, steps, reached = rounds + 1, steps + n_steps, reached + float(dt) * n_steps
                left = 0.0 if took >= left else left - took
            out = cur.redistance(band) if cur is self else cur
        except Exception:
            if cur is not self:
                cur.close()
            raise
        if last is not None:
            out.advect_info = last
        out.flow_info = FlowInfo(rounds, steps, reached)
        return out

    def morph(self, target: "BandField", time: float, band, **flow) -> "BandField":
        """This field morphed towards `target` over `time`: `flow` with the speed -target.sample(centers, mode=Trilinear), which moves
        the surface outward where it lies inside the target and inward where it lies outside, and rests on the target's zero set
        (OpenVDB's LevelSetMorph).  flow: `cfl`, `reach`."""
        if not isinstance(target, BandField):
            raise M2SPanic(_lib.ERR_BAD_ARG, "morph: target is not a BandField")
        return self.flow(time, band, speed=lambda centers: -target.sample(centers, mode=SampleMode.Trilinear), **flow)

    def resample(self, grid, transform=None, *, mode: SampleMode = SampleMode.Trilinear, background=None,
                 timings: M2STimings = None) -> "BandField":
        """This field evaluated at the cell centres of another grid, as a new resident BandField on that grid (include/m2s.h
        m2s_band_resample states the result per target grid point, to the bit): crop, pad, move, turn, scale, refine.  grid: a Grid, or
        another BandField whose grid is used (OpenVDB's resampleToMatch).  transform: a 3 x 4 or 4 x 4 array that maps source space to
        target space and places the solid; it must be a similarity (rotation, uniform scale s, reflection, translation), so that
        distances stay distances: the values are multiplied by s.  None is the identity.  mode: SampleMode.Snap keeps every bit where
        the grids agree by whole cells (crop and pad); Trilinear and Tetrahedral interpolate and lose the band's outermost cells.
        background: a scalar or (inside, outside); None is this field's times s.  After an interpolating mode the result is not a
        distance field: follow it with `redistance`.  It carries `.resample_info` (a ResampleInfo)."""
        if isinstance(grid, BandField):
            grid = grid.grid
        if not isinstance(grid, Grid):
            raise M2SPanic(_lib.ERR_BAD_ARG, "resample: grid is neither a Grid nor a BandField")
        ro = _lib.M2SBandResampleOpts()
        ro.struct_size, ro.mode, ro.value_scale = C.sizeof(_lib.M2SBandResampleOpts), int(mode), 1.0
        ro.to_source[0] = ro.to_source[5] = ro.to_source[10] = 1.0
        if transform is not None:
            to_source, scale = _similarity(transform)
            ro.to_source[:] = [float(v) for v in to_source]
            ro.value_scale = float(scale)
        q = self._side(timings)
        fo = None
        if background is not None:
            bg_in, bg_out = _backgrounds(background)
            fo = C.byref(_lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in))))
        info = _lib.M2SBandResampleInfo(C.sizeof(_lib.M2SBandResampleInfo))
        h = C.c_void_p()
        rc = _lib.lib().m2s_band_resample(self._handle(), C.byref(grid._g), C.byref(ro), fo, C.byref(q.opts), C.byref(h), C.byref(info))
        if rc != _lib.M2S_OK:
            _raise(rc)
        out = BandField._adopt(h, grid, self._dev)
        out.resample_info = ResampleInfo(int(info.n_cells), int(info.n_partial), int(info.n_nonfinite), int(info.n_open))
        return out

    def components(self, connectivity=6, *, timings: M2STimings = None) -> "Components":
        """The connected components of the field's cells (include/m2s.h m2s_band_components; connectivity 6, 18 or 26 or a
        Connectivity): a Components with the labels in list order and each component's first cell, cell count, negative-cell count
        and bounding box.  One labelling; a second call only when there are more components than the first had room for."""
        conn = _connectivity(connectivity)
        h = self._handle()
        q = self._side(timings)
        n = self.count
        co = _lib.M2SBandComponentsOpts(C.sizeof(_lib.M2SBandComponentsOpts), int(conn))
        labels, p_l = q.empty(n, np.uint32)
        count = C.c_uint64(0)
        cap = 256
        while True:
            stats, p_s = q.empty((cap, 6), np.uint64)
            rc = _lib.lib().m2s_band_components(h, C.byref(co), C.byref(q.opts), p_l, p_s, cap, C.byref(count))
            if rc == _lib.M2S_OK:
                break
            if rc != _lib.ERR_BAD_ARG or count.value <= cap:
                _raise(rc)
            cap = int(count.value)
        c = int(count.value)
        stats = (stats.cpu().numpy() if q.device else stats)[:c].view(np.uint64).reshape(c, 6)
        box = np.ascontiguousarray(stats[:, 3:]).view(np.uint32).reshape(c, 6)
        if q.device and hasattr(q.torch, "uint32"):
            labels = labels.view(q.torch.uint32)
        return Components(labels, conn, stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy(), box[:, :3].copy(), box[:, 3:].copy())

    def _labels_arg(self, q, labels, what):
        """One label per cell, a device tensor or a host array, as the 32-bit array a call on q's side reads (one entry at least)."""
        if q.device:
            t = q.torch
            lab = labels if _is_torch(labels) else t.as_tensor(np.ascontiguousarray(np.asarray(labels)).astype(np.uint32).view(np.int32))
            lab = lab.detach()
            if lab.dtype != t.int32:
                lab = lab.view(t.int32) if lab.dtype == getattr(t, "uint32", None) else lab.to(t.int32)
            lab = lab.to(device=q.dev).contiguous().reshape(-1)
            have = lab.numel()
            if have == 0:
                lab = t.zeros(1, dtype=t.int32, device=q.dev)
        else:
            lab = labels.detach().cpu().numpy() if _is_torch(labels) else np.asarray(labels)
            lab = np.ascontiguousarray(lab.reshape(-1))
            lab = lab.view(np.uint32) if lab.dtype in (np.uint32, np.int32) else lab.astype(np.uint32)
            have = lab.size
            if have == 0:
                lab = np.zeros(1, np.uint32)
        if have != self.count:
            raise M2SPanic(_lib.ERR_BAD_ARG, f"{what}: {have} labels, the field has {self.count} cells")
        return lab

    def measure(self, iso: float = 0.0, components=None, *, n_groups: int = None, timings: M2STimings = None):
        """The level set d = iso of this field measured as `isosurface` would mesh it, without building the mesh (include/m2s.h
        m2s_band_measure): a Measure with the triangle and vertex counts, area, enclosed volume and centroid.  components: a Components
        of this field (a list of Measures, one per component), or a labels array with one entry per cell and n_groups (cells whose
        label is n_groups or more, LABEL_NONE among them, are left out).  Label with connectivity 26 to measure per mesh component.
        The last call's `m2s_band_measure_info` is kept as `.measure_info` = (area_exponent, n_groups, n_skipped)."""
        h = self._handle()
        q = self._side(timings)
        mo = _lib.M2SBandMeasureOpts(C.sizeof(_lib.M2SBandMeasureOpts), float(np.float32(iso)))
        p_l, groups = None, 1
        if components is not None:
            if isinstance(components, Components):
                labels, groups = components.labels, components.count
            else:
                if n_groups is None:
                    raise M2SPanic(_lib.ERR_BAD_ARG, "measure: labels need n_groups")
                labels, groups = components, int(n_groups)
            if groups == 0 and self.count == 0:
                return []
            lab = self._labels_arg(q, labels, "measure")
            p_l = q.ptr(lab)
        out = (_lib.M2SBandMeasureRecord * max(groups, 1))()
        info = _lib.M2SBandMeasureInfo(C.sizeof(_lib.M2SBandMeasureInfo))
        rc = _lib.lib().m2s_band_measure(h, C.byref(mo), p_l, groups, C.byref(q.opts), out, C.byref(info), None)
        if rc != _lib.M2S_OK:
            _raise(rc)
        self.measure_info = (int(info.area_exponent), int(info.n_groups), int(info.n_skipped))
        res = [Measure(int(m.n_triangles), int(m.n_vertices), int(m.n_open), int(m.n_border), int(m.area_q), int(m.volume_q), tuple(int(v) for v in m.moment_q),
                       float(m.area), float(m.volume), tuple(float(v) for v in m.centroid), m.n_open == 0 and m.n_border == 0,
                       int(m.n_vertices) - int(m.n_triangles) // 2) for m in out[:groups]]
        return res[0] if components is None else res

    def area(self, iso: float = 0.0) -> float:
        """The area of the level set d = iso (`measure(iso).area`)."""
        return self.measure(iso).area

    def volume(self, iso: float = 0.0) -> float:
        """The volume the level set d = iso encloses (`measure(iso).volume`; a volume only where the surface is closed)."""
        return self.measure(iso).volume

    def centroid(self, iso: float = 0.0):
        """The centre of mass of the solid the level set d = iso bounds (`measure(iso).centroid`; only where the surface is closed)."""
        return self.measure(iso).centroid

    def select(self, components, keep, background=None, *, timings: M2STimings = None) -> "BandField":
        """This field with some components erased, as a new resident BandField (include/m2s.h m2s_band_select).  components: a
        Components of this field, or a labels array with one entry per cell.  keep: the numbers of the components to keep, or a
        boolean mask over them.  The kept cells keep every bit; an erased cell becomes inactive and outside, and so does the solid
        interior that only erased cells bracketed along k, so that `sample` and `raymarch` no longer see an erased island.  Erase
        islands, not voids: erasing the band around a cavity leaves the solid around it without a band cell on that side.
        background: a scalar or (inside, outside); None keeps this field's.  The result carries `.select_info` (a SelectInfo)."""
        h = self._handle()
        q = self._side(timings)
        labels = components.labels if isinstance(components, Components) else components
        keep = np.asarray(keep.detach().cpu().numpy() if _is_torch(keep) else keep)
        if keep.dtype == bool:
            mask = keep.reshape(-1).astype(np.uint8)
        else:
            ids = keep.reshape(-1).astype(np.int64)
            size = components.count if isinstance(components, Components) else (int(ids.max()) + 1 if ids.size else 0)
            if ids.size and (ids.min() < 0 or ids.max() >= size):
                raise M2SPanic(_lib.ERR_BAD_ARG, f"select: component numbers must be 0 .. {size - 1}")
            mask = np.zeros(size, np.uint8)
            mask[ids] = 1
        lab = self._labels_arg(q, labels, "select")
        kp = q.torch.as_tensor(mask, device=q.dev) if q.device else mask
        fo = None
        if background is not None:
            bg_in, bg_out = _backgrounds(background)
            fo = C.byref(_lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), float(np.float32(bg_out)), float(np.float32(bg_in))))
        info = _lib.M2SBandSelectInfo(C.sizeof(_lib.M2SBandSelectInfo))
        out = C.c_void_p()
        rc = _lib.lib().m2s_band_select(h, q.ptr(lab), q.ptr(kp), int(mask.size), fo, C.byref(q.opts), C.byref(out), C.byref(info))
        if rc != _lib.M2S_OK:
            _raise(rc)
        res = BandField._adopt(out, self.grid, self._dev)
        res.select_info = SelectInfo(int(info.n_cells), int(info.n_dropped), int(info.n_sign_cleared))
        return res

    def keep_largest(self, k: int = 1, connectivity=6) -> "BandField":
        """The field with all but its k largest components (by cell count; a tie goes to the lower number) erased."""
        comps = self.components(connectivity)
        return self.select(comps, comps.largest(k))

    def remove_islands(self, min_cells: int, connectivity=6) -> "BandField":
        """The field with every component of fewer than min_cells cells erased."""
        comps = self.components(connectivity)
        return self.select(comps, comps.at_least(min_cells))

    def split(self, connectivity=6):
        """One field per component, in the components' order, each with that component alone kept."""
        comps = self.components(connectivity)
        return [self.select(comps, [c]) for c in range(comps.count)]

    def smooth(self, kind, iterations: int, band, *, where: "BandField" = None) -> "BandField":
        """`filter(kind, iterations, where=where)` followed by `redistance(band)`: a smoothed field that is a distance field again.
        The result carries both `.filter_info` and `.redistance_info`."""
        with self.filter(kind, iterations, where=where) as filtered:
            out = filtered.redistance(band)
            out.filter_info = filtered.filter_info
        return out

    def offset(self, distance: float, band, max_sweeps: int = 0) -> "BandField":
        """The solid grown (distance > 0) or shrunk (distance < 0) by `distance`, as a new BandField of half-widths `band`: the lists
        out, `distance` subtracted from the values, the sign mask rebuilt from the shifted values on the band's cells and kept
        elsewhere, a field of them with this one's backgrounds, then `redistance`.  Raises if the shifted zero set leaves what the
        band brackets (n_open > 0): redistance to a band wider than |distance| first."""
        nb = self.to_band()
        d = np.float32(distance)
        nx, ny, nz = (int(v) for v in self.grid.get_cell_count())
        nzw = (nz + 31) // 32
        if _is_torch(nb.cells):
            import torch as t

            moved = nb.distances - float(d)
            L = nb.cells
            word = (L // nz) * nzw + (L % nz) // 32
            bit = t.ones_like(L) << ((L % nz) % 32)
            bits = nb.bits.view(t.int32).reshape(-1).to(t.int64) & 0xffffffff
            clear = t.zeros_like(bits).scatter_add_(0, word, bit)                      # the cells of a word are distinct bits: a sum is an OR
            setb = t.zeros_like(bits).scatter_add_(0, word, t.where(moved < 0, bit, t.zeros_like(bit)))
            bits = (bits & ~clear) | setb
            bits = t.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(t.int32).reshape(nx, ny, nzw)
        else:
            moved = (np.asarray(nb.distances, np.float32) - d).astype(np.float32)
            L = np.asarray(nb.cells).astype(np.int64)
            word = (L // nz) * nzw + (L % nz) // 32
            bit = np.uint32(1) << ((L % nz) % 32).astype(np.uint32)
            bits = np.array(nb.bits, np.uint32).reshape(-1)
            np.bitwise_and.at(bits, word, ~bit)
            np.bitwise_or.at(bits, word[moved < 0], bit[moved < 0])
            bits = bits.reshape(nx, ny, nzw)
        with BandField(self.grid, nb.cells, moved, background=self.background, inside=bits) as shifted:
            out = shifted.redistance(band, max_sweeps=max_sweeps)
        if out.redistance_info.n_open:
            n_open = out.redistance_info.n_open
            out.close()
            raise M2SError(_lib.ERR_BAD_ARG, f"offset: the zero set moved by {float(d)} leaves the band at {n_open} cell faces; redistance to a wider band first")
        return out

    def to_band(self, *, timings: M2STimings = None) -> NarrowBand:
        """The field's lists back out (include/m2s.h m2s_band_export, the inverse of creating it): a NarrowBand of its cells (ascending),
        their distances bit for bit and, as `bits`, its sign mask in the layout of Voxels.bits (all zero for a field made without
        one).  Device tensors for a field made from device tensors, host arrays otherwise."""
        h = self._handle()
        q = self._side(timings)
        nx, ny, nz = (int(v) for v in self.grid.get_cell_count())
        n = self.count
        cells, p_c = q.empty(n, np.uint64)
        dist, p_d = q.empty(n)
        bits, p_b = q.empty((nx, ny, (nz + 31) // 32), np.uint32)
        rc = _lib.lib().m2s_band_export(h, p_c, p_d, n, p_b, C.byref(q.opts))
        if rc != _lib.M2S_OK:
            _raise(rc)
        if q.device and hasattr(q.torch, "uint32"):
            bits = bits.view(q.torch.uint32)
        return NarrowBand(cells, dist, bits, n, self.grid)

    def isosurface(self, iso: float = 0.0, *, timings: M2STimings = None):
        """band_isosurface of the field's own cells and distances: (vertices, indices, n_open)."""
        return self.to_band().isosurface(iso, timings=timings)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().m2s_band_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class PeerMode(enum.IntEnum):
    """include/m2s.h `m2s_peer_mode`: how a slab reaches the peers' whole-grid buffers."""
    Push = 0    # one wide copy kernel per slab piece, overlapped with the next piece's walk
    Store = 1   # the walk's epilogue stores every value to every peer
    Trail = 2   # one walk; a copy kernel beside it pushes each unit of 8 x-layers as soon as the walk has finished it


class Partition(enum.IntEnum):
    """include/m2s.h `m2s_partition`."""
    Auto = 0
    Contiguous = 1
    Interleaved = 2
    Adaptive = 3


class Exchange(enum.IntEnum):
    """include/m2s.h `m2s_exchange` (device-resident results of generate_grid_sdf_multi)."""
    Auto = 0
    Peer = 1
    Rccl = 2
    Nothing = 3


def generate_grid_sdf(vertices, indices: Topology, grid: Grid, sign_method: SignMethod = SignMethod.Raycast, *,
                      timings: M2STimings = None, algorithm: int = 0, x_slab: Sequence[int] = None, out=None,
                      peer_out=None, peer_mode: PeerMode = PeerMode.Push, lane: int = 0, synchronous: bool = True,
                      x_period: int = 0):
    """generate/grid.rs:265-378.  `x_slab=(x0, x1)` computes only cells with x0 <= x < x1 (the rest
    of `out` is left untouched); used by the multi-GPU driver in distributed.py.  With `x_period` > 0 the call owns the
    interleaved chunks [x0 + j * x_period, x1 + j * x_period), j = 0, 1, ... (m2s_opts.x_period).  `peer_out`: whole-grid
    device buffers (tensors or raw pointers, usually on other GPUs) that receive the same cells (m2s_opts.peer_out)."""
    a = _Args(vertices, indices)
    total = grid.get_total_cell_count()
    if out is None:
        if a.device:
            out = a.torch.empty(total, dtype=a.torch.float32, device=a.dev)
        else:
            out = np.empty(total, np.float32)
    if a.device:
        assert out.is_cuda and out.dtype == a.torch.float32 and out.numel() == total and out.is_contiguous()
        p_out = out.data_ptr() if total else None
    else:
        assert out.dtype == np.float32 and out.size == total and out.flags["C_CONTIGUOUS"]
        p_out = out.ctypes.data if total else None
    xb, xe = (0, 0) if x_slab is None else (int(x_slab[0]), int(x_slab[1]))
    if x_slab is not None and xb == xe:
        return out
    o = a.opts(timings, algorithm, xb, xe, synchronous or not a.device, peer_out, peer_mode, lane, x_period)
    rc = _lib.lib().m2s_generate_grid_sdf(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology,
                                          C.byref(grid._g), int(sign_method), p_out, C.byref(o))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return out


def interleaved_slab(grid: "Grid", n: int, k: int):
    """m2s_interleaved_slab: (x0, x1, x_period) of shard k of n — the chunks k and n + k of 2n where the grid allows it
    (x_period > 0), else the contiguous slab with x_period = 0."""
    a, b, p = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _lib.lib().m2s_interleaved_slab(C.byref(grid._g), int(n), int(k), C.byref(a), C.byref(b), C.byref(p))
    return int(a.value), int(b.value), int(p.value)


def slab_bounds(nx: int, n: int, k: int):
    """m2s_slab_bounds: contiguous x-slab [x0, x1) of shard k out of n (sizes differ by at most one layer)."""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _lib.lib().m2s_slab_bounds(int(nx), int(n), int(k), C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def generate_grid_sdf_multi(vertices, indices: Topology, grid: Grid, sign_method: SignMethod = SignMethod.Raycast, *,
                            devices: Sequence[int] = None, outs=None, exchange: Exchange = Exchange.Auto,
                            peer_mode: PeerMode = PeerMode.Push, algorithm: int = 0, info: dict = None,
                            partition: Partition = Partition.Auto):
    """generate_grid_sdf over several GPUs from this one process (m2s_generate_grid_sdf_multi): one host thread per
    device inside the library, contiguous x-slabs, no data-path collective.

    numpy in  -> one numpy array out (every device streams its slab into it over its own PCIe link);
    torch CUDA tensors in (on devices[0]) -> a list of whole-grid CUDA tensors, one per entry of `devices`, each
    holding the WHOLE grid on return (peer writes over xGMI, or RCCL where peer access is unavailable).
    `devices` may repeat a device (two shards on one GPU).  `info` (optional dict) receives wall_ms, exchange, timings."""
    a = _Args(vertices, indices)
    total = grid.get_total_cell_count()
    L = _lib.lib()
    if devices is None:
        devices = list(range(L.m2s_device_count()))
    devices = [int(d) for d in devices]
    n = len(devices)
    mo = _lib.M2SMultiOpts()
    mo.struct_size = C.sizeof(_lib.M2SMultiOpts)
    mo.n_devices = n
    dev_arr = (C.c_int32 * max(n, 1))(*devices)
    mo.devices = C.cast(dev_arr, C.POINTER(C.c_int32))
    mo.exchange = int(exchange)
    mo.peer_mode = int(peer_mode)
    mo.algorithm = int(algorithm)
    mo.partition = int(partition)
    tims = (M2STimings * max(n, 1))()
    mo.timings = C.cast(tims, C.POINTER(M2STimings))
    wall, used, part_used = C.c_float(0.0), C.c_int32(-1), C.c_int32(-1)
    mo.wall_ms = C.pointer(wall)
    mo.exchange_used = C.pointer(used)
    mo.partition_used = C.pointer(part_used)
    slabs = (C.c_uint64 * (3 * max(n, 1)))()
    mo.slabs = C.cast(slabs, C.POINTER(C.c_uint64))
    if a.device:
        mo.mem_kind = _lib.MEM_DEVICE
        dev0 = a.dev.index if a.dev.index is not None else a.torch.cuda.current_device()
        assert n == 0 or devices[0] == dev0, "the mesh tensors must live on devices[0]"
        if outs is None:
            outs = [a.torch.empty(total, dtype=a.torch.float32, device=f"cuda:{d}") for d in devices]
        assert len(outs) == n and all(o.is_cuda and o.dtype == a.torch.float32 and o.numel() == total and o.is_contiguous() for o in outs)
        a.torch.cuda.synchronize(a.dev)      # the library uses streams of its own: inputs must be complete
        ptrs = (C.c_void_p * max(n, 1))(*[(o.data_ptr() if total else None) for o in outs])
        result = outs
    else:
        mo.mem_kind = _lib.MEM_HOST
        if outs is None:
            outs = np.empty(total, np.float32)
        assert outs.dtype == np.float32 and outs.size == total and outs.flags["C_CONTIGUOUS"]
        ptrs = (C.c_void_p * 1)(outs.ctypes.data if total else None)
        result = outs
    rc = L.m2s_generate_grid_sdf_multi(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, C.byref(grid._g),
                                       int(sign_method), C.cast(ptrs, C.POINTER(C.c_void_p)), C.byref(mo))
    if rc != _lib.M2S_OK:
        _raise(rc)
    if info is not None:
        info["wall_ms"] = float(wall.value)
        info["exchange"] = Exchange(used.value).name if used.value >= 0 else None
        info["timings"] = [tims[k] for k in range(n)]
        info["partition"] = Partition(part_used.value).name if part_used.value >= 0 else None
        info["slabs"] = [(int(slabs[3 * k]), int(slabs[3 * k + 1]), int(slabs[3 * k + 2])) for k in range(n)]
        info["_keep"] = tims
    return result


def warmup(device: int = -1, workspace_bytes: int = 0, host_ring_bytes: int = 0):
    """m2s_warmup: pay the one-off costs of a process's first call now (runtime, code objects, context, optional workspace / pinned ring)."""
    rc = _lib.lib().m2s_warmup(int(device), int(workspace_bytes), int(host_ring_bytes))
    if rc != _lib.M2S_OK:
        _raise(rc)


def peer_bandwidth(src, peers, n_cells: int = None):
    """m2s_peer_bandwidth: GB/s of the peer-push copy kernel from the CUDA tensor `src` into each tensor / SharedGrid of `peers` (one at
    a time) and into all of them at once.  Returns (per_peer_gbps, all_together_gbps)."""
    n = len(peers)
    if n == 0:
        return [], 0.0
    n_cells = int(n_cells if n_cells is not None else src.numel())
    ptrs = (C.c_void_p * n)(*[int(p.data_ptr()) for p in peers])
    each = (C.c_float * n)()
    allg = C.c_float(0.0)
    dev = src.device.index if src.device.index is not None else -1
    rc = _lib.lib().m2s_peer_bandwidth(int(src.data_ptr()), C.cast(ptrs, C.POINTER(C.c_void_p)), n, n_cells, dev, each, C.byref(allg))
    if rc != _lib.M2S_OK:
        _raise(rc)
    return [float(x) for x in each], float(allg.value)


def balanced_slabs(nx: int, unit: int, prev_bounds: Sequence[int], cost: Sequence[float]):
    """m2s_balanced_slabs: n + 1 slab boundaries of equal cost from the boundaries and per-shard costs of a previous call."""
    n = len(cost)
    assert len(prev_bounds) == n + 1
    pb = (C.c_uint64 * (n + 1))(*[int(b) for b in prev_bounds])
    cs = (C.c_float * n)(*[float(c) for c in cost])
    nb = (C.c_uint64 * (n + 1))()
    rc = _lib.lib().m2s_balanced_slabs(int(nx), n, int(unit), pb, cs, nb)
    if rc != _lib.M2S_OK:
        _raise(rc)
    return [int(b) for b in nb]


def generate_sdf_multi(vertices, indices: Topology, query_points, acceleration_method: AccelerationMethod = None, *,
                       devices: Sequence[int] = None, outs=None, exchange: Exchange = Exchange.Auto, algorithm: int = 0,
                       info: dict = None):
    """generate_sdf over several GPUs from this one process (m2s_generate_sdf_multi): shard k computes a contiguous range of the
    queries.  numpy in -> one numpy array out; torch CUDA tensors in (on devices[0]) -> a list of CUDA tensors, one per entry of
    `devices`, each holding ALL distances on return.  `devices` may repeat a device."""
    am = acceleration_method if acceleration_method is not None else AccelerationMethod.RtreeBvh
    a = _Args(vertices, indices, query_points)
    L = _lib.lib()
    if devices is None:
        devices = list(range(L.m2s_device_count()))
    devices = [int(d) for d in devices]
    n = len(devices)
    mo = _lib.M2SMultiOpts()
    mo.struct_size = C.sizeof(_lib.M2SMultiOpts)
    mo.n_devices = n
    dev_arr = (C.c_int32 * max(n, 1))(*devices)
    mo.devices = C.cast(dev_arr, C.POINTER(C.c_int32))
    mo.exchange = int(exchange)
    mo.algorithm = int(algorithm)
    tims = (M2STimings * max(n, 1))()
    mo.timings = C.cast(tims, C.POINTER(M2STimings))
    wall, used = C.c_float(0.0), C.c_int32(-1)
    mo.wall_ms = C.pointer(wall)
    mo.exchange_used = C.pointer(used)
    if a.device:
        mo.mem_kind = _lib.MEM_DEVICE
        dev0 = a.dev.index if a.dev.index is not None else a.torch.cuda.current_device()
        assert n == 0 or devices[0] == dev0, "mesh and queries must live on devices[0]"
        if outs is None:
            outs = [a.torch.empty(a.n_q, dtype=a.torch.float32, device=f"cuda:{d}") for d in devices]
        assert len(outs) == n and all(o.is_cuda and o.dtype == a.torch.float32 and o.numel() == a.n_q and o.is_contiguous() for o in outs)
        a.torch.cuda.synchronize(a.dev)      # the library uses streams of its own: inputs must be complete
        ptrs = (C.c_void_p * max(n, 1))(*[(o.data_ptr() if a.n_q else None) for o in outs])
    else:
        mo.mem_kind = _lib.MEM_HOST
        if outs is None:
            outs = np.empty(a.n_q, np.float32)
        assert outs.dtype == np.float32 and outs.size == a.n_q and outs.flags["C_CONTIGUOUS"]
        ptrs = (C.c_void_p * 1)(outs.ctypes.data if a.n_q else None)
    n_out = C.c_size_t(0)
    rc = L.m2s_generate_sdf_multi(a.p_verts, a.n_verts, a.p_idx, a.n_idx, a.index_bytes, a.topology, a.p_q, a.n_q, int(am.kind),
                                  int(am.sign), C.cast(ptrs, C.POINTER(C.c_void_p)), C.byref(n_out), C.byref(mo))
    if rc != _lib.M2S_OK:
        _raise(rc)
    if info is not None:
        info["wall_ms"] = float(wall.value)
        info["exchange"] = Exchange(used.value).name if used.value >= 0 else None
        info["timings"] = [tims[k] for k in range(n)]
        info["_keep"] = tims
    if a.device:
        return [o[: n_out.value] for o in outs]
    return outs[: n_out.value]


class SharedGrid:
    """A whole-grid device buffer other PROCESSES can map (m2s_shared_alloc / m2s_ipc_*): the one-process-per-GPU form of
    the peer exchange.  `tensor` views it as a torch CUDA tensor; `handle` is the 64-byte token to send to the other ranks;
    `SharedGrid.open(handle, device)` maps a peer's buffer and returns its device pointer wrapper."""

    def __init__(self, n_cells: int, device: int):
        self.n, self.device, self.owner = int(n_cells), int(device), True
        p = C.c_void_p()
        rc = _lib.lib().m2s_shared_alloc(self.n * 4, self.device, C.byref(p))
        if rc != _lib.M2S_OK:
            _raise(rc)
        self.ptr = int(p.value)

    @property
    def handle(self) -> bytes:
        buf = C.create_string_buffer(_lib.IPC_HANDLE_BYTES)
        rc = _lib.lib().m2s_ipc_export(self.ptr, buf)
        if rc != _lib.M2S_OK:
            _raise(rc)
        return bytes(buf.raw)

    @classmethod
    def open(cls, handle: bytes, n_cells: int, device: int):
        g = cls.__new__(cls)
        g.n, g.device, g.owner = int(n_cells), int(device), False
        p = C.c_void_p()
        rc = _lib.lib().m2s_ipc_open(C.create_string_buffer(bytes(handle), _lib.IPC_HANDLE_BYTES), g.device, C.byref(p))
        if rc != _lib.M2S_OK:
            _raise(rc)
        g.ptr = int(p.value)
        return g

    def data_ptr(self):
        return self.ptr

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.n,), "typestr": "<f4", "data": (self.ptr, False), "version": 2, "strides": None}

    @property
    def tensor(self):
        import torch

        t = torch.as_tensor(self, device=f"cuda:{self.device}")
        assert t.data_ptr() == self.ptr, "torch copied the buffer instead of wrapping it"
        return t

    def close(self):
        if getattr(self, "ptr", 0):
            L = _lib.lib()
            (L.m2s_shared_free if self.owner else L.m2s_ipc_close)(self.ptr, self.device)
            self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mesh:
    """Persistent mesh (include/m2s.h `m2s_mesh`): triangle records + LBVH built once and kept on the
    device; `generate_grid_sdf` / `generate_sdf` then skip the build, and the sign planes of the last
    grid are cached.  Results are identical to the one-shot functions.  The reference rebuilds its
    trees in every call (generate/grid.rs:95-111); its client regenerates on every parameter change
    (mesh_to_sdf_client/src/sdf.rs:32-137), which is what this object is for."""

    def __init__(self, vertices, indices: Topology):
        self._a = _Args(vertices, indices)
        self._h = C.c_void_p()
        o = self._a.opts()
        rc = _lib.lib().m2s_mesh_create(self._a.p_verts, self._a.n_verts, self._a.p_idx, self._a.n_idx, self._a.index_bytes,
                                        self._a.topology, C.byref(o), C.byref(self._h))
        if rc != _lib.M2S_OK:
            self._h = C.c_void_p()
            _raise(rc)

    @property
    def device(self):
        return self._a.device

    def triangle_count(self):
        return int(_lib.lib().m2s_mesh_triangle_count(self._h))

    def generate_grid_sdf(self, grid: Grid, sign_method: SignMethod = SignMethod.Raycast, *, timings: M2STimings = None,
                          algorithm: int = 0, x_slab: Sequence[int] = None, out=None, synchronous: bool = True,
                          peer_out=None, peer_mode: PeerMode = PeerMode.Push):
        a = self._a
        total = grid.get_total_cell_count()
        if out is None:
            out = a.torch.empty(total, dtype=a.torch.float32, device=a.dev) if a.device else np.empty(total, np.float32)
        p_out = (out.data_ptr() if a.device else out.ctypes.data) if total else None
        xb, xe = (0, 0) if x_slab is None else (int(x_slab[0]), int(x_slab[1]))
        if x_slab is not None and xb == xe:
            return out
        o = a.opts(timings, algorithm, xb, xe, synchronous or not a.device, peer_out, peer_mode)
        rc = _lib.lib().m2s_mesh_generate_grid_sdf(self._h, C.byref(grid._g), int(sign_method), p_out, C.byref(o))
        if rc != _lib.M2S_OK:
            _raise(rc)
        return out

    def generate_sdf(self, query_points, acceleration_method: AccelerationMethod = None, *, timings: M2STimings = None,
                     algorithm: int = 0):
        am = acceleration_method if acceleration_method is not None else AccelerationMethod.RtreeBvh
        a = self._a
        if a.device:
            q = query_points if _is_torch(query_points) else a.torch.as_tensor(np.asarray(query_points, np.float32), device=a.dev)
            q = q.detach().to(device=a.dev, dtype=a.torch.float32).contiguous().reshape(-1, 3)
            n_q, p_q = q.shape[0], (q.data_ptr() if q.numel() else None)
            out = a.torch.empty(n_q, dtype=a.torch.float32, device=a.dev)
            p_out = out.data_ptr() if n_q else None
        else:
            q = np.ascontiguousarray(np.asarray(query_points, np.float32)).reshape(-1, 3)
            n_q, p_q = q.shape[0], (q.ctypes.data if q.size else None)
            out = np.empty(n_q, np.float32)
            p_out = out.ctypes.data if n_q else None
        n_out = C.c_size_t(0)
        o = a.opts(timings, algorithm)
        rc = _lib.lib().m2s_mesh_generate_sdf(self._h, p_q, n_q, int(am.kind), int(am.sign), p_out, C.byref(n_out), C.byref(o))
        if rc != _lib.M2S_OK:
            _raise(rc)
        return out[: n_out.value]

    def closest_points(self, query_points, *, timings: M2STimings = None, algorithm: int = 0):
        """closest_points on the resident tree: same results as the one-shot function."""
        a = self._a
        if a.device:
            q = query_points if _is_torch(query_points) else a.torch.as_tensor(np.asarray(query_points, np.float32), device=a.dev)
            q = q.detach().to(device=a.dev, dtype=a.torch.float32).contiguous().reshape(-1, 3)
            n_q, p_q = q.shape[0], (q.data_ptr() if q.numel() else None)
        else:
            q = np.ascontiguousarray(np.asarray(query_points, np.float32)).reshape(-1, 3)
            n_q, p_q = q.shape[0], (q.ctypes.data if q.size else None)
        bufs, ptrs = _closest_buffers(a, n_q)
        o = a.opts(timings, algorithm)
        rc = _lib.lib().m2s_mesh_closest_points(self._h, p_q, n_q, *ptrs, C.byref(o))
        if rc != _lib.M2S_OK:
            _raise(rc)
        return _closest_result(a, bufs)

    def grid_closest_points(self, grid: Grid, *, timings: M2STimings = None, algorithm: int = 0, x_slab: Sequence[int] = None,
                            out=None):
        """grid_closest_points on the resident tree: same results as the one-shot function."""
        a = self._a
        total = grid.get_total_cell_count()
        if out is None:
            bufs, ptrs = _closest_buffers(a, total)
        else:
            bufs = tuple(out)
            ptrs = [(x.data_ptr() if a.device else x.ctypes.data) if total else None for x in bufs]
        xb, xe = (0, 0) if x_slab is None else (int(x_slab[0]), int(x_slab[1]))
        if x_slab is not None and xb == xe:
            return _closest_result(a, bufs)
        o = a.opts(timings, algorithm, xb, xe)
        rc = _lib.lib().m2s_mesh_grid_closest_points(self._h, C.byref(grid._g), *ptrs, C.byref(o))
        if rc != _lib.M2S_OK:
            _raise(rc)
        return _closest_result(a, bufs)

    def _mesh_winding_queries(self, query_points, beta, threshold, signed, timings, algorithm, synchronous):
        q, n_q, p_q = _queries_of(self._a, query_points)   # q stays alive through the call
        L = _lib.lib()
        return _winding_queries(lambda *r: L.m2s_mesh_winding_numbers(self._h, *r), self._a, n_q, p_q, beta, threshold, signed, timings,
                                algorithm, synchronous)

    def _mesh_winding_grid(self, grid, beta, threshold, signed, timings, algorithm, x_slab, out, synchronous):
        L = _lib.lib()
        return _winding_grid(lambda *r: L.m2s_mesh_grid_winding_numbers(self._h, *r), self._a, grid, beta, threshold, signed, timings,
                             algorithm, x_slab, out, synchronous)

    def winding_numbers(self, query_points, *, beta: float = WINDING_BETA_DEFAULT, algorithm: int = 0, timings: M2STimings = None,
                        synchronous: bool = True):
        """winding_numbers on the resident tree; its moments are made by the first winding call and kept.  On one Mesh a point's value
        depends only on the point and beta: the grid forms, their x-slabs and the point forms agree bit for bit."""
        return self._mesh_winding_queries(query_points, beta, 0.5, False, timings, algorithm, synchronous)

    def grid_winding_numbers(self, grid: Grid, *, beta: float = WINDING_BETA_DEFAULT, algorithm: int = 0, timings: M2STimings = None,
                             x_slab: Sequence[int] = None, out=None, synchronous: bool = True):
        return self._mesh_winding_grid(grid, beta, 0.5, False, timings, algorithm, x_slab, out, synchronous)

    def generate_sdf_winding(self, query_points, *, beta: float = WINDING_BETA_DEFAULT, threshold: float = 0.5, algorithm: int = 0,
                             timings: M2STimings = None, synchronous: bool = True):
        return self._mesh_winding_queries(query_points, beta, threshold, True, timings, algorithm, synchronous)

    def generate_grid_sdf_winding(self, grid: Grid, *, beta: float = WINDING_BETA_DEFAULT, threshold: float = 0.5, algorithm: int = 0,
                                  timings: M2STimings = None, x_slab: Sequence[int] = None, out=None, synchronous: bool = True):
        return self._mesh_winding_grid(grid, beta, threshold, True, timings, algorithm, x_slab, out, synchronous)

    def _mesh_rays(self, origins, directions, t_min, t_max, want, timings, algorithm, synchronous):
        L = _lib.lib()
        return _ray_call(lambda *r: L.m2s_mesh_cast_rays(self._h, *r), self._a, origins, directions, t_min, t_max, want, timings, algorithm,
                         synchronous)

    def cast_rays(self, origins, directions, t_min: float = 0.0, t_max: float = float("inf"), algorithm: int = 0, *,
                  timings: M2STimings = None, synchronous: bool = True) -> RayHits:
        """cast_rays on the resident tree as it is (no build, no re-marking of its leaves): the same bits as the one-shot function."""
        return self._mesh_rays(origins, directions, t_min, t_max, "hits", timings, algorithm, synchronous)

    def count_intersections(self, origins, directions, t_min: float = 0.0, t_max: float = float("inf"), algorithm: int = 0, *,
                            timings: M2STimings = None, synchronous: bool = True):
        return self._mesh_rays(origins, directions, t_min, t_max, "count", timings, algorithm, synchronous)

    def test_occlusions(self, origins, directions, t_min: float = 0.0, t_max: float = float("inf"), algorithm: int = 0, *,
                        timings: M2STimings = None, synchronous: bool = True):
        return self._mesh_rays(origins, directions, t_min, t_max, "occluded", timings, algorithm, synchronous)

    def sample_surface(self, n: int, seed: int = 0, first_sample: int = 0, normals: bool = False, *, algorithm: int = 0,
                       timings: M2STimings = None, synchronous: bool = True, points_only: bool = False) -> SurfaceSamples:
        """sample_surface on the resident triangles: the same bits as the one-shot function.  The weight table is made by the first
        sampling call and kept.  `points_only`: triangle and uv are not written (None)."""
        L = _lib.lib()
        return _sample_call(lambda *r: L.m2s_mesh_sample_surface(self._h, *r), self._a, n, seed, first_sample, normals, timings, algorithm,
                            synchronous, points_only)

    def surface_area(self) -> float:
        area = C.c_double(0.0)
        o = self._a.opts()
        rc = _lib.lib().m2s_mesh_sample_surface(self._h, 0, None, None, None, None, None, C.byref(area), C.byref(o))
        if rc != _lib.M2S_OK:
            _raise(rc)
        return float(area.value)

    def voxelize(self, grid: Grid, solid: bool = False, *, bits: bool = False, cells: bool = False, algorithm: int = 0,
                 timings: M2STimings = None, synchronous: bool = True, occupancy: bool = True, count: bool = True) -> Voxels:
        """voxelize on the resident triangles: the same bits as the one-shot function.  The tree is not consulted."""
        L = _lib.lib()
        return _voxel_call(lambda *r: L.m2s_mesh_voxelize(self._h, *r), self._a, grid, solid, bits, cells, timings, algorithm, synchronous,
                           occupancy, count)

    def narrow_band_sdf(self, grid: Grid, band, sign_method: SignMethod = SignMethod.Raycast, *, bits: bool = False, algorithm: int = 0,
                        timings: M2STimings = None, capacity: Optional[int] = None, synchronous: bool = True) -> NarrowBand:
        """narrow_band_sdf on the resident mesh: the same bits as the one-shot function."""
        L = _lib.lib()
        return _band_call(lambda *r: L.m2s_mesh_narrow_band_sdf(self._h, *r), self._a, grid, band, sign_method, bits, algorithm, timings,
                          capacity, synchronous)

    def narrow_band_field(self, grid: Grid, band, sign_method: SignMethod = SignMethod.Raycast, inside=True, *, background=None) -> "BandField":
        """narrow_band_sdf and, with inside=True, voxelize(solid=True, bits=True) on the same grid, as one resident BandField: the cells
        beyond the band take -background inside the mesh and +background outside it.  inside may also be a sign mask of the caller's, or
        None (everything beyond the band is outside)."""
        nb = self.narrow_band_sdf(grid, band, sign_method)
        if inside is True:
            inside = self.voxelize(grid, solid=True, bits=True, occupancy=False, count=False)
        return nb.field(background, inside)

    def remesh(self, grid: Grid, *, iso: float = 0.0, sign_method: SignMethod = SignMethod.Raycast, keep_largest: int = 0):
        """remesh on the resident mesh: the same bits as the one-shot function."""
        return _remesh(self.narrow_band_sdf(grid, isosurface_band(grid, iso), sign_method), iso, int(keep_largest))

    def boolean(self, other: "Mesh", op, grid: Grid, *, sign_method: SignMethod = SignMethod.Raycast, keep_largest: int = 0):
        """boolean on two resident meshes: the same bits as the one-shot function."""
        return _boolean(self, other, op, grid, sign_method, int(keep_largest))

    def sample_sdf_near_surface(self, n: int, sigmas=None, uniform_fraction: float = 0.05, sign: str = "winding", seed: int = 0):
        """sample_sdf_near_surface on this mesh."""
        return _sample_sdf_near_surface(self, n, sigmas, uniform_fraction, sign, seed)

    def debug_digest(self):
        """FNV-1a digests of the resident arrays (test hook `m2s_debug_mesh_digest`): triangle records, pre-test planes, box nodes,
        oriented bounds, centroids, slot table, scene words, triangle count."""
        L = _lib.lib()
        L.m2s_debug_mesh_digest.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.m2s_debug_mesh_digest.restype = C.c_int
        out = (C.c_uint64 * 8)()
        rc = L.m2s_debug_mesh_digest(self._h, out)
        if rc != _lib.M2S_OK:
            _raise(rc)
        return [int(x) for x in out]

    DEBUG_ARRAYS = ("tris", "planes", "nodes", "ext", "slot_of", "slot_first", "scene")   # `which` of m2s_debug_mesh_arrays, in order

    def debug_arrays(self, dtypes=None):
        """The resident arrays as they stand on the device (test hook `m2s_debug_mesh_arrays`): a dict with the triangle records, the
        pre-test planes, the box nodes, the oriented bounds, the slot table, slot_first, the scene words and `leaf_max`, the leaf size the
        tree is marked with now.  `dtypes` maps a name to the numpy (structured) dtype its array is viewed through; a name it lacks
        comes back as uint32 words.  The record layouts are csrc/common.h; tests/bounds_model.py keeps the one Python copy of them."""
        L = _lib.lib()
        L.m2s_debug_mesh_arrays.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.m2s_debug_mesh_arrays.restype = C.c_int

        def fetch(which):
            nbytes = C.c_size_t(0)
            rc = L.m2s_debug_mesh_arrays(self._h, which, None, 0, C.byref(nbytes))
            if rc != _lib.M2S_OK:
                _raise(rc)
            raw = np.zeros(nbytes.value // 4, np.uint32)
            rc = L.m2s_debug_mesh_arrays(self._h, which, raw.ctypes.data if raw.size else None, raw.nbytes, C.byref(nbytes))
            if rc != _lib.M2S_OK:
                _raise(rc)
            return raw

        out = {}
        for which, name in enumerate(self.DEBUG_ARRAYS):
            raw = fetch(which)
            out[name] = raw.view(np.dtype(dtypes[name])) if dtypes and name in dtypes else raw
        out["leaf_max"] = int(fetch(len(self.DEBUG_ARRAYS))[0])
        return out

    def debug_cut_lists(self, grid: Grid = None, *, x_slab: Sequence[int] = None, x_period: int = 0, coarse: bool = False, queries=None):
        """The cut lists k_cut leaves for a call on this mesh (test hook `m2s_debug_cut_lists`), as uint32 words, 16 per list: of a grid call
        over `grid` (its slab `x_slab`, interleaved with `x_period`), one list per packet brick of the slab — `coarse`: the coarse records of
        a two-level plan instead, 64 words per block: 8 sub-lists of 8 —, or of a query call over `queries` (host array), one list per packet.
        An empty array where the call takes no lists.  The list format is csrc/dist.hip.h: word 0 the number of ranges, one word per range;
        the words behind a list's last range, which k_cut never writes, come back as 0."""
        L = _lib.lib()
        L.m2s_debug_cut_lists.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.M2SGrid), C.POINTER(_lib.M2SOpts), C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.m2s_debug_cut_lists.restype = C.c_int
        xb, xe = (0, 0) if x_slab is None else (int(x_slab[0]), int(x_slab[1]))
        o = self._a.opts(x_begin=xb, x_end=xe, x_period=x_period)
        if queries is not None:
            q = np.ascontiguousarray(np.asarray(queries, np.float32)).reshape(-1, 3)
            args = (self._h, 2, None, C.byref(o), q.ctypes.data if q.size else None, q.shape[0])
        else:
            args = (self._h, 1 if coarse else 0, C.byref(grid._g), C.byref(o), None, 0)
        n = C.c_size_t(0)
        rc = L.m2s_debug_cut_lists(*args, None, 0, C.byref(n))
        if rc != _lib.M2S_OK:
            _raise(rc)
        words = np.zeros(n.value, np.uint32)
        if n.value:
            rc = L.m2s_debug_cut_lists(*args, words.ctypes.data, words.size, C.byref(n))
            if rc != _lib.M2S_OK:
                _raise(rc)
        per = words.reshape(-1, 8 if coarse and queries is None else 16)
        per[np.arange(per.shape[1])[None, :] > per[:, :1]] = 0
        return words

    def drain_timings(self) -> M2STimings:
        t = M2STimings()
        rc = _lib.lib().m2s_mesh_drain_timings(self._h, C.byref(t))
        if rc != _lib.M2S_OK:
            _raise(rc)
        return t

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib.lib().m2s_mesh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
