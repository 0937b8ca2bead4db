"""The argument checks of the sixteen query-feature entry points (closest points, winding numbers, ray casting, surface sampling,
voxelization, narrow bands) through ctypes: the return code and the full m2s_last_error text of every bad argument that is rejected
before a device is looked for, pairs of bad arguments that pin which check comes first, and the successes that need no device with
the values they write.  No case here reaches the device, so the module passes with and without a GPU; the resident forms, whose
m2s_mesh needs a device, are at the end under the gpu mark."""
import ctypes as C
import os

import numpy as np
import pytest

from mesh_to_sdf_amd import _lib

OK, BAD, EMPTY = _lib.M2S_OK, _lib.ERR_BAD_ARG, _lib.ERR_EMPTY_MESH
F = np.float32
INF, NAN = float("inf"), float("nan")

V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)       # one triangle
I32 = np.array([0, 1, 2], np.uint32)
I16 = np.array([0, 1, 2], np.uint16)
OOB32 = np.array([0, 1, 5], np.uint32)
OOB16 = np.array([0, 7, 2], np.uint16)
Q = np.array([[0.25, 0.25, 1.0]], F)
DIR = np.array([[0, 0, -1]], F)
BUF = np.zeros(64, np.uint64)                            # any output: no case here gets as far as writing one
MANY = 0xFFFFFFC0
TRIS_2_25 = 3 * (2 ** 25 + 1)                            # vertices of 2^25 + 1 triangles without indices (never read before the check)

MSG_OOB5 = "vertex index 5 out of range (3 vertices; the reference panics indexing `vertices`)"
MSG_OOB7 = "vertex index 7 out of range (3 vertices; the reference panics indexing `vertices`)"
MSG_EMPTY_CLOSEST = "closest points on a mesh without triangles"


def p(a):
    return a.ctypes.data


def grid(count=(4, 2, 2), size=(1, 1, 1), first=(0, 0, 0)):
    return _lib.M2SGrid((C.c_float * 3)(*first), (C.c_float * 3)(*size), (C.c_uint64 * 3)(*count))


def opts(**kw):
    o = _lib.M2SOpts(struct_size=C.sizeof(_lib.M2SOpts), device=-1)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def ray_opts(size=None, t_min=0.0, t_max=INF):
    return _lib.M2SRayOpts(C.sizeof(_lib.M2SRayOpts) if size is None else size, t_min, t_max)


def sample_opts(size=None, reserved=0, seed=1, first=0):
    return _lib.M2SSurfaceSampleOpts(C.sizeof(_lib.M2SSurfaceSampleOpts) if size is None else size, reserved, seed, first)


def voxel_opts(size=None, mode=0):
    return _lib.M2SVoxelizeOpts(C.sizeof(_lib.M2SVoxelizeOpts) if size is None else size, mode)


def band_opts(size=None, exterior=1.0, interior=1.0):
    return _lib.M2SBandOpts(C.sizeof(_lib.M2SBandOpts) if size is None else size, exterior, interior)


MESH = ["vertices", "n_vertices", "indices", "n_indices", "index_bytes", "topology"]
# argument names of every entry point, in the order of include/m2s.h
SIG = {
    "m2s_closest_points": MESH + ["queries", "n", "triangle_out", "point_out", "distance_out", "opts"],
    "m2s_grid_closest_points": MESH + ["grid", "triangle_out", "point_out", "distance_out", "opts"],
    "m2s_mesh_closest_points": ["mesh", "queries", "n", "triangle_out", "point_out", "distance_out", "opts"],
    "m2s_mesh_grid_closest_points": ["mesh", "grid", "triangle_out", "point_out", "distance_out", "opts"],
    "m2s_winding_numbers": MESH + ["queries", "n", "beta", "threshold", "winding_out", "sdf_out", "opts"],
    "m2s_grid_winding_numbers": MESH + ["grid", "beta", "threshold", "winding_out", "sdf_out", "opts"],
    "m2s_mesh_winding_numbers": ["mesh", "queries", "n", "beta", "threshold", "winding_out", "sdf_out", "opts"],
    "m2s_mesh_grid_winding_numbers": ["mesh", "grid", "beta", "threshold", "winding_out", "sdf_out", "opts"],
    "m2s_cast_rays": MESH + ["origins", "directions", "n", "ropts", "t_out", "triangle_out", "uv_out", "count_out", "occluded_out", "opts"],
    "m2s_mesh_cast_rays": ["mesh", "origins", "directions", "n", "ropts", "t_out", "triangle_out", "uv_out", "count_out", "occluded_out", "opts"],
    "m2s_sample_surface": MESH + ["n", "sopts", "point_out", "triangle_out", "uv_out", "normal_out", "area_out", "opts"],
    "m2s_mesh_sample_surface": ["mesh", "n", "sopts", "point_out", "triangle_out", "uv_out", "normal_out", "area_out", "opts"],
    "m2s_voxelize": MESH + ["grid", "vopts", "bits_out", "occupancy_out", "cells_out", "capacity", "n_set_out", "opts"],
    "m2s_mesh_voxelize": ["mesh", "grid", "vopts", "bits_out", "occupancy_out", "cells_out", "capacity", "n_set_out", "opts"],
    "m2s_narrow_band_sdf": MESH + ["grid", "sign_method", "bopts", "cells_out", "distances_out", "capacity", "bits_out", "n_active_out", "opts"],
    "m2s_mesh_narrow_band_sdf": ["mesh", "grid", "sign_method", "bopts", "cells_out", "distances_out", "capacity", "bits_out", "n_active_out", "opts"],
}
ONE_SHOT = [n for n in SIG if "_mesh_" not in n]
RESIDENT = [n for n in SIG if "_mesh_" in n]
NO_OUT = {k: None for k in ("triangle_out", "point_out", "distance_out", "winding_out", "sdf_out", "t_out", "uv_out", "count_out", "occluded_out",
                            "normal_out", "area_out", "bits_out", "occupancy_out", "cells_out", "n_set_out", "distances_out", "n_active_out")}


def defaults():
    """A good value for every argument name (a fresh dict: the ctypes structs in it must outlive the call)."""
    d = dict(vertices=p(V), n_vertices=3, indices=p(I32), n_indices=3, index_bytes=4, topology=0, queries=p(Q), origins=p(Q), directions=p(DIR),
             n=1, grid=grid(), beta=3.0, threshold=0.5, ropts=None, sopts=None, vopts=None, bopts=band_opts(), sign_method=0, capacity=64,
             opts=None, mesh=None)
    for k in NO_OUT:
        d[k] = p(BUF)
    d["area_out"] = C.cast(p(BUF), C.POINTER(C.c_double))
    d["n_set_out"] = d["n_active_out"] = C.cast(p(BUF), C.POINTER(C.c_uint64))
    return d


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def call(lib, name, **over):
    d = defaults()
    unknown = set(over) - set(SIG[name])
    assert not unknown, (name, unknown)
    d.update(over)
    rc = getattr(lib, name)(*[d[a] for a in SIG[name]])
    return rc, lib.m2s_last_error().decode()


def no_outputs(name):
    return {k: None for k in NO_OUT if k in SIG[name]}


# ---- the mesh arguments of the eight one-shot forms ------------------------------------------------------------------------------
BAD_MESH = [
    ("null_vertices", dict(vertices=None), BAD, "vertices is NULL"),
    ("index_bytes_3", dict(index_bytes=3), BAD, "index_bytes must be 2 or 4"),
    ("index_bytes_8", dict(index_bytes=8), BAD, "index_bytes must be 2 or 4"),
    ("topology_2", dict(topology=2), BAD, "bad topology 2"),
    ("topology_negative", dict(topology=-1), BAD, "bad topology -1"),
    ("null_indices_with_count", dict(indices=None), BAD, "n_indices > 0 with NULL indices"),
    ("too_many_vertices", dict(n_vertices=0x7FFFFFFF), BAD, "mesh too large for 32-bit indexing"),
    ("index_out_of_range_u32", dict(indices=p(OOB32)), BAD, MSG_OOB5),
    ("index_out_of_range_u16", dict(indices=p(OOB16), index_bytes=2), BAD, MSG_OOB7),
    ("index_out_of_range_strip", dict(indices=p(OOB32), topology=1), BAD, MSG_OOB5),
    # which comes first
    ("topology_before_vertices", dict(topology=2, vertices=None), BAD, "bad topology 2"),
    ("vertices_before_index_bytes", dict(vertices=None, index_bytes=3), BAD, "vertices is NULL"),
    ("index_bytes_before_range", dict(indices=p(OOB32), index_bytes=3), BAD, "index_bytes must be 2 or 4"),
]


@pytest.mark.parametrize("name", ONE_SHOT)
@pytest.mark.parametrize("case", BAD_MESH, ids=[c[0] for c in BAD_MESH])
def test_bad_mesh_arguments(lib, name, case):
    _, over, rc, msg = case
    assert call(lib, name, **over) == (rc, msg)


def test_host_index_check_reads_whole_triples_only(lib):
    # a triangle list never reads a trailing partial triple; a strip reads every index
    idx = np.array([0, 1, 2, 9], np.uint32)
    assert call(lib, "m2s_closest_points", indices=p(idx), n_indices=4, n=0) == (OK, "")
    assert call(lib, "m2s_closest_points", indices=p(idx), n_indices=4, topology=1, n=0) == (
        BAD, "vertex index 9 out of range (3 vertices; the reference panics indexing `vertices`)")
    # device memory: the build checks the indices, not the host
    assert call(lib, "m2s_closest_points", indices=p(OOB32), n=0, opts=opts(mem_kind=_lib.MEM_DEVICE)) == (OK, "")


@pytest.mark.parametrize("name", ONE_SHOT)
def test_mesh_checks_against_the_feature_checks(lib, name):
    """Voxelization and narrow bands check the grid and their options before the mesh; the other four families the mesh first."""
    bad_mesh = dict(topology=2)
    first = {"m2s_voxelize": "bits_out, occupancy_out, cells_out and n_set_out are all NULL",
             "m2s_narrow_band_sdf": "cells_out, distances_out, bits_out and n_active_out are all NULL"}.get(name, "bad topology 2")
    assert call(lib, name, **bad_mesh, **no_outputs(name)) == (BAD, first)
    if "grid" in SIG[name]:
        grid_first = name in ("m2s_voxelize", "m2s_narrow_band_sdf")
        assert call(lib, name, **bad_mesh, grid=None) == (BAD, "grid is NULL" if grid_first else "bad topology 2")


@pytest.mark.parametrize("name", ["m2s_sample_surface", "m2s_voxelize", "m2s_narrow_band_sdf"])
def test_triangle_limit_of_sampling_voxelization_and_bands(lib, name):
    huge = dict(n_vertices=TRIS_2_25, indices=None, n_indices=0)
    assert call(lib, name, **huge) == (BAD, "more than 2^25 triangles")
    assert call(lib, name, **huge, topology=2) == (BAD, "bad topology 2")                        # after the mesh arguments
    # ... and before the host index check
    idx = np.zeros(TRIS_2_25, np.uint16)
    idx[0] = 7
    assert call(lib, name, indices=p(idx), n_indices=TRIS_2_25, index_bytes=2) == (BAD, "more than 2^25 triangles")


@pytest.mark.parametrize("name", ["m2s_closest_points", "m2s_winding_numbers", "m2s_cast_rays"])
def test_no_triangle_limit_elsewhere(lib, name):
    assert call(lib, name, n_vertices=TRIS_2_25, indices=None, n_indices=0, n=0) == (OK, "")


# ---- per family --------------------------------------------------------------------------------------------------------------------
GRID_CASES = [   # closest_grid_params: the grid forms of closest points and winding numbers
    (dict(grid=None), "grid is NULL"),
    (dict(grid=grid(count=(4, 0, 2))), "grid without cells"),
    (dict(opts=opts(x_period=4)), "m2s_opts.x_period / peer_out do not apply to closest-point calls"),
    (dict(opts=opts(n_peer_out=1)), "m2s_opts.x_period / peer_out do not apply to closest-point calls"),
    (dict(grid=grid(count=(0x7FFFFFFF, 1, 1))), "cell_count too large"),
    (dict(grid=grid(count=(2 ** 20, 2 ** 20, 1))), "grid face with 2^32 or more lines (cell_count 1048576 x 1048576 x 1)"),
    (dict(opts=opts(x_begin=3, x_end=2)), "x-slab [3,2) outside [0,4)"),
    (dict(opts=opts(x_begin=0, x_end=5)), "x-slab [0,5) outside [0,4)"),
    (dict(grid=None, opts=opts(x_period=4)), "grid is NULL"),
    (dict(grid=grid(count=(4, 0, 2)), opts=opts(x_period=4)), "grid without cells"),
]


@pytest.mark.parametrize("name", ["m2s_grid_closest_points", "m2s_grid_winding_numbers"])
@pytest.mark.parametrize("k", range(len(GRID_CASES)))
def test_slab_grid_arguments(lib, name, k):
    over, msg = GRID_CASES[k]
    assert call(lib, name, **over) == (BAD, msg)


QUERY_CASES = [
    (dict(queries=None), "queries is NULL"),
    (dict(n=MANY), "too many queries for one call"),
    (dict(queries=None, n=MANY), "queries is NULL"),
]


@pytest.mark.parametrize("name", ["m2s_closest_points", "m2s_winding_numbers"])
@pytest.mark.parametrize("k", range(len(QUERY_CASES)))
def test_query_arguments(lib, name, k):
    over, msg = QUERY_CASES[k]
    assert call(lib, name, **over) == (BAD, msg)
    assert call(lib, name, **over, **no_outputs(name))[1] != msg      # the outputs are checked before the queries


def test_closest_points(lib):
    all_null = "triangle_out, point_out and distance_out are all NULL"
    empty = dict(n_vertices=0, indices=None, n_indices=0)
    for name in ("m2s_closest_points", "m2s_grid_closest_points"):
        assert call(lib, name, **no_outputs(name)) == (BAD, all_null)
        assert call(lib, name, **empty) == (EMPTY, MSG_EMPTY_CLOSEST)
        assert call(lib, name, **empty, **no_outputs(name)) == (BAD, all_null)
        assert call(lib, name, n_indices=2) == (EMPTY, MSG_EMPTY_CLOSEST)            # two indices: no whole triple
    # the queries and the grid before the triangle count; the triangle count before the host index check and before "nothing to do"
    assert call(lib, "m2s_closest_points", **empty, queries=None) == (BAD, "queries is NULL")
    assert call(lib, "m2s_closest_points", **empty, n=0) == (EMPTY, MSG_EMPTY_CLOSEST)
    assert call(lib, "m2s_grid_closest_points", **empty, grid=None) == (BAD, "grid is NULL")
    assert call(lib, "m2s_grid_closest_points", **empty, opts=opts(x_begin=2, x_end=2)) == (EMPTY, MSG_EMPTY_CLOSEST)
    assert call(lib, "m2s_closest_points", indices=p(OOB32), n=0) == (BAD, MSG_OOB5)
    assert call(lib, "m2s_grid_closest_points", indices=p(OOB32), opts=opts(x_begin=2, x_end=2)) == (BAD, MSG_OOB5)
    # nothing to do, no device needed
    assert call(lib, "m2s_closest_points", n=0) == (OK, "")
    assert call(lib, "m2s_closest_points", n=0, queries=None) == (OK, "")
    assert call(lib, "m2s_grid_closest_points", opts=opts(x_begin=2, x_end=2)) == (OK, "")


def test_winding_numbers(lib):
    both_null = "winding_out and sdf_out are both NULL"
    for name in ("m2s_winding_numbers", "m2s_grid_winding_numbers"):
        assert call(lib, name, winding_out=None, sdf_out=None) == (BAD, both_null)
        assert call(lib, name, beta=0.5) == (BAD, "beta must be >= 1 (or +inf: no expansion is ever used), got 0.5")
        assert call(lib, name, beta=NAN) == (BAD, "beta must be >= 1 (or +inf: no expansion is ever used), got nan")
        assert call(lib, name, beta=-INF) == (BAD, "beta must be >= 1 (or +inf: no expansion is ever used), got -inf")
        assert call(lib, name, beta=0.5, winding_out=None, sdf_out=None) == (BAD, both_null)
    assert call(lib, "m2s_winding_numbers", beta=0.5, queries=None) == (BAD, "beta must be >= 1 (or +inf: no expansion is ever used), got 0.5")
    assert call(lib, "m2s_grid_winding_numbers", beta=0.5, grid=None) == (BAD, "beta must be >= 1 (or +inf: no expansion is ever used), got 0.5")
    assert call(lib, "m2s_winding_numbers", indices=p(OOB32), n=0) == (BAD, MSG_OOB5)
    assert call(lib, "m2s_grid_winding_numbers", indices=p(OOB32), opts=opts(x_begin=2, x_end=2)) == (BAD, MSG_OOB5)
    assert call(lib, "m2s_winding_numbers", n=0, beta=INF) == (OK, "")
    assert call(lib, "m2s_grid_winding_numbers", opts=opts(x_begin=4, x_end=4)) == (OK, "")


def test_winding_of_a_mesh_without_triangles(lib):
    """w = 0 for every query or cell of the slab, written by the host for host memory; signed distances do not exist."""
    empty = dict(n_vertices=0, indices=None, n_indices=0)
    no_sdf = "signed distances on a mesh without triangles"
    w = np.full(5, 7.0, F)
    q = np.zeros((3, 3), F)
    assert call(lib, "m2s_winding_numbers", **empty, queries=p(q), n=3, winding_out=p(w), sdf_out=None) == (OK, "")
    assert w.tolist() == [0, 0, 0, 7, 7]
    assert call(lib, "m2s_winding_numbers", **empty, queries=p(q), n=3, winding_out=p(w)) == (EMPTY, no_sdf)
    assert call(lib, "m2s_winding_numbers", **empty, n=0, winding_out=None) == (EMPTY, no_sdf)
    assert call(lib, "m2s_winding_numbers", **empty, n=0, sdf_out=None) == (OK, "")
    assert call(lib, "m2s_winding_numbers", **empty, queries=None, sdf_out=None) == (BAD, "queries is NULL")      # the queries come first
    assert call(lib, "m2s_winding_numbers", n_indices=2, queries=p(q), n=2, winding_out=p(w[3:]), sdf_out=None, opts=opts()) == (OK, "")
    assert w.tolist() == [0, 0, 0, 0, 0]
    g = grid(count=(4, 2, 2))
    w = np.full(16, 7.0, F)
    assert call(lib, "m2s_grid_winding_numbers", **empty, grid=g, winding_out=p(w), sdf_out=None, opts=opts(x_begin=1, x_end=3)) == (OK, "")
    assert w.tolist() == [7] * 4 + [0] * 8 + [7] * 4
    assert call(lib, "m2s_grid_winding_numbers", **empty, grid=g, winding_out=p(w), sdf_out=None) == (OK, "")
    assert not w.any()
    assert call(lib, "m2s_grid_winding_numbers", **empty, grid=g, winding_out=p(w), opts=opts(x_begin=2, x_end=2)) == (EMPTY, no_sdf)
    assert call(lib, "m2s_grid_winding_numbers", **empty, grid=None, sdf_out=None) == (BAD, "grid is NULL")


def common_opts_cases(what):
    return [
        (dict(opts=opts(x_begin=1)), f"m2s_opts.x_begin / x_end do not apply to {what} calls"),
        (dict(opts=opts(x_end=1)), f"m2s_opts.x_begin / x_end do not apply to {what} calls"),
        (dict(opts=opts(x_period=4)), f"m2s_opts.x_period / peer_out do not apply to {what} calls"),
        (dict(opts=opts(n_peer_out=1)), f"m2s_opts.x_period / peer_out do not apply to {what} calls"),
        (dict(opts=opts(peer_out=(C.c_void_p * 1)(None))), f"m2s_opts.x_period / peer_out do not apply to {what} calls"),
        (dict(opts=opts(mem_kind=2)), "bad mem_kind"),
        (dict(opts=opts(algorithm=2)), "bad algorithm"),
        (dict(opts=opts(x_begin=1, x_period=4, mem_kind=2)), f"m2s_opts.x_begin / x_end do not apply to {what} calls"),
        (dict(opts=opts(x_period=4, mem_kind=2, algorithm=2)), f"m2s_opts.x_period / peer_out do not apply to {what} calls"),
        (dict(opts=opts(mem_kind=2, algorithm=2)), "bad mem_kind"),
    ]


def test_cast_rays(lib):
    name = "m2s_cast_rays"
    rng = "ray range needs t_min <= t_max, neither NaN (got %s)"
    cases = [
        (dict(ropts=ray_opts(size=8)), "m2s_ray_opts.struct_size too small"),
        (dict(ropts=ray_opts(size=0)), "m2s_ray_opts.struct_size too small"),
        (dict(ropts=ray_opts(t_min=2.0, t_max=1.0)), rng % "2, 1"),
        (dict(ropts=ray_opts(t_min=NAN)), rng % "nan, inf"),
        (dict(ropts=ray_opts(t_max=NAN)), rng % "0, nan"),
        (no_outputs(name), "every ray output is NULL"),
        (dict(origins=None), "origins / directions is NULL"),
        (dict(directions=None), "origins / directions is NULL"),
        (dict(n=MANY), "too many rays for one call"),
        # in this order
        (dict(ropts=ray_opts(size=8, t_min=2.0, t_max=1.0)), "m2s_ray_opts.struct_size too small"),
        (dict(ropts=ray_opts(t_min=2.0, t_max=1.0), **no_outputs(name)), rng % "2, 1"),
        (dict(origins=None, **no_outputs(name)), "every ray output is NULL"),
        (dict(origins=None, n=MANY), "origins / directions is NULL"),
        (dict(n=MANY, opts=opts(x_begin=1)), "too many rays for one call"),
        (dict(topology=2, ropts=ray_opts(size=8)), "bad topology 2"),
    ] + common_opts_cases("ray")
    for over, msg in cases:
        assert call(lib, name, **over) == (BAD, msg), over
    assert call(lib, name, indices=p(OOB32), ropts=ray_opts(size=8)) == (BAD, "m2s_ray_opts.struct_size too small")   # before the index check
    assert call(lib, name, indices=p(OOB32), n=0) == (BAD, MSG_OOB5)
    # no rays: nothing is written, so NULL arrays pass; a larger m2s_ray_opts of a later version passes too
    assert call(lib, name, n=0, origins=None, directions=None, **no_outputs(name)) == (OK, "")
    assert call(lib, name, n=0, ropts=ray_opts(size=64)) == (OK, "")
    assert call(lib, name, n=0, n_vertices=0, indices=None, n_indices=0) == (OK, "")


def test_sample_surface(lib):
    name = "m2s_sample_surface"
    cases = [
        (no_outputs(name), "every sampling output is NULL, area_out included"),
        (dict(sopts=sample_opts(size=16)), "m2s_surface_sample_opts.struct_size is not sizeof(m2s_surface_sample_opts)"),
        (dict(sopts=sample_opts(size=32)), "m2s_surface_sample_opts.struct_size is not sizeof(m2s_surface_sample_opts)"),
        (dict(sopts=sample_opts(reserved=1)), "m2s_surface_sample_opts.reserved must be 0"),
        (dict(sopts=sample_opts(first=2 ** 64 - 1), n=1), "first_sample + n_samples overflows 64 bits"),
        (dict(n=MANY), "too many samples for one call"),
        # in this order
        (dict(sopts=sample_opts(size=16), **no_outputs(name)), "every sampling output is NULL, area_out included"),
        (dict(sopts=sample_opts(size=16, reserved=1)), "m2s_surface_sample_opts.struct_size is not sizeof(m2s_surface_sample_opts)"),
        (dict(sopts=sample_opts(reserved=1, first=2 ** 64 - 1)), "m2s_surface_sample_opts.reserved must be 0"),
        (dict(sopts=sample_opts(first=2 ** 64 - 1), n=MANY), "first_sample + n_samples overflows 64 bits"),
        (dict(n=MANY, opts=opts(x_begin=1)), "too many samples for one call"),
        (dict(topology=2, **no_outputs(name)), "bad topology 2"),
    ] + common_opts_cases("sampling")
    for over, msg in cases:
        assert call(lib, name, **over) == (BAD, msg), over
    assert call(lib, name, indices=p(OOB32), n=MANY) == (BAD, "too many samples for one call")       # before the index check
    assert call(lib, name, indices=p(OOB32), n=0) == (BAD, MSG_OOB5)
    assert call(lib, name, sopts=sample_opts(first=2 ** 64 - 2), n=1, n_vertices=0, indices=None, n_indices=0)[0] == EMPTY   # just fits


def test_sampling_a_mesh_without_triangles(lib):
    """The area is 0 and written; no samples is fine, samples are M2S_ERR_EMPTY_MESH; no device is needed."""
    name = "m2s_sample_surface"
    empty = dict(n_vertices=0, indices=None, n_indices=0)
    area = C.c_double(5.0)
    assert call(lib, name, **empty, n=0, area_out=C.pointer(area)) == (OK, "")
    assert area.value == 0.0
    area.value = 5.0
    assert call(lib, name, **empty, n=3, area_out=C.pointer(area)) == (EMPTY, "surface samples of a mesh without area")
    assert area.value == 0.0
    assert call(lib, name, **empty, n=3, area_out=None) == (EMPTY, "surface samples of a mesh without area")
    assert call(lib, name, n_indices=2, n=0, area_out=None) == (OK, "")
    # the index check comes first: a strip of two indices has no triangle, so nothing is read; a bad option still wins
    assert call(lib, name, **empty, n=3, opts=opts(algorithm=2)) == (BAD, "bad algorithm")


def whole_grid_cases(what):
    return [
        (dict(grid=None), "grid is NULL"),
        (dict(grid=grid(count=(4, 0, 2))), "cell_count[1] is 0"),
        (dict(grid=grid(count=(0, 0, 2))), "cell_count[0] is 0"),
        (dict(grid=grid(size=(0, 1, 1))), "cell_size[0] must be positive and finite"),
        (dict(grid=grid(size=(1, -1, 1))), "cell_size[1] must be positive and finite"),
        (dict(grid=grid(size=(1, 1, INF))), "cell_size[2] must be positive and finite"),
        (dict(grid=grid(size=(1, NAN, 1))), "cell_size[1] must be positive and finite"),
        (dict(grid=grid(first=(0, 0, NAN))), "first_cell[2] is not finite"),
        (dict(grid=grid(first=(-INF, 0, 0))), "first_cell[0] is not finite"),
        (dict(grid=grid(count=(0x7FFFFFFF, 1, 1))), "cell_count too large"),
        (dict(grid=grid(count=(2 ** 20, 2 ** 20, 1))), "grid face with 2^32 or more lines (cell_count 1048576 x 1048576 x 1)"),
        (dict(grid=grid(count=(2 ** 12, 2 ** 12, 2 ** 12))), "2^36 or more cells"),
        # in this order: m2s_opts, then the grid cell by cell (count, size, first per axis), then its size
        (dict(grid=grid(count=(4, 0, 2)), opts=opts(algorithm=2)), "bad algorithm"),
        (dict(grid=grid(count=(4, 0, 2), size=(0, 1, 1))), "cell_size[0] must be positive and finite"),
        (dict(grid=grid(count=(0, 2, 2), size=(0, 1, 1))), "cell_count[0] is 0"),
        (dict(grid=grid(size=(1, 0, 1), first=(NAN, 0, 0))), "first_cell[0] is not finite"),
        (dict(grid=grid(count=(0x7FFFFFFF, 1, 1), first=(0, 0, NAN))), "first_cell[2] is not finite"),
    ] + common_opts_cases(what)


def test_voxelize(lib):
    name = "m2s_voxelize"
    all_null = "bits_out, occupancy_out, cells_out and n_set_out are all NULL"
    cases = [
        (no_outputs(name), all_null),
        (dict(vopts=voxel_opts(size=4)), "m2s_voxelize_opts.struct_size is not sizeof(m2s_voxelize_opts)"),
        (dict(vopts=voxel_opts(size=16)), "m2s_voxelize_opts.struct_size is not sizeof(m2s_voxelize_opts)"),
        (dict(vopts=voxel_opts(mode=2)), "bad m2s_voxelize_opts.mode 2"),
        # in this order: the grid pointer, the outputs, the options, m2s_opts and the grid, the mesh
        (dict(grid=None, **no_outputs(name)), "grid is NULL"),
        (dict(vopts=voxel_opts(size=4), **no_outputs(name)), all_null),
        (dict(vopts=voxel_opts(size=4, mode=2)), "m2s_voxelize_opts.struct_size is not sizeof(m2s_voxelize_opts)"),
        (dict(vopts=voxel_opts(mode=2), opts=opts(x_begin=1)), "bad m2s_voxelize_opts.mode 2"),
        (dict(vopts=voxel_opts(mode=2), grid=grid(count=(4, 0, 2))), "bad m2s_voxelize_opts.mode 2"),
        (dict(grid=grid(count=(4, 0, 2)), topology=2), "cell_count[1] is 0"),
        (dict(opts=opts(algorithm=2), vertices=None), "bad algorithm"),
    ] + whole_grid_cases("voxelization")
    for over, msg in cases:
        assert call(lib, name, **over) == (BAD, msg), over
    assert call(lib, name, indices=p(OOB32)) == (BAD, MSG_OOB5)
    assert call(lib, name, indices=p(OOB32), grid=grid(size=(0, 1, 1))) == (BAD, "cell_size[0] must be positive and finite")


def test_narrow_band(lib):
    name = "m2s_narrow_band_sdf"
    all_null = "cells_out, distances_out, bits_out and n_active_out are all NULL"
    neg = "m2s_band_opts.exterior / interior must be >= 0 (+inf allowed)"
    cases = [
        (dict(sign_method=2), "bad sign_method 2"),
        (dict(sign_method=-1), "bad sign_method -1"),
        (dict(bopts=None), "bopts is NULL"),
        (dict(bopts=band_opts(size=8)), "m2s_band_opts.struct_size is not sizeof(m2s_band_opts)"),
        (dict(bopts=band_opts(size=16)), "m2s_band_opts.struct_size is not sizeof(m2s_band_opts)"),
        (dict(bopts=band_opts(exterior=-1.0)), neg),
        (dict(bopts=band_opts(interior=-0.5)), neg),
        (dict(bopts=band_opts(exterior=NAN)), neg),
        (dict(bopts=band_opts(interior=NAN)), neg),
        (no_outputs(name), all_null),
        # in this order: the grid pointer, the sign method, the band options, the outputs, m2s_opts and the grid, the mesh
        (dict(grid=None, sign_method=2), "grid is NULL"),
        (dict(sign_method=2, bopts=None), "bad sign_method 2"),
        (dict(bopts=None, **no_outputs(name)), "bopts is NULL"),
        (dict(bopts=band_opts(size=8, exterior=-1.0)), "m2s_band_opts.struct_size is not sizeof(m2s_band_opts)"),
        (dict(bopts=band_opts(exterior=-1.0), **no_outputs(name)), neg),
        (dict(opts=opts(x_begin=1), **no_outputs(name)), all_null),
        (dict(grid=grid(count=(4, 0, 2)), topology=2), "cell_count[1] is 0"),
        (dict(opts=opts(algorithm=2), vertices=None), "bad algorithm"),
    ] + whole_grid_cases("narrow-band")
    for over, msg in cases:
        assert call(lib, name, **over) == (BAD, msg), over
    assert call(lib, name, indices=p(OOB32)) == (BAD, MSG_OOB5)
    assert call(lib, name, indices=p(OOB32), bopts=band_opts(exterior=INF, interior=INF), grid=None) == (BAD, "grid is NULL")


@pytest.mark.parametrize("name", RESIDENT)
def test_null_mesh_handle(lib, name):
    assert call(lib, name, mesh=None) == (BAD, "mesh is NULL")
    # ... before anything else is looked at
    assert call(lib, name, mesh=None, opts=opts(algorithm=2, x_begin=1), **no_outputs(name)) == (BAD, "mesh is NULL")


def test_a_success_clears_the_last_error(lib):
    assert call(lib, "m2s_closest_points", topology=2)[0] == BAD
    assert call(lib, "m2s_closest_points", n=0) == (OK, "")


# ---- the resident forms: an m2s_mesh needs a device ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes(lib):
    """(a mesh of one triangle, a mesh without triangles) on device 0."""
    handles = []
    for n_vertices in (3, 0):
        h = C.c_void_p()
        rc = lib.m2s_mesh_create(p(V), n_vertices, None, 0, 4, 0, None, C.byref(h))
        assert rc == OK, lib.m2s_last_error()
        handles.append(h)
    yield handles
    for h in handles:
        lib.m2s_mesh_destroy(h)


def other_device():
    return opts(device=1 << 20)


MSG_DEVICE = "mesh lives on device 0, call asked for 1048576"


@pytest.mark.gpu
def test_resident_closest_points(lib, meshes):
    one, none = meshes
    all_null = "triangle_out, point_out and distance_out are all NULL"
    q, g = "m2s_mesh_closest_points", "m2s_mesh_grid_closest_points"
    for name in (q, g):
        assert call(lib, name, mesh=one, **no_outputs(name)) == (BAD, all_null)
        assert call(lib, name, mesh=none) == (EMPTY, MSG_EMPTY_CLOSEST)
        assert call(lib, name, mesh=none, **no_outputs(name)) == (BAD, all_null)
        # the options of the call are resolved after the checks and the early returns
        assert call(lib, name, mesh=none, opts=other_device()) == (EMPTY, MSG_EMPTY_CLOSEST)
        assert call(lib, name, mesh=one, opts=other_device()) == (BAD, MSG_DEVICE)
    for over, msg in QUERY_CASES:
        assert call(lib, q, mesh=one, **over) == (BAD, msg)
    assert call(lib, q, mesh=one, queries=None, **no_outputs(q)) == (BAD, all_null)
    assert call(lib, q, mesh=none, queries=None) == (BAD, "queries is NULL")
    assert call(lib, q, mesh=none, n=0) == (EMPTY, MSG_EMPTY_CLOSEST)
    assert call(lib, q, mesh=one, n=0, opts=other_device()) == (OK, "")
    for over, msg in GRID_CASES:
        assert call(lib, g, mesh=one, **over) == (BAD, msg)
    assert call(lib, g, mesh=none, grid=None) == (BAD, "grid is NULL")
    assert call(lib, g, mesh=one, opts=opts(x_begin=2, x_end=2, device=1 << 20)) == (OK, "")
    # n = 1 on the device
    tri, pt, d = np.full(1, 9, np.uint32), np.zeros(3, F), np.zeros(1, F)
    assert call(lib, q, mesh=one, triangle_out=p(tri), point_out=p(pt), distance_out=p(d)) == (OK, "")
    assert tri[0] == 0 and np.allclose(pt, [0.25, 0.25, 0.0], atol=1e-6) and d[0] == 1.0
    tri[0], d[0] = 9, 0
    g1 = grid(count=(1, 1, 1), first=(0.25, 0.25, 1.0))
    assert call(lib, g, mesh=one, grid=g1, triangle_out=p(tri), point_out=p(pt), distance_out=p(d)) == (OK, "")
    assert tri[0] == 0 and np.allclose(pt, [0.25, 0.25, 0.0], atol=1e-6) and d[0] == 1.0


@pytest.mark.gpu
def test_resident_winding_numbers(lib, meshes):
    one, none = meshes
    q, g = "m2s_mesh_winding_numbers", "m2s_mesh_grid_winding_numbers"
    no_sdf = "signed distances on a mesh without triangles"
    for name in (q, g):
        assert call(lib, name, mesh=one, winding_out=None, sdf_out=None) == (BAD, "winding_out and sdf_out are both NULL")
        assert call(lib, name, mesh=one, beta=0.5) == (BAD, "beta must be >= 1 (or +inf: no expansion is ever used), got 0.5")
        assert call(lib, name, mesh=none) == (EMPTY, no_sdf)
        # the options of the call are resolved before the mesh without triangles returns
        assert call(lib, name, mesh=none, opts=other_device()) == (BAD, MSG_DEVICE)
        assert call(lib, name, mesh=one, opts=other_device()) == (BAD, MSG_DEVICE)
    for over, msg in QUERY_CASES:
        assert call(lib, q, mesh=one, **over) == (BAD, msg)
    assert call(lib, q, mesh=one, n=MANY, opts=other_device()) == (BAD, "too many queries for one call")
    assert call(lib, q, mesh=one, n=0, opts=other_device()) == (BAD, MSG_DEVICE)
    assert call(lib, q, mesh=one, n=0) == (OK, "")
    for over, msg in GRID_CASES:
        assert call(lib, g, mesh=one, **over) == (BAD, msg)
    assert call(lib, g, mesh=one, opts=opts(x_begin=2, x_end=2)) == (OK, "")
    # w = 0 of a mesh without triangles, written by the host (no options: host memory)
    w = np.full(3, 7.0, F)
    assert call(lib, q, mesh=none, queries=p(np.zeros((2, 3), F)), n=2, winding_out=p(w), sdf_out=None) == (OK, "")
    assert w.tolist() == [0, 0, 7]
    w = np.full(16, 7.0, F)
    assert call(lib, g, mesh=none, winding_out=p(w), sdf_out=None, opts=opts(x_begin=1, x_end=3, synchronous=1)) == (OK, "")
    assert w.tolist() == [7] * 4 + [0] * 8 + [7] * 4
    # n = 1 on the device: the query sits above the triangle's inside, far below half a turn
    w, s = np.full(1, 7.0, F), np.zeros(1, F)
    assert call(lib, q, mesh=one, winding_out=p(w), sdf_out=p(s)) == (OK, "")
    assert 0 < abs(w[0]) < 0.5 and s[0] == 1.0
    w[0], s[0] = 7, 0
    g1 = grid(count=(1, 1, 1), first=(0.25, 0.25, 1.0))
    assert call(lib, g, mesh=one, grid=g1, winding_out=p(w), sdf_out=p(s)) == (OK, "")
    assert 0 < abs(w[0]) < 0.5 and s[0] == 1.0


@pytest.mark.gpu
def test_resident_cast_rays(lib, meshes):
    one, none = meshes
    name = "m2s_mesh_cast_rays"
    cases = [
        (dict(ropts=ray_opts(size=8)), "m2s_ray_opts.struct_size too small"),
        (dict(ropts=ray_opts(t_min=2.0, t_max=1.0)), "ray range needs t_min <= t_max, neither NaN (got 2, 1)"),
        (no_outputs(name), "every ray output is NULL"),
        (dict(origins=None), "origins / directions is NULL"),
        (dict(n=MANY), "too many rays for one call"),
        (dict(opts=other_device()), MSG_DEVICE),
        (dict(n=0, opts=other_device()), MSG_DEVICE),
        (dict(n=MANY, opts=other_device()), "too many rays for one call"),
    ] + common_opts_cases("ray")
    for over, msg in cases:
        assert call(lib, name, mesh=one, **over) == (BAD, msg), over
    assert call(lib, name, mesh=one, n=0, **no_outputs(name)) == (OK, "")
    t, count = np.zeros(1, F), np.full(1, 9, np.uint32)
    only = {**no_outputs(name), "t_out": p(t), "count_out": p(count)}
    assert call(lib, name, mesh=one, **only) == (OK, "")
    assert abs(t[0] - 1.0) < 1e-6 and count[0] == 1
    assert call(lib, name, mesh=none, **only) == (OK, "")            # a mesh without triangles: no hit
    assert count[0] == 0


@pytest.mark.gpu
def test_resident_sample_surface(lib, meshes):
    one, none = meshes
    name = "m2s_mesh_sample_surface"
    cases = [
        (no_outputs(name), "every sampling output is NULL, area_out included"),
        (dict(sopts=sample_opts(size=16)), "m2s_surface_sample_opts.struct_size is not sizeof(m2s_surface_sample_opts)"),
        (dict(sopts=sample_opts(reserved=1)), "m2s_surface_sample_opts.reserved must be 0"),
        (dict(sopts=sample_opts(first=2 ** 64 - 1)), "first_sample + n_samples overflows 64 bits"),
        (dict(n=MANY), "too many samples for one call"),
        (dict(opts=other_device()), MSG_DEVICE),
        (dict(n=MANY, opts=other_device()), "too many samples for one call"),
    ] + common_opts_cases("sampling")
    for over, msg in cases:
        assert call(lib, name, mesh=one, **over) == (BAD, msg), over
    area = C.c_double(5.0)
    assert call(lib, name, mesh=none, opts=other_device()) == (BAD, MSG_DEVICE)
    assert call(lib, name, mesh=none, n=3, area_out=C.pointer(area)) == (EMPTY, "surface samples of a mesh without area")
    assert area.value == 0.0
    assert call(lib, name, mesh=none, n=0, area_out=C.pointer(area)) == (OK, "")
    pt, tri = np.full(3, 9.0, F), np.full(1, 9, np.uint32)
    only = {**no_outputs(name), "point_out": p(pt), "triangle_out": p(tri), "area_out": C.pointer(area)}
    assert call(lib, name, mesh=one, **only) == (OK, "")
    assert abs(area.value - 0.5) < 1e-6 and tri[0] == 0 and pt[2] == 0 and pt[0] >= 0 and pt[1] >= 0 and pt[0] + pt[1] <= 1


@pytest.mark.gpu
def test_resident_voxelize(lib, meshes):
    one, none = meshes
    name = "m2s_mesh_voxelize"
    cases = [
        (no_outputs(name), "bits_out, occupancy_out, cells_out and n_set_out are all NULL"),
        (dict(vopts=voxel_opts(size=4)), "m2s_voxelize_opts.struct_size is not sizeof(m2s_voxelize_opts)"),
        (dict(vopts=voxel_opts(mode=2)), "bad m2s_voxelize_opts.mode 2"),
        (dict(vopts=voxel_opts(mode=2), opts=other_device()), "bad m2s_voxelize_opts.mode 2"),
        (dict(grid=grid(count=(4, 0, 2)), opts=other_device()), "cell_count[1] is 0"),
        (dict(opts=other_device()), MSG_DEVICE),
    ] + whole_grid_cases("voxelization")
    for over, msg in cases:
        assert call(lib, name, mesh=one, **over) == (BAD, msg), over
    assert call(lib, name, mesh=none, opts=other_device()) == (BAD, MSG_DEVICE)
    g1 = grid(count=(1, 1, 1), first=(0.25, 0.25, 0.0))
    occ, n_set = np.full(1, 9, np.uint8), C.c_uint64(9)
    only = {**no_outputs(name), "occupancy_out": p(occ), "n_set_out": C.pointer(n_set)}
    assert call(lib, name, mesh=one, grid=g1, **only) == (OK, "")
    assert (occ[0], n_set.value) == (1, 1)
    cells = np.zeros(1, np.uint64)
    assert call(lib, name, mesh=one, grid=g1, **{**only, "cells_out": p(cells), "capacity": 0}) == (
        BAD, "cell_capacity 0 is below the number of set cells (*n_set_out)")
    assert call(lib, name, mesh=none, grid=g1, **only) == (OK, "")
    assert (occ[0], n_set.value) == (0, 0)


@pytest.mark.gpu
def test_resident_narrow_band(lib, meshes):
    one, none = meshes
    name = "m2s_mesh_narrow_band_sdf"
    cases = [
        (dict(sign_method=2), "bad sign_method 2"),
        (dict(bopts=None), "bopts is NULL"),
        (dict(bopts=band_opts(size=8)), "m2s_band_opts.struct_size is not sizeof(m2s_band_opts)"),
        (dict(bopts=band_opts(exterior=-1.0)), "m2s_band_opts.exterior / interior must be >= 0 (+inf allowed)"),
        (no_outputs(name), "cells_out, distances_out, bits_out and n_active_out are all NULL"),
        (dict(sign_method=2, opts=other_device()), "bad sign_method 2"),
        (dict(grid=grid(count=(4, 0, 2)), opts=other_device()), "cell_count[1] is 0"),
        (dict(opts=other_device()), MSG_DEVICE),
    ] + whole_grid_cases("narrow-band")
    for over, msg in cases:
        assert call(lib, name, mesh=one, **over) == (BAD, msg), over
    assert call(lib, name, mesh=none, opts=other_device()) == (BAD, MSG_DEVICE)
    g1 = grid(count=(1, 1, 1), first=(0.25, 0.25, 1.0))
    cells, dist, n_active = np.full(1, 9, np.uint64), np.zeros(1, F), C.c_uint64(9)
    only = {**no_outputs(name), "cells_out": p(cells), "distances_out": p(dist), "n_active_out": C.pointer(n_active), "sign_method": 1}
    assert call(lib, name, mesh=one, grid=g1, bopts=band_opts(exterior=2.0, interior=2.0), **only) == (OK, "")
    assert (n_active.value, cells[0], abs(dist[0])) == (1, 0, 1.0)
    assert call(lib, name, mesh=one, grid=g1, bopts=band_opts(exterior=2.0, interior=2.0), **{**only, "capacity": 0}) == (
        BAD, "capacity 0 is below the number of active cells (*n_active_out)")
    assert call(lib, name, mesh=one, grid=g1, bopts=band_opts(exterior=0.5, interior=0.5), **only) == (OK, "")
    assert n_active.value == 0
