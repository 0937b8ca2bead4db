"""Ray casts and closest points on the MI355X against float64 geometry (tests/geometry_f64.py): the assertions of tests/test_truth_cpu.py
applied to what the device returns, straight against float64 and not through the float32 twins.  Run with `-m gpu`.

Rays: cast_rays, count_intersections and test_occlusions, the tree walk and the all-pairs form, one-shot and on a resident Mesh, over
[0, inf] and RANGE.  Closest points: closest_points (walk and all pairs), grid_closest_points, and the distances of generate_sdf and
generate_grid_sdf, against the bounds recorded in tests/golden/truth_error.json.  At these sizes (3 000 queries, 9 576 cells, at most
8 000 triangles) the library's own choice is the all-pairs kernels for nearly every first pass (brute.hip query_is_tiny, grid_is_tiny), so
every mesh is run three times, WALKS: as the library chooses, with the walks forced (the query walk; the lane or packet walk of the grid),
and with packet walks over cut lists."""
import numpy as np
import pytest

import geometry_f64 as g64
import ray_model as rm
from mesh_to_sdf_amd import (AccelerationMethod, Grid, Mesh, SignMethod, Topology, _lib, closest_points, generate_grid_sdf, generate_sdf,
                             grid_closest_points, meshes)
from test_closest_cpu import assert_same_closest, closest_oracle
from test_gpu_rays import ONE_SHOT, _all_outputs, _mesh_calls
from test_truth_cpu import (CLOSEST_CASES, GRID, RANGES, RAY_CASES, assert_within_file, check_rays, closest_case, closest_figures,
                            grid_points, ray_case)

F = np.float32
pytestmark = pytest.mark.gpu


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.mark.parametrize("name", list(RAY_CASES))
def test_rays_against_f64(name):
    v, idx, o, d, ref = ray_case(name)   # (asserts the conditions on the inputs before anything is cast)
    topo = Topology.TriangleList(idx)
    worst = [0.0, 0.0]
    with Mesh(v, topo) as m:
        for how, calls in (("one-shot", ONE_SHOT), ("Mesh", _mesh_calls(m))):
            args = (v, topo, o, d) if calls is ONE_SHOT else (o, d)
            for t_min, t_max in RANGES:
                for algorithm in (0, 1):
                    got = _all_outputs(calls, *args, t_min, t_max, algorithm=algorithm)
                    e = check_rays(ref, got, t_min, t_max, f"{name} {how} [{t_min}, {t_max}] algorithm {algorithm}")
                    worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"{name}: |t - t64| <= {worst[0]:.3f} tb, |uv - uv64| <= {worst[1]:.3f} wb")


# how the first pass and the generate calls run: the library's choice (all pairs at these sizes), walks, packet walks over cut lists
WALKS = {"default": {}, "walks": {"M2S_BRUTE_MAX": 0},
         "packets + cut lists": {"M2S_BRUTE_MAX": 0, "M2S_LANE_WALK": 0, "M2S_CUT_MIN_PACKETS": 8, "M2S_QUERY_CUT_MIN": 1, "M2S_GROUP": 0, "M2S_SPLIT": 0}}


@pytest.mark.parametrize("name", list(CLOSEST_CASES))
def test_closest_points_and_distances_against_f64(name):
    v, idx, q, grid = closest_case(name)
    topo = Topology.TriangleList(idx)
    tris = rm.triangles_of(v, idx).astype(np.float64)
    cells = grid_points(grid)
    for what, p, call in (("closest_points", q, lambda **kw: closest_points(v, topo, q, **kw)),
                          ("grid_closest_points", cells, lambda **kw: grid_closest_points(v, topo, grid, **kw))):
        truth = g64.mesh_distance(p, tris)[0]
        dist = None
        for how, knobs in WALKS.items():
            with _lib.knobs(**knobs):
                for algorithm in (0, 1) if how == "default" else (0,):
                    tri, cp, d = (_np(x) for x in call(algorithm=algorithm))
                    tri, cp, d = tri.reshape(-1), cp.reshape(-1, 3), d.reshape(-1)
                    fig = closest_figures(v, idx, p, tri, cp, d, truth)
                    print(f"{name} {what} {how} algorithm {algorithm}:", {k: float(f"{x:.4g}") for k, x in fig.items()})
                    assert_within_file(name, fig, f"{name} {what} {how} algorithm {algorithm}")
                    assert dist is None or np.array_equal(dist.view(np.uint32), d.view(np.uint32)), f"{name} {what} {how} algorithm {algorithm}"
                    dist = d
                # the signed calls return the same distances, so they are never below the truth either
                if what == "closest_points":
                    signed = _np(generate_sdf(v, topo, q, AccelerationMethod.RtreeBvh)).reshape(-1)
                else:
                    signed = _np(generate_grid_sdf(v, topo, grid, SignMethod.Raycast)).reshape(-1)
            assert np.array_equal(np.abs(signed).view(np.uint32), dist.view(np.uint32)), f"{name} {how}: the signed call's |d| against {what}"


@pytest.mark.parametrize("factor", [1.0, 30.0])
def test_long_triangles_about_the_origin_keep_their_nearest(factor):
    """The strip's two 10 x 0.01 triangles have their box centres at 0.0025 and their vertices at 5.  The walks' absolute slack was
    4e-6 x the scale of the CENTRES, 5e-8 for a query near the origin, against roundings of u x 5 = 3e-7 in the distances: a query
    1.24e-5 from the shared diagonal, whose computed distance is 1.0e-7 below the true one, had its nearest triangle pruned by the
    pre-test plane in k_closest and got the other one, 1.5e-3 away (query 2863 of the set).  The slack now takes the scale of the
    vertices, and so does the margin of k_cut.  Walks (the library's choice, forced, and packets over cut lists), all pairs and the CPU
    oracle agree bit for bit, and so do the generate calls."""
    v, idx, q, _ = closest_case("strip")
    v, q = (v * F(factor)).astype(F), (q * F(factor)).astype(F)
    grid = Grid.from_bounding_box(*meshes.extended_bbox(v, 0.1), list(GRID))
    topo = Topology.TriangleList(idx)
    want_q, want_g = closest_oracle(v, idx, q), closest_oracle(v, idx, grid_points(grid))
    for knobs in WALKS.values():
        with _lib.knobs(**knobs):
            for algorithm in (0, 1):
                assert_same_closest(closest_points(v, topo, q, algorithm=algorithm), want_q, f"x {factor} {knobs} queries, algorithm {algorithm}")
                got = grid_closest_points(v, topo, grid, algorithm=algorithm)
                assert_same_closest(tuple(np.asarray(x).reshape(w.shape) for x, w in zip(got, want_g)), want_g, f"x {factor} {knobs} grid, algorithm {algorithm}")
            sdf = _np(generate_sdf(v, topo, q, AccelerationMethod.RtreeBvh)).reshape(-1)
            gsdf = _np(generate_grid_sdf(v, topo, grid, SignMethod.Raycast)).reshape(-1)
        assert np.array_equal(np.abs(sdf).view(np.uint32), want_q[2].view(np.uint32)), f"x {factor} {knobs}: generate_sdf"
        assert np.array_equal(np.abs(gsdf).view(np.uint32), want_g[2].view(np.uint32)), f"x {factor} {knobs}: generate_grid_sdf"


@pytest.mark.parametrize("name", ["strip", "blob-768-far", "random slivers", "cube"])
def test_vertex_scale_word(name):
    """scene[8], the scale of the walks' slack: the largest |coordinate| of the triangle boxes, i.e. of the vertices plus the boxes' 1e-4
    padding, and never below scene[6], the scale of the box centres that tests/test_gpu_bounds.py checks the pruning comparison with."""
    v, idx, _, _ = closest_case(name)
    with Mesh(v, Topology.TriangleList(idx)) as m:
        scene = m.debug_arrays()["scene"]
    assert scene.size == 9
    centres, vertices = (float(scene[k:k + 1].view(F)[0]) for k in (6, 8))
    vmax = float(np.abs(v[np.unique(idx)]).max())
    print(f"{name}: centres {centres!r}, vertices {vertices!r}, max |vertex| {vmax!r}")
    assert vmax <= vertices <= vmax * (1 + 2.0 ** -22) + 1.01e-4 and centres <= vertices
