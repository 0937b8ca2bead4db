"""Winding numbers (include/m2s.h m2s_winding_numbers & co.) without a GPU: the test oracle (tests/winding_model.py) against the
definition's own properties, the model's expansion error E_model(beta) recorded in tests/golden/winding_model_error.json, and the
library's argument checks, which fail before any device work."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import winding_model as wm
from mesh_to_sdf_amd import (Grid, M2SPanic, Topology, _lib, generate_sdf_winding, grid_winding_numbers, meshes, winding_numbers)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "winding_model_error.json")
BETAS = (2.0, 3.0, 4.0)


def fixed_case(holed=False):
    """The fixed test mesh and point set of the recorded figures: a blob of 6,144 triangles (optionally without the triangles above
    z = 0.8) and 3,000 uniform points in 1.8x its box."""
    v, idx = meshes.blob(48, 65)
    lo, hi = meshes.extended_bbox(v, 0.4)
    q = meshes.uniform_queries(lo, hi, 3000)
    if holed:
        idx = wm.holed(v, idx)
    return v, idx, q


def away_from(tris, pts, dist):
    """Points farther than `dist` from every vertex and centroid of the mesh (a cheap 'away from the surface' for fine meshes)."""
    ref = np.concatenate([tris.reshape(-1, 3), tris.mean(1)])
    d2 = ((pts[:, None, :].astype(np.float64) - ref[None]) ** 2).sum(-1).min(1)
    return d2 > dist * dist


# ---- the model against the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["blob", "cube"])
def test_closed_meshes_give_integers(mesh):
    if mesh == "blob":
        v, idx, q = fixed_case()
        clear = 0.1
    else:
        v, idx = meshes.cube(1.0)
        q = meshes.uniform_queries(np.array([-2, -2, -2], F), np.array([2, 2, 2], F), 2000)
        clear = 0.0
    tris = wm.triangles_of(v, idx)
    w = wm.exact_winding(tris, q)
    if mesh == "cube":
        keep = np.abs(np.abs(q).max(1) - 1.0) > 0.05
        inside = np.abs(q).max(1) < 1.0
        assert np.array_equal((w > 0.5)[keep], inside[keep])
    else:
        keep = away_from(tris, q, clear)
    assert keep.sum() > q.shape[0] // 2
    assert np.abs(w[keep] - np.round(w[keep])).max() < 1e-9
    assert set(np.round(w[keep]).astype(int)) == {0, 1}


def test_flipping_every_triangle_negates():
    v, idx, q = fixed_case(holed=True)
    tris = wm.triangles_of(v, idx)
    w = wm.exact_winding(tris, q)
    flipped = wm.exact_winding(tris[:, ::-1], q)
    assert np.abs(w + flipped).max() < 1e-12
    tree, tree_f = wm.Tree(tris), wm.Tree(tris[:, ::-1])
    assert np.abs(wm.tree_winding(tree, q, 3.0) + wm.tree_winding(tree_f, q, 3.0)).max() < 1e-12


def test_single_triangle_on_its_axis():
    R = 0.7
    ang = np.deg2rad([90.0, 210.0, 330.0])
    tri = np.stack([R * np.cos(ang), R * np.sin(ang), np.zeros(3)], -1)[None]
    for h in (0.05, 0.5, 1.0, 7.0):
        want = wm.single_triangle_on_axis(R, h)
        below, above = wm.exact_winding(tri, [[0, 0, -h]])[0], wm.exact_winding(tri, [[0, 0, h]])[0]
        assert abs(below - want) < 1e-7 and abs(above + want) < 1e-7, (h, below, above, want)   # the points are f32
    assert 0.49 < wm.single_triangle_on_axis(R, 1e-6) < 0.5   # a point just off the face sees half the sphere


def test_zero_contribution_rules():
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float64)
    assert wm.exact_winding(tri, [[0.2, 0.2, 0.0]])[0] == 0.0                 # in the plane, inside the triangle: numerator 0
    assert wm.exact_winding(tri, [[5.0, 5.0, 0.0]])[0] == 0.0                 # in the plane, outside
    degenerate = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[1, 2, 3], [1, 2, 3], [4, 4, 4]]], np.float64)
    assert (wm.exact_winding(degenerate, [[0.5, 0.5, 0.5], [3, 1, 2]]) == 0.0).all()
    assert np.isnan(wm.exact_winding(tri, [[np.nan, 0, 1]])[0])
    assert wm.exact_winding(np.zeros((0, 3, 3)), [[0, 0, 0]])[0] == 0.0


def test_tree_with_infinite_beta_is_the_exact_sum():
    v, idx, q = fixed_case()
    tris = wm.triangles_of(v, idx)
    assert np.abs(wm.tree_winding(wm.Tree(tris), q[:500], np.inf) - wm.exact_winding(tris, q[:500])).max() < 1e-12


# ---- the recorded figure --------------------------------------------------------------------------------------------------------
def test_model_error_is_recorded():
    """E_model(beta), the model's own expansion error against its exact sum on the fixed mesh and points, closed and holed, with the
    inside / outside disagreements and the share of points with |w - 1/2| < 0.1; equal to tests/golden/winding_model_error.json."""
    got = {}
    for name, holed in (("closed", False), ("holed", True)):
        v, idx, q = fixed_case(holed)
        tris = wm.triangles_of(v, idx)
        err, w = wm.model_error(tris, q, BETAS)
        tree = wm.Tree(tris)
        disagree = int(((wm.tree_winding(tree, q, 3.0) >= 0.5) != (w >= 0.5)).sum())
        got[name] = {"triangles": int(tris.shape[0]), "points": int(q.shape[0]), "E_model": {str(b): err[b] for b in BETAS},
                     "inside_outside_disagreements_beta_3": disagree, "share_within_0.1_of_half": float((np.abs(w - 0.5) < 0.1).mean())}
        print(name, json.dumps(got[name]))
    want = json.load(open(GOLDEN))
    for name in got:
        assert got[name]["triangles"] == want[name]["triangles"] and got[name]["points"] == want[name]["points"]
        assert got[name]["inside_outside_disagreements_beta_3"] == want[name]["inside_outside_disagreements_beta_3"] == 0
        for b in BETAS:
            assert abs(got[name]["E_model"][str(b)] - want[name]["E_model"][str(b)]) <= 1e-6 * want[name]["E_model"][str(b)]
        assert got[name]["share_within_0.1_of_half"] <= 0.01
    e = got["closed"]["E_model"]
    assert e["2.0"] > e["3.0"] > e["4.0"] > 0


# ---- the library: exports and argument checks that need no device ------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


NAMES = ("m2s_winding_numbers", "m2s_grid_winding_numbers", "m2s_mesh_winding_numbers", "m2s_mesh_grid_winding_numbers")


def test_new_entry_points_are_exported(lib):
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "m2s.h")).read()
    assert "#define M2S_WINDING_BETA_DEFAULT %.1ff" % _lib.WINDING_BETA_DEFAULT in hdr
    assert "#define M2S_VERSION_MINOR 5" in hdr


def test_bad_arguments_fail_before_the_device(lib):
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    q, w, s = np.zeros((4, 3), F), np.zeros(64, F), np.zeros(64, F)
    V, I, Q, W, S = v.ctypes.data, idx.ctypes.data, q.ctypes.data, w.ctypes.data, s.ctypes.data
    BAD = _lib.ERR_BAD_ARG
    wn = lib.m2s_winding_numbers
    assert wn(V, 4, I, 6, 4, 0, Q, 4, 3.0, 0.5, None, None, None) == BAD                  # no output at all
    for beta in (0.5, 0.999, -1.0, 0.0, float("nan"), float("-inf")):
        assert wn(V, 4, I, 6, 4, 0, Q, 4, beta, 0.5, W, S, None) == BAD, beta              # beta < 1 or NaN
        assert "beta" in _lib.last_error()
    assert wn(V, 4, I, 6, 4, 0, None, 4, 3.0, 0.5, W, S, None) == BAD                     # NULL queries, n > 0
    assert wn(V, 4, I, 6, 3, 0, Q, 4, 3.0, 0.5, W, S, None) == BAD                        # index_bytes
    assert wn(V, 4, I, 6, 4, 7, Q, 4, 3.0, 0.5, W, S, None) == BAD                        # topology
    bad_idx = np.array([0, 1, 2, 0, 2, 4], np.uint32)
    assert wn(V, 4, bad_idx.ctypes.data, 6, 4, 0, Q, 4, 3.0, 0.5, W, S, None) == BAD      # vertex index out of range
    assert "out of range" in _lib.last_error()
    assert wn(V, 4, bad_idx.ctypes.data, 6, 4, 1, Q, 4, float("inf"), 0.5, W, None, None) == BAD
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 4, 4])
    gw = lib.m2s_grid_winding_numbers
    assert gw(V, 4, I, 6, 4, 0, C.byref(g._g), 3.0, 0.5, None, None, None) == BAD
    assert gw(V, 4, I, 6, 4, 0, None, 3.0, 0.5, W, S, None) == BAD                        # NULL grid
    assert gw(V, 4, I, 6, 4, 0, C.byref(g._g), 0.9, 0.5, W, S, None) == BAD               # beta
    g0 = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 0, 4])
    assert gw(V, 4, I, 6, 4, 0, C.byref(g0._g), 3.0, 0.5, W, S, None) == BAD              # a zero cell count
    assert gw(V, 4, bad_idx.ctypes.data, 6, 4, 0, C.byref(g._g), 3.0, 0.5, W, S, None) == BAD
    for field, value in (("x_period", 4), ("n_peer_out", 1)):                             # grid-distance features only
        o = _lib.M2SOpts()
        o.struct_size = C.sizeof(_lib.M2SOpts)
        o.device = -1
        o.synchronous = 1
        setattr(o, field, value)
        assert gw(V, 4, I, 6, 4, 0, C.byref(g._g), 3.0, 0.5, W, S, C.byref(o)) == BAD, field
    o = _lib.M2SOpts()
    o.struct_size = C.sizeof(_lib.M2SOpts)
    o.device = -1
    o.x_begin, o.x_end = 3, 9
    assert gw(V, 4, I, 6, 4, 0, C.byref(g._g), 3.0, 0.5, W, S, C.byref(o)) == BAD         # x-slab outside the grid
    assert lib.m2s_mesh_winding_numbers(None, Q, 4, 3.0, 0.5, W, S, None) == BAD
    assert lib.m2s_mesh_grid_winding_numbers(None, C.byref(g._g), 3.0, 0.5, W, S, None) == BAD
    with pytest.raises(M2SPanic):
        winding_numbers(v, Topology.TriangleList(idx), q, beta=0.5)


def test_empty_mesh_without_the_device(lib):
    """No triangles: w = 0 everywhere (host memory: written without any device work); M2S_ERR_EMPTY_MESH only if distances are asked for."""
    v = np.zeros((4, 3), F)
    q = np.ones((5, 3), F)
    w = winding_numbers(v, Topology.TriangleList(np.zeros(0, np.uint32)), q)
    assert w.shape == (5,) and (w == 0).all()
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [3, 2, 2])
    out = np.full(12, 7.0, F)
    grid_winding_numbers(v[:2], Topology.TriangleStrip(), g, x_slab=(1, 2), out=out)
    assert (out[4:8] == 0).all() and (out[:4] == 7.0).all() and (out[8:] == 7.0).all()
    with pytest.raises(M2SPanic) as e:
        generate_sdf_winding(v, Topology.TriangleList(np.zeros(0, np.uint32)), q)
    assert e.value.code == _lib.ERR_EMPTY_MESH


def _compile(tmp_path, cc, std, src, extra=()):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64", *extra,
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_c_declarations_compile(tmp_path, lib):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    assert os.path.exists(_compile(tmp_path, "gcc", "-std=c99", "tests/c/winding_smoke.c", ["-lm"]))


def test_cpp_declarations_compile(tmp_path, lib):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    assert os.path.exists(_compile(tmp_path, "g++", "-std=c++17", "tests/cpp/winding_tests.cpp"))
