"""Grid queries (include/m2s.h m2s_sample_grid / m2s_raymarch_grid) without a GPU: the test oracle (tests/grid_query_model.py) against
a scalar line-by-line transliteration of the shader and against fields whose answer is known; the argument checks that fail before
any device work; the C and C++ declarations compile with -Wall -Werror."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import grid_query_model as gqm
from mesh_to_sdf_amd import M2SPanic, SampleMode, _lib, raymarch_grid, sample_grid
from mesh_to_sdf_amd.api import Grid

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a scalar transliteration of draw_raymarching.wgsl, one f32 operation per step -------------------------------------------------
class Scalar:
    def __init__(self, q, d, mode, iso, outside):
        self.q, self.d, self.mode, self.iso, self.outside = q, d, mode, F(iso), F(outside)

    def get_distance(self, c):                                       # :92-99
        q = self.q
        x, y, z = (min(max(int(c[k]), 0), int(q.n[k]) - 1) for k in range(3))
        return self.d[z + y * int(q.n[2]) + x * int(q.n[2]) * int(q.n[1])] - self.iso

    def sdf_grid(self, p):                                           # :118-200
        q = self.q
        if any(np.isnan(v) for v in p):
            return gqm.QNAN
        if any(p[k] < q.start[k] for k in range(3)) or any(p[k] > q.end[k] for k in range(3)):
            return self.outside
        if self.mode == gqm.SNAP:
            idx = [np.floor((p[k] - (q.start[k] - q.cs[k] * F(0.5))) / q.cs[k]) for k in range(3)]
            return self.get_distance(idx)
        ci = [(p[k] - q.start[k]) / q.cs[k] for k in range(3)]
        fr = [ci[k] - np.floor(ci[k]) for k in range(3)]
        idx = [int(np.floor(ci[k])) for k in range(3)]

        def g(dx, dy, dz):
            return self.get_distance((idx[0] + dx, idx[1] + dy, idx[2] + dz))

        if self.mode == gqm.TRILINEAR:
            one = F(1)
            c_x00 = g(0, 0, 0) * (one - fr[0]) + g(1, 0, 0) * fr[0]
            c_x01 = g(0, 0, 1) * (one - fr[0]) + g(1, 0, 1) * fr[0]
            c_x10 = g(0, 1, 0) * (one - fr[0]) + g(1, 1, 0) * fr[0]
            c_x11 = g(0, 1, 1) * (one - fr[0]) + g(1, 1, 1) * fr[0]
            c_xy0 = c_x00 * (one - fr[1]) + c_x10 * fr[1]
            c_xy1 = c_x01 * (one - fr[1]) + c_x11 * fr[1]
            return c_xy0 * (one - fr[2]) + c_xy1 * fr[2]
        bary, v2, v3 = self.tetra(fr)
        samples = (g(0, 0, 0), g(*v2), g(*v3), g(1, 1, 1))
        return ((bary[0] * samples[0] + bary[1] * samples[1]) + bary[2] * samples[2]) + bary[3] * samples[3]

    @staticmethod
    def tetra(f):                                                    # :585-640
        r, g, b = f
        one = F(1)
        out = ((F(0),) * 4, (0, 0, 0), (0, 0, 0))
        if g >= b and b >= r:
            out = ((one - g, g - b, b - r, r), (0, 1, 0), (0, 1, 1))
        if b > r and r > g:
            out = ((one - b, b - r, r - g, g), (0, 0, 1), (1, 0, 1))
        if b > g and g >= r:
            out = ((one - b, b - g, g - r, r), (0, 0, 1), (0, 1, 1))
        if r >= g and g > b:
            out = ((one - r, r - g, g - b, b), (1, 0, 0), (1, 1, 0))
        if g > r and r >= b:
            out = ((one - g, g - r, r - b, b), (0, 1, 0), (1, 1, 0))
        if r >= b and b >= g:
            out = ((one - r, r - b, b - g, g), (1, 0, 0), (1, 0, 1))
        return out

    def estimate_normal(self, p):                                    # :202-209
        e = self.q.eps
        x, y, z = p
        v = (self.sdf_grid((x + e, y, z)) - self.sdf_grid((x - e, y, z)),
             self.sdf_grid((x, y + e, z)) - self.sdf_grid((x, y - e, z)),
             self.sdf_grid((x, y, z + e)) - self.sdf_grid((x, y, z - e)))
        if any(np.isnan(c) for c in p):
            return (gqm.QNAN,) * 3
        ln = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        if ln == 0:
            return (F(0),) * 3
        return tuple(c / ln for c in v)

    def sdf_3d(self, eye, ray, max_steps):                           # :265-287 -> (pos, dist, steps, hit)
        q = self.q
        eps = q.eps
        if any(np.isnan(v) for v in tuple(eye) + tuple(ray)):
            return (gqm.QNAN,) * 3, gqm.QNAN, 0, False
        pos = tuple(eye)
        if any(eye[k] < q.start[k] for k in range(3)) or any(eye[k] > q.end[k] for k in range(3)):
            tmin = [(q.start[k] - eye[k]) / ray[k] for k in range(3)]
            tmax = [(q.end[k] - eye[k]) / ray[k] for k in range(3)]
            t1 = [np.fmin(tmin[k], tmax[k]) for k in range(3)]
            t2 = [np.fmax(tmin[k], tmax[k]) for k in range(3)]
            t_near = np.fmax(np.fmax(t1[0], t1[1]), t1[2])
            t_far = np.fmin(np.fmin(t2[0], t2[1]), t2[2])
            if t_near > t_far:
                return (F(0),) * 3, F(1), 0, False
            pos = tuple(eye[k] + (t_near + eps) * ray[k] for k in range(3))
        dist, steps = F(0), 0
        for _ in range(max_steps):
            dist = self.sdf_grid(pos)
            if dist < eps:
                break
            pos = tuple(pos[k] + ray[k] * dist for k in range(3))
            steps += 1
        return pos, dist, steps, bool(dist < eps)


def _random_grid(seed, count=(5, 4, 6)):
    rng = np.random.default_rng(seed)
    q = gqm.GridQ(rng.uniform(-2, 2, 3), rng.uniform(0.05, 0.7, 3), count)
    d = rng.uniform(-1, 1, int(np.prod(count))).astype(F)
    return q, d


def _points(q, rng, n, scale=1.3):
    lo, hi = q.start.astype(np.float64), q.end.astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * scale
    return rng.uniform(mid - half, mid + half, (n, 3)).astype(F)


@pytest.mark.parametrize("mode", [gqm.SNAP, gqm.TRILINEAR, gqm.TETRAHEDRAL])
def test_model_equals_scalar_transliteration(mode):
    rng = np.random.default_rng(10 + mode)
    with np.errstate(all="ignore"):
        for seed in range(3):
            q, d = _random_grid(seed)
            pts = _points(q, rng, 1000)
            pts[::97] = q.end                                        # on the upper faces
            pts[1::101, 1] = np.nan
            for iso in (0.0, 0.05):
                s = Scalar(q, d, mode, iso, 100.0)
                want = np.array([s.sdf_grid(tuple(p)) for p in pts], F)
                assert gqm.same_bits(gqm.sample(q, d, pts, mode, iso), want)
                wn = np.array([s.estimate_normal(tuple(p)) for p in pts[:300]], F)
                assert gqm.same_bits(gqm.normal(q, d, pts[:300], mode, iso), wn)
            s = Scalar(q, d, mode, 0.0, 100.0)
            o = _points(q, rng, 200, 3.0)
            o[:50] = _points(q, rng, 50, 0.8)                         # rays starting inside
            r = rng.normal(size=(200, 3)).astype(F)
            r /= np.linalg.norm(r, axis=1, keepdims=True).astype(F)
            r[::7, 0] = 0                                            # zero direction components
            r[::11, 1:] = 0
            d_sdf = (np.linalg.norm(_cell_centres(q), axis=1) - 0.6).astype(F)   # a sphere, so rays hit
            s = Scalar(q, d_sdf, mode, 0.0, 100.0)
            hit, steps, is_hit, nrm = gqm.raymarch(q, d_sdf, o, r, mode, max_steps=40, normals=True)
            for i in range(200):
                pos, dist, st, h = s.sdf_3d(tuple(o[i]), tuple(r[i]), 40)
                assert gqm.same_bits(hit[i], np.array(list(pos) + [dist], F)), i
                assert steps[i] == st and is_hit[i] == h
                want_n = s.estimate_normal(pos) if h else (F(0),) * 3
                assert gqm.same_bits(nrm[i], np.array(want_n, F))


def _cell_centres(q):
    ix, iy, iz = np.meshgrid(*[np.arange(n) for n in q.n], indexing="ij")
    idx = np.stack([ix, iy, iz], -1).reshape(-1, 3)
    return (q.start + idx.astype(F) * q.cs).astype(F)


# ---- fields whose answer is known --------------------------------------------------------------------------------------------
def test_affine_field_is_exact_and_snap_returns_the_nearest_centre():
    q = gqm.GridQ([0.5, 1.0, -2.0], [0.5, 0.25, 1.0], [8, 8, 8])     # dyadic: every operation below is exact
    a, b, c, k = F(2), F(-3), F(0.5), F(1.25)
    cc = _cell_centres(q)
    d = (a * cc[:, 0] + b * cc[:, 1] + c * cc[:, 2] + k).astype(F)
    rng = np.random.default_rng(3)
    cell = rng.integers(0, 7, (500, 3))
    frac = rng.integers(0, 8, (500, 3)) / 8.0
    p = (q.start + (cell + frac) * q.cs).astype(F)
    want = a * p[:, 0] + b * p[:, 1] + c * p[:, 2] + k
    for mode in (gqm.TRILINEAR, gqm.TETRAHEDRAL):
        assert np.array_equal(gqm.sample(q, d, p, mode), want)
        assert np.array_equal(gqm.sample(q, d, p, mode, iso=0.5), want - F(0.5))
    # snap: the cell whose centre is nearest (no point on a cell boundary here)
    nearest = np.round((p - q.start) / q.cs).astype(np.int64)
    off = gqm.cell_off(q, nearest[:, 0], nearest[:, 1], nearest[:, 2])
    keep = np.all(np.abs(frac - 0.5) > 1e-9, axis=1)
    assert np.array_equal(gqm.sample(q, d, p[keep], gqm.SNAP), d[off[keep]])
    # the gradient of an affine field: every normal points along (a, b, c) away from the clamped border
    inner = np.all((cell >= 1) & (cell <= 5), axis=1)
    n = gqm.normal(q, d, p[inner], gqm.TRILINEAR)
    g = np.array([a, b, c], np.float64)
    assert np.allclose(n, g / np.linalg.norm(g), atol=1e-5)


def test_every_tetrahedral_case_is_hit_and_ties_go_to_the_last():
    vals = [F(0.1), F(0.4), F(0.7)]
    import itertools
    fx, fy, fz = (np.array(v, F) for v in zip(*itertools.permutations(vals)))
    _, _, _, case = gqm.tetra_cases(fx, fy, fz)
    assert sorted(case.tolist()) == [1, 2, 3, 4, 5, 6]
    h = F(0.5)
    ties = {  # (fx, fy, fz) -> the case that wins
        (h, h, h): 6,        # cases 1 and 6 match
        (F(0.2), h, h): 1,   # y = z > x
        (h, F(0.2), h): 6,   # x = z > y: case 6 (not 2 or 3)
        (h, h, F(0.2)): 4,   # x = y > z
        (h, F(0.2), F(0.2)): 6,
        (F(0.2), h, F(0.2)): 5,
        (F(0.2), F(0.2), h): 3,
    }
    for (x, y, z), want in ties.items():
        assert gqm.tetra_cases(np.array([x]), np.array([y]), np.array([z]))[3][0] == want, (x, y, z)


def test_box_faces_and_clamped_reads():
    q = gqm.GridQ([0, 0, 0], [1, 1, 1], [3, 3, 3])                 # start 0, end 3: the last centre is 2
    d = np.arange(27, dtype=F)
    out = F(-7)
    below = np.array([[-1e-7, 1, 1], [1, 1, -np.inf], [np.inf, 1, 1], [3.0000002, 1, 1]], F)
    assert np.array_equal(gqm.sample(q, d, below, gqm.TRILINEAR, outside=out), [out] * 4)
    v = gqm.sample(q, d, np.array([[3, 3, 3], [2.5, 2.5, 2.5], [2, 2, 2]], F), gqm.TRILINEAR)
    assert np.array_equal(v, [26, 26, 26])                           # between the last centre and end: the corner cell twice
    assert np.array_equal(gqm.sample(q, d, np.array([[3, 3, 3]], F), gqm.SNAP), [26])
    assert np.array_equal(gqm.sample(q, d, np.array([[0, 0, 0]], F), gqm.SNAP), [0])
    assert np.isnan(gqm.sample(q, d, np.array([[np.nan, -np.inf, 0]], F), gqm.TETRAHEDRAL)[0])
    assert np.isnan(gqm.normal(q, d, np.array([[np.nan, 1, 1]], F))).all()
    assert np.array_equal(gqm.normal(q, np.zeros(27, F), np.array([[1, 1, 1]], F)), [[0, 0, 0]])


def test_raymarch_over_a_sphere_grid():
    n = 32
    q = gqm.GridQ([-1 + 1 / n] * 3, [2 / n] * 3, [n] * 3)
    d = (np.linalg.norm(_cell_centres(q).astype(np.float64), axis=1) - 0.5).astype(F)
    rng = np.random.default_rng(5)
    # a pinhole camera outside the box, looking at the sphere
    u = rng.uniform(-0.1, 0.1, (400, 2))     # every ray meets the sphere
    r = np.stack([u[:, 0], u[:, 1], np.ones(400)], 1)
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)
    o = np.tile(F([0, 0, -3]), (400, 1))
    hit, steps, is_hit, nrm = gqm.raymarch(q, d, o, r, normals=True)
    assert is_hit.all() and (steps > 0).all()
    assert np.all(np.abs(np.linalg.norm(hit[:, :3], axis=1) - 0.5) < 2 / n)   # within one cell of the sphere
    assert np.all(np.einsum("ij,ij->i", nrm, hit[:, :3]) > 0)                 # outward normals
    # rays that miss the box: (0, 0, 0, 1), no steps
    m, ms, mh = gqm.raymarch(q, d, np.array([[0, 0, -3], [5, 5, 5]], F), np.array([[1, 0, 0], [1, 0, 0]], F))
    assert np.array_equal(m, [[0, 0, 0, 1]] * 2) and not ms.any() and not mh.any()
    # axis-parallel rays (zero direction components) from outside, and from inside
    ap_o = np.array([[0, 0, -3], [-3, 0.1, 0], [0.1, 3, 0.05], [0, 0, 0.9]], F)
    ap_r = np.array([[0, 0, 1], [1, 0, 0], [0, -1, 0], [0, 0, -1]], F)
    h2, s2, i2 = gqm.raymarch(q, d, ap_o, ap_r)
    assert i2.all() and np.all(np.abs(np.linalg.norm(h2[:, :3], axis=1) - 0.5) < 2 / n)
    # a ray starting inside the sphere is a hit at once; a NaN ray is NaN x 4 with no step
    h3, s3, i3 = gqm.raymarch(q, d, np.array([[0, 0, 0], [np.nan, 0, 0]], F), np.array([[1, 0, 0], [1, 0, 0]], F))
    assert i3[0] and s3[0] == 0 and np.isnan(h3[1]).all() and s3[1] == 0 and not i3[1]
    # max_steps bounds the march
    _, s4, _ = gqm.raymarch(q, d, o[:20], r[:20], max_steps=1)
    assert (s4 <= 1).all()


# ---- argument checks that need no device ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


def test_new_entry_points_are_exported(lib):
    for name in ("m2s_sample_grid", "m2s_raymarch_grid"):
        assert name in _lib.EXPORTS and hasattr(lib, name)


def _so(mode=1, max_steps=100, size=None):
    so = _lib.M2SSampleOpts()
    so.struct_size = C.sizeof(so) if size is None else size
    so.mode, so.iso, so.outside, so.max_steps = mode, 0.0, 100.0, max_steps
    return so


def test_bad_arguments_fail_before_the_device(lib):
    g = Grid.from_bounding_box([0, 0, 0], [1, 1, 1], [4, 4, 4])
    G = C.byref(g._g)
    d = np.zeros(64, F)
    p = np.zeros((4, 3), F)
    v, nrm, hit = np.zeros(4, F), np.zeros((4, 3), F), np.zeros((4, 4), F)
    st = np.zeros(4, np.uint32)
    D, P, V, N, H, S = d.ctypes.data, p.ctypes.data, v.ctypes.data, nrm.ctypes.data, hit.ctypes.data, st.ctypes.data
    BAD = _lib.ERR_BAD_ARG
    sg, rm = lib.m2s_sample_grid, lib.m2s_raymarch_grid
    assert sg(G, D, P, 4, None, None, None, None) == BAD                       # no output at all
    assert rm(G, D, P, P, 4, None, None, None, None, None) == BAD
    assert sg(G, D, None, 4, None, V, N, None) == BAD                          # NULL points, n > 0
    assert rm(G, D, P, None, 4, None, H, S, N, None) == BAD
    assert rm(G, D, None, P, 4, None, H, S, N, None) == BAD
    assert sg(None, D, P, 4, None, V, N, None) == BAD                          # NULL grid / distances
    assert sg(G, None, P, 4, None, V, N, None) == BAD
    assert rm(G, None, P, P, 4, None, H, S, N, None) == BAD
    assert sg(G, D, P, 4, C.byref(_so(mode=3)), V, N, None) == BAD             # bad mode
    assert rm(G, D, P, P, 4, C.byref(_so(mode=-1)), H, S, N, None) == BAD
    assert rm(G, D, P, P, 4, C.byref(_so(max_steps=0)), H, S, N, None) == BAD  # no step
    assert sg(G, D, P, 4, C.byref(_so(size=8)), V, N, None) == BAD             # struct_size
    for count, size in [([4, 0, 4], [0.25] * 3), ([4, 4, 4], [0.25, 0.0, 0.25]), ([4, 4, 4], [0.25, -0.25, 0.25]),
                        ([4, 4, 4], [0.25, np.inf, 0.25]), ([4, 4, 4], [0.25, 0.25, np.nan])]:
        bad = Grid([0, 0, 0], size, count)
        assert sg(C.byref(bad._g), D, P, 4, None, V, N, None) == BAD, (count, size)
        assert rm(C.byref(bad._g), D, P, P, 4, None, H, S, N, None) == BAD, (count, size)
    for field, value in [("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4)]:
        o = _lib.M2SOpts()
        o.struct_size = C.sizeof(o)
        o.device = -1
        setattr(o, field, value)
        assert sg(G, D, P, 4, None, V, N, C.byref(o)) == BAD, field
        assert rm(G, D, P, P, 4, None, H, S, N, C.byref(o)) == BAD, field
    assert sg(G, D, P, 0, None, V, None, None) == _lib.M2S_OK                  # n = 0: nothing to do, no device needed
    assert rm(G, D, P, P, 0, None, H, None, None, None) == _lib.M2S_OK
    with pytest.raises(M2SPanic):
        sample_grid(g, np.zeros(63, F), p)                                     # distances do not match the grid
    with pytest.raises(M2SPanic):
        raymarch_grid(g, d, p, p[:3])
    with pytest.raises(M2SPanic):
        sample_grid(Grid([0, 0, 0], [1, 0, 1], [4, 4, 4]), d, p, mode=SampleMode.Snap)   # a zero cell size


# ---- the declarations compile in C and C++ with -Wall -Werror ---------------------------------------------------------------------
@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/grid_query_smoke.c"), ("g++", "-std=c++17", "tests/cpp/grid_query_tests.cpp")])
def test_declarations_compile(tmp_path, cc, std, src):
    if not shutil.which(cc):
        pytest.skip(f"no {cc}")
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src),
                           "-L", os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64"]
                          + (["-lm"] if cc == "gcc" else []) + ["-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"),
                                                                 "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    assert os.path.exists(exe)
