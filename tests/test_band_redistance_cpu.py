"""m2s_band_redistance without a GPU: the exports and the header, every argument check that can be reached without a handle, the
consumers, the model tests/band_redistance_model.py against its own definition (idempotence, frozen cells, zero widths, an empty band, a
band without a sign mask, the truncated iterates), and the accuracy of the definition itself: a sphere against its analytic distance
and the seam of a union against a brute-force distance, where the min rule of m2s_band_csg is off by more than a cell.

The accuracy figures are those of the committed model, measured once and asserted at 1.25 x: nothing is random, so the margin covers
numpy and libm differences only.  DESIGN.md 4.18 records them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_csg_model as cm
import band_redistance_model as rm
from mesh_to_sdf_amd import BandField, RedistanceInfo, _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HZ = rm.CELLS[2]
CELL = (0.125, 0.25, 0.1875)
# max |r - analytic| / hz, measured with this model: the sphere at widths of 3 and 5 cells, the union's seam, the offsets by +-2 hy
SPHERE_ERR = {3: 0.1445, 5: 0.2972}
SEAM_ERR = 0.2071
OFFSET_ERR = {2: 0.1247, -2: 0.1769}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. exports, header, argument checks, consumers ------------------------------------------------------------------------------------------
def test_the_entry_point_is_exported_and_declared(lib):
    assert "m2s_band_redistance" in _lib.EXPORTS and hasattr(lib, "m2s_band_redistance")
    hdr = " ".join(open(os.path.join(ROOT, "include", "m2s.h")).read().split())
    for text in ("typedef struct m2s_band_redistance_opts { uint32_t struct_size; float exterior, interior; uint32_t max_sweeps; } m2s_band_redistance_opts;",
                 "typedef struct m2s_band_redistance_info { uint32_t struct_size, sweeps, converged, reserved; uint64_t n_frozen, n_open, n_candidates; } "
                 "m2s_band_redistance_info;",
                 "int m2s_band_redistance(const m2s_band* band, const m2s_band_redistance_opts* ropts, const m2s_band_field_opts* fopts /* NULL = the widths */, "
                 "const m2s_opts* opts, m2s_band** out, m2s_band_redistance_info* info_out /* may be NULL */);",
                 "m2s_band_field_info, m2s_band_redistance);", "IT MUST BE JACOBI", "K_a = min(ceil(W(L) / h_a) + 1, n_a)"):
        assert text in hdr, text
    assert lib.m2s_version() == 5
    assert C.sizeof(_lib.M2SBandRedistanceOpts) == 16 and C.sizeof(_lib.M2SBandRedistanceInfo) == 40
    for name in ("redistance", "offset"):
        assert hasattr(BandField, name), name
    assert RedistanceInfo._fields == ("sweeps", "converged", "n_frozen", "n_open", "n_candidates")
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    for text in ("struct RedistanceInfo", "BandField redistance(float exterior, float interior, uint32_t max_sweeps = 0, RedistanceInfo* info = nullptr)"):
        assert text in hpp, text
    for doc, text in (("README.md", "redistance"), ("DESIGN.md", "4.18")):
        assert text in open(os.path.join(ROOT, doc)).read(), doc


def test_the_call_rejects_what_needs_no_handle(lib):
    BAD = _lib.ERR_BAD_ARG
    SENTINEL = 0x1234
    fake = C.c_void_p(SENTINEL)                   # never dereferenced: every call below fails before it looks at the handle
    good = _lib.M2SBandRedistanceOpts(16, 0.5, 0.5, 0)
    h = C.c_void_p(SENTINEL)
    assert lib.m2s_band_redistance(None, C.byref(good), None, None, C.byref(h), None) == BAD
    assert "band is NULL" in _lib.last_error() and h.value is None             # *out = NULL on every failure
    assert lib.m2s_band_redistance(fake, C.byref(good), None, None, None, None) == BAD and "out is NULL" in _lib.last_error()
    h = C.c_void_p(SENTINEL)
    assert lib.m2s_band_redistance(fake, None, None, None, C.byref(h), None) == BAD and h.value is None
    for ro in ((12, 0.5, 0.5, 0), (0, 0.5, 0.5, 0), (16, -0.5, 0.5, 0), (16, 0.5, -0.0001, 0), (16, float("inf"), 0.5, 0), (16, 0.5, float("nan"), 0)):
        h = C.c_void_p(SENTINEL)
        assert lib.m2s_band_redistance(fake, C.byref(_lib.M2SBandRedistanceOpts(*ro)), None, None, C.byref(h), None) == BAD, ro
        assert h.value is None
    for fo in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
        h = C.c_void_p(SENTINEL)
        assert lib.m2s_band_redistance(fake, C.byref(good), C.byref(_lib.M2SBandFieldOpts(*fo)), None, C.byref(h), None) == BAD, fo
        assert h.value is None
    h = C.c_void_p(SENTINEL)
    assert lib.m2s_band_redistance(fake, C.byref(good), None, None, C.byref(h), C.byref(_lib.M2SBandRedistanceInfo(8))) == BAD and h.value is None
    for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5)):
        o = _lib.M2SOpts()
        o.struct_size, o.device = C.sizeof(o), -1
        setattr(o, field, value)
        h = C.c_void_p(SENTINEL)
        assert lib.m2s_band_redistance(fake, C.byref(good), None, C.byref(o), C.byref(h), None) == BAD, field
        assert h.value is None


@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/band_redistance_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_redistance_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 2. the model against itself -----------------------------------------------------------------------------------------------------------------
def smooth_band(rng, shape, bits=True):
    """The band of a random low-order trigonometric field: long same-sign runs, so the sweeps have somewhere to go."""
    i, j, k = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    a = rng.uniform(0.2, 0.9, 3)
    d = (np.sin(a[0] * i + rng.uniform(0, 6)) + np.sin(a[1] * j + rng.uniform(0, 6)) + np.sin(a[2] * k + rng.uniform(0, 6))).astype(F) * F(0.2)
    d = d.reshape(-1)
    cells = np.flatnonzero((np.abs(d) <= 0.3) & (rng.random(d.size) < 0.9))
    return cm.Band(shape, cells, d[cells], cm.pack_bits(shape, (d < 0).reshape(shape)) if bits else None, 0.75, 0.5)


@pytest.fixture(scope="module")
def sphere():
    return rm.band_of(rm.sphere((0, 0, 0), 0.6), 1.8 * HZ)


@pytest.mark.parametrize("shape", [(7, 9, 11), (5, 3, 70), (3, 65, 1)], ids=lambda n: "x".join(map(str, n)))
def test_the_model_is_idempotent_and_keeps_the_frozen_cells(shape):
    rng = np.random.default_rng(41 + sum(shape))
    for bits in (True, False):
        band = smooth_band(rng, shape, bits)
        act, x, s = cm.dense(band)
        frozen, n_open = rm.frozen_set(act, s)
        for ext, inn in ((0.47, 0.47), (0.47, 0.1), (0.0, 0.3)):
            r, info = rm.redistance(band, CELL, ext, inn)
            assert info.converged == 1 and info.n_frozen == int(frozen.sum()) > 0 and info.n_open == n_open
            ract, rx, rs = cm.dense(r)
            assert (ract & frozen).sum() == frozen.sum()
            assert np.array_equal(rx[frozen].view(np.uint32), x[frozen].view(np.uint32))                  # every bit, -0 included
            assert np.array_equal(rs, s) and np.array_equal(cm.unpack_bits(shape, r.bits), s)            # s on every grid point
            assert (r.bg_out, r.bg_in) == (F(ext), F(inn))
            free = ract & ~frozen
            assert (np.abs(rx[free]) <= np.where(rs[free], F(inn), F(ext))).all() and ((rx[free] < 0) == rs[free]).all()
            # a second pass starts from the same F unless the first one grew two cells of opposite sign next to each other (a sign
            # change between two inactive points, which the definition does not look for); from the same F it ends in the same bits
            again, info2 = rm.redistance(r, CELL, ext, inn)
            if info2.n_frozen == info.n_frozen:
                assert cm.same(again, r)


def test_idempotence_holds_bit_for_bit_on_the_sphere(sphere):
    for cells in (3, 5):
        r, info = rm.redistance(sphere, rm.CELLS, cells * HZ, cells * HZ)
        again, info2 = rm.redistance(r, rm.CELLS, cells * HZ, cells * HZ)
        assert info.converged == 1 == info2.converged and info.n_open == 0 == info2.n_open and cm.same(again, r)
        assert info2.n_frozen == info.n_frozen and info.sweeps <= rm.default_sweeps(cells * HZ, cells * HZ, rm.CELLS, rm.SHAPE) - 8


def test_zero_widths_give_exactly_the_frozen_set(sphere):
    act, x, s = cm.dense(sphere)
    frozen, _ = rm.frozen_set(act, s)
    r, info = rm.redistance(sphere, rm.CELLS, 0.0, 0.0)
    assert np.array_equal(r.cells, np.flatnonzero(frozen.reshape(-1))) and info.n_frozen == r.cells.size and info.converged == 1
    assert np.array_equal(r.distances.view(np.uint32), x.reshape(-1)[r.cells].view(np.uint32))
    assert info.n_candidates > info.n_frozen                              # K = 1: the frozen cells' neighbours are swept, and dropped
    assert (r.bg_out, r.bg_in) == (F(0), F(0))


def test_an_empty_band_and_a_band_without_a_sign_mask():
    shape = (5, 6, 7)
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, (5, 6, 1), dtype=np.uint64).astype(np.uint32)
    r, info = rm.redistance(cm.Band(shape, [], [], bits, 0.5, 0.5), CELL, 0.3, 0.3)
    assert r.cells.size == 0 and info == (0, 1, 0, 0, 0)
    assert np.array_equal(r.bits, cm.pack_bits(shape, cm.unpack_bits(shape, bits)))                      # the sign mask, the bits at k >= nz zero
    r, info = rm.redistance(cm.Band(shape, [], [], None, 0.5, 0.5), CELL, 0.3, 0.3)
    assert r.cells.size == 0 and info == (0, 1, 0, 0, 0) and r.bits is not None and not r.bits.any()     # a result always has a mask
    # without a mask every inactive cell is outside: a lone negative cell has no active neighbour of the other sign, so nothing is frozen
    r, info = rm.redistance(cm.Band(shape, [100], [-0.1], None, 0.5, 0.5), CELL, 0.3, 0.3)
    assert r.cells.size == 0 and info.n_frozen == 0 and info.n_open == 6 and cm.unpack_bits(shape, r.bits).reshape(-1)[100]
    band = smooth_band(rng, shape, bits=False)
    r, info = rm.redistance(band, CELL, 0.3, 0.3)
    assert info.n_frozen > 0 and np.array_equal(cm.unpack_bits(shape, r.bits), cm.dense(band)[2])


def test_a_cap_on_the_sweeps_gives_the_truncated_iterates(sphere):
    full, info = rm.redistance(sphere, rm.CELLS, 3 * HZ, 3 * HZ)
    assert info.sweeps > 3
    sizes = []
    for n in (1, 2, 3):
        r, i = rm.redistance(sphere, rm.CELLS, 3 * HZ, 3 * HZ, max_sweeps=n)
        assert (i.sweeps, i.converged) == (n, 0) and i[2:] == info[2:]
        sizes.append(r.cells.size)
    assert sizes[0] < sizes[1] < sizes[2] < full.cells.size
    r, i = rm.redistance(sphere, rm.CELLS, 3 * HZ, 3 * HZ, max_sweeps=info.sweeps)
    assert cm.same(r, full) and (i.sweeps, i.converged) == (info.sweeps, 0)                # all of them ran, none was seen to change nothing
    r, i = rm.redistance(sphere, rm.CELLS, 3 * HZ, 3 * HZ, max_sweeps=info.sweeps + 1)
    assert cm.same(r, full) and i == info


def test_the_update_is_the_exact_distance_along_an_axis():
    """The slab |x - 2| <= 1 on cells of 0.5 (tests/c/band_redistance_smoke.c): every sum is exact, so the result is |x - 2| - 1."""
    shape = (8, 8, 8)
    L = np.arange(512)
    value = (np.abs(F(0.25) + F(0.5) * (L // 64).astype(F) - F(2)) - F(1)).astype(F)
    keep = ((L // 64) >= 1) & ((L // 64) <= 6)
    band = cm.Band(shape, L[keep], value[keep], None, 0.75, 0.75)
    r, info = rm.redistance(band, (0.5, 0.5, 0.5), 1.0, 1.0)
    assert info == (1, 1, 256, 0, 512) and np.array_equal(r.cells, L) and np.array_equal(r.distances, value)
    r, info = rm.redistance(band, (0.5, 0.5, 0.5), 0.25, 0.25)
    assert info.sweeps == 1 and info.converged == 1 and r.cells.size == 256                 # the one sweep's 0.75 lies beyond the widths


# ---- 3. accuracy of the definition on a sphere ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [3, 5])
def test_accuracy_on_a_sphere(sphere, cells):
    analytic = rm.sphere((0, 0, 0), 0.6)
    r, info = rm.redistance(sphere, rm.CELLS, cells * HZ, cells * HZ)
    err = np.abs(r.distances.astype(np.float64) - analytic.reshape(-1)[r.cells]).max() / HZ
    print(f"sphere, {cells} cells: max error {err:.4f} cells, {info}, {r.cells.size} cells of {info.n_candidates} candidates")
    assert info.converged == 1 and err <= 1.25 * SPHERE_ERR[cells]
    assert r.cells.size > sphere.cells.size


@pytest.mark.parametrize("cells", [2, -2])
def test_accuracy_of_an_offset_sphere(cells):
    """+-2 cells of hy = 0.04 and not of hz: the grid reaches 0.70 in y, so the sphere of radius 0.6 grown by 2 hz would leave it."""
    analytic = rm.sphere((0, 0, 0), 0.6)
    dist = float(F(cells * rm.CELLS[1]))
    r, info = rm.offset(rm.band_of(analytic, 4 * HZ), rm.CELLS, dist, 3 * HZ, 3 * HZ)
    err = np.abs(r.distances.astype(np.float64) - (analytic.reshape(-1)[r.cells] - dist)).max() / HZ
    print(f"offset by {cells} hy: max error {err:.4f} cells, {info}")
    assert info.converged == 1 and info.n_open == 0 and err <= 1.25 * OFFSET_ERR[cells]


# ---- 4. the seam ------------------------------------------------------------------------------------------------------------------------------
def brute_nearest(points, queries, chunk=512):
    """The distance from every query to its nearest point, every pair evaluated: the nearest by |p|^2 - 2 q.p (one product per chunk),
    its distance from the difference itself."""
    p2 = (points * points).sum(1)
    out = np.empty(len(queries))
    for at in range(0, len(queries), chunk):
        q = queries[at:at + chunk]
        best = points[(p2[None, :] - 2.0 * (q @ points.T)).argmin(1)]
        out[at:at + chunk] = np.sqrt(((q - best) ** 2).sum(1))
    return out


def nearest(points, queries, cell=0.15, stride=96):
    """The same distances as brute_nearest(points, queries), with fewer pairs.  One point in `stride` gives every query an upper
    bound; the queries of one cube of side `cell` then meet only the points of the box around them that the largest bound of the cube
    reaches, which holds each one's nearest point."""
    bound = brute_nearest(points[::stride], queries)
    pts = points[np.argsort(points[:, 0])]
    key = np.floor(queries / cell).astype(np.int64) + 512
    key = (key[:, 0] * 1024 + key[:, 1]) * 1024 + key[:, 2]
    order = np.argsort(key, kind="stable")
    starts = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1], True])
    out = np.empty(len(queries))
    for g in range(len(starts) - 1):
        idx = order[starts[g]:starts[g + 1]]
        q = queries[idx]
        reach = bound[idx].max() * (1 + 1e-9)
        lo, hi = q.min(0) - reach, q.max(0) + reach
        first, last = np.searchsorted(pts[:, 0], [lo[0], hi[0]])
        c = pts[first:last]
        c = c[(c[:, 1] >= lo[1]) & (c[:, 1] <= hi[1]) & (c[:, 2] >= lo[2]) & (c[:, 2] <= hi[2])]
        out[idx] = brute_nearest(c, q)
    return out


def test_the_seam_of_a_union():
    """Two spheres whose surfaces cross.  Inside the union, near the seam, min(dA, dB) is the distance to a part of a sphere that lies
    inside the other one and is no surface of the union: the min rule is off by more than a cell there.  The reference is the distance
    to 150 000 Fibonacci points per sphere that lie outside the other sphere (their spacing, 0.005, is 0.08 cells)."""
    ca, ra, cb, rb = (-0.25, 0.0, 0.0), 0.5, (0.3, 0.05, 0.0), 0.45
    a, b = rm.band_of(rm.sphere(ca, ra), 4 * HZ), rm.band_of(rm.sphere(cb, rb), 4 * HZ)
    union = cm.csg(a, b, cm.UNION)
    red, info = rm.redistance(union, rm.CELLS, 3 * HZ, 3 * HZ)
    pa, pb = rm.fibonacci_sphere(ca, ra, 150000), rm.fibonacci_sphere(cb, rb, 150000)
    pts = np.concatenate([pa[np.linalg.norm(pa - np.array(cb), axis=1) > rb], pb[np.linalg.norm(pb - np.array(ca), axis=1) > ra]])
    centres = np.stack([c.reshape(-1) for c in rm.centres()], 1)
    near = union.cells[np.abs(union.distances) <= F(3 * HZ)]                    # the min rule where it claims to be within the widths
    both = np.union1d(near, red.cells)
    ref = np.zeros(union.total)
    ref[both] = nearest(pts, centres[both])
    dense_u = cm.dense(union)[1].reshape(-1).astype(np.float64)
    err_min = np.abs(np.abs(dense_u[near]) - ref[near]).max() / HZ
    err_red = np.abs(np.abs(red.distances.astype(np.float64)) - ref[red.cells]).max() / HZ
    print(f"seam: min rule {err_min:.4f} cells, redistanced {err_red:.4f} cells, {info}")
    assert info.converged == 1 and info.n_open == 0
    assert err_red < err_min and err_min > 1.0
    assert err_red <= 1.25 * SEAM_ERR
