"""m2s_band_components and m2s_band_select without a GPU: the model tests/band_components_model.py against scipy.ndimage.label (where
scipy imports) and against a second, independent pure-Python flood fill; the model on two spheres' bands (two components; erasing the
small one clears exactly its solid interior; erasing nothing is the identity) and on a shell whose inner band is erased (the cavity
limit include/m2s.h documents, pinned); every argument check that is decided before device work and needs no handle; the exports, the
header's declarations and struct sizes, and the C and C++ consumers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_components_model as ccm
import band_csg_model as cm
from mesh_to_sdf_amd import BandField, Components, Connectivity, SelectInfo, _lib
from mesh_to_sdf_amd import api

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTURE_RANK = {6: 1, 18: 2, 26: 3}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        _lib.build()
    return _lib.lib()


# ---- 1. the model against scipy and against a pure-Python flood fill --------------------------------------------------------------------
def random_masks():
    rng = np.random.default_rng(11)
    for t in range(120):
        shape = tuple(int(v) for v in rng.integers(1, 9, 3))
        yield shape, rng.random(shape) < rng.uniform(0.1, 0.7)


def band_of_mask(active, rng=None):
    cells = np.flatnonzero(active.reshape(-1))
    d = np.ones(cells.size, F) if rng is None else rng.uniform(-1, 1, cells.size).astype(F)
    return cm.Band(active.shape, cells, d, None, 1.0, 1.0)


def flood_fill(active, connectivity):
    """Labels by a stack-based flood fill in raster order, written with nothing of the model's: -> (int array, -1 where inactive; count)."""
    nx, ny, nz = active.shape
    axes = STRUCTURE_RANK[connectivity]
    steps = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 0 < abs(a) + abs(b) + abs(c) <= axes]
    lab = np.full(active.shape, -1, np.int64)
    count = 0
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                if not active[i, j, k] or lab[i, j, k] >= 0:
                    continue
                lab[i, j, k] = count
                stack = [(i, j, k)]
                while stack:
                    x, y, z = stack.pop()
                    for a, b, c in steps:
                        u, v, w = x + a, y + b, z + c
                        if 0 <= u < nx and 0 <= v < ny and 0 <= w < nz and active[u, v, w] and lab[u, v, w] < 0:
                            lab[u, v, w] = count
                            stack.append((u, v, w))
                count += 1
    return lab, count


@pytest.mark.parametrize("connectivity", ccm.CONNECTIVITIES)
def test_the_model_numbers_components_as_a_flood_fill_in_raster_order(connectivity):
    rng = np.random.default_rng(5)
    multi = 0
    for shape, active in random_masks():
        band = band_of_mask(active, rng)
        got = ccm.components(band, connectivity)
        lab, count = flood_fill(active, connectivity)
        assert got.count == count and np.array_equal(got.labels, lab.reshape(-1)[band.cells]), (shape, connectivity)
        multi += count > 1
        # the statistics, recomputed from the labels
        i, j, k = np.unravel_index(band.cells, shape)
        for c in range(count):
            mine = got.labels == c
            assert got.first_cell[c] == band.cells[mine].min() and got.n_cells[c] == mine.sum()
            assert got.n_negative[c] == (band.distances[mine] < 0).sum()
            assert got.lo[c].tolist() == [i[mine].min(), j[mine].min(), k[mine].min()]
            assert got.hi[c].tolist() == [i[mine].max(), j[mine].max(), k[mine].max()]
        assert np.all(np.diff(got.first_cell.astype(np.int64)) > 0)
    assert multi >= 30                                                            # no vacuous set: many masks have several components


@pytest.mark.parametrize("connectivity", ccm.CONNECTIVITIES)
def test_the_model_against_scipy(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, STRUCTURE_RANK[connectivity])
    for shape, active in random_masks():
        band = band_of_mask(active)
        got = ccm.components(band, connectivity)
        lab, count = ndimage.label(active, structure)
        assert got.count == count and np.array_equal(got.labels.astype(np.int64), lab.reshape(-1)[band.cells] - 1), (shape, connectivity)


def test_negative_zero_is_not_negative_and_steps_do_not_wrap():
    band = cm.Band((1, 2, 3), [0, 2, 3, 5], np.array([-0.0, -1.0, 0.0, -2.0], F), None, 1.0, 1.0)
    got = ccm.components(band, 26)
    # (0,0,0) and (0,1,0) are joined; (0,0,2) and (0,1,2) are joined; k = 2 of one row and k = 0 of the next are neighbours in L only
    assert got.count == 2 and got.labels.tolist() == [0, 1, 0, 1] and got.n_negative.tolist() == [0, 2]
    assert len(ccm.backward_steps(6)) == 3 and len(ccm.backward_steps(18)) == 9 and len(ccm.backward_steps(26)) == 13


def test_the_row_rule_point_by_point():
    rng = np.random.default_rng(23)
    for _ in range(300):
        nz = int(rng.integers(1, 40))
        active = rng.random(nz) < rng.uniform(0, 0.6)
        dropped = active & (rng.random(nz) < 0.5)
        inside = rng.random(nz) < 0.6
        assert np.array_equal(ccm.clear_row(active, dropped, inside), ccm.clear_row_plain(active, dropped, inside))
    t, f = True, False
    # no active cell in the row: nothing to clear; one side only, dropped: cleared; dropped on one side and kept on the other: kept
    assert not ccm.clear_row(np.array([f, f, f]), np.array([f, f, f]), np.array([t, t, t])).any()
    assert ccm.clear_row(np.array([t, f, f]), np.array([t, f, f]), np.array([f, t, t])).tolist() == [f, t, t]
    assert not ccm.clear_row(np.array([t, f, f, t]), np.array([t, f, f, f]), np.array([f, t, t, f])).any()
    assert ccm.clear_row(np.array([t, f, t, f, t]), np.array([t, f, t, f, f]), np.array([f, t, f, t, f])).tolist() == [f, t, f, f, f]


# ---- 2. the model on geometry -------------------------------------------------------------------------------------------------------------
def sphere_distance(shape, centre, radius):
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(F)


def band_of_distance(dist, half):
    cells = np.flatnonzero(np.abs(dist).reshape(-1) <= F(half))
    return cm.Band(dist.shape, cells, dist.reshape(-1)[cells], cm.pack_bits(dist.shape, dist < 0), half, half)


def test_two_spheres_are_two_components_and_erasing_one_clears_its_interior_only():
    shape = (24, 24, 24)
    big, small = sphere_distance(shape, (8.5, 8.5, 8.5), 6.0), sphere_distance(shape, (18.0, 18.0, 18.0), 2.5)
    both = np.minimum(big, small)
    band = band_of_distance(both, 1.8)
    for connectivity in ccm.CONNECTIVITIES:
        cc = ccm.components(band, connectivity)
        assert cc.count == 2 and cc.n_cells[0] > cc.n_cells[1] > 50
        assert cc.n_cells[1] == (np.abs(small) <= F(1.8)).sum() and cc.n_negative[1] == ((np.abs(small) <= F(1.8)) & (small < 0)).sum()
        at = np.argwhere(np.abs(small) <= F(1.8))
        assert cc.lo[1].tolist() == at.min(0).tolist() == [14, 14, 14] and cc.hi[1].tolist() == at.max(0).tolist() == [22, 22, 22]
        # erasing nothing is the identity in every bit
        same, info = ccm.select(band, cc.labels, [1, 1])
        assert cm.same(same, band) and info == (band.cells.size, 0, 0)
        # erasing the small sphere clears exactly the inactive inside points that lie in it
        out, info = ccm.select(band, cc.labels, [1, 0])
        inner_small = small < -F(1.8)
        assert info.n_sign_cleared == inner_small.sum() > 0 and info.n_dropped == cc.n_cells[1] and info.n_cells == cc.n_cells[0]
        assert cm.same(out, band_of_distance(big, 1.8)), "erasing the small sphere does not leave the large one's band"
        # ... and erasing the large one leaves the small one's
        out, info = ccm.select(band, cc.labels, [0, 1])
        assert cm.same(out, band_of_distance(small, 1.8)) and info.n_sign_cleared == (big < -F(1.8)).sum()


def test_erasing_the_band_around_a_cavity_is_the_documented_limit():
    """A shell with its inner band erased: the cavity stays outside, the inner skin's cells become outside, and the solid around the
    cavity keeps its inside bits (every row segment of it still ends on the kept outer skin), so the field now steps from solid to
    outside with no band cell between.  n_sign_cleared is 0: the rule knows rows, not solids.  Erase islands, not voids."""
    shape = (24, 24, 24)
    c = (11.5, 11.5, 11.5)
    outer, inner = sphere_distance(shape, c, 8.0), sphere_distance(shape, c, 4.0)
    shell = np.maximum(outer, -inner)
    band = band_of_distance(shell, 1.5)
    cc = ccm.components(band, 6)
    assert cc.count == 2 and cc.first_cell[0] < cc.first_cell[1] and cc.n_cells[0] > cc.n_cells[1]      # 0 the outer skin, 1 the inner
    out, info = ccm.select(band, cc.labels, [1, 0])
    assert info.n_sign_cleared == 0 and info.n_dropped == cc.n_cells[1]
    act, d, s = cm.dense(out)
    was_act, _, was_s = cm.dense(band)
    skin = was_act & ~act                                                               # the erased inner skin
    assert not s[skin].any() and was_s[skin].any()                                     # all of it outside now, part of it was solid
    cavity = inner < -F(1.5)
    assert cavity.any() and not s[cavity].any() and not was_s[cavity].any()             # the cavity was outside and stays outside
    solid = ~was_act & was_s
    assert solid.any() and np.array_equal(s[solid], was_s[solid])                      # the solid keeps every bit
    unbracketed = (solid[:, :, 1:] & skin[:, :, :-1]) | (solid[:, :, :-1] & skin[:, :, 1:])
    assert unbracketed.sum() > 0                                                        # solid next to outside, no band cell between


def test_the_chain_holds_in_the_models():
    """(A | B) | D with all but the two largest components erased is A | B in every bit, by band_csg_model and this model alone: what
    test_gpu_band_components.py then asks of the library."""
    a, b, d, ab, abd = ccm.chain_bands()
    assert a.cells.size > b.cells.size > d.cells.size > 100
    for connectivity in ccm.CONNECTIVITIES:
        cc = ccm.components(abd, connectivity)
        assert cc.count == 3 and sorted(cc.n_cells.tolist()) == sorted([a.cells.size, b.cells.size, d.cells.size])
        keep = np.zeros(3, bool)
        keep[np.argsort(-cc.n_cells.astype(np.int64), kind="stable")[:2]] = True
        out, info = ccm.select(abd, cc.labels, keep)
        assert cm.same(out, ab) and info.n_dropped == d.cells.size and info.n_sign_cleared > 0


# ---- 3. errors without a device ----------------------------------------------------------------------------------------------------------
def _opts(**kw):
    o = _lib.M2SOpts()
    o.struct_size, o.device = C.sizeof(o), -1
    for k, v in kw.items():
        setattr(o, k, v)
    return C.byref(o)


_PEER = (C.c_void_p * 1)(0x1000)
# the m2s_opts fields no band call takes, peer_out among them (a count or a pointer alone is refused too)
BAD_OPTS = (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 5), ("n_peer_out", 1),
            ("peer_out", C.cast(_PEER, C.POINTER(C.c_void_p))))


def test_components_rejects_what_needs_no_handle(lib):
    BAD = _lib.ERR_BAD_ARG
    fake = C.c_void_p(0x1234)                     # never dereferenced: every call below fails before it looks at the handle
    n = C.c_uint64(77)
    good = _lib.M2SBandComponentsOpts(8, 6)
    assert lib.m2s_band_components(None, C.byref(good), None, None, None, 0, C.byref(n)) == BAD and "band is NULL" in _lib.last_error()
    assert lib.m2s_band_components(fake, C.byref(good), None, None, None, 0, None) == BAD and "n_components_out" in _lib.last_error()
    for size in (0, 4, 12):
        assert lib.m2s_band_components(fake, C.byref(_lib.M2SBandComponentsOpts(size, 6)), None, None, None, 0, C.byref(n)) == BAD
        assert "struct_size" in _lib.last_error()
    for conn in (0, 1, 4, 8, 19, 27, -6):
        assert lib.m2s_band_components(fake, C.byref(_lib.M2SBandComponentsOpts(8, conn)), None, None, None, 0, C.byref(n)) == BAD
        assert "connectivity" in _lib.last_error()
    for field, value in BAD_OPTS:
        assert lib.m2s_band_components(fake, C.byref(good), _opts(**{field: value}), None, None, 0, C.byref(n)) == BAD, field
    assert n.value == 77                          # invalid arguments: the count is not written


def test_select_rejects_what_needs_no_handle(lib):
    BAD = _lib.ERR_BAD_ARG
    SENTINEL = 0x1234
    fake = C.c_void_p(SENTINEL)
    labels = (C.c_uint32 * 4)()
    keep = (C.c_uint8 * 2)(1, 1)

    def call(band=fake, lab=labels, kp=keep, n_keep=2, fo=None, opts=None, info=None):
        h = C.c_void_p(SENTINEL)
        rc = lib.m2s_band_select(band, lab, kp, n_keep, fo, opts, C.byref(h), info)
        assert h.value is None                    # *out = NULL on every failure
        return rc

    assert call(band=None) == BAD and "band is NULL" in _lib.last_error()
    assert call(lab=None) == BAD and "labels is NULL" in _lib.last_error()
    assert call(kp=None) == BAD and "keep is NULL" in _lib.last_error()
    assert lib.m2s_band_select(fake, labels, keep, 2, None, None, None, None) == BAD and "out is NULL" in _lib.last_error()
    for fo in ((8, 0.5, 0.5), (12, -0.5, 0.5), (12, 0.5, float("inf")), (12, float("nan"), 0.5)):
        assert call(fo=C.byref(_lib.M2SBandFieldOpts(*fo))) == BAD, fo
    for size in (0, 8, 24, 40):
        assert call(info=C.byref(_lib.M2SBandSelectInfo(size))) == BAD and "m2s_band_select_info" in _lib.last_error()
    for field, value in BAD_OPTS:
        assert call(opts=_opts(**{field: value})) == BAD, field


# ---- 4. the ABI surface and the consumers ------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_and_declared(lib):
    for name in ("m2s_band_components", "m2s_band_select"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    hdr = " ".join(open(os.path.join(ROOT, "include", "m2s.h")).read().split())
    for text in ("enum m2s_connectivity { M2S_CONNECT_6 = 6, M2S_CONNECT_18 = 18, M2S_CONNECT_26 = 26 };",
                 "typedef struct m2s_band_components_opts { uint32_t struct_size; int32_t connectivity; } m2s_band_components_opts;",
                 "typedef struct m2s_band_component { uint64_t first_cell, n_cells, n_negative; uint32_t lo[3], hi[3]; } m2s_band_component;",
                 "typedef struct m2s_band_select_info { uint32_t struct_size, reserved; uint64_t n_cells, n_dropped, n_sign_cleared; } m2s_band_select_info;",
                 "#define M2S_LABEL_NONE 0xffffffffu",
                 "int m2s_band_components(const m2s_band* band, const m2s_band_components_opts* copts",
                 "int m2s_band_select(const m2s_band* band, const uint32_t* labels /* n_cells */, const uint8_t* keep, uint64_t n_keep,",
                 "labels[r] < n_keep && keep[labels[r]] != 0", "is NO clamping", "raster numbering of scipy.ndimage.label",
                 "Erase islands, not voids", "signedFloodFill", "2^32 - 1 or more active cells"):
        assert text in hdr, text
    assert C.sizeof(_lib.M2SBandComponent) == 48 and C.sizeof(_lib.M2SBandComponentsOpts) == 8 and C.sizeof(_lib.M2SBandSelectInfo) == 32
    assert _lib.M2SBandComponent.lo.offset == 24 and _lib.M2SBandComponent.hi.offset == 36 and _lib.LABEL_NONE == 0xffffffff
    assert [int(c) for c in Connectivity] == [6, 18, 26]
    assert SelectInfo._fields == ("n_cells", "n_dropped", "n_sign_cleared")
    for name in ("components", "select", "keep_largest", "remove_islands", "split"):
        assert hasattr(BandField, name), name
    for name in ("largest", "at_least"):
        assert hasattr(Components, name), name
    import inspect
    for fn in (api.boolean, api.remesh, api.Mesh.boolean, api.Mesh.remesh):
        assert inspect.signature(fn).parameters["keep_largest"].default == 0
    hpp = open(os.path.join(ROOT, "include", "mesh_to_sdf.hpp")).read()
    for text in ("enum class Connectivity", "struct Components", "struct SelectInfo", "Components components(Connectivity connectivity = Connectivity::Faces) const",
                 "BandField select(const std::vector<uint32_t>& labels, const std::vector<uint8_t>& keep, SelectInfo* info = nullptr) const"):
        assert text in hpp, text
    for doc, text in (("README.md", "m2s_band_components"), ("README.md", "m2s_band_select"), ("DESIGN.md", "m2s_band_components"), ("DESIGN.md", "4.21"),
                      ("DESIGN.md", "cavity")):
        assert text in open(os.path.join(ROOT, doc)).read(), (doc, text)


def test_largest_and_at_least_order_components():
    z = np.zeros(0, np.uint64)
    cc = Components(np.zeros(0, np.uint32), Connectivity.Faces, np.arange(5, dtype=np.uint64), np.array([3, 9, 9, 1, 9], np.uint64), np.zeros(5, np.uint64),
                    np.zeros((5, 3), np.uint32), np.zeros((5, 3), np.uint32))
    assert cc.count == 5 and cc.largest().tolist() == [1] and cc.largest(3).tolist() == [1, 2, 4] and cc.largest(9).tolist() == [1, 2, 4, 0, 3]
    assert cc.largest(0).tolist() == [] and cc.at_least(3).tolist() == [0, 1, 2, 4] and cc.at_least(10).tolist() == []
    empty = Components(np.zeros(0, np.uint32), Connectivity.Faces, z, z, z, np.zeros((0, 3), np.uint32), np.zeros((0, 3), np.uint32))
    assert empty.count == 0 and empty.largest(2).tolist() == []


@pytest.mark.parametrize("cc,std,src", [("gcc", "-std=c99", "tests/c/band_components_smoke.c"), ("g++", "-std=c++17", "tests/cpp/band_components_tests.cpp")])
def test_consumers_compile_and_check_their_arguments(lib, tmp_path, cc, std, src):
    exe = str(tmp_path / os.path.basename(src).split(".")[0])
    subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                           os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
