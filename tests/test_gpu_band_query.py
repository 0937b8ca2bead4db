"""m2s_band_create / m2s_band_sample / m2s_band_raymarch on the GPU, bit for bit against tests/band_query_model.py (the definition in numpy)
and against the library's own sample_grid / raymarch_grid on the dense grid D' the band stands for: random fields with random active sets
and sign masks, real narrow bands of meshes under both sign rules, the validation and handle contract, the call forms, and a 4.6e9-point
grid whose cell indices pass 2^32.  Every comparison is exact equality of bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import band_query_model as bqm
import grid_query_model as gqm
from mesh_to_sdf_amd import BandField, Grid, M2SError, M2STimings, Mesh, SampleMode, SignMethod, Topology, _lib, meshes, raymarch_grid, sample_grid

F = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNS = [SignMethod.Raycast, SignMethod.Normal]
MODES = [SampleMode.Snap, SampleMode.Trilinear, SampleMode.Tetrahedral]
K_OF = {SampleMode.Snap: 1, SampleMode.Trilinear: 8, SampleMode.Tetrahedral: 4}
BG_OUT, BG_IN = 0.75, 0.5


def _np(x):
    if hasattr(x, "cpu"):
        if x.dtype == getattr(torch, "uint32", None):
            x = x.view(torch.int32)
        x = x.cpu().numpy()
    return np.asarray(x)


def _same(got, want, what):
    """Bit equality; every NaN counts as one value (grid_query_model.same_bits)."""
    got, want = _np(got), _np(want)
    if got.dtype == np.float32:
        assert gqm.same_bits(got, want), f"{what}: {got.shape} vs {want.shape}, {int((got.view(np.uint32) != np.asarray(want, F).view(np.uint32)).sum()) if got.shape == want.shape else '?'} values differ"
    else:
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), f"{what}: integers differ"


def _dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x).astype(dtype) if dtype else x, device=DEV)


def _bits_dev(bits):
    return torch.as_tensor(np.ascontiguousarray(bits).view(np.int32), device=DEV)


def _d_prime(n, cells, vals, bg_out, bg_in, bits):
    """The dense grid of the definition, built with numpy alone (not with the model's fetch)."""
    n = tuple(int(c) for c in n)
    if bits is None:
        d = np.full(n, F(bg_out), F)
    else:
        k = np.arange(n[2])
        inside = ((np.asarray(bits, np.uint32).reshape(n[0], n[1], -1)[:, :, k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)
        d = np.where(inside, -F(bg_in), F(bg_out)).astype(F)
    d = d.reshape(-1)
    d[np.asarray(cells).astype(np.int64)] = vals
    return d


# ---- 1. random fields with random active sets ----------------------------------------------------------------------------------------------------
def _points(rng, q, n):
    lo, hi = q.start - q.cs, q.end + q.cs                     # the box grown by one cell: some points are outside
    uni = (lo + rng.random((4000, 3)) * (hi - lo)).astype(F)
    idx = np.stack(np.meshgrid(*(np.arange(c) for c in n), indexing="ij"), -1).reshape(-1, 3)
    centres = (q.start + idx.astype(F) * q.cs).astype(F)      # first_cell is the centre of cell 0
    corners = np.array([[(q.start, q.end)[b][a] for a, b in enumerate(c)] for c in np.ndindex(2, 2, 2)], F)
    odd = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [np.nan, np.inf, -np.inf]], F)
    mid = ((q.start + q.end) * F(0.5)).astype(F)
    odd = np.where(odd == 0, mid, odd).astype(F)
    return np.concatenate([uni, centres, corners, odd]).astype(F)


@pytest.mark.parametrize("n", [(5, 7, 67), (2, 2, 2), (1, 6, 6), (9, 1, 9), (33, 20, 31)], ids=lambda n: "x".join(map(str, n)))
def test_random_fields_with_random_active_sets(n):
    """Uniform values in [-1, 1], active fractions 1, 0.9, 0.5 and 0, with and without a random sign mask.  5 x 7 x 67 has rows of nz that
    cross a 64-bit mask word; 1 x 6 x 6 and 9 x 1 x 9 have an axis where both reads clamp to one cell."""
    rng = np.random.default_rng(sum(n))
    grid = Grid(rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.3, 3), list(n))
    q = gqm.GridQ.of(grid)
    d = rng.uniform(-1, 1, n).astype(F).reshape(-1)
    pts = _points(rng, q, n)
    inside = gqm._state(q, pts) == 0
    assert inside.any() and (~inside).any()
    if n == (5, 7, 67):
        # the upper z-neighbour of a sample's low corner lies in the next mask word
        i = np.floor((pts[inside] - q.start) / q.cs).astype(np.int64)
        L = gqm.cell_off(q, i[:, 0], i[:, 1], i[:, 2])
        assert (((L & 63) == 63) & (i[:, 2] + 1 <= n[2] - 1) & (i[:, 2] >= 0)).any(), "no sample crosses a mask word along z"
    dpts = _dev(pts)
    call = 0
    mixed = 0
    for frac in (1.0, 0.9, 0.5, 0.0):
        active = rng.random(d.size) < frac
        cells, vals = np.flatnonzero(active).astype(np.uint64), d[active]
        for with_bits in (False, True):
            bits = rng.integers(0, 2 ** 32, (n[0], n[1], (n[2] + 31) // 32), dtype=np.uint64).astype(np.uint32) if with_bits else None
            model = bqm.Band(n, cells, vals, BG_OUT, BG_IN, bits)
            dp = _d_prime(n, cells, vals, BG_OUT, BG_IN, bits)
            ddp = _dev(dp)
            on_device = call % 2 == 0
            call += 1
            if on_device:
                field = BandField(grid, _dev(cells, np.int64), _dev(vals), background=(BG_IN, BG_OUT), inside=None if bits is None else _bits_dev(bits))
            else:
                field = BandField(grid, cells, vals, background=(BG_IN, BG_OUT), inside=bits)
            with field:
                assert field.count == cells.size and field.grid is grid
                for mode in MODES:
                    for iso in (0.0, 0.25):
                        what = f"{n} fraction {frac} bits {with_bits} {mode.name} iso {iso}"
                        gv, gn, gs = field.sample(dpts if on_device else pts, mode=mode, iso=iso, normals=True, support=True)
                        assert (torch.is_tensor(gv) and gv.is_cuda) == on_device
                        # the numpy model is the slow side: every point where the band is mixed and iso is 0, every fifth point otherwise
                        # (the dense call below, itself pinned to grid_query_model by its own tests, sees every point in every case)
                        sel = slice(None) if (iso == 0.0 and frac in (0.9, 0.5)) or pts.shape[0] < 6000 else slice(None, None, 5)
                        wv, ws = bqm.sample(q, model, pts[sel], int(mode), iso)
                        wn = bqm.normal(q, model, pts[sel], int(mode), iso)
                        _same(_np(gv)[sel], wv, what + " values / model")
                        _same(_np(gn)[sel], wn, what + " normals / model")
                        _same(_np(gs)[sel], ws, what + " support / model")
                        dv, dn = sample_grid(grid, ddp, dpts, mode=mode, iso=iso, normals=True)
                        _same(gv, dv, what + " values / sample_grid on D'")
                        _same(gn, dn, what + " normals / sample_grid on D'")
                        gs = _np(gs)
                        if frac == 1.0:
                            assert np.array_equal(gs, np.where(inside, K_OF[mode], 0)), what
                        if frac == 0.0:
                            assert (gs == 0).all(), what
                            if bits is None:   # the interpolated background
                                _same(gv, gqm.sample(q, np.full(d.size, BG_OUT, F), pts, int(mode), iso), what + " background")
                        if frac == 0.5 and mode != SampleMode.Snap and d.size > 8:
                            part = (gs > 0) & (gs < K_OF[mode])
                            assert part.any(), what + ": no sample mixes band cells and background"
                            mixed += int(part.sum())
    assert mixed > 0 or d.size <= 8


def test_a_random_field_ray_marched():
    """The march on a random field: rays from outside and inside the box, every mode, against the model and raymarch_grid on D'."""
    n = (9, 8, 70)
    rng = np.random.default_rng(5)
    grid = Grid(rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.3, 3), list(n))
    q = gqm.GridQ.of(grid)
    d = (rng.uniform(-0.2, 1, n).astype(F) * F(0.3)).reshape(-1)       # mostly positive and small: the marches take several steps
    lo, hi = q.start - F(3) * q.cs, q.end + F(3) * q.cs
    o = (lo + rng.random((1500, 3)) * (hi - lo)).astype(F)
    target = (q.start + rng.random((1500, 3)) * (q.end - q.start)).astype(F)
    r = target - o
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)
    r[:40] = -r[:40]                                                   # some point away from the box
    o[40:44, 0] = np.nan
    r[44:48, 1] = np.nan
    r[48:52, 2] = 0                                                    # a zero direction component
    active = rng.random(d.size) < 0.6
    cells, vals = np.flatnonzero(active).astype(np.uint64), d[active]
    bits = rng.integers(0, 2 ** 32, (n[0], n[1], (n[2] + 31) // 32), dtype=np.uint64).astype(np.uint32)
    bits &= rng.integers(0, 2 ** 32, bits.shape, dtype=np.uint64).astype(np.uint32)   # a quarter of the cells inside
    for use_bits in (None, bits):
        model = bqm.Band(n, cells, vals, 0.07, 0.05, use_bits)
        ddp = _dev(_d_prime(n, cells, vals, 0.07, 0.05, use_bits))
        with BandField(grid, cells, vals, background=(0.05, 0.07), inside=use_bits) as field:
            for mode in MODES:
                what = f"march {mode.name} bits {use_bits is not None}"
                w_hit, w_steps, w_is, w_sup, w_n = bqm.raymarch(q, model, o, r, int(mode), 0.02, max_steps=24, normals=True)
                pos, dist, steps, hit, nrm, sup = field.raymarch(_dev(o), _dev(r), mode=mode, iso=0.02, max_steps=24, normals=True, support=True)
                _same(torch.cat([pos, dist[:, None]], 1), w_hit, what + " hit / model")
                _same(steps, w_steps, what + " steps / model")
                _same(nrm, w_n, what + " normals / model")
                _same(sup, w_sup, what + " support / model")
                assert np.array_equal(_np(hit), w_is)
                d_pos, d_dist, d_steps, d_hit, d_n = raymarch_grid(grid, ddp, _dev(o), _dev(r), mode=mode, iso=0.02, max_steps=24, normals=True)
                _same(pos, d_pos, what + " positions / raymarch_grid on D'")
                _same(dist, d_dist, what + " dist / raymarch_grid on D'")
                _same(steps, d_steps, what + " steps / raymarch_grid on D'")
                _same(nrm, d_n, what + " normals / raymarch_grid on D'")
                assert w_is.any() and (~w_is).any() and (w_steps > 2).any() and (w_steps == 24).any()
                # host arrays: the same bits
                h = field.raymarch(o[:200], r[:200], mode=mode, iso=0.02, max_steps=24, normals=True, support=True)
                for a, b in zip(h, (pos, dist, steps, hit, nrm, sup)):
                    assert isinstance(a, np.ndarray)
                    _same(a, _np(b)[:200], what + " host arrays")


# ---- 2. real bands -----------------------------------------------------------------------------------------------------------------------------------
REAL = [(name, s) for name in ("suzanne-64", "ragged") for s in SIGNS]


@pytest.fixture(scope="module")
def real(suzanne):
    """(name, sign) -> everything the tests of a real band share, computed once and left unchanged."""
    inputs = {"suzanne-64": (suzanne, (64, 64, 64)), "ragged": (meshes.named("blob-11k"), (70, 45, 83))}
    out = {}
    for name, ((v, idx), count) in inputs.items():
        lo, hi = meshes.extended_bbox(v, 0.1)
        grid = Grid.from_bounding_box(lo, hi, list(count))
        h = float(max(grid.get_cell_size()))
        dv, topo = _dev(v), Topology.TriangleList(_dev(idx, np.int64).reshape(-1))
        with Mesh(dv, topo) as mesh:
            surf = _np(mesh.sample_surface(20000, seed=3).points)
            vox = mesh.voxelize(grid, solid=True, bits=True)
            rng = np.random.default_rng(17)
            step = rng.normal(size=surf.shape)
            step *= (rng.random((surf.shape[0], 1)) * 2.0 * h) / np.linalg.norm(step, axis=1, keepdims=True)   # up to two cells
            pts = (surf + step).astype(F)
            for sign in SIGNS:
                dense = mesh.generate_grid_sdf(grid, sign)
                nb = mesh.narrow_band_sdf(grid, 3.0 * h, sign)
                bg_in, bg_out = float(max(-float(nb.distances.min()), 0.0)), float(max(float(nb.distances.max()), 0.0))
                dp = _d_prime(count, _np(nb.cells), _np(nb.distances), bg_out, bg_in, _np(vox.bits))
                out[(name, sign)] = dict(v=v, mesh_args=(dv, topo), grid=grid, h=h, dense=dense, nb=nb, vox=vox, dp=_dev(dp), pts=_dev(pts), lo=lo, hi=hi)
    return out


def _camera(lo, hi, res=96):
    """A pinhole camera outside the box looking at its centre: res x res normalised rays."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre, size = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    eye = centre + np.array([0.9, 0.55, 1.3]) * size
    fwd = (centre - eye) / np.linalg.norm(centre - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    u = (np.arange(res) + 0.5) / res * 2 - 1
    uu, vv = np.meshgrid(u, u)
    r = fwd + 0.45 * (uu[..., None] * right + vv[..., None] * up)
    r = (r / np.linalg.norm(r, axis=-1, keepdims=True)).reshape(-1, 3).astype(F)
    return np.repeat(eye[None].astype(F), r.shape[0], 0), r


@pytest.mark.parametrize("name,sign", REAL, ids=[f"{n}-{s.name.lower()}" for n, s in REAL])
def test_real_bands(real, name, sign):
    c = real[(name, sign)]
    grid, nb, pts = c["grid"], c["nb"], c["pts"]
    with nb.field(inside=c["vox"]) as field:
        assert field.count == nb.count
        o, r = _camera(c["lo"], c["hi"])
        do, dr = _dev(o), _dev(r)
        for mode in MODES:
            what = f"{name} {sign.name} {mode.name}"
            gv, gn, gs = field.sample(pts, mode=mode, normals=True, support=True)
            dv, dn = sample_grid(grid, c["dp"], pts, mode=mode, normals=True)
            _same(gv, dv, what + " values / sample_grid on D'")
            _same(gn, dn, what + " normals / sample_grid on D'")
            full = _np(gs) == K_OF[mode]
            assert full.sum() > pts.shape[0] // 2, f"{what}: only {int(full.sum())} of {pts.shape[0]} samples lie in the band"
            tv = sample_grid(grid, c["dense"], pts, mode=mode)
            _same(_np(gv)[full], _np(tv)[full], what + " values / sample_grid on the dense grid, where support is full")
            pos, dist, steps, hit, nrm, sup = field.raymarch(do, dr, mode=mode, normals=True, support=True)
            w = raymarch_grid(grid, c["dp"], do, dr, mode=mode, normals=True)
            for got, want, part in zip((pos, dist, steps, hit, nrm), w, ("positions", "dist", "steps", "hit", "normals")):
                _same(got, want, f"{what} march {part} / raymarch_grid on D'")
            hit = _np(hit)
            assert hit.any() and (~hit).any(), what
    if sign == SignMethod.Raycast:
        # the one-call route gives the same field
        with Mesh(*c["mesh_args"]) as mesh, mesh.narrow_band_field(grid, 3.0 * c["h"], sign) as auto, nb.field(inside=c["vox"]) as manual:
            assert auto.count == manual.count and auto.device_bytes == manual.device_bytes and auto.background == manual.background
            for mode in MODES:
                a = auto.sample(pts, mode=mode, normals=True, support=True)
                b = manual.sample(pts, mode=mode, normals=True, support=True)
                for x, y in zip(a, b):
                    _same(x, y, f"{name} narrow_band_field {mode.name}")


def test_every_fetch_form_gives_the_same_bits(real):
    """M2S_BAND_FETCH: the three rounds with larger or smaller groups and the per-corner chain, against the automatic choice."""
    c = real[("ragged", SignMethod.Normal)]
    o, r = (_dev(x) for x in _camera(c["lo"], c["hi"], 48))
    for inside in (None, c["vox"]):
        with c["nb"].field(inside=inside) as field:
            for mode in MODES:
                want_s = field.sample(c["pts"], mode=mode, normals=True, support=True)
                want_m = field.raymarch(o, r, mode=mode, normals=True, support=True)
                for form in (0, 1, 2):
                    with _lib.knobs(M2S_BAND_FETCH=form):
                        for got, want in zip(field.sample(c["pts"], mode=mode, normals=True, support=True), want_s):
                            _same(got, want, f"form {form} {mode.name} sample")
                        for got, want in zip(field.raymarch(o, r, mode=mode, normals=True, support=True), want_m):
                            _same(got, want, f"form {form} {mode.name} march")


# ---- 3. the contract ---------------------------------------------------------------------------------------------------------------------------------
def _small():
    grid = Grid([0.0, 0.0, 0.0], [0.25, 0.25, 0.25], [8, 8, 8])
    cells = np.arange(128, 384, dtype=np.uint64)
    vals = np.linspace(-0.5, 0.5, 256).astype(F)
    return grid, cells, vals


def _create(lib, grid, cells, vals, device, fo=None):
    """m2s_band_create on host arrays or device tensors -> (rc, handle value)."""
    h = C.c_void_p(0x1234)
    fo = _lib.M2SBandFieldOpts(C.sizeof(_lib.M2SBandFieldOpts), 0.5, 0.5) if fo is None else fo
    o = _lib.M2SOpts()
    o.struct_size, o.device, o.synchronous = C.sizeof(_lib.M2SOpts), -1, 1
    if device:
        tc, tv = _dev(np.asarray(cells).astype(np.uint64).view(np.int64)), _dev(vals)
        o.mem_kind, o.device = _lib.MEM_DEVICE, 0
        pc, pv = tc.data_ptr(), tv.data_ptr()
    else:
        tc, tv = np.ascontiguousarray(cells, np.uint64), np.ascontiguousarray(vals, F)
        pc, pv = tc.ctypes.data, tv.ctypes.data
    rc = lib.m2s_band_create(C.byref(grid._g), pc, pv, len(tc), None, C.byref(fo), C.byref(o), C.byref(h))
    torch.cuda.synchronize()
    return rc, h.value


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_bad_list_or_value_gives_no_handle(device):
    lib = _lib.lib()
    grid, cells, vals = _small()
    for bad in ([5, 4, 9], [4, 5, 5], [4, 5, 512], [0, 2 ** 63], list(range(300, 556))):
        c = np.array(bad, np.uint64)
        rc, h = _create(lib, grid, c, np.zeros(c.size, F), device)
        assert rc == _lib.ERR_BAD_ARG and h is None, bad
    for bad_value in (np.nan, np.inf, -np.inf):
        v = vals.copy()
        v[200] = bad_value
        rc, h = _create(lib, grid, cells, v, device)
        assert rc == _lib.ERR_NAN and h is None
    v = vals.copy()
    v[0], v[-1] = -np.finfo(F).max, np.finfo(F).max                          # f32::MAX is finite and legal
    rc, h = _create(lib, grid, cells, v, device)
    assert rc == _lib.M2S_OK and h
    lib.m2s_band_destroy(h)
    with BandField(grid, _dev(cells, np.int64) if device else cells, _dev(v) if device else v, background=0.5) as f:
        got = _np(f.sample(np.array([[0.5, 0.0, 0.0], [1.25, 1.75, 1.75]], F), mode=SampleMode.Snap))
        assert got[0] == -np.finfo(F).max and got[1] == np.finfo(F).max


def test_an_empty_band_and_empty_queries():
    grid, cells, vals = _small()
    pts = np.array([[0.3, 0.4, 0.5], [-5.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], F)
    with BandField(grid, np.zeros(0, np.uint64), np.zeros(0, F), background=(0.5, 0.75)) as empty:
        assert empty.count == 0 and empty.background == (0.5, 0.75)
        v, n, s = empty.sample(pts, mode=SampleMode.Snap, normals=True, support=True)
        assert v[0] == F(0.75) and v[1] == F(100.0) and np.isnan(v[2]) and (s == 0).all() and (n[:2] == 0).all() and np.isnan(n[2]).all()
        assert empty.sample(np.zeros((0, 3), F)).shape == (0,)
        assert empty.sample(torch.zeros((0, 3), device=DEV)).shape == (0,)
        assert all(x.shape[0] == 0 for x in empty.raymarch(np.zeros((0, 3), F), np.zeros((0, 3), F), normals=True, support=True))
    with BandField(grid, np.zeros(0, np.uint64), np.zeros(0, F)) as zero:   # the default background of an empty band is (0, 0)
        assert zero.background == (0.0, 0.0) and (zero.sample(pts[:1]) == 0).all()
    with BandField(grid, cells, vals) as f:                                # the default: the band's own reach
        assert f.background == (0.5, 0.5)


def test_the_query_calls_reject_what_the_dense_calls_reject():
    lib = _lib.lib()
    grid, cells, vals = _small()
    p = _dev(np.full((4, 3), 0.5, F))
    v, n3, s = torch.zeros(4, device=DEV), torch.zeros((4, 3), device=DEV), torch.zeros(4, dtype=torch.uint8, device=DEV)
    hit, steps = torch.zeros((4, 4), device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    with BandField(grid, cells, vals) as f:
        h = f._h

        def opts(**kw):
            o = _lib.M2SOpts()
            o.struct_size, o.device, o.mem_kind, o.synchronous = C.sizeof(_lib.M2SOpts), 0, _lib.MEM_DEVICE, 1
            for k, val in kw.items():
                setattr(o, k, val)
            return C.byref(o)

        def sopts(mode=1, max_steps=100):
            so = _lib.M2SSampleOpts()
            so.struct_size, so.mode, so.outside, so.max_steps = C.sizeof(_lib.M2SSampleOpts), mode, 100.0, max_steps
            return C.byref(so)

        BAD = _lib.ERR_BAD_ARG
        sample, march = lib.m2s_band_sample, lib.m2s_band_raymarch
        assert sample(h, p.data_ptr(), 4, None, None, None, s.data_ptr(), opts()) == BAD          # support_out alone is no output
        assert march(h, p.data_ptr(), p.data_ptr(), 4, None, None, None, None, s.data_ptr(), opts()) == BAD
        assert sample(h, None, 4, None, v.data_ptr(), None, None, opts()) == BAD                    # NULL points, n > 0
        assert march(h, p.data_ptr(), None, 4, None, hit.data_ptr(), None, None, None, opts()) == BAD
        assert sample(h, p.data_ptr(), 4, sopts(mode=3), v.data_ptr(), None, None, opts()) == BAD
        assert march(h, p.data_ptr(), p.data_ptr(), 4, sopts(max_steps=0), hit.data_ptr(), None, None, None, opts()) == BAD
        for field, value in (("algorithm", 1), ("x_begin", 1), ("x_end", 2), ("x_period", 4), ("mem_kind", 7)):
            assert sample(h, p.data_ptr(), 4, None, v.data_ptr(), None, None, opts(**{field: value})) == BAD, field
        if torch.cuda.device_count() > 1:
            assert sample(h, p.data_ptr(), 4, None, v.data_ptr(), None, None, opts(device=1)) == BAD
        assert sample(h, p.data_ptr(), 4, None, v.data_ptr(), None, None, opts(device=torch.cuda.device_count())) == BAD
        assert (v == 0).all() and (s == 0).all() and (hit == 0).all()                              # no failed call wrote anything
        assert sample(h, None, 0, None, v.data_ptr(), None, None, opts()) == _lib.M2S_OK            # n = 0
        assert march(h, None, None, 0, None, hit.data_ptr(), steps.data_ptr(), n3.data_ptr(), s.data_ptr(), opts()) == _lib.M2S_OK
        # every output alone
        want_v, want_n, want_s = f.sample(p, normals=True, support=True)
        assert sample(h, p.data_ptr(), 4, None, None, n3.data_ptr(), None, opts()) == _lib.M2S_OK
        _same(n3, want_n, "normals alone")
        assert sample(h, p.data_ptr(), 4, None, None, n3.data_ptr(), s.data_ptr(), opts()) == _lib.M2S_OK
        _same(s, want_s, "support beside normals: the centre sample's")


def test_an_asynchronous_call_two_handles_and_timings():
    lib = _lib.lib()
    grid, cells, vals = _small()
    rng = np.random.default_rng(3)
    pts = _dev(rng.uniform(-0.2, 2.2, (5000, 3)).astype(F))
    t = M2STimings()
    a = BandField(grid, cells, vals, timings=t)
    assert t.seed_ms > 0 and t.n_units == 256
    b = BandField(grid, cells[:100], -vals[:100], background=0.125)          # two handles alive at once
    want_a, want_b = a.sample(pts, support=True), b.sample(pts, support=True)
    assert not np.array_equal(_np(want_a[0]), _np(want_b[0]))
    out, sup = torch.zeros(5000, device=DEV), torch.zeros(5000, dtype=torch.uint8, device=DEV)
    o = _lib.M2SOpts()
    o.struct_size, o.device, o.mem_kind, o.synchronous, o.stream_mode = C.sizeof(_lib.M2SOpts), 0, _lib.MEM_DEVICE, 0, 1
    o.stream = torch.cuda.current_stream().cuda_stream
    assert lib.m2s_band_sample(a._h, pts.data_ptr(), 5000, None, out.data_ptr(), None, sup.data_ptr(), C.byref(o)) == _lib.M2S_OK
    torch.cuda.current_stream().synchronize()
    _same(out, want_a[0], "asynchronous values")
    _same(sup, want_a[1], "asynchronous support")
    t2 = M2STimings()
    got = b.sample(pts, support=True, timings=t2)
    assert t2.distance_ms > 0 and t2.n_units == 5000
    _same(got[0], want_b[0], "second handle")
    a.close()
    a.close()                                                                 # closing twice is fine
    with pytest.raises(M2SError, match="closed"):
        a.sample(pts)                                                         # raised in Python: the library is not called
    with pytest.raises(M2SError, match="closed"):
        a.raymarch(pts, pts)
    _same(b.sample(pts), want_b[0], "the other handle lives on")
    b.close()


def test_device_bytes_is_the_stated_size(real):
    c = real[("suzanne-64", SignMethod.Raycast)]
    nb, words = c["nb"], 64 ** 3 // 64
    with nb.field() as plain, nb.field(inside=c["vox"]) as signed:
        assert plain.device_bytes == 16 * words + 4 * nb.count                # 1 bit + 8 B per 64 points, 4 B per band cell
        assert signed.device_bytes == plain.device_bytes + 8 * words          # + the sign mask, 1 bit per point
        assert signed.device_bytes < 64 ** 3 * 4
        info_grid, n, nbytes = _lib.M2SGrid(), C.c_uint64(0), C.c_uint64(0)
        assert _lib.lib().m2s_band_info(signed._h, C.byref(info_grid), C.byref(n), C.byref(nbytes)) == _lib.M2S_OK
        assert n.value == nb.count and nbytes.value == signed.device_bytes and list(info_grid.cell_count) == [64, 64, 64]
    grid = Grid([0, 0, 0], [0.5] * 3, [5, 7, 9])                              # 315 points: 5 words
    with BandField(grid, np.array([3, 314], np.uint64), np.zeros(2, F), background=1.0, inside=np.zeros((5, 7, 1), np.uint32)) as f:
        assert f.device_bytes == 16 * 5 + 4 * 2 + 8 * 5


def test_c_and_cpp_consumers_run_clean(tmp_path):
    for cc, std, src, extra in (("gcc", "-std=c99", "tests/c/band_query_smoke.c", ["-lm"]), ("g++", "-std=c++17", "tests/cpp/band_query_tests.cpp", [])):
        exe = str(tmp_path / os.path.basename(src).split(".")[0])
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, src), "-L",
                               os.path.join(ROOT, "mesh_to_sdf_amd"), "-lm2s_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath," + os.path.join(ROOT, "mesh_to_sdf_amd"), "-Wl,-rpath,/opt/rocm/lib", *extra, "-o", exe])
        r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


# ---- 4. indices past 2^32 ----------------------------------------------------------------------------------------------------------------------------
def _block(n, lo, side=6):
    i, j, k = np.meshgrid(*(np.arange(a, a + side, dtype=np.int64) for a in lo), indexing="ij")
    return np.sort((k + j * n[2] + i * n[1] * n[2]).reshape(-1))


def test_cell_indices_past_2_32():
    """1664^3 = 4.6e9 grid points: the index takes 1.1 GiB, a dense grid would take 17.  Two blocks of 6 x 6 x 6 cells, one at the origin
    and one at the far corner (every L above 2^32), 200 points around each, against the model alone."""
    free, _ = torch.cuda.mem_get_info()
    if free < 4 << 30:
        pytest.skip("less than 4 GiB of device memory free")
    n = (1664, 1664, 1664)
    grid = Grid([-3.0, 0.5, 2.0], [0.01, 0.02, 0.015], list(n))
    q = gqm.GridQ.of(grid)
    near, far = _block(n, (1, 2, 1)), _block(n, (1657, 1656, 1657))
    assert int(far[0]) > 2 ** 32 and int(far[-1]) < n[0] * n[1] * n[2] and int(near[-1]) < int(far[0])
    cells = np.concatenate([near, far])
    rng = np.random.default_rng(9)
    vals = rng.uniform(-1, 1, cells.size).astype(F)
    pts = []
    for lo in ((1, 2, 1), (1657, 1656, 1657)):
        a = q.start + (np.array(lo, F) - F(2)) * q.cs
        pts.append((a + rng.random((200, 3)) * (F(10) * q.cs)).astype(F))
    pts = np.concatenate(pts).astype(F)
    model = bqm.Band(n, cells, vals, BG_OUT, BG_IN)
    with BandField(grid, _dev(cells), _dev(vals), background=(BG_IN, BG_OUT)) as field:
        assert field.device_bytes == 16 * ((n[0] * n[1] * n[2] + 63) // 64) + 4 * cells.size < 2 << 30
        seen = 0
        for mode in MODES:
            wv, ws = bqm.sample(q, model, pts, int(mode))
            wn = bqm.normal(q, model, pts, int(mode))
            gv, gn, gs = field.sample(_dev(pts), mode=mode, normals=True, support=True)
            _same(gv, wv, f"2^32 {mode.name} values")
            _same(gn, wn, f"2^32 {mode.name} normals")
            _same(gs, ws, f"2^32 {mode.name} support")
            assert (ws[:200] == K_OF[mode]).any() and (ws[200:] == K_OF[mode]).any() and (ws == 0).any()
            seen += int((ws[200:] > 0).sum())
            o = pts[150:250]
            r = np.tile(np.array([[0.6, 0.0, 0.8]], F), (100, 1))
            w = bqm.raymarch(q, model, o, r, int(mode), max_steps=6, normals=True)
            pos, dist, steps, hit, nrm, sup = field.raymarch(_dev(o), _dev(r), mode=mode, max_steps=6, normals=True, support=True)
            _same(torch.cat([pos, dist[:, None]], 1), w[0], f"2^32 {mode.name} march")
            _same(steps, w[1], f"2^32 {mode.name} steps")
            _same(sup, w[3], f"2^32 {mode.name} march support")
            _same(nrm, w[4], f"2^32 {mode.name} march normals")
        assert seen > 0
