"""The per-call constants the host resolves for the walks' kernels (common.h set_super_brick_magic, dist.hip.h cut_list_for; test hook
m2s_debug_walk_consts): the super-brick x-log, the brick and super-brick counts along y and z, the two division magics and the start bits
of the cut-list words, against a restatement of the rules in Python.  Host arithmetic only, no device."""
import ctypes as C

import pytest

from mesh_to_sdf_amd import _lib
from mesh_to_sdf_amd._lib import M2SGrid, M2SOpts

# cell sizes that make choose_brick_shape pick the brick logs named (the brick as close to a cube in world space as powers of two allow)
CELL_SIZES = {(2, 2, 2): (1.0, 1.0, 1.0), (1, 2, 3): (4.0, 2.0, 1.0), (3, 2, 1): (1.0, 2.0, 4.0)}


def hook():
    fn = _lib.lib().m2s_debug_walk_consts
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(M2SGrid), C.POINTER(M2SOpts), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    return fn


def resolved(counts, sizes, slab=None, xl_cap=0, n_nodes=1, x_period=0):
    g = M2SGrid()
    for k in range(3):
        g.first_cell[k], g.cell_size[k], g.cell_count[k] = 0.0, sizes[k], counts[k]
    o = M2SOpts()
    o.struct_size = C.sizeof(M2SOpts)
    if slab is not None:
        o.x_begin, o.x_end = slab
    o.x_period = x_period
    out = (C.c_uint32 * 12)()
    rc = hook()(C.byref(g), C.byref(o), xl_cap, n_nodes, out)
    assert rc == 0, _lib.last_error()
    keys = ("sb_xl", "nby", "nbz", "sy", "sz", "sz_magic", "sy_magic", "start_bits", "bl0", "bl1", "bl2", "nbx")
    return dict(zip(keys, (int(x) for x in out)))


def ceil_shift(n, log):
    return (n + (1 << log) - 1) >> log


def model_xlog(nbx, xl_cap):
    """The widest super-brick (8, 4, 2 bricks along x; under a cap of k at most 2^(k-1)) whose padding is at most 1/8 of the bricks."""
    for xl in range(xl_cap - 1 if xl_cap else 3, 0, -1):
        padded = ceil_shift(nbx, xl) << xl
        if (padded - nbx) * 8 <= nbx:
            return xl
    return 0


def model_start_bits(n_nodes):
    """Bits that hold every record index of the tree, at least 1 and at most 27."""
    return min(27, max(1, (n_nodes - 1).bit_length()))


def model_encode_len(length, M):
    """5 bits of exponent above M bits of mantissa: the smallest mantissa << exponent that is >= length."""
    if length < 1 << M:
        return length
    e = length.bit_length() - M
    mant = (length + (1 << e) - 1) >> e
    if mant == 1 << M:
        mant, e = mant >> 1, e + 1
    return (e << M) | mant


def model(counts, bl, layers, xl_cap):
    nbx_grid = ceil_shift(counts[0], bl[0])
    nby, nbz = ceil_shift(counts[1], bl[1]), ceil_shift(counts[2], bl[2])
    sy, sz = (nby + 7) >> 3, (nbz + 7) >> 3
    safe = (nbx_grid + 1) * sy * sz * max(sy, sz) < 1 << 32
    magic = lambda d: ((1 << 32) + d - 1) // d if safe and d > 1 else 0   # noqa: E731
    return {"sb_xl": model_xlog(ceil_shift(layers, bl[0]), xl_cap), "nby": nby, "nbz": nbz, "sy": sy, "sz": sz, "sz_magic": magic(sz),
            "sy_magic": magic(sy), "nbx": ceil_shift(layers, bl[0]), "bl0": bl[0], "bl1": bl[1], "bl2": bl[2]}


@pytest.mark.parametrize("bl", sorted(CELL_SIZES))
def test_super_brick_constants(bl):
    # every count of bricks along x from 1 to 70 (ragged last brick included) under every cap; y and z ragged, more than one super-brick
    ny, nz = 37 << bl[1] >> 2, 70 << bl[2] >> 2
    for nbx in range(1, 71):
        for ragged in (0, 1):
            nx = (nbx << bl[0]) - ragged * ((1 << bl[0]) - 1)
            for xl_cap in range(5):
                got = resolved((nx, ny, nz), CELL_SIZES[bl], xl_cap=xl_cap)
                want = model((nx, ny, nz), bl, nx, xl_cap)
                assert {k: got[k] for k in want} == want, (bl, nbx, ragged, xl_cap)


@pytest.mark.parametrize("bl", sorted(CELL_SIZES))
def test_slab_constants(bl):
    # a slab's x-log follows ITS bricks along x, the magics the whole grid's; y and z do not change with the slab
    counts = (70 << bl[0], 9 << bl[1], 100 << bl[2])
    for xb, xe in ((0, counts[0]), (5, 23), (5, 6), (16, 16 + (4 << bl[0])), (3, counts[0] - 1)):
        for xl_cap in range(5):
            got = resolved(counts, CELL_SIZES[bl], slab=(xb, xe), xl_cap=xl_cap)
            want = model(counts, bl, xe - xb, xl_cap)
            assert {k: got[k] for k in want} == want, (bl, xb, xe, xl_cap)


def test_interleaved_slab_constants():
    # x_period: the constants are those of the VIRTUAL slab, the call's chunks laid end to end (two chunks of 16 layers here)
    got = resolved((40, 40, 40), CELL_SIZES[(2, 2, 2)], slab=(8, 24), x_period=16)
    want = model((40, 40, 40), (2, 2, 2), 32, 0)
    assert {k: got[k] for k in want} == want


def test_magic_division_is_exact_where_it_is_used():
    # what brick_coords does with the constants: super-brick index -> (sbx, sby, sbz), for every index of the padded launch
    for counts in ((20, 36, 52), (8, 64, 64), (4, 40, 40), (256, 250, 254), (33, 700, 9)):
        c = resolved(counts, CELL_SIZES[(2, 2, 2)])
        n_super = ceil_shift(c["nbx"], c["sb_xl"]) * c["sy"] * c["sz"]
        for sb in list(range(min(n_super, 4096))) + [n_super - 1]:
            t = (sb * c["sz_magic"]) >> 32 if c["sz_magic"] else sb // c["sz"]
            sbx = (t * c["sy_magic"]) >> 32 if c["sy_magic"] else t // c["sy"]
            assert (t, sbx) == (sb // c["sz"], sb // c["sz"] // c["sy"]), (counts, sb)


N_NODES = sorted({1, 2, 3, 4, 5, (1 << 27) + 5} | {(1 << k) + d for k in range(2, 28) for d in (-1, 0, 1)})


def test_start_bits_and_list_words():
    cut_code = _lib.lib().m2s_debug_cut_code
    cut_code.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    cut_code.restype = C.c_int
    out = (C.c_uint32 * 3)()
    for n in N_NODES:
        S = resolved((8, 8, 8), CELL_SIZES[(2, 2, 2)], n_nodes=n)["start_bits"]
        assert S == model_start_bits(n), n
        if n > 1 << 26:
            continue   # (m2s_debug_cut_code takes trees of up to 2^26 records: the build's limit is 2^25 triangles)
        # the list word of a range, written and read back, is what these start bits give: the start exact, the length as the smallest
        # mantissa << exponent that covers it (M = 27 - S bits of mantissa, 5 of exponent), the end clipped to the tree
        M = 27 - S
        for start, length in {(0, 1), (0, n), (n - 1, 1), (n // 2, n - n // 2), (n // 3, max(1, n // 5))}:
            assert cut_code(n, start, length, out) == 0, (n, start, length)
            word, first, end = int(out[0]), int(out[1]), int(out[2])
            code = model_encode_len(length, M)
            decoded = (code & ((1 << M) - 1)) << (code >> M)
            assert word == start | (code << S), (n, start, length)
            assert first == start and end == min(start + decoded, n) and start + length <= end, (n, start, length)


def test_bad_arguments():
    out = (C.c_uint32 * 12)()
    g = M2SGrid()
    assert hook()(None, None, 0, 1, out) != 0
    assert hook()(C.byref(g), None, 5, 1, out) != 0
