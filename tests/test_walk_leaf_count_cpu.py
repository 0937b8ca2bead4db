"""The packet walk's leaf loop has no triangle count any more (distance.hip walk_span): a byte cursor starts at the record behind the
leaf's own and steps over two records per triangle until it has passed the leaf's skip link.  Its trip count (csrc/geo.hip.h
leaf_cursor_steps, built for the host into the CPU probe library) must be the count the walk divided out before,
(skip - off + NB) / (2 NB) with NB the size of a node record, for every (off, skip) a leaf can have (where that count is at least 1: the
counted loop took no triangle for a count of 0, the cursor always takes one — a case no tree has): a leaf of cnt triangles is a
subtree of 2 cnt - 1 pre-order records (cnt = 1: the leaf's record alone), anywhere in a tree of up to 2^25 triangles."""
import ctypes as C
import os

import numpy as np
import pytest

from mesh_to_sdf_amd import _lib

PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
NB = 48                      # sizeof(NodeExt)
MAX_TRIS = 1 << 25           # the build's limit (walk.hip.h record_at_bytes)
MAX_RECORDS = 2 * MAX_TRIS - 1


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail(f"{PROBE} missing: run __graft_entry__.build()")
    L = C.CDLL(PROBE)
    L.probe_leaf_cursor_steps_n.restype = None
    L.probe_leaf_cursor_steps_n.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def steps(probe, off, skip, nb=NB):
    off, skip = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(skip, np.uint32)
    out = np.empty(off.size, np.uint32)
    probe.probe_leaf_cursor_steps_n(off.size, off.ctypes.data, skip.ctypes.data, nb, out.ctypes.data)
    return out


def by_division(off, skip, nb=NB):
    """The count the walk formed before, in the kernel's own 32-bit arithmetic, raised to 1 where it is 0 (the do-while's first step)."""
    off, skip = np.asarray(off, np.uint32), np.asarray(skip, np.uint32)
    return np.maximum((skip - off + np.uint32(nb)) // np.uint32(2 * nb), 1).astype(np.uint32)


def test_every_leaf_size_at_every_place_in_the_largest_tree(probe):
    # leaves of 1 .. 64 triangles (the grid's rule asks for at most 16, M2S_LEAF_MAX may ask for more) at the first records, at the last
    # records the largest tree can have (byte offsets just below 2^32: the cursor's last step must not wrap), and at random records between
    rng = np.random.default_rng(20261020)
    for cnt in range(1, 65):
        records = 2 * cnt - 1
        first = np.concatenate([np.arange(0, 200), MAX_RECORDS - records - np.arange(0, 200), rng.integers(0, MAX_RECORDS - records, 2000)])
        off = (first.astype(np.uint64) * NB).astype(np.uint32)
        skip = ((first + records).astype(np.uint64) * NB).astype(np.uint32)
        assert int((first + records).max()) * NB + 2 * NB < 1 << 32
        got = steps(probe, off, skip)
        assert (got == cnt).all(), (cnt, got[got != cnt][:5])
        assert (got == by_division(off, skip)).all(), cnt


def _collapse(n_tris, leaf_max, rng, first_record, out):
    """Pre-order records of a random binary tree over n_tris triangles as the builder marks them: a subtree of at most leaf_max triangles
    is a leaf (its descendants stay in the array, behind it).  Appends (record index, skip record index, triangles) of every marked leaf."""
    records = 2 * n_tris - 1
    if n_tris <= leaf_max:
        out.append((first_record, first_record + records, n_tris))
        return records
    left = int(rng.integers(1, n_tris))
    used = 1 + _collapse(left, leaf_max, rng, first_record + 1, out)
    used += _collapse(n_tris - left, leaf_max, rng, first_record + used, out)
    assert used == records
    return records


@pytest.mark.parametrize("leaf_max", [1, 2, 3, 4, 8, 16])
def test_leaves_of_random_trees(probe, leaf_max):
    rng = np.random.default_rng(leaf_max)
    for n_tris in (1, 2, 3, 5, 17, 300, 5000):
        leaves = []
        _collapse(n_tris, leaf_max, rng, 0, leaves)
        rec, skip, cnt = (np.array(c, np.uint64) for c in zip(*leaves))
        assert int(cnt.sum()) == n_tris and int(cnt.max()) <= leaf_max
        off32, skip32 = (rec * NB).astype(np.uint32), (skip * NB).astype(np.uint32)
        got = steps(probe, off32, skip32)
        assert (got == cnt).all() and (got == by_division(off32, skip32)).all(), (n_tris, leaf_max)


def test_the_first_triangle_is_taken_whatever_the_link(probe):
    # max(.., 1): with a link less than a record behind `off` the division gives 0 and the counted loop the walk had (for k < cnt) took no
    # triangle, where the do-while takes one.  The builder never emits such a link (a leaf's skip is at least its own record further on: the
    # first two tests), so the two walks differ on no tree; this only pins what the cursor does there.  Links that are no whole number of
    # records behind `off` follow the division as well
    off = np.repeat(np.arange(0, 50, dtype=np.uint32) * NB, 400)
    skip = off + np.tile(np.arange(0, 400, dtype=np.uint32), 50)
    got = steps(probe, off, skip)
    assert (got == by_division(off, skip)).all()
    assert (got[skip <= off + NB] == 1).all()
    for nb in (16, 32, 64):
        assert (steps(probe, off, skip, nb) == by_division(off, skip, nb)).all(), nb
