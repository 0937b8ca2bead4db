"""The packet walk passes over its packet's seed triangle (distance.hip walk_span, SEEDED): one test per leaf says whether the seed's slot is one
of the leaf's triangles (csrc/geo.hip.h seed_in_leaf, built for the host into the CPU probe library).  It is one multiplication and one compare in
32-bit arithmetic that wraps, with no range check in front, so it is restated here in exact integers — tri <= seed < tri + cnt, cnt the
leaf's triangle count — and held for every leaf size, every position of the seed in the leaf, the slots next to the leaf on either side,
slots anywhere else in the largest tree the build allows (2^25 triangles, 2^26 - 1 records of 48 bytes), and "none" (0xffffffff), which must
never be found."""
import ctypes as C
import os

import numpy as np
import pytest

from mesh_to_sdf_amd import _lib

PROBE = os.path.join(os.path.dirname(_lib.SO_PATH), "libm2s_probe.so")
NB = 48                      # sizeof(NodeExt)
MAX_TRIS = 1 << 25           # the build's limit (walk.hip.h record_at_bytes)
MAX_RECORDS = 2 * MAX_TRIS - 1
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail(f"{PROBE} missing: run __graft_entry__.build()")
    L = C.CDLL(PROBE)
    L.probe_seed_in_leaf_n.restype = None
    L.probe_seed_in_leaf_n.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def found(probe, seed, tri, first_record, cnt):
    """seed_in_leaf for leaves given by their first triangle, their own record's index and their triangle count, as the walk calls it:
    below = the record behind the leaf's own, skip = the end of its 2 cnt - 1 records, both as byte offsets."""
    seed, tri, first_record, cnt = np.broadcast_arrays(*(np.atleast_1d(np.asarray(a, np.uint64)) for a in (seed, tri, first_record, cnt)))
    below = np.ascontiguousarray((first_record + 1) * NB, np.uint32)
    skip = np.ascontiguousarray((first_record + 2 * cnt - 1) * NB, np.uint32)
    assert int(((first_record + 2 * cnt - 1) * NB).max()) < 1 << 32
    seed32, tri32 = np.ascontiguousarray(seed, np.uint32), np.ascontiguousarray(tri, np.uint32)
    out = np.empty(seed32.size, np.uint8)
    probe.probe_seed_in_leaf_n(seed32.size, seed32.ctypes.data, tri32.ctypes.data, below.ctypes.data, skip.ctypes.data, NB, out.ctypes.data)
    return out.astype(bool)


def exact(seed, tri, cnt):
    seed, tri, cnt = (np.asarray(a, np.int64) for a in (seed, tri, cnt))
    return (tri <= seed) & (seed < tri + cnt) & (seed != NONE)


def test_every_leaf_size_and_every_position_of_the_seed(probe):
    # leaves of 1 .. 16 triangles at the tree's first slots, at its last, and at random places; the seed at every slot from 20 in front of the
    # leaf to 20 behind it (clipped to the tree), which covers every position inside it and both neighbours
    rng = np.random.default_rng(20261020)
    for cnt in range(1, 17):
        tri = np.concatenate([np.arange(0, 40), MAX_TRIS - cnt - np.arange(0, 40), rng.integers(0, MAX_TRIS - cnt, 500)])
        rec = np.minimum(2 * tri, MAX_RECORDS - (2 * cnt - 1))      # a pre-order record index such a leaf can have (2 first + left turns)
        for d in range(-20, cnt + 20):
            seed = tri + d
            ok = (seed >= 0) & (seed < MAX_TRIS)
            got = found(probe, seed[ok], tri[ok], rec[ok], cnt)
            want = exact(seed[ok], tri[ok], cnt)
            assert (got == want).all(), (cnt, d)
            assert want.all() == (0 <= d < cnt)


def test_seeds_anywhere_in_the_largest_tree_and_none(probe):
    rng = np.random.default_rng(7)
    n = 200000
    cnt = rng.integers(1, 17, n)
    tri = rng.integers(0, MAX_TRIS - 16, n)
    rec = rng.integers(0, MAX_RECORDS - 31, n)                      # the test reads the leaf's span alone: any place of the record will do
    seed = rng.integers(0, MAX_TRIS, n)
    seed[::4] = np.where(rng.random(n // 4) < 0.5, 0, MAX_TRIS - 1)       # the extremes: the largest differences either way
    assert (found(probe, seed, tri, rec, cnt) == exact(seed, tri, cnt)).all()
    # "none" is found in no leaf, the tree's last leaves and its first included
    for t in (0, 1, 15, 16, MAX_TRIS - 16, MAX_TRIS - 1):
        for c in range(1, 17):
            if t + c <= MAX_TRIS:
                assert not found(probe, NONE, t, min(2 * t, MAX_RECORDS - (2 * c - 1)), c).any(), (t, c)


def test_the_walk_of_a_collapsed_leaf_leaves_out_the_seed_alone(probe):
    # what walk_span does with the answer, on the host: a leaf that holds the seed is entered — its pre-order records are a tree of their own,
    # every subtree marked as the leaf it is — and a single-triangle leaf that IS the seed is passed over; every other triangle of the
    # collapsed leaf is then met exactly once, whatever the shape of the tree below it
    rng = np.random.default_rng(11)

    def build(first_tri, n, records):       # random binary tree over n triangles, pre-order: (first triangle, count, skip record)
        me = len(records)
        records.append(None)
        if n > 1:
            left = int(rng.integers(1, n))
            build(first_tri, left, records)
            build(first_tri + left, n - left, records)
        records[me] = (first_tri, n, len(records))

    for cnt in range(1, 17):
        for position in range(cnt):
            for first_tri, first_rec in ((0, 0), (1000, 3000), (MAX_TRIS - cnt, MAX_RECORDS - (2 * cnt - 1))):
                records = []
                build(first_tri, cnt, records)
                assert len(records) == 2 * cnt - 1
                seed, met, at = first_tri + position, [], 0
                while at < len(records):
                    tri, n, skip = records[at]
                    if found(probe, seed, tri, first_rec + at, n)[0]:
                        at += 1                                   # `below`: the first child, or (n == 1) the record behind the seed's own
                        continue
                    met.extend(range(tri, tri + n))               # the leaf loop
                    at = skip
                assert met == [t for t in range(first_tri, first_tri + cnt) if t != seed], (cnt, position)
