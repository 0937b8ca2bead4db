"""numpy restatement of m2s_voxelize as include/m2s.h defines it: the 13-clause triangle / cell overlap test in IEEE binary32 with no FMA
and sums left to right, the SURFACE set, and the output layouts.  Independent of the HIP sources: the candidate box of a triangle is found
by trying every index of every axis, not by a search.  `classify64` is the float64 yardstick of the conservative / tight property."""
import numpy as np

F = np.float32
_ERR = dict(over="ignore", invalid="ignore", under="ignore")


def triangles_of(vertices, indices=None, topology=0):
    """[n, 3, 3] f32 in the caller's order.  topology 0: consecutive triples; 1: a sliding window."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    idx = np.arange(v.shape[0]) if indices is None else np.asarray(indices).astype(np.int64).reshape(-1)
    if topology == 0:
        idx = idx[: idx.size // 3 * 3].reshape(-1, 3)
    else:
        idx = np.stack([idx[:-2], idx[1:-1], idx[2:]], -1) if idx.size >= 3 else np.zeros((0, 3), np.int64)
    return v[idx].reshape(-1, 3, 3)


def centres(first, size, n):
    """q(idx) = first + (float)idx * size for idx = 0 .. n-1."""
    with np.errstate(**_ERR):
        return (F(first) + (np.arange(n, dtype=np.uint64).astype(F) * F(size)).astype(F)).astype(F)


def _all_gt(x, y, z, r):
    return (x > r) & (y > r) & (z > r)


def _all_lt(x, y, z, r):
    return (x < r) & (y < r) & (z < r)


def box_pass(pa, pb, pc, q, h):
    """Box clause of one axis for every centre in q: False where it misses."""
    with np.errstate(**_ERR):
        va, vb, vc = (F(pa) - q).astype(F), (F(pb) - q).astype(F), (F(pc) - q).astype(F)
        return ~(_all_gt(va, vb, vc, F(h)) | _all_lt(va, vb, vc, F(-h)))


def overlap(tris, q, h):
    """overlap(t, cell) for broadcastable tris [..., 3, 3], centres q [..., 3] and half extents h [..., 3]."""
    tris, q, h = np.asarray(tris, F), np.asarray(q, F), np.asarray(h, F)
    with np.errstate(**_ERR):
        a, b, c = tris[..., 0, :], tris[..., 1, :], tris[..., 2, :]
        finite = np.isfinite(tris).all((-1, -2))
        e = [(b - a).astype(F), (c - b).astype(F), (a - c).astype(F)]
        n = [(e[0][..., (m + 1) % 3] * e[1][..., (m + 2) % 3]).astype(F) - (e[0][..., (m + 2) % 3] * e[1][..., (m + 1) % 3]).astype(F) for m in range(3)]
        n = [x.astype(F) for x in n]
        v = [(a - q).astype(F), (b - q).astype(F), (c - q).astype(F)]
        ok = finite & np.ones(np.broadcast(tris[..., 0, 0], q[..., 0]).shape, bool)
        for m in range(3):
            hm = h[..., m]
            ok = ok & ~(_all_gt(v[0][..., m], v[1][..., m], v[2][..., m], hm) | _all_lt(v[0][..., m], v[1][..., m], v[2][..., m], -hm))
        d = (((n[0] * v[0][..., 0]).astype(F) + (n[1] * v[0][..., 1]).astype(F)).astype(F) + (n[2] * v[0][..., 2]).astype(F)).astype(F)
        r = (((h[..., 0] * np.abs(n[0])).astype(F) + (h[..., 1] * np.abs(n[1])).astype(F)).astype(F) + (h[..., 2] * np.abs(n[2])).astype(F)).astype(F)
        ok = ok & ~((d > r) | (d < -r))
        for ej in e:
            for m in range(3):
                m1, m2 = (m + 1) % 3, (m + 2) % 3
                p = [((ej[..., m1] * vi[..., m2]).astype(F) - (ej[..., m2] * vi[..., m1]).astype(F)).astype(F) for vi in v]
                r = ((h[..., m1] * np.abs(ej[..., m2])).astype(F) + (h[..., m2] * np.abs(ej[..., m1])).astype(F)).astype(F)
                ok = ok & ~(_all_gt(p[0], p[1], p[2], r) | _all_lt(p[0], p[1], p[2], -r))
    return ok


def candidate_ranges(tri, first, size, count):
    """Per axis, the indices that pass the box clause when every index is tried (always one run); None when some axis has none."""
    out = []
    for m in range(3):
        ok = np.flatnonzero(box_pass(tri[0, m], tri[1, m], tri[2, m], centres(first[m], size[m], count[m]), F(size[m]) * F(0.5)))
        if ok.size == 0:
            return None
        assert ok[-1] - ok[0] + 1 == ok.size, "the cells that pass a box clause form one interval"
        out.append((int(ok[0]), int(ok[-1]) + 1))
    return out


def surface(tris, first, size, count):
    """occupancy uint8[nx, ny, nz] of M2S_VOXELIZE_SURFACE, and the number of candidate (column, z) cells that were examined."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    first, size = np.asarray(first, F), np.asarray(size, F)
    occ = np.zeros(tuple(int(c) for c in count), np.uint8)
    h = (size * F(0.5)).astype(F)
    q = [centres(first[m], size[m], count[m]) for m in range(3)]
    examined = 0
    for tri in tris:
        if not np.isfinite(tri).all():
            continue
        r = candidate_ranges(tri, first, size, count)
        if r is None:
            continue
        qq = np.stack(np.meshgrid(q[0][r[0][0]:r[0][1]], q[1][r[1][0]:r[1][1]], q[2][r[2][0]:r[2][1]], indexing="ij"), -1)
        examined += qq[..., 0].size
        occ[r[0][0]:r[0][1], r[1][0]:r[1][1], r[2][0]:r[2][1]] |= overlap(tri, qq, h).astype(np.uint8)
    return occ, examined


def surface_all_pairs(tris, first, size, count):
    """The definition, literally: every triangle against every cell (small inputs only)."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    first, size = np.asarray(first, F), np.asarray(size, F)
    q = np.stack(np.meshgrid(*[centres(first[m], size[m], count[m]) for m in range(3)], indexing="ij"), -1)
    h = (size * F(0.5)).astype(F)
    occ = np.zeros(q.shape[:-1], bool)
    for tri in tris:
        occ |= overlap(tri, q, h)
    return occ.astype(np.uint8)


def pack_bits(occ):
    """uint32[nx, ny, ceil(nz / 32)]: cell k of a row is bit k & 31 of word k >> 5; padding bits 0."""
    nx, ny, nz = occ.shape
    nzw = (nz + 31) // 32
    padded = np.zeros((nx, ny, nzw * 32), np.uint64)
    padded[:, :, :nz] = occ
    w = (padded.reshape(nx, ny, nzw, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


def unpack_bits(bits, nz):
    bits = np.asarray(bits).astype(np.uint32)
    b = (bits[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(bits.shape[0], bits.shape[1], -1)[:, :, :nz].astype(np.uint8)


def scan_tiles(cells, count, tile=4096):
    """(the number of tiles of `tile` mask words in a grid of `count` cells, the sorted tiles that hold any of the flat cell indices
    `cells`): the tiles whose sums the library scans when it counts or lists the set cells of a mask."""
    cells = np.asarray(cells).astype(np.int64)
    nz = int(count[2])
    nzw = (nz + 31) // 32
    words = int(count[0]) * int(count[1]) * nzw
    return -(-words // tile), np.unique(((cells // nz) * nzw + (cells % nz) // 32) // tile)


def classify64(tris, first, size, count, rel=2.0 ** -20):
    """(sure_in, sure_out) bool[nx, ny, nz]: the clauses in float64 on the exact products, each compared with a margin of `rel` times
    the magnitude of its terms.  sure_in: some triangle passes every clause by the margin; sure_out: every triangle misses some clause by
    the margin.  Cells in neither class are too close to a clause's boundary for binary32 to be held to either answer."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3).astype(np.float64)
    first, size = np.asarray(first, F).astype(np.float64), np.asarray(size, F).astype(np.float64)
    axes = [first[m] + np.arange(count[m], dtype=np.float64) * size[m] for m in range(3)]
    h = size * 0.5
    shape = tuple(int(c) for c in count)
    sure_in = np.zeros(shape, bool)
    sure_out = np.ones(shape, bool)
    for tri in tris:
        if not np.isfinite(tri).all():
            continue
        # where a box clause alone misses by the margin the triangle is surely out: only the rest of the grid needs the other clauses
        sl = []
        for m in range(3):
            mag = rel * (np.abs(tri[:, m]).max() + np.abs(axes[m]) + h[m])
            maybe = np.flatnonzero(~((tri[:, m].min() - axes[m] > h[m] + mag) | (tri[:, m].max() - axes[m] < -h[m] - mag)))
            sl.append(slice(int(maybe[0]), int(maybe[-1]) + 1) if maybe.size else None)
        if any(x is None for x in sl):
            continue
        q = np.stack(np.meshgrid(*[axes[m][sl[m]] for m in range(3)], indexing="ij"), -1)
        a, b, c = tri
        e = [b - a, c - b, a - c]
        n = np.cross(e[0], e[1])
        v = [a - q, b - q, c - q]
        inside = np.ones(q.shape[:-1], bool)
        outside = np.zeros(q.shape[:-1], bool)

        def clause(lo, hi, r, mag):
            # the projections span [lo, hi]; the box spans [-r, r]
            nonlocal inside, outside
            m = rel * mag
            outside |= (lo > r + m) | (hi < -r - m)
            inside &= (lo <= r - m) & (hi >= -r + m)

        for m in range(3):
            p = np.stack([vi[..., m] for vi in v])
            clause(p.min(0), p.max(0), h[m], np.abs(tri[:, m]).max() + np.abs(q[..., m]) + h[m])
        d = (n * v[0]).sum(-1)
        r = (h * np.abs(n)).sum()
        clause(d, d, r, (np.abs(n) * np.abs(v[0])).sum(-1) + r)
        for ej in e:
            for m in range(3):
                m1, m2 = (m + 1) % 3, (m + 2) % 3
                p = np.stack([ej[m1] * vi[..., m2] - ej[m2] * vi[..., m1] for vi in v])
                r = h[m1] * abs(ej[m2]) + h[m2] * abs(ej[m1])
                mag = np.stack([abs(ej[m1]) * np.abs(vi[..., m2]) + abs(ej[m2]) * np.abs(vi[..., m1]) for vi in v]).max(0) + r
                clause(p.min(0), p.max(0), r, mag)
        sure_in[sl[0], sl[1], sl[2]] |= inside
        keep = np.ones(shape, bool)
        keep[sl[0], sl[1], sl[2]] = outside
        sure_out &= keep
    return sure_in, sure_out
