"""A float64 model of what the nearest-triangle walks rely on (plain numpy, nothing of the library): the record layouts of
csrc/common.h as numpy dtypes, the exact point-triangle distance, the decoding of the resident pre-order tree, the point sets at which a
lower bound is most likely to be wrong, and the checks of the stored bounds against the geometry they must contain.

Every truth value is computed in float64 FROM the float32 inputs as they are (points are formed in float64, rounded to float32, and only
the rounded point is used afterwards)."""
import numpy as np

F = np.float32
U = 2.0 ** -24            # unit roundoff of float32

# ---- csrc/common.h ----------------------------------------------------------------------------------------------------------------------
TRI = np.dtype([("a", "<f4", 3), ("cls", "<u4"), ("b", "<f4", 3), ("index", "<u4"), ("c", "<f4", 3), ("pad0", "<f4"),
                ("ab", "<f4", 3), ("nrx", "<f4"), ("ac", "<f4", 3), ("nry", "<f4"), ("bc", "<f4", 3), ("nrz", "<f4")])
PLANES = np.dtype([("n", "<f4", 3), ("dn", "<f4"), ("m0", "<f4", 3), ("o0", "<f4"), ("m1", "<f4", 3), ("o1", "<f4"),
                   ("m2", "<f4", 3), ("o2", "<f4")])
NODE = np.dtype([("mn", "<f4", 3), ("skip", "<u4"), ("mx", "<f4", 3), ("tri", "<i4")])
EXT = np.dtype([("c", "<f4", 3), ("R", "<f4"), ("n", "<f4", 3), ("mid", "<f4"), ("half", "<f4"), ("skip", "<u4"), ("tri", "<i4"),
                ("pad", "<u4")])
DTYPES = {"tris": TRI, "planes": PLANES, "nodes": NODE, "ext": EXT}
ITEMSIZE = {"tris": 96, "planes": 64, "nodes": 32, "ext": 48}     # the static_asserts of common.h
TRI_REGULAR = 0                                                    # geo.hip.h tri_class


def mesh_scale(scene):
    """scene[6]: the largest finite |coordinate| of the triangle-box centres, as float bits.  (The walks' slack takes the scale of the
    vertices, csrc/common.h mesh_scale, which is never smaller: a comparison that prunes nothing with this scale prunes nothing with theirs.)"""
    return float(np.asarray(scene, np.uint32)[6:7].view(F)[0])


# ---- exact distance ---------------------------------------------------------------------------------------------------------------------
def _seg_dist2(p, a, b):
    ab, ap = b - a, p - a
    den = np.einsum("ij,ij->i", ab, ab)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(den > 0, np.einsum("ij,ij->i", ap, ab) / np.where(den > 0, den, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    d = ap - t[:, None] * ab
    return np.einsum("ij,ij->i", d, d)


def point_triangle_dist2(p, a, b, c):
    """Squared distance from p[i] to the triangle (a[i], b[i], c[i]) in float64: the regions of Ericson's closest-point routine (Real-Time
    Collision Detection 5.1.5) decide whether the foot of the perpendicular lies inside, where the plane distance counts; everywhere else
    the nearest point lies on an edge, and the three clamped edge projections cover the edge and vertex regions.  A triangle whose vertices
    coincide or are collinear has no inside, so segments and points come out of the same code."""
    p, a, b, c = (np.asarray(x, np.float64).reshape(-1, 3) for x in (p, a, b, c))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d2 = np.minimum(np.minimum(_seg_dist2(p, a, b), _seg_dist2(p, b, c)), _seg_dist2(p, c, a))
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        dot = lambda x, y: np.einsum("ij,ij->i", x, y)   # noqa: E731
        d1, d2_, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2_          # Ericson: the barycentric weights of c, b and a, unnormalised
        vb = d5 * d2_ - d1 * d6
        va = d3 * d6 - d5 * d4
        n = np.cross(ab, ac)
        nn = dot(n, n)
        inside = (va > 0) & (vb > 0) & (vc > 0) & (nn > 0)
        h = dot(n, ap)
        face = np.where(inside, h * h / np.where(nn > 0, nn, 1.0), np.inf)
    return np.minimum(d2, face)


def point_triangle_distance(p, a, b, c):
    return np.sqrt(point_triangle_dist2(p, a, b, c))


# ---- the resident tree ------------------------------------------------------------------------------------------------------------------
def subtree_counts(skip):
    """Triangles below every pre-order slot: cnt = (skip - i + 1) / 2."""
    skip = np.asarray(skip, np.int64)
    return (skip - np.arange(skip.size) + 1) // 2


def tree_errors(skip, slot_first, n_tris):
    """What is wrong with the skip links as a pre-order binary tree of 2 n - 1 slots over the triangles [0, n) (empty list: nothing).
    The left child of i is i + 1, the right child is where the left one's skip points, and both end where i ends."""
    skip, first = np.asarray(skip, np.int64), np.asarray(slot_first, np.int64)
    n_nodes = 2 * n_tris - 1 if n_tris else 0
    bad = []
    if skip.size != n_nodes or first.size != n_nodes:
        return [f"{skip.size} nodes, {first.size} slot_first entries for {n_tris} triangles"]
    if n_nodes == 0:
        return bad
    i = np.arange(n_nodes)
    if skip[0] != n_nodes or first[0] != 0:
        bad.append(f"root: skip {skip[0]}, first {first[0]}")
    if ((skip - i) % 2 != 1).any() or (skip <= i).any() or (skip > n_nodes).any():
        return bad + ["a skip link is not an odd number of slots ahead, inside the array"]
    cnt = subtree_counts(skip)
    inner = np.flatnonzero(cnt > 1)
    left = inner + 1
    right = skip[left]
    if (right >= skip[inner]).any():
        return bad + ["a left subtree does not end inside its parent"]
    for what, ok in (("right child ends with its parent", skip[right] == skip[inner]),
                     ("children's counts add up", cnt[left] + cnt[right] == cnt[inner]),
                     ("left child starts at the parent's first triangle", first[left] == first[inner]),
                     ("right child starts behind the left one's triangles", first[right] == first[inner] + cnt[left])):
        if not ok.all():
            bad.append(f"{what}: fails at slot {inner[np.flatnonzero(~ok)[0]]}")
    if (first < 0).any() or (first + cnt > n_tris).any():
        bad.append("a subtree's triangles leave [0, n)")
    return bad


def ancestors(skip, slot_first, tri_slots):
    """Every (triangle, node) pair with the node on the path from the root to the triangle's own slot, both ends included, found by
    descending from the root: returns (k, node) with k an index into tri_slots."""
    skip, first = np.asarray(skip, np.int64), np.asarray(slot_first, np.int64)
    cnt = subtree_counts(skip)
    t = np.asarray(tri_slots, np.int64)
    k = np.arange(t.size)
    node = np.zeros(t.size, np.int64)
    out_k, out_n = [], []
    for _ in range(4 * 64):
        out_k.append(k)
        out_n.append(node)
        go = cnt[node] > 1
        k, node, tt = k[go], node[go], t[k[go]]
        if k.size == 0:
            break
        left = node + 1
        node = np.where(tt < first[left] + cnt[left], left, skip[left])
    else:
        raise AssertionError("the descent does not end: the skip links are no tree")
    return np.concatenate(out_k), np.concatenate(out_n)


# ---- point sets -------------------------------------------------------------------------------------------------------------------------
LADDER = np.array([1e-6, 1e-3, 1.0, 1e3])
RADII = np.array([0.0, 0.99, 1.0, 1.01, 6.4, 100.0])          # 6.4 node radii: where walk.hip.h's e_B <= 7 u starts to hold
ALONG = np.array([0.0, 1.0, -1.0, 1.01, -1.01])               # mid +- half x {0, 1, 1.01}
INTERIOR = np.array([[1 / 3, 1 / 3, 1 / 3], [0.6, 0.3, 0.1], [0.1, 0.15, 0.75]])
N_FAR = 6


def _unit(v, fallback):
    """v / |v| row by row; `fallback` rows where that is not a finite unit vector."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        l = np.sqrt(np.einsum("ij,ij->i", v, v))
        u = v / l[:, None]
    ok = np.isfinite(u).all(1) & (l > 0)
    return np.where(ok[:, None], u, fallback)


def _perpendiculars(n):
    """Two unit vectors perpendicular to each row of n and to each other."""
    k = np.argmin(np.abs(n), axis=1)
    e = np.eye(3)[k]
    w0 = _unit(np.cross(n, e), np.array([0.0, 1.0, 0.0]))
    w1 = _unit(np.cross(n, w0), np.array([0.0, 0.0, 1.0]))
    return w0, w1


def triangle_points(a, b, c, scale, rng):
    """The points of one triangle set, float64 [K, P, 3]: on the triangle, above interior points, in its plane outside it, and far away."""
    a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
    K = a.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        ab, ac, bc = b - a, c - a, c - b
        L = np.sqrt(np.maximum(np.maximum((ab * ab).sum(1), (ac * ac).sum(1)), (bc * bc).sum(1)))
        nh = _unit(np.cross(ab, ac), np.array([0.0, 0.0, 1.0]))
        cen = (a + b + c) / 3.0
        inner = [w[0] * a + w[1] * b + w[2] * c for w in INTERIOR]
        mids = [(a + b) / 2, (b + c) / 2, (c + a) / 2]
        pts = inner + mids + [a, b, c]                                                     # on T
        steps = L[:, None, None] * LADDER[None, :, None]                                    # [K, 4, 1]
        for q in inner[1:]:                                                                 # above T: the l^2 = v^2 - t^2 cancellation
            for s in (1.0, -1.0):
                pts += list(np.moveaxis(q[:, None, :] + s * steps * nh[:, None, :], 1, 0))
        for (m, e, opp) in zip(mids, (ab, bc, -ac), (c, a, b)):                             # across each edge
            out = _unit(np.cross(e, nh), np.array([1.0, 0.0, 0.0]))
            out = np.where((np.einsum("ij,ij->i", out, opp - m) > 0)[:, None], -out, out)
            pts += list(np.moveaxis(m[:, None, :] + steps * out[:, None, :], 1, 0))
        for v in (a, b, c):                                                                 # beyond each vertex: the planes bound underestimates
            out = _unit(v - cen, np.array([1.0, 0.0, 0.0]))
            pts += list(np.moveaxis(v[:, None, :] + steps * out[:, None, :], 1, 0))
        d = _unit(rng.standard_normal((N_FAR, K, 3)).reshape(-1, 3), np.array([1.0, 0.0, 0.0])).reshape(N_FAR, K, 3)
        r = L[None, :] * 10.0 ** rng.uniform(-6.0, 4.0, (N_FAR, K))
        pts += list(cen[None] + d * r[:, :, None])                                          # far away
        pts += [np.broadcast_to(1.0e6 * scale * np.eye(3)[k], (K, 3)) for k in range(3)]
    return np.stack(pts, 1)


def disc_points(ext):
    """Around the disc-shaped slab of every record of `ext`: c + n (mid +- half {0, 1, 1.01}) + R {0, .99, 1, 1.01, 6.4, 100} w for two unit
    vectors w perpendicular to n; float64 [len(ext), 60, 3]."""
    c, n = ext["c"].astype(np.float64), ext["n"].astype(np.float64)
    mid, half, R = (ext[k].astype(np.float64) for k in ("mid", "half", "R"))
    w0, w1 = _perpendiculars(n)
    with np.errstate(invalid="ignore", over="ignore"):
        t = mid[:, None] + half[:, None] * ALONG[None, :]                                   # [E, 5]
        axis = c[:, None, :] + t[:, :, None] * n[:, None, :]                                # [E, 5, 3]
        lat = [R[:, None, None] * RADII[None, :, None] * w[:, None, :] for w in (w0, w1)]   # 2 x [E, 6, 3]
        pts = [axis[:, :, None, :] + l[:, None, :, :] for l in lat]                         # 2 x [E, 5, 6, 3]
    return np.concatenate([q.reshape(len(ext), -1, 3) for q in pts], 1)


def round_points(p64):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(p64, np.float64).astype(F)


# ---- the stored bounds against the geometry ---------------------------------------------------------------------------------------------
def tri_vertices(tris):
    """float64 [n, 3 vertices, 3] and the mask of finite vertices [n, 3]."""
    v = np.stack([tris["a"], tris["b"], tris["c"]], 1).astype(np.float64)
    return v, np.isfinite(v).all(2)


def box_violations(nodes, tris, pair_tri, pair_node):
    """(triangle, node, vertex) triples whose finite vertex lies outside the node's box: exact float32 comparisons."""
    v32 = np.stack([tris["a"], tris["b"], tris["c"]], 1)[pair_tri]                        # [P, 3, 3]
    fin = np.isfinite(v32).all(2)
    mn, mx = nodes["mn"][pair_node][:, None, :], nodes["mx"][pair_node][:, None, :]
    with np.errstate(invalid="ignore"):
        out = ((v32 < mn) | (v32 > mx)).any(2) & fin
    return np.argwhere(out)


def ext_reserves(ext, tris, pair_tri, pair_node):
    """For every (triangle, node) pair and vertex: what the slab and the radius have left over, float64 on the stored float32 n and c as they
    are: slab = half - |n.(x - c) - mid|, rad = R^2 - (|x - c|^2 - (n.(x - c))^2), and |x - c|.  A vertex is OUTSIDE where slab < 0 or rad < 0;
    a comparison that a NaN in the record makes false counts as inside, as ext_dist2's fmaxf(NaN, 0) = 0 counts it.  Non-finite vertices: +inf."""
    v, fin = tri_vertices(tris)
    e = ext[pair_node]
    with np.errstate(invalid="ignore", over="ignore"):
        w = v[pair_tri] - e["c"].astype(np.float64)[:, None, :]
        n = e["n"].astype(np.float64)[:, None, :]
        t = (w * n).sum(2)
        w2 = (w * w).sum(2)
        slab = e["half"].astype(np.float64)[:, None] - np.abs(t - e["mid"].astype(np.float64)[:, None])
        rad = e["R"].astype(np.float64)[:, None] ** 2 - (w2 - t * t)
    f = fin[pair_tri]
    size = np.sqrt(w2)
    return np.where(f, slab, np.inf), np.where(f, rad, np.inf), size


def outside(reserve):
    """The negation of `reserve >= 0` that a NaN does not satisfy: what the walk's own comparisons would prune by."""
    with np.errstate(invalid="ignore"):
        return reserve < 0


def plane_reserves(planes, tris):
    """Per triangle with a non-zero pre-test record (mask `has`), over its three vertices, in float64:
    edge = min over k and x of -(m_k.x - o_k);  face = 8 x 2^-23 vmax - max |n.x - dn|;  unit = 4 x 2^-24 - max(||n| - 1|, ||m_k| - 1|);
    and vmax, the largest |coordinate| of the triangle."""
    has = planes.view(np.uint32).reshape(len(planes), 16).any(1)
    v, _ = tri_vertices(tris)
    with np.errstate(invalid="ignore", over="ignore"):
        vmax = np.abs(v).max((1, 2))
        edge = np.full(len(planes), np.inf)
        unit_err = np.abs(np.sqrt((planes["n"].astype(np.float64) ** 2).sum(1)) - 1.0)
        for m, o in (("m0", "o0"), ("m1", "o1"), ("m2", "o2")):
            mk = planes[m].astype(np.float64)
            e = (v * mk[:, None, :]).sum(2) - planes[o].astype(np.float64)[:, None]
            edge = np.minimum(edge, (-e).min(1))
            unit_err = np.maximum(unit_err, np.abs(np.sqrt((mk ** 2).sum(1)) - 1.0))
        h = np.abs((v * planes["n"].astype(np.float64)[:, None, :]).sum(2) - planes["dn"].astype(np.float64)[:, None]).max(1)
        face = 8.0 * 2.0 ** -23 * vmax - h
        unit = 4.0 * U - unit_err
    return has, edge, face, unit, vmax


# ---- the pruning comparison -------------------------------------------------------------------------------------------------------------
def lowered_d2(d2):
    """The largest float32 not above (max(sqrt(d2) (1 - 2^-22) - 1e-6, 0))^2: a computed distance lowered by the Normal fold's approx_eq
    window (2 ulps, or 1e-6 absolute)."""
    d2 = np.asarray(d2, F)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.maximum(np.sqrt(d2.astype(np.float64)) * (1.0 - 2.0 ** -22) - 1.0e-6, 0.0) ** 2
        y = x.astype(F)
        y = np.where(y.astype(np.float64) > x, np.nextafter(y, F(-np.inf)), y).astype(F)
    return np.where(np.isnan(d2), d2, y).astype(F)


def pruned(bound, thr):
    """The walks' comparison: a node or a triangle is skipped where its bound exceeds the threshold; a NaN keeps it."""
    with np.errstate(invalid="ignore"):
        return np.asarray(bound) > np.asarray(thr)


def needed_margin(bound, slack, delta, scale):
    """What a bound asks of the margin at each element: rel = (sqrt(bound) - slack) / delta - 1 where delta > 0, and abs = sqrt(bound) / scale
    where delta == 0 (NaN elsewhere)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b = np.sqrt(np.asarray(bound, np.float64))
        delta = np.asarray(delta, np.float64)
        rel = np.where(delta > 0, (b - slack) / delta - 1.0, np.nan)
        ab = np.where(delta == 0, b / scale, np.nan)
    return rel, ab
