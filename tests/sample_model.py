"""numpy model of area-weighted surface sampling: the contract of include/m2s.h (m2s_sample_surface) restated independently of
mesh_to_sdf_amd/csrc/sample.hip.h.  IEEE binary32 with no FMA and sums left to right for everything geometric, uint64 for the weights and
their running sums, Python integers for the 128-bit product.  The GPU must reproduce every output of `sample` bit for bit."""
import numpy as np

F = np.float32
U32 = np.uint32
U64 = np.uint64
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = U64(0xFFFFFFFF)


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011).  counter: [..., 4], key: [..., 2], both of 32-bit words held in uint64 arrays."""
    c = [np.asarray(counter[..., k], U64) & MASK for k in range(4)]
    k0, k1 = (np.asarray(key[..., k], U64) & MASK for k in range(2))
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                     # 32 x 32 bits: no overflow in uint64
        c = [(p1 >> U64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + U64(W0)) & MASK, (k1 + U64(W1)) & MASK
    return np.stack(c, -1).astype(U32)


def sample_random(seed, g):
    """The four words of the global samples g (uint64 array) under `seed`: counter (g lo, g hi, 0, 0), key (seed lo, seed hi)."""
    g = np.asarray(g, U64)
    z = np.zeros_like(g)
    seed = int(seed) & (2 ** 64 - 1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], U64), g.shape + (2,))
    return philox4x32_10(np.stack([g & MASK, g >> U64(32), z, z], -1), key)


# ---- the weights ---------------------------------------------------------------------------------------------------------------------
def triangles_of(vertices, indices=None, topology=0):
    """[n, 3, 3] f32: the triangles in the caller's order.  topology 0: consecutive triples (a trailing partial triple is dropped),
    1: a sliding window with no winding flip."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    idx = np.arange(v.shape[0]) if indices is None else np.asarray(indices).astype(np.int64).reshape(-1)
    if topology == 0:
        idx = idx[: idx.size // 3 * 3].reshape(-1, 3)
    else:
        idx = np.stack([idx[:-2], idx[1:-1], idx[2:]], -1) if idx.size >= 3 else np.zeros((0, 3), np.int64)
    return v[idx]


def raw_normal(tris):
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        e1, e2 = (b - a).astype(F), (c - a).astype(F)
        return np.stack([(e1[:, 1] * e2[:, 2]).astype(F) - (e1[:, 2] * e2[:, 1]).astype(F),
                         (e1[:, 2] * e2[:, 0]).astype(F) - (e1[:, 0] * e2[:, 2]).astype(F),
                         (e1[:, 0] * e2[:, 1]).astype(F) - (e1[:, 1] * e2[:, 0]).astype(F)], -1).astype(F)


def tri_area2(tris):
    """(A_t, n): A_t = |n| = twice the area, 0 where it is not finite."""
    n = raw_normal(tris)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s = ((n[:, 0] * n[:, 0]).astype(F) + (n[:, 1] * n[:, 1]).astype(F)).astype(F) + (n[:, 2] * n[:, 2]).astype(F)
        A = np.sqrt(s.astype(F)).astype(F)
    return np.where(np.isfinite(A), A, F(0)).astype(F), n


def exponent_of(amax):
    """floor(log2(amax)) of a positive finite f32, subnormals included (frexp is exact)."""
    m, e = np.frexp(np.float64(amax))   # amax = m 2^e, 0.5 <= m < 1
    return int(e) - 1


def weights(A):
    """(w uint64[n], e): w_t = floor(A_t 2^(37 - e)); e = None and all weights 0 when no triangle has area."""
    A = np.asarray(A, F)
    amax = A.max() if A.size else F(0)
    if not amax > 0:
        return np.zeros(A.shape, U64), None
    e = exponent_of(amax)
    w = np.floor(np.ldexp(A.astype(np.float64), 37 - e))   # exact: a power-of-two scale
    assert (w < 2.0 ** 38).all()
    return w.astype(U64), e


def table(tris):
    """(C uint64[n], W, e, area): the running sums, their total, the exponent and *area_out."""
    A, _ = tri_area2(tris)
    w, e = weights(A)
    if e is None:
        return np.zeros(A.shape, U64), 0, None, 0.0
    C = np.cumsum(w, dtype=U64)
    W = int(C[-1])
    return C, W, e, float(np.ldexp(np.float64(W), e - 38))


# ---- the pick, the fold, the point, the normal ----------------------------------------------------------------------------------------
def target(r0, r1, W):
    """floor(x W / 2^64), x = r0 | r1 << 32, with Python integers."""
    x = np.asarray(r0, U64) | (np.asarray(r1, U64) << U64(32))
    return np.array([(int(xi) * int(W)) >> 64 for xi in x.reshape(-1)], U64).reshape(x.shape)


def pick(C, T):
    return np.searchsorted(C, T, side="right").astype(np.int64)


def unit(r):
    return ((np.asarray(r, U32) >> U32(9)).astype(F) * F(2.0 ** -23)).astype(F) + F(2.0 ** -24)


def fold(r2, r3):
    up, vp = unit(r2), unit(r3)
    flip = (up + vp).astype(F) > F(1)
    return np.where(flip, (F(1) - up).astype(F), up).astype(F), np.where(flip, (F(1) - vp).astype(F), vp).astype(F)


def point(a, b, c, u, v):
    u, v = np.asarray(u, F)[..., None], np.asarray(v, F)[..., None]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return ((a + (u * (b - a).astype(F)).astype(F)).astype(F) + (v * (c - a).astype(F)).astype(F)).astype(F)


def unit_normal(n, A):
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        return (n / np.asarray(A, F)[..., None]).astype(F)


def sample(tris, n, seed=0, first_sample=0):
    """All five outputs of m2s_sample_surface for the samples first_sample .. first_sample + n - 1 of `tris` ([m, 3, 3] f32):
    dict(point f32[n, 3], triangle uint32[n], uv f32[n, 2], normal f32[n, 3], area float)."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    C, W, e, area = table(tris)
    if n == 0 or W == 0:
        return dict(point=np.zeros((0, 3), F), triangle=np.zeros(0, U32), uv=np.zeros((0, 2), F), normal=np.zeros((0, 3), F), area=area)
    g = (np.arange(n, dtype=U64) + U64(int(first_sample)))
    r = sample_random(seed, g)
    t = pick(C, target(r[:, 0], r[:, 1], W))
    u, v = fold(r[:, 2], r[:, 3])
    a, b, c = tris[t, 0], tris[t, 1], tris[t, 2]
    A, nrm = tri_area2(tris[t])
    return dict(point=point(a, b, c, u, v), triangle=t.astype(U32), uv=np.stack([u, v], -1), normal=unit_normal(nrm, A), area=area)


# ---- test meshes -----------------------------------------------------------------------------------------------------------------------
def graded_fan(n_tris=64, ratio=4000.0, seed=3):
    """A non-indexed triangle list whose areas span 1 : ratio geometrically: n_tris right triangles in the plane z = 0, side by side."""
    rng = np.random.default_rng(seed)
    side = np.sqrt(np.geomspace(1.0, ratio, n_tris))
    rng.shuffle(side)
    x0 = np.concatenate([[0.0], np.cumsum(side[:-1] + 0.25)])
    v = np.zeros((n_tris, 3, 3), F)
    v[:, 0, 0], v[:, 1, 0], v[:, 2, 0] = x0, x0 + side, x0
    v[:, 2, 1] = side
    return np.ascontiguousarray(v.reshape(-1, 3))


def with_degenerates(vertices, indices):
    """(vertices, indices) with zero-area triangles (a repeated vertex, three collinear points) and NaN-area ones (a NaN vertex, an
    overflowing cross product) mixed in between the originals, one after every third triangle."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    idx = np.asarray(indices, np.uint32).reshape(-1, 3)
    nv = v.shape[0]
    extra = np.array([[0.25, 0.5, 0.75], [1.25, 1.5, 1.75], [2.25, 2.5, 2.75],            # collinear
                      [np.nan, 0, 0],                                                       # NaN
                      [3.0e38, 0, 0], [0, 3.0e38, 0], [-3.0e38, -3.0e38, 0]], F)            # |n| overflows: not finite
    bad = np.array([[0, 0, 1], [nv, nv + 1, nv + 2], [0, 1, nv + 3], [nv + 4, nv + 5, nv + 6]], np.uint32)
    out = []
    for k, t in enumerate(idx):
        out.append(t)
        if k % 3 == 0:
            out.append(bad[(k // 3) % 4])
    return np.concatenate([v, extra]), np.asarray(out, np.uint32).reshape(-1)


def one_huge(vertices, indices, factor=1.0e6):
    """The mesh plus one far triangle whose area is `factor` times the mean area of the rest."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    idx = np.asarray(indices, np.uint32).reshape(-1)
    A, _ = tri_area2(triangles_of(v, idx))
    s = float(np.sqrt(A.astype(np.float64).mean() * factor))       # legs of a right triangle of twice-area s^2
    big = np.array([[50, 50, 50], [50 + s, 50, 50], [50, 50 + s, 50]], F)
    nv = v.shape[0]
    return np.concatenate([v, big]), np.concatenate([idx, np.array([nv, nv + 1, nv + 2], np.uint32)])
