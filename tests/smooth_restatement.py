"""The rules of include/supnerf_hip.h ("Mesh smoothing") restated in numpy: one plain function per rule, exact integers and float64
arithmetic in the order the header fixes, no kernel code.  The GPU tests compare the package against it bit for bit; the CPU tests hold
the restatement itself against hand results and against what smoothing must do to a noisy sphere.  ``planted`` switches in a deliberate
mistake, so that the checks can be shown to reject one.

Every float64 sum runs over the neighbours of a vertex in ascending order from 0.0.  ``_ring_sum`` does that for all vertices at once:
pass k adds every vertex's k-th neighbour, so each vertex sees its own terms one after the other in its own order."""
import numpy as np

from simplify_restatement import Rejected, box_mesh, signed_volume, tetrahedron  # noqa: F401  (shared with the tests)

MAX_CHANNELS = 16
LAMBDA, MU = 0.5, -0.53
PLANTED = ("multiplicity", "gauss_seidel", "stale_mu")


# ------------------------------------------------------------------ rule 1
def face_pairs(faces, n_verts):
    """Per face the set of unordered pairs {i, j}, i < j, of its distinct indices; a face with an index outside [0, V) is rejected."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if ((f < 0) | (f >= n_verts)).any():
        raise Rejected("a face index lies outside the mesh")
    return [{(min(a, b), max(a, b)) for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])) if a != b} for t in f.tolist()]


# ------------------------------------------------------------------ rule 2
def adjacency(faces, n_verts):
    """dict(nbr_start (V + 1) int64, nbr (E2) int32 ascending within each vertex, edge_faces (E2) int32, degree (V) int32)."""
    count = {}
    for pairs in face_pairs(faces, n_verts):
        for e in pairs:
            count[e] = count.get(e, 0) + 1
    rings = [[] for _ in range(n_verts)]
    for (a, b), c in count.items():
        rings[a].append((b, c))
        rings[b].append((a, c))
    rings = [sorted(r) for r in rings]
    degree = np.array([len(r) for r in rings], np.int32).reshape(n_verts)
    flat = [e for r in rings for e in r]
    return dict(nbr_start=np.concatenate([[0], np.cumsum(degree, dtype=np.int64)]).astype(np.int64),
                nbr=np.array([j for j, _ in flat], np.int32).reshape(-1), edge_faces=np.array([c for _, c in flat], np.int32).reshape(-1),
                degree=degree)


# ------------------------------------------------------------------ rule 3
def classes(adj, n_faces):
    """dict(boundary (V) bool, nonmanifold (V) bool, boundary_edges, nonmanifold_edges, closed)."""
    V = adj["degree"].shape[0]
    owner = np.repeat(np.arange(V), adj["degree"])
    one, many = adj["edge_faces"] == 1, adj["edge_faces"] > 2
    boundary, nonmanifold = np.zeros(V, bool), np.zeros(V, bool)
    boundary[owner[one]] = True
    nonmanifold[owner[many]] = True
    lower = owner < adj["nbr"]                           # every undirected edge once
    be, ne = int((one & lower).sum()), int((many & lower).sum())
    return dict(boundary=boundary, nonmanifold=nonmanifold, boundary_edges=be, nonmanifold_edges=ne, closed=n_faces > 0 and be == 0 and ne == 0)


# ------------------------------------------------------------------ rule 4
def _ring_sum(values64, adj, weights=None):
    """s (V, C) float64: s = 0.0; for j over N(i) ascending: s += values[j] (times weights[entry], for the planted mistake)."""
    start, nbr, deg = adj["nbr_start"], adj["nbr"], adj["degree"]
    s = np.zeros_like(values64)
    for k in range(int(deg.max(initial=0))):
        has = np.nonzero(deg > k)[0]
        e = start[has] + k
        term = values64[nbr[e]]
        s[has] += term if weights is None else term * weights[e][:, None]
    return s


def umbrella(x, adj, planted=None):
    """U (V, C) float64 of x (V, C) fp32: s / d - x, 0 where d = 0."""
    x64 = np.asarray(x, np.float32).astype(np.float64).reshape(len(x), -1)
    d = adj["degree"].astype(np.float64)
    if planted == "multiplicity":                        # neighbours weighted by the number of faces on the edge
        w = adj["edge_faces"].astype(np.float64)
        s, d = _ring_sum(x64, adj, w), _ring_sum(np.ones((len(x64), 1)), adj, w)[:, 0]
    else:
        s = _ring_sum(x64, adj)
    with np.errstate(all="ignore"):
        u = s / d[:, None] - x64
    u[adj["degree"] == 0] = 0.0
    return u


# ------------------------------------------------------------------ rule 5
def step(x, adj, f, pinned=None, planted=None):
    """x' (V, C) fp32 = (float)((double) x + f U); a pinned vertex and one of degree 0 keep their bits."""
    x = np.asarray(x, np.float32).reshape(len(x), -1)
    keep = adj["degree"] == 0
    if pinned is not None:
        keep = keep | np.asarray(pinned, bool)
    if planted == "gauss_seidel":                        # in place: a vertex reads neighbours that have already moved
        out = x.copy()
        for i in np.nonzero(~keep)[0]:
            ring = adj["nbr"][adj["nbr_start"][i]:adj["nbr_start"][i + 1]]
            s = np.zeros(x.shape[1])
            for j in ring:
                s += out[j].astype(np.float64)
            out[i] = (out[i].astype(np.float64) + float(f) * (s / len(ring) - out[i].astype(np.float64))).astype(np.float32)
        return out
    with np.errstate(all="ignore"):
        out = (x.astype(np.float64) + float(f) * umbrella(x, adj, planted)).astype(np.float32)
    out[keep] = x[keep]
    return out


# ------------------------------------------------------------------ rule 6
def taubin(x, adj, iterations=10, lam=LAMBDA, mu=MU, pinned=None, planted=None):
    """``iterations`` times: a step with lam, then (mu not None) a step with mu on its result."""
    x = np.asarray(x, np.float32).reshape(len(x), -1).copy()
    for _ in range(iterations):
        if planted == "stale_mu" and mu is not None:     # the mu step with the U of before the lam step
            u = umbrella(x, adj)
            y = step(x, adj, lam, pinned)
            z = (y.astype(np.float64) + float(mu) * u).astype(np.float32)
            keep = (adj["degree"] == 0) | (np.zeros(len(x), bool) if pinned is None else np.asarray(pinned, bool))
            z[keep] = x[keep]
            x = z
            continue
        x = step(x, adj, lam, pinned, planted)
        if mu is not None:
            x = step(x, adj, mu, pinned, planted)
    return x


# ------------------------------------------------------------------ rule 7
def laplacian(x, adj):
    with np.errstate(all="ignore"):
        return umbrella(x, adj).astype(np.float32)


def transpose64(g, adj):
    """(V, C) float64: t = 0.0; for j over N(i) ascending: t += g_j / d_j; t - g_i where d_i > 0, else t."""
    g64 = np.asarray(g).astype(np.float64).reshape(len(g), -1)
    with np.errstate(all="ignore"):
        t = _ring_sum(g64 / adj["degree"].astype(np.float64)[:, None], adj)
        return np.where((adj["degree"] > 0)[:, None], t - g64, t)


def transpose(g, adj):
    with np.errstate(all="ignore"):
        return transpose64(np.asarray(g, np.float32), adj).astype(np.float32)


def dense_operator(adj):
    """L (V, V) float64 with U = L x: 1 / d_i at (i, j in N(i)), -1 at (i, i) where d_i > 0."""
    V = adj["degree"].shape[0]
    L = np.zeros((V, V))
    owner = np.repeat(np.arange(V), adj["degree"])
    L[owner, adj["nbr"]] = 1.0 / adj["degree"][owner]
    L[np.arange(V), np.arange(V)] = -(adj["degree"] > 0).astype(np.float64)
    return L


# ------------------------------------------------------------------ the energy and its gradient, float64
def energy_and_gradient(x, adj):
    """(E, dE/dx (V, C) float64, bound (V, C)) of E = mean over the vertices of degree > 0 of |U_i|^2 (0 for none), x fp32.  dE/dU = g =
    2 U / n, dE/dx = L^T g.  ``bound`` = sum_{j in N(i)} |g_j| / d_j + |g_i|: what the fp32 roundings on the way are relative to."""
    u = umbrella(x, adj)
    n = max(int((adj["degree"] > 0).sum()), 1)
    g = 2.0 * u / n
    bound = _ring_sum(np.abs(g) / np.maximum(adj["degree"], 1).astype(np.float64)[:, None], adj) + np.abs(g)
    return float((u ** 2).sum() / n), transpose64(g, adj), bound


# ------------------------------------------------------------------ meshes
def fan(n):
    """An open fan: hub 0 and n rim vertices 1 .. n on an arc of a wobbling circle, faces (0, i, i + 1): the hub has degree n."""
    assert n >= 2
    a = np.linspace(0.0, 1.5 * np.pi, n)
    r = 1.0 + 0.1 * np.cos(7.0 * a)
    rim = np.stack([r * np.cos(a), r * np.sin(a), 0.05 * np.sin(3.0 * a)], 1)
    verts = np.concatenate([[[0.013, -0.021, 0.1]], rim]).astype(np.float32)
    i = np.arange(1, n)
    return verts, np.stack([np.zeros_like(i), i, i + 1], 1).astype(np.int32)


def strip(n):
    """A triangle strip of n vertices, faces (i, i + 1, i + 2) with alternating winding, gently curved."""
    assert n >= 3
    i = np.arange(n)
    verts = np.stack([0.01 * i, 0.25 * (i & 1) + 0.02 * np.sin(0.3 * i), 0.05 * np.cos(0.11 * i)], 1).astype(np.float32)
    k = np.arange(n - 2)
    f = np.stack([k, k + 1, k + 2], 1)
    f[1::2] = f[1::2, ::-1]
    return verts, f.astype(np.int32)


def icosphere(level=3, radius=1.0):
    """A subdivided icosahedron on the sphere of ``radius``, wound outward: 10 4^level + 2 vertices, 20 4^level faces (3: 642 / 1 280)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    pts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
           (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
             (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    pts = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in pts]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = pts[a] + pts[b]
                pts.append(m / np.linalg.norm(m))
                mid[key] = len(pts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return (radius * np.asarray(pts)).astype(np.float32), np.asarray(faces, np.int32)


def noisy_sphere(level=3, radius=0.3, noise=0.01, seed=0):
    """The icosphere with each vertex moved along its radius by noise * standard_normal, rounded to fp32."""
    unit, faces = icosphere(level, 1.0)
    r = radius + noise * np.random.default_rng(seed).standard_normal(unit.shape[0])
    return (unit.astype(np.float64) * r[:, None]).astype(np.float32), faces


def open_box(half=(0.25, 0.2, 0.15), n=24):
    """``box_mesh`` without the faces of its side z = +half: the rim is that side's outline, 4 n vertices and 4 n boundary edges; the
    (n - 1)^2 vertices inside the removed side stay in the vertex array with no face."""
    verts, faces = box_mesh(half, n)
    top = (verts[faces][:, :, 2] == verts[:, 2].max()).all(1)
    return verts, np.ascontiguousarray(faces[~top])


def radii(verts):
    return np.sqrt((np.asarray(verts, np.float64) ** 2).sum(1))
