"""The rules of include/supnerf_hip.h ("Mesh containment") restated in numpy float64: one plain function per rule, no kernel code.  The
library is built without fused multiply-adds, so IEEE float64 operations in the written order give the same bits here as on the device,
and the results are integers: the GPU tests compare them with ``==``.  ``brute_force`` is W5 -- the definition of the answer; ``walk``
is the pruned form over the grid of "Mesh distance" D3 (tests/nearest_restatement.py's ``grid`` / ``cell_of`` / ``cell_lists``) and must
give the same, as must ``column_walk``, the form W6 allows on a run of z-points.  ``planted`` switches in one deliberate mistake, so that
the checks can be shown to reject it.

Inputs are what the kernels take (fp32 vertices and queries), widened."""
import functools

import numpy as np

import nearest_restatement as NR
import smooth_restatement as MS

PLANTED = ("no_eps_both", "no_eps_neither", "stored_anchor", "guard_le", "t_ge", "sigma_dropped", "every_cell")
RULES = ("nonzero", "positive", "odd")
F32 = np.float32


def _sign(x):
    return (x > 0).astype(np.int64) - (x < 0).astype(np.int64)


# ------------------------------------------------------------------ W1
def box_guard(p, a, b, c, planted=None):
    """min x <= p_x < max x, min y <= p_y < max y and p_z < max z over the three corners; broadcastable (..., 3) float64."""
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    if planted == "guard_le":
        return (lo[..., 0] <= p[..., 0]) & (p[..., 0] <= hi[..., 0]) & (lo[..., 1] <= p[..., 1]) & (p[..., 1] <= hi[..., 1]) & \
            (p[..., 2] <= hi[..., 2])
    return (lo[..., 0] <= p[..., 0]) & (p[..., 0] < hi[..., 0]) & (lo[..., 1] <= p[..., 1]) & (p[..., 1] < hi[..., 1]) & \
        (p[..., 2] < hi[..., 2])


# ------------------------------------------------------------------ W2
def edge_side(u, v, p, planted=None):
    """The side of p of the directed edge u -> v: +1 left, -1 right, from the endpoints in lexicographic (x, y) order; ties as if the
    query were (p_x + e, p_y + e^2).  0 only for an edge without projected length."""
    swapped = (v[..., 0] < u[..., 0]) | ((v[..., 0] == u[..., 0]) & (v[..., 1] < u[..., 1]))
    if planted == "stored_anchor":
        swapped = np.zeros_like(swapped)
    s3 = swapped[..., None]
    a, b = np.where(s3, v, u), np.where(s3, u, v)
    dx, dy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    e = dx * (p[..., 1] - a[..., 1]) - dy * (p[..., 0] - a[..., 0])
    s = _sign(e)
    if planted not in ("no_eps_both", "no_eps_neither"):
        s = np.where(s == 0, _sign(-dy), s)
        s = np.where(s == 0, _sign(dx), s)
    return np.where(swapped, -s, s)


# ------------------------------------------------------------------ W3
def crossing(p, a, b, c, planted=None):
    """sigma where the face's column contains p (all three sides equal and not 0), else 0."""
    s0, s1, s2 = edge_side(a, b, p, planted), edge_side(b, c, p, planted), edge_side(c, a, p, planted)
    if planted == "no_eps_both":                                       # a point on an edge's line belongs to both of its sides
        sides = np.stack(np.broadcast_arrays(s0, s1, s2))
        pos, neg = (sides >= 0).all(0) & (sides > 0).any(0), (sides <= 0).all(0) & (sides < 0).any(0)
        return pos.astype(np.int64) - neg.astype(np.int64)
    return np.where((s0 == s1) & (s1 == s2), s0, 0)


# ------------------------------------------------------------------ W4
def plane_term(p, a, b, c):
    """t = (n_x (a_x - p_x) + n_y (a_y - p_y)) + n_z (a_z - p_z), n = (b - a) x (c - a) with each component as the header writes it."""
    e1, e2 = b - a, c - a
    nx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
    ny = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
    nz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    return (nx * (a[..., 0] - p[..., 0]) + ny * (a[..., 1] - p[..., 1])) + nz * (a[..., 2] - p[..., 2])


def ahead(p, a, b, c, sigma, planted=None):
    t = sigma * plane_term(p, a, b, c)
    return t >= 0 if planted == "t_ge" else t > 0


def contributions(p, a, b, c, planted=None):
    """The contribution of every (query, face) pair, broadcast: sigma where W1, W3 and W4 hold, else 0."""
    with np.errstate(all="ignore"):
        sigma = crossing(p, a, b, c, planted)
        term = np.where(box_guard(p, a, b, c, planted) & (sigma != 0) & ahead(p, a, b, c, sigma, planted), sigma, 0)
    return np.abs(term) if planted == "sigma_dropped" else term


# ------------------------------------------------------------------ W5
def _inputs(verts, faces, points):
    v = np.asarray(verts, F32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(points, F32).reshape(-1, 3).astype(np.float64)
    return v, f, p


def brute_force(verts, faces, points, planted=None):
    """(Q,) int32: the sum over all usable faces of the object; 0 for a query with a non-finite coordinate."""
    v, f, p = _inputs(verts, faces, points)
    ids = np.nonzero(NR.usable_faces(verts, faces))[0]
    out = np.zeros(len(p), np.int32)
    live = np.isfinite(p).all(1)
    if len(ids) and live.any():
        tri = v[f[ids]]                                                # (F, 3 corners, 3)
        for q0 in range(0, len(p), 512):                               # (in slabs, to bound the (Q, F) temporaries)
            q = slice(q0, q0 + 512)
            term = contributions(p[q, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], planted)
            out[q] = np.where(live[q], term.sum(1), 0)
    return out


def bad_flag(verts, faces):
    """Whether a face names a vertex outside [0, V): what *bad reports once such a face is met."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return bool(((f < 0) | (f >= np.asarray(verts).reshape(-1, 3).shape[0])).any())


def _column(v, f, lists, g, px, py, pzs, k_first, planted=None):
    """The cells (c_x, c_y, k), k = k_first .. n_z - 1; a face counts in cell max(c_z(its min z), k_first) only.  pzs: the heights of
    the points of this column that share the walk.  Returns (their winding numbers, faces looked at)."""
    n = g["n"]
    c = NR.cell_of(g, np.array([px, py, 0.0]))
    w, looked = np.zeros(len(pzs), np.int64), 0
    for k in range(k_first, int(n[2])):
        ids = np.asarray(lists.get(int((c[0] * n[1] + c[1]) * n[2] + k), []), np.int64)
        looked += len(ids)
        if not len(ids):
            continue
        tri = v[f[ids]]
        if planted != "every_cell":
            kf = NR.cell_of(g, np.stack([np.zeros(len(ids)), np.zeros(len(ids)), tri[:, :, 2].min(1)], 1))[:, 2]
            tri = tri[np.maximum(kf, k_first) == k]
        p = np.stack([np.full(len(pzs), px), np.full(len(pzs), py), np.asarray(pzs, np.float64)], 1)
        w += contributions(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2], planted).sum(1)
    return w, looked


def walk(verts, faces, points, h, planted=None):
    """W5's pruned form for one object over the grid of edge ``h``: (winding (Q,) int32, faces looked at per query (Q,))."""
    v, f, p = _inputs(verts, faces, points)
    g = NR.grid(verts, h)
    lists = NR.cell_lists(verts, faces, g)
    out, looked = np.zeros(len(p), np.int32), np.zeros(len(p), np.int64)
    for q in range(len(p)):
        if np.isfinite(p[q]).all() and lists:
            w, looked[q] = _column(v, f, lists, g, p[q, 0], p[q, 1], p[q, 2:3], int(NR.cell_of(g, p[q])[2]), planted)
            out[q] = w[0]
    return out, looked


# ------------------------------------------------------------------ W6
def lattice_axes(lo, h, n):
    """Per axis the fp32 coordinates lo + h * index: an fp32 multiply, then an fp32 add."""
    lo, h = np.asarray(lo, F32), np.asarray(h, F32)
    with np.errstate(all="ignore"):
        return [(lo[a] + (h[a] * np.arange(int(n[a])).astype(F32)).astype(F32)).astype(F32) for a in range(3)]


def lattice_points(lo, h, n):
    """(n_x n_y n_z, 3) fp32 in the lattice's order (x-major, z fastest)."""
    X, Y, Z = np.meshgrid(*lattice_axes(lo, h, n), indexing="ij")
    return np.stack([X, Y, Z], -1).reshape(-1, 3).astype(F32)


def column_walk(verts, faces, lo, h, n, cell, tile):
    """W6 as the rule allows it to be computed: per (i, j) column and run of ``tile`` consecutive z-points one walk, from the cell of the
    run's lowest finite point.  (n_x, n_y, n_z) int32; must equal ``brute_force`` on ``lattice_points``."""
    v, f, _ = _inputs(verts, faces, np.zeros((0, 3)))
    g = NR.grid(verts, cell)
    lists = NR.cell_lists(verts, faces, g)
    xs, ys, zs = (ax.astype(np.float64) for ax in lattice_axes(lo, h, n))
    out = np.zeros(tuple(int(x) for x in n), np.int32)
    for i, px in enumerate(xs):
        for j, py in enumerate(ys):
            for z0 in range(0, len(zs), tile):
                run = zs[z0:z0 + tile]
                fin = np.isfinite(run)
                if not (fin.any() and np.isfinite(px) and np.isfinite(py) and lists):
                    continue
                k_first = int(NR.cell_of(g, np.array([0.0, 0.0, run[fin].min()]))[2])
                w, _ = _column(v, f, lists, g, px, py, run[fin], k_first)
                out[i, j, z0:z0 + tile][fin] = w
    return out


# ------------------------------------------------------------------ occupancy and IoU
def contained(w, rule):
    w = np.asarray(w)
    return {"nonzero": w != 0, "positive": w > 0, "odd": (w & 1) != 0}[rule]


def iou_lattice(box_lo, box_hi, resolution):
    """(lo, h) fp32 of ``geometry.mesh_iou``'s lattice over the box: h = (box_hi - box_lo) / resolution, lo = box_lo + h * 0.5, each
    operation rounded to fp32 -- the centres of resolution^3 equal boxes."""
    box_lo, box_hi = np.asarray(box_lo, F32), np.asarray(box_hi, F32)
    h = ((box_hi - box_lo).astype(F32) / F32(resolution)).astype(F32)
    return (box_lo + (h * F32(0.5)).astype(F32)).astype(F32), h


def iou_counts(a, b):
    """(iou, intersection, union, count_a, count_b) of two bool grids."""
    inter, union = int((a & b).sum()), int((a | b).sum())
    return (inter / union if union else 0.0), inter, union, int(a.sum()), int(b.sum())


# ------------------------------------------------------------------ closed forms and meshes
def box_signed_distance(p, half):
    """The signed distance from p (Q, 3) to the axis-parallel box +-half in float64: outside ``nearest_restatement.box_distance``, inside
    -min_a(half_a - |p_a|)."""
    q, half = np.abs(np.asarray(p, np.float64).reshape(-1, 3)), np.asarray(half, np.float64)
    inside = (q < half).all(1)
    return np.where(inside, -(half - q).min(1), NR.box_distance(p, half))


def box12(half=(0.25, 0.2, 0.15), centre=(0.0, 0.0, 0.0)):
    """The closed box centre +- half with 8 vertices and 12 faces wound counter-clockwise seen from outside.  Vertex 4 i + 2 j + k."""
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * np.asarray(half) + np.asarray(centre)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return v.astype(F32), f


def octahedron(r=0.5):
    """Corners +-r on the axes, 8 faces wound outward: every face spans the whole z-range of its half."""
    v = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], F32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def merged(*meshes):
    """Several meshes as one object (vertex indices shifted)."""
    verts, faces, base = [], [], 0
    for v, f in meshes:
        verts.append(np.asarray(v, F32))
        faces.append(np.asarray(f, np.int32) + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


def skew_mesh():
    """Two triangles in the plane z = 1 that share the edge (0, 0) - (2^40, 2^40), and a query just left of that edge near its low end.
    Anchored at the far endpoint, p_x - 2^40 is rounded and E comes out 0: a face that anchors E at its own first endpoint then
    disagrees with its neighbour about the side.  From the canonical endpoint both see the exact E."""
    big = 2.0 ** 40
    verts = np.array([[0, 0, 1], [big, big, 1], [0, big, 1], [big, 0, 1]], F32)
    faces = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    return verts, faces, np.array([[1.0, 1.0 + 2.0 ** -23, 0.0]], F32)


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)       # flat, counter-clockwise seen from +z
# queries below TRI (z = -1) and what they get: the query counts as (x + e, y + e^2)
UNDER = [((0.25, 0.25), 1), ((0, 0), 1), ((1, 0), 0), ((0, 1), 0), ((0.5, 0), 1), ((0, 0.5), 1), ((0.5, 0.5), 0), ((-0.25, 0.5), 0),
         ((0.75, 0.5), 0), ((0.25, -0.25), 0)]
TILTED = np.array([[0, 0, 0], [1, 0, 1], [0, 1, 1]], F32)    # the plane z = x + y
SQUARE = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
FAN = (np.array([[0, 0, 0], [1, 0, 0.5], [0.5, 1, 0.25], [-0.5, 1, 0.5], [-1, 0, 0.25], [-0.5, -1, 0.5], [0.5, -1, 0.25]], F32),
       np.array([[0, k, k % 6 + 1] for k in range(1, 7)], np.int32))
# a triangle with full mantissas and its highest corner b: at b itself p_z < max z fails, so the face cannot count; without the guard
# the rounding of t = n . (a - b), which is 0 in exact arithmetic, decides
GUARD_TRI = np.array([[0.19133703410625458, -0.321428120136261, -0.10374383628368378],
                      [-0.49417540431022644, -0.23750528693199158, -0.07881118357181549],
                      [-0.3940787613391876, 0.13315995037555695, -0.11957573145627975]], F32)
ONE = np.array([[0, 1, 2]], np.int32)
# faces that never count -- without area, collinear, vertical -- and queries under their corners and edges among others
NEVER = (np.array([[0, 0, 1], [1, 0, 1], [2, 0, 1], [1, 0, 3], [0, 1, 1]], F32),
         np.array([[0, 0, 1], [0, 1, 2], [2, 1, 0], [0, 1, 3], [3, 1, 0], [4, 4, 4], [0, 4, 0]], np.int32),
         np.array([[x, y, z] for x in (-0.5, 0, 0.5, 1, 1.5, 2, 2.5) for y in (-0.5, 0, 0.5, 1) for z in (0, 1, 2)], F32))
IOU_A, IOU_B, IOU_R = ((0.25, 0.25, 0.25), (0.0, 0.0, 0.0)), ((0.25, 0.25, 0.25), (0.125, 0.0, 0.0)), 20
IOU_WANT = (4800, 8000, 6400, 6400)              # the union box is 20 x 20 x 20 steps of (1/32, 1/40, 1/40); each box 16 x 20 x 20, 4 apart


def box_tie_queries():
    """336 queries around the box +-(0.25, 0.2, 0.15), many of them exactly on its planes, edges and corners."""
    g = [-0.5, -0.25, -0.125, 0, 0.125, 0.2, 0.25, 0.5]
    return np.array([[x, y, z] for x in g for y in (-0.3, -0.2, -0.1, 0, 0.1, 0.2, 0.3) for z in (-0.3, -0.15, -0.05, 0, 0.15, 0.3)], F32)


@functools.lru_cache(maxsize=None)
def sphere_case():
    """The 320-face icosphere of radius 0.4 and 2 000 random queries plus queries under 40 vertices and 40 edge midpoints."""
    verts, faces = MS.icosphere(2, 0.4)
    assert faces.shape == (320, 3) and signed_volume(verts, faces) > 0
    rng = np.random.default_rng(0)
    q = rng.uniform(-0.5, 0.5, (2000, 3))
    under_v = np.c_[verts[:40, :2], np.zeros(40)]
    under_e = np.c_[(verts[faces[:40, 0]].astype(np.float64) + verts[faces[:40, 1]])[:, :2] / 2, np.zeros(40)]
    return verts, faces, np.concatenate([q, under_v, under_e]).astype(F32)


THIN = F32([1 / 64, 1 / 64, 1])


def octa_queries(scale=(1, 1, 1), seed=3):
    """Random queries around the octahedron, queries outside the grid on every side, and queries under its corners and edges."""
    rng = np.random.default_rng(seed)
    v, f = octahedron()
    around = rng.uniform(-0.55, 0.55, (120, 3))
    outside = rng.uniform(-0.45, 0.45, (36, 3))
    for k in range(36):
        outside[k, k % 3] = (-1) ** (k // 3) * rng.uniform(0.51, 3.0)
    border = rng.uniform(-0.5, 0.5, (24, 3))
    border[:, 2] = np.where(rng.uniform(size=24) < 0.5, -0.499, 0.47)
    under = np.concatenate([np.c_[v[:, :2], -np.ones(6)], np.c_[(v[f[:, 0]] + v[f[:, 1]])[:, :2] / 2, -0.75 * np.ones(8)],
                            np.c_[v[:4, :2] / 2, np.zeros(4)]])
    return (np.concatenate([around, outside, border, under]) * np.asarray(scale)).astype(F32)
