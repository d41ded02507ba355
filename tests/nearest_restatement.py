"""The rules of include/supnerf_hip.h ("Mesh distance") restated in numpy float64: one plain function per rule, no kernel code.  The
library is built without fused multiply-adds, so IEEE float64 operations in the written order give the same bits here as on the
device: the GPU tests compare ``face``, ``dist2``, the weights and the sample points with ``==``.  ``brute_force`` is D2 -- the
definition of the answer; ``ring_search`` is D4 over the grid of D3 and must give the same.  ``planted`` switches in one deliberate
mistake, so that the checks can be shown to reject it.

Inputs are what the kernels take (fp32 vertices and queries), widened; a float64 query that fp32 cannot hold is taken as it is, which
lets the CPU tests put queries a float64 ulp from a cell plane."""
import numpy as np

MAX_CELLS = 256
SLACK = 2.0 ** -40
PLANTED = ("stop_ge_no_slack", "centroid_cell_only", "tie_high", "edge_to_vertex", "s_linear")
INF = np.inf
# one triangle and a query in each region of D1 (query, region, weights, d^2; all exact in binary), one on the plane, one at a vertex
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
REGIONS = [((-1, -1, 0), "a", (1, 0, 0), 2.0), ((2, -0.5, 0), "b", (0, 1, 0), 1.25), ((0.5, -1, 0), "ab", (0.5, 0.5, 0), 1.0),
           ((-0.5, 2, 0), "c", (0, 0, 1), 1.25), ((-1, 0.5, 0), "ac", (0.5, 0, 0.5), 1.0), ((1, 1, 0), "bc", (0, 0.5, 0.5), 0.5),
           ((0.25, 0.25, 1), "interior", (0.5, 0.25, 0.25), 1.0), ((0.25, 0.5, 0), "interior", (0.25, 0.25, 0.5), 0.0),
           ((1, 0, 0), "b", (0, 1, 0), 0.0)]


def _f64(x, cols=3):
    return np.asarray(x, np.float64).reshape(-1, cols)


# ------------------------------------------------------------------ D1
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def point_triangle(p, a, b, c, planted=None):
    """(w (..., 3), d2 (...)) float64 for broadcastable p, a, b, c (..., 3): the region walk of D1, the first test that holds decides.
    Every branch is evaluated and the walk selects, so the selected values went through the header's operations and no others."""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, c)))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp, bc = b - a, c - a, p - a, p - b, p - c, c - b
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        g, h = d4 - d3, d5 - d6
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), g / (g + h)
        s = (va + vb) + vc
        v, u = vb / s, vc / s
        vertex_c = (d6 >= 0) if planted == "edge_to_vertex" else (d6 >= 0) & (d5 <= d6)
        regions = [
            ((d1 <= 0) & (d2 <= 0), (one, zero, zero), ap),
            ((d3 >= 0) & (d4 <= d3), (zero, one, zero), bp),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0) & (d1 - d3 > 0), (1.0 - t_ab, t_ab, zero), ap - t_ab[..., None] * ab),
            (vertex_c, (zero, zero, one), cp),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0) & (d2 - d6 > 0), (1.0 - t_ac, zero, t_ac), ap - t_ac[..., None] * ac),
            ((va <= 0) & (g >= 0) & (h >= 0) & (g + h > 0), (zero, 1.0 - t_bc, t_bc), bp - t_bc[..., None] * bc),
        ]
        w = np.stack([(1.0 - v) - u, v, u], -1)                       # interior: what is left
        e = (ap - v[..., None] * ab) - u[..., None] * ac
        for test, wr, er in reversed(regions):                         # (the first test that holds is applied last)
            w = np.where(test[..., None], np.stack(wr, -1), w)
            e = np.where(test[..., None], er, e)
        d2v = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return w, d2v


def region_of(p, a, b, c):
    """The name of the region that decides, for one query (the hand cases)."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    tests = [("a", d1 <= 0 and d2 <= 0), ("b", d3 >= 0 and d4 <= d3), ("ab", vc <= 0 and d1 >= 0 and d3 <= 0 and d1 - d3 > 0),
             ("c", d6 >= 0 and d5 <= d6), ("ac", vb <= 0 and d2 >= 0 and d6 <= 0 and d2 - d6 > 0),
             ("bc", va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0 and (d4 - d3) + (d5 - d6) > 0)]
    return next((name for name, holds in tests if holds), "interior")


# ------------------------------------------------------------------ D2
def usable_faces(verts, faces):
    """(F,) bool: all three indices in [0, V) and all nine coordinates finite."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    fin = np.isfinite(v).all(1)
    ok[ok] &= fin[f[ok]].all(1)
    return ok


def _better(d2, face, best_d2, best_face, planted=None):
    if planted == "tie_high":
        return d2 < best_d2 or (d2 == best_d2 and face > best_face)
    return d2 < best_d2 or (d2 == best_d2 and face < best_face)


def _test_faces(p, verts64, faces, ids, best, planted=None):
    """Test the faces ``ids`` (ascending or not) against one query; best = [d2, face, w]."""
    if len(ids) == 0:
        return
    f = faces[ids]
    w, d2 = point_triangle(p[None], verts64[f[:, 0]], verts64[f[:, 1]], verts64[f[:, 2]], planted)
    for k in range(len(ids)):
        if _better(d2[k], int(ids[k]), best[0], best[1], planted):     # (false for a NaN)
            best[0], best[1], best[2] = d2[k], int(ids[k]), w[k]


def _result(bests):
    face = np.array([b[1] for b in bests], np.int32)
    d2 = np.array([b[0] for b in bests], np.float64)
    w = np.array([b[2] for b in bests], np.float64).reshape(-1, 3)
    return dict(face=face, dist2=d2, weights64=w, weights=w.astype(np.float32))


def brute_force(verts, faces, points, planted=None):
    """D2 for one object: face (Q,) int32 (-1 for none), dist2 (Q,) float64, weights (Q, 3) fp32 (and float64)."""
    v64 = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ids = np.nonzero(usable_faces(verts, faces))[0]
    bests = []
    for p in _f64(points):
        best = [INF, -1, np.zeros(3)]
        if np.isfinite(p).all():
            _test_faces(p, v64, f, ids, best, planted)
        bests.append(best)
    return _result(bests)


def closest_points(verts, faces, r):
    """(Q, 3) float64: sum_k w_k verts[faces[face, k]] with the fp32 weights, as ``geometry.closest_point`` forms it (in float64 here)."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)[np.maximum(r["face"], 0)]
    return (r["weights"].astype(np.float64)[:, :, None] * v[f]).sum(1)


# ------------------------------------------------------------------ D3
def grid(verts, h):
    """The grid of one object: lo, hi (fp32 minimum and maximum, widened; 0 without vertices), h, n (3,) cells per axis, E."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    h = float(np.float32(h))
    assert h > 0 and np.isfinite(h)
    lo = v.min(0).astype(np.float64) if v.shape[0] else np.zeros(3)
    hi = v.max(0).astype(np.float64) if v.shape[0] else np.zeros(3)
    extent = hi - lo
    n = np.clip(np.ceil(extent / h), 1, MAX_CELLS).astype(np.int64)
    return dict(lo=lo, hi=hi, h=h, n=n, extent=float(extent.max()))


def cell_of(g, x):
    """clamp(floor((x - lo) / h), 0, n - 1) per axis for x (..., 3) float64; a NaN gives 0."""
    with np.errstate(all="ignore"):
        t = np.floor((np.asarray(x, np.float64) - g["lo"]) / g["h"])
    t = np.where(t >= 1.0, np.minimum(t, g["n"] - 1), 0.0)
    return t.astype(np.int64)


def face_boxes(verts, faces, g, planted=None):
    """(lo (F, 3), hi (F, 3), usable (F,)): the index box of every face, from its component-wise minimum and maximum corner."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = usable_faces(verts, faces)
    tri = v[np.where(ok[:, None], f, 0)]                              # (F, 3 corners, 3 axes)
    lo, hi = cell_of(g, tri.min(1).astype(np.float64)), cell_of(g, tri.max(1).astype(np.float64))
    if planted == "centroid_cell_only":
        lo = hi = cell_of(g, tri.astype(np.float64).sum(1) / 3.0)
    return lo, hi, ok


def cell_counts(verts, faces, g):
    """(F,) int32: what ``snr_nearest_count`` writes."""
    lo, hi, ok = face_boxes(verts, faces, g)
    return np.where(ok, (hi - lo + 1).prod(1), 0).astype(np.int32)


def cell_lists(verts, faces, g, planted=None):
    """{local cell id: ascending face indices}: every face in every cell of its index box."""
    lo, hi, ok = face_boxes(verts, faces, g, planted)
    n = g["n"]
    lists = {}
    for f in np.nonzero(ok)[0]:
        for x in range(lo[f, 0], hi[f, 0] + 1):
            for y in range(lo[f, 1], hi[f, 1] + 1):
                for z in range(lo[f, 2], hi[f, 2] + 1):
                    lists.setdefault(int((x * n[1] + y) * n[2] + z), []).append(int(f))
    return lists


def pairs(verts, faces, g):
    """(pair_cell int64, pair_face int32) in the order ``snr_nearest_emit`` writes them: face after face, x-major within a face."""
    lo, hi, ok = face_boxes(verts, faces, g)
    n = g["n"]
    cells, fs = [], []
    for f in np.nonzero(ok)[0]:
        for x in range(lo[f, 0], hi[f, 0] + 1):
            for y in range(lo[f, 1], hi[f, 1] + 1):
                for z in range(lo[f, 2], hi[f, 2] + 1):
                    cells.append((x * n[1] + y) * n[2] + z)
                    fs.append(f)
    return np.asarray(cells, np.int64), np.asarray(fs, np.int32)


# ------------------------------------------------------------------ D4
def ring_search(verts, faces, points, h, planted=None):
    """D4 for one object over the grid of edge ``h``: the dict of ``brute_force`` plus ``tested`` (Q,), the faces tested per query
    (repeats counted) and ``rings`` (Q,), the rings walked."""
    v64 = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    g = grid(verts, h)
    lists = cell_lists(verts, faces, g, planted)
    n, hh, E = g["n"], g["h"], g["extent"]
    bests, tested, rings = [], [], []
    for p in _f64(points):
        best, count, r = [INF, -1, np.zeros(3)], 0, -1
        if np.isfinite(p).all() and lists:
            tp = p - g["lo"]
            c0 = cell_of(g, p)
            for r in range(MAX_CELLS):
                for x in range(max(c0[0] - r, 0), min(c0[0] + r, n[0] - 1) + 1):
                    for y in range(max(c0[1] - r, 0), min(c0[1] + r, n[1] - 1) + 1):
                        for z in range(max(c0[2] - r, 0), min(c0[2] + r, n[2] - 1) + 1):
                            if max(abs(x - c0[0]), abs(y - c0[1]), abs(z - c0[2])) != r:
                                continue
                            ids = np.asarray(lists.get(int((x * n[1] + y) * n[2] + z), []), np.int64)
                            count += len(ids)
                            _test_faces(p, v64, f, ids, best, planted)
                sides = []
                for a in range(3):
                    kl, kh = c0[a] - r, c0[a] + r + 1
                    if kl >= 1:
                        sides.append(tp[a] - float(kl) * hh)
                    if kh <= n[a] - 1:
                        sides.append(float(kh) * hh - tp[a])
                if not sides:
                    break
                m = min(sides)
                if planted == "stop_ge_no_slack":
                    if m > 0 and m * m >= best[0]:
                        break
                else:
                    s = m - SLACK * (E + m)
                    if s > 0 and s * s > best[0]:
                        break
        bests.append(best)
        tested.append(count)
        rings.append(r + 1)
    out = _result(bests)
    out.update(tested=np.asarray(tested), rings=np.asarray(rings))
    return out


# ------------------------------------------------------------------ D5
def face_areas(verts, faces):
    """(F,) float64: rule 3 of "Mesh components": |(b - a) x (c - a)| / 2 on the widened vertices."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.sqrt(nx * nx + ny * ny + nz * nz) / 2.0


def sample(verts, faces, cum, u, planted=None):
    """D5 for one object: n = len(u) samples from the uniforms u (n, 3) float64 and the inclusive cumulative area ``cum`` (F,) float64.
    points (n, 3) fp32, face (n,) int32, weights (n, 3) fp32."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cum = np.asarray(cum, np.float64)
    u = _f64(u)
    n = u.shape[0]
    points, face, weights = np.zeros((n, 3), np.float32), np.full(n, -1, np.int32), np.zeros((n, 3), np.float32)
    if f.shape[0] == 0 or not (cum[-1] > 0 and np.isfinite(cum[-1])):
        return dict(points=points, face=face, weights=weights)
    total = cum[-1]
    target = (np.arange(n, dtype=np.float64) + u[:, 0]) / float(n) * total
    k = np.searchsorted(cum, target, side="right")                    # the first f with cum[f] > target
    last = int(np.searchsorted(cum, total, side="left"))              # the first f with cum[f] >= total: the last face with area
    k = np.where(target < total, np.minimum(k, f.shape[0] - 1), last)
    s = u[:, 1] if planted == "s_linear" else np.sqrt(u[:, 1])
    w = np.stack([1.0 - s, s * (1.0 - u[:, 2]), s * u[:, 2]], 1)
    tri = v[f[k]]
    x = (w[:, 0:1] * tri[:, 0] + w[:, 1:2] * tri[:, 1]) + w[:, 2:3] * tri[:, 2]
    return dict(points=x.astype(np.float32), face=k.astype(np.int32), weights=w.astype(np.float32))


# ------------------------------------------------------------------ closed forms and meshes
def box_distance(p, half):
    """The distance from p (Q, 3) to the SURFACE of the axis-parallel box +-half, in float64: outside, the distance to the solid;
    inside, the distance to the nearest side."""
    p, half = np.abs(_f64(p)), np.asarray(half, np.float64)
    out = np.sqrt((np.maximum(p - half, 0.0) ** 2).sum(1))
    inside = (p <= half).all(1)
    return np.where(inside, (half - p).min(1), out)


def sheets_mesh():
    """Four triangles in the unit cube whose grid of edge 1/4 has its planes at dyadic coordinates: face 0 lies exactly IN the cell
    plane x = 1/2, face 1 in x = 3/8 (inside a cell); faces 2 and 3 are small and only stretch the bounds to (0, 0, 0) and (1, 1, 1).
    The query (7/16, 3/8, 3/8) is exactly 1/16 from both sheets, sits in the cell of face 1 and has the plane of face 0 as its nearest
    cell plane: the right answer is face 0 (the tie goes to the lower index), found only if ring 1 is still walked."""
    verts = np.array([[0.5, 0, 0], [0.5, 1, 0], [0.5, 0, 1], [0.375, 0, 0], [0.375, 1, 0], [0.375, 0, 1],
                      [0, 0, 0], [0, 0.125, 0], [0, 0, 0.125], [1, 1, 1], [1, 0.875, 1], [1, 1, 0.875]], np.float32)
    faces = np.arange(12, dtype=np.int32).reshape(4, 3)
    return verts, faces, np.array([[0.4375, 0.375, 0.375]], np.float32)


def roof_mesh():
    """Two triangles that share the edge (0, 0, 0) - (1, 0, 0) and fall away from it symmetrically (z = -|y|): a query above the edge
    is equally far from both, bit for bit, since the two computations mirror each other in y."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, -1], [0.5, -1, -1]], np.float32)
    faces = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    return verts, faces


def box_queries(half=(0.25, 0.2, 0.15), seed=5):
    """450 fp32 queries for the box +-half: 250 around it (within 1.6 half), 120 inside, 50 far outside the grid (up to 40 half, some on
    the axes), and 30 on the surface itself or at its vertices and edge midpoints."""
    rng = np.random.default_rng(seed)
    h = np.asarray(half, np.float64)
    around = rng.uniform(-1.6, 1.6, (250, 3)) * h
    inside = rng.uniform(-1.0, 1.0, (120, 3)) * h
    far = rng.uniform(-40.0, 40.0, (50, 3)) * h
    far[:10, 1:] = 0.0
    ax = rng.integers(0, 3, 30)
    on = rng.uniform(-1.0, 1.0, (30, 3)) * h
    on[np.arange(30), ax] = np.sign(rng.uniform(-1, 1, 30)) * h[ax]   # on a side
    on[:8] = (np.array(list(np.ndindex(2, 2, 2))) * 2.0 - 1.0) * h    # the eight corners
    return np.concatenate([around, inside, far, on]).astype(np.float32)
