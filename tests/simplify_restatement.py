"""The rules of include/supnerf_hip.h ("Mesh simplification") restated step by step in numpy: one plain function per rule, float64 sums
and exact integers, no kernel code.  ``simplify`` chains them for one object; the GPU tests compare the package against it, the CPU
tests hold the restatement itself against what a tessellated box must give.  ``planted`` switches in a deliberate mistake, so that the
checks can be shown to reject one."""
import numpy as np

EPS = 1e-3                    # rule 4's ridge weight (SNR_SIMPLIFY_EPS)
Q_LIMIT = 1 << 20
MAX_CHANNELS = 16
PLANTED = ("first_corner_only", "flipped_d", "no_clamp")


class Rejected(ValueError):
    """What the package reports as SnrError: a vertex without a usable cell, or a face index outside the mesh."""


# ------------------------------------------------------------------ rule 1
def cell_index(verts, cell, origin):
    """q (V, 3) int32 = floor((x - origin) / cell), the subtraction and the division each one fp32 operation."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    cell = np.float32(cell)
    if not (cell > 0 and np.isfinite(cell)):
        raise Rejected("cell")
    with np.errstate(all="ignore"):
        d = v - np.asarray(origin, np.float32).reshape(1, 3)
        qf = np.floor(d / cell)
    assert d.dtype == np.float32 and qf.dtype == np.float32
    if not (np.abs(qf) < Q_LIMIT).all():                 # (NaN and infinities fail the comparison too)
        raise Rejected("a vertex is not finite or lies 2^20 cells or more from the origin")
    return qf.astype(np.int32)                           # (-0.0 -> 0)


# ------------------------------------------------------------------ rule 2
def numbering(q):
    """(vert_map (V,) int32, members (K,) int32, cluster_q (K, 3) int32): clusters in ascending lexicographic (qx, qy, qz) order."""
    q = np.asarray(q, np.int64).reshape(-1, 3)
    if q.shape[0] == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 3), np.int32)
    order = np.lexsort((q[:, 2], q[:, 1], q[:, 0]))      # the last key is the primary one
    sq = q[order]
    head = np.ones(q.shape[0], bool)
    head[1:] = (sq[1:] != sq[:-1]).any(1)
    cid = np.cumsum(head) - 1
    vert_map = np.empty(q.shape[0], np.int32)
    vert_map[order] = cid
    return vert_map, np.bincount(cid).astype(np.int32), sq[head].astype(np.int32)


# ------------------------------------------------------------------ rule 3
def cluster_means(values, vert_map, K):
    """(K, C) float64: per cluster the sum of the members' rows widened to float64, over the count."""
    x = np.asarray(values, np.float32).astype(np.float64)
    x = x.reshape(x.shape[0], -1)
    out = np.zeros((K, x.shape[1]), np.float64)
    np.add.at(out, np.asarray(vert_map, np.int64), x)
    return out / np.maximum(np.bincount(vert_map, minlength=K), 1)[:, None]


# ------------------------------------------------------------------ rule 4
def cell_centres(cluster_q, cell, origin, t=0.5):
    """origin + (q + t) cell in float64: t = 1/2 the centre c0, t = 0 and 1 the faces of the cell."""
    return np.asarray(origin, np.float32).astype(np.float64)[None] + (cluster_q.astype(np.float64) + t) * float(np.float32(cell))


def quadric_sums(verts, faces, vert_map, c0, corners=(0, 1, 2), d_sign=-1.0):
    """A (K, 3, 3), v (K, 3): over every (face, corner) pair of the original faces whose corner vertex lies in the cluster.
    (``corners`` and ``d_sign`` exist for the planted mistakes.)"""
    K = c0.shape[0]
    A, v = np.zeros((K, 3, 3)), np.zeros((K, 3))
    x = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    for corner in corners:
        k = np.asarray(vert_map, np.int64)[f[:, corner]]
        a, b, c = (x[f[:, i]] - c0[k] for i in range(3))
        n = np.cross(b - a, c - a)
        d = d_sign * (n * a).sum(1)
        np.add.at(A, k, n[:, :, None] * n[:, None, :])
        np.add.at(v, k, d[:, None] * n)
    return A, v


def quadric_positions(A, v, m, c0, lo, hi, cell, clamp=True):
    """x (K, 3) float64: the ridge-regularised minimiser, clamped to the cell; the mean where no face with area touches the cluster."""
    cell = float(np.float32(cell))
    x = m.copy()
    tr = np.trace(A, axis1=1, axis2=2)
    for k in np.nonzero(tr > (1e-12 * cell * cell) ** 2)[0]:
        lam = EPS * tr[k]
        y = np.linalg.solve(A[k] + lam * np.eye(3), lam * (m[k] - c0[k]) - v[k])
        x[k] = c0[k] + y
        if clamp:
            x[k] = np.minimum(np.maximum(x[k], lo[k]), hi[k])
    return x


# ------------------------------------------------------------------ rule 6
def remap_faces(faces, vert_map, n_verts):
    """(new faces (F', 3) int32, face_index (F',) int64): kept iff the three new indices differ, in the original order."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if ((f < 0) | (f >= n_verts)).any():
        raise Rejected("a face index lies outside the mesh")
    nf = np.asarray(vert_map, np.int32)[f].reshape(-1, 3)
    keep = (nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 0] != nf[:, 2])
    return np.ascontiguousarray(nf[keep]), np.nonzero(keep)[0].astype(np.int64)


# ------------------------------------------------------------------ the chain, one object
def simplify(verts, faces, cell, origin=(0.0, 0.0, 0.0), placement="quadric", attributes=None, planted=None):
    """Rules 1 to 7 for one object.  ``planted`` switches in one deliberate mistake of rule 4: "first_corner_only" (a face counted for
    its first corner's cluster alone), "flipped_d" (d = +n . a') or "no_clamp"."""
    assert placement in ("mean", "quadric") and planted in (None,) + PLANTED
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    q = cell_index(verts, cell, origin)
    vert_map, members, cq = numbering(q)
    K = members.shape[0]
    new_faces, face_index = remap_faces(faces, vert_map, verts.shape[0])
    m = cluster_means(verts, vert_map, K).reshape(K, 3)
    if placement == "mean":
        x = m
    else:
        c0, lo, hi = (cell_centres(cq, cell, origin, t) for t in (0.5, 0.0, 1.0))
        A, v = quadric_sums(verts, faces, vert_map, c0, (0,) if planted == "first_corner_only" else (0, 1, 2),
                            1.0 if planted == "flipped_d" else -1.0)
        x = quadric_positions(A, v, m, c0, lo, hi, cell, clamp=planted != "no_clamp")
    out = dict(verts=x.astype(np.float32), verts64=x, faces=new_faces, vert_map=vert_map, members=members, face_index=face_index,
               cluster_q=cq, attributes=None)
    if attributes is not None:                                                   # rule 7
        a = np.asarray(attributes, np.float32)
        assert a.ndim == 2 and a.shape[0] == verts.shape[0] and 1 <= a.shape[1] <= MAX_CHANNELS
        out["attributes64"] = cluster_means(a, vert_map, K)
        out["attributes"] = out["attributes64"].astype(np.float32)
    return out


def drop_unreferenced(s):
    """The host policy of ``geometry.simplify_mesh``: the new vertices no kept face names go; vert_map -1 where the cluster went."""
    K = s["members"].shape[0]
    used = np.zeros(K, bool)
    used[s["faces"].reshape(-1)] = True
    renumber = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    out = dict(s)
    out.update(verts=s["verts"][used], faces=renumber[s["faces"]].reshape(-1, 3), vert_map=renumber[s["vert_map"]], members=s["members"][used])
    if s.get("attributes") is not None:
        out["attributes"] = s["attributes"][used]
    return out


# ------------------------------------------------------------------ meshes and measures
def box_mesh(half=(0.25, 0.2, 0.15), n=24):
    """The closed box +-half, n x n quads per side, shared vertices (n^3 - (n - 2)^3 ... of the (n + 1)^3 lattice: those on the surface),
    two triangles per quad, wound counter-clockwise seen from outside.  n = 24: 3 458 vertices, 6 912 faces."""
    idx = {}
    pts = []

    def vid(p):
        if p not in idx:
            idx[p] = len(pts)
            pts.append(p)
        return idx[p]

    faces = []
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3                  # e_u x e_w = e_a
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def p(di, dj):
                        c = [0, 0, 0]
                        c[a], c[u], c[w] = side, i + di, j + dj
                        return vid(tuple(c))
                    quad = [p(0, 0), p(1, 0), p(1, 1), p(0, 1)]
                    if side == 0:
                        quad.reverse()
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    h = np.asarray(half, np.float64)
    verts = (-h + 2.0 * h * np.asarray(pts, np.float64) / n).astype(np.float32)
    return verts, np.asarray(faces, np.int32)


def tetrahedron(p):
    """The closed tetrahedron of four points (4, 3), wound outward."""
    p = np.asarray(p, np.float32).reshape(4, 3)
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    if signed_volume(p, faces) < 0:
        faces = faces[:, ::-1].copy()
    return p, faces


def strip(n_inside, tail=6):
    """A triangle strip laid along x in the plane z = 0, faces (i, i + 1, i + 2) with alternating winding: ``n_inside`` (<= 8192)
    vertices at x = i / 8192, y = 0 or 1/4, which a cell of edge 1 at origin (0, -1/2, -1/2) puts into ONE cluster, then ``tail`` vertices
    at x = 1, 3/2, 2, ... and y = 0 or 1, each in a cell of its own, so that the faces among them survive."""
    assert 3 <= n_inside <= 8192 and tail >= 3
    i, j = np.arange(n_inside), np.arange(tail)
    x = np.concatenate([i / 8192.0, 1.0 + 0.5 * j])
    y = np.concatenate([0.25 * (i & 1), 1.0 * (j & 1)])
    verts = np.stack([x, y, np.zeros_like(x)], 1).astype(np.float32)
    k = np.arange(n_inside + tail - 2)
    f = np.stack([k, k + 1, k + 2], 1)
    f[1::2] = f[1::2, ::-1]
    return verts, f.astype(np.int32)


def wedge(n=12, step=0.25, slope=0.1, rows=3):
    """A thin open wedge seen edge-on: two sheets z = +-slope x over x = 0 .. n step and y = 0 .. rows - 1, joined along the sharp edge
    x = 0.  Away from that edge both sheets pass through one cell, and their planes meet outside it."""
    idx, pts, faces = {}, [], []

    def vid(i, j, s):
        key = (i, j, s if i else 0)
        if key not in idx:
            idx[key] = len(pts)
            pts.append((i * step, float(j), s * slope * i * step))
        return idx[key]

    for s in (1, -1):
        for i in range(n):
            for j in range(rows - 1):
                quad = [vid(i, j, s), vid(i + 1, j, s), vid(i + 1, j + 1, s), vid(i, j + 1, s)]
                if s < 0:
                    quad.reverse()
                faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.asarray(pts, np.float32), np.asarray(faces, np.int32)


def inside_cells(s, cell, origin, slack=0.0):
    """Every new vertex (float64, before rounding) lies in the closed box of its cell."""
    x = s["verts64"]
    lo, hi = cell_centres(s["cluster_q"], cell, origin, 0.0), cell_centres(s["cluster_q"], cell, origin, 1.0)
    return bool(((x >= lo - slack) & (x <= hi + slack)).all())


def signed_volume(verts, faces):
    x = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float((x[f[:, 0]] * np.cross(x[f[:, 1]], x[f[:, 2]])).sum() / 6.0)


def directed_edges_balance(faces):
    """Closed as an integer chain: every directed edge a -> b occurs as often as b -> a."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return True
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    fwd, cnt = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    bwd, cnt2 = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
    return bool(np.array_equal(fwd, bwd) and np.array_equal(cnt, cnt2))


def corner_error(verts, half=(0.25, 0.2, 0.15)):
    """The largest distance from a corner of the box +-half to its nearest vertex."""
    x = np.asarray(verts, np.float64)
    h = np.asarray(half, np.float64)
    worst = 0.0
    for s in np.ndindex(2, 2, 2):
        corner = (2.0 * np.asarray(s) - 1.0) * h
        worst = max(worst, float(np.sqrt(((x - corner) ** 2).sum(1)).min()))
    return worst


def ulp_distance(got, want64, floor=0.0):
    """|got - want| in units of one fp32 ulp: np.spacing of the larger of the two magnitudes.  ``want64`` is the float64 value before
    rounding.  ``floor`` (broadcast against the values) is the smallest magnitude a component counts with: a coordinate is c0 + y, and
    where the two cancel the error of y, relative to |y| <= cell, does not shrink with the sum."""
    got = np.asarray(got, np.float32)
    want = np.asarray(want64, np.float64).astype(np.float32)
    big = np.maximum(np.maximum(np.abs(got), np.abs(want)).astype(np.float64), np.broadcast_to(np.asarray(floor, np.float64), got.shape))
    ulp = np.spacing(np.maximum(big, float(np.finfo(np.float32).tiny)).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp


def position_floor(s, cell, origin):
    """The magnitude floor of ``ulp_distance`` for positions: 2^-20 of max(|c0|, cell) per cluster and axis.  Both sides solve for y in
    float64, where summation order and solve method move it by a relative 1e-13 of |y| <= cell (condition number <= 1e3); one fp32 ulp of
    the magnitude 2^-20 max(|c0|, cell) is 2^-43 of it, about that 1e-13.  A coordinate larger than the floor is held to its own ulp."""
    c0 = cell_centres(s["cluster_q"], cell, origin, 0.5)
    return np.maximum(np.abs(c0), float(np.float32(cell))) * 2.0 ** -20
