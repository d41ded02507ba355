"""The rules of include/supnerf_hip.h ("Mesh ray casting", R1 - R6) restated in numpy float64: one plain function per rule, no kernel code.
The library is built without fused multiply-adds, so IEEE float64 operations in the written order give the same bits here as on the
device: the GPU tests compare integers with ``==``, ``t`` bit for bit in float64 and the weights bit for bit in fp32.  ``brute_force`` is
R5 -- the definition of the answer; ``walk`` is the pruned form R6 over the grid of "Mesh distance" D3 (tests/nearest_restatement.py's
``grid`` / ``cell_of`` / ``cell_lists``) and must give the same.  ``planted`` switches in one deliberate mistake, so that the checks can
be shown to reject it.

Inputs are what the kernels take (fp32 vertices, rays and bounds), widened."""
import numpy as np

import inside_restatement as IR
import nearest_restatement as NR

PLANTED = ("stored_order", "no_fallback", "tmin_le", "tie_high", "stop_at_first_hit", "every_cell", "unswapped")
SLACK = 2.0 ** -40
F32 = np.float32
INF = np.inf


def _sign(x):
    return (x > 0).astype(np.int64) - (x < 0).astype(np.int64)


def _pick(x, k):
    """x (Q, ..., 3), k (Q,): component k[q] of every row of ray q."""
    idx = k.reshape((-1,) + (1,) * (x.ndim - 1))
    return np.take_along_axis(x, np.broadcast_to(idx, x.shape[:-1] + (1,)), -1)[..., 0]


# ------------------------------------------------------------------ R1
def ray_frame(o, d, planted=None):
    """The frame of every ray (o, d (Q, 3) float64): kz the axis of the largest |d| (ties to the lowest), kx and ky the next two axes
    cyclically, swapped for d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]; ``live``: all six numbers finite, d != 0."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    live = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    with np.errstate(all="ignore"):
        kz = np.argmax(np.where(np.isnan(d), 0.0, np.abs(d)), 1)          # (the first of equal maxima: the lowest axis)
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        dz = _pick(d, kz)
        if planted != "unswapped":
            kx, ky = np.where(dz < 0, ky, kx), np.where(dz < 0, kx, ky)
        return dict(o=o, d=d, live=live, kx=kx, ky=ky, kz=kz, Sx=_pick(d, kx) / dz, Sy=_pick(d, ky) / dz, Sz=1.0 / dz)


def project(fr, v):
    """(x', y', z') of the vertices v (Q or 1, ..., 3) in the frames of the Q rays: A = v - o; x' = A[kx] - Sx A[kz], y' = A[ky] - Sy
    A[kz], z' = Sz A[kz]."""
    extra = (1,) * (v.ndim - 2)
    A = v - fr["o"].reshape((-1,) + extra + (3,))
    Az = _pick(A, fr["kz"])
    S = [fr[k].reshape((-1,) + extra) for k in ("Sx", "Sy", "Sz")]
    return _pick(A, fr["kx"]) - S[0] * Az, _pick(A, fr["ky"]) - S[1] * Az, S[2] * Az


# ------------------------------------------------------------------ R2
def edge_side(ux, uy, vx, vy, planted=None):
    """(side, E) of the directed edge u -> v for the query at the origin of the projected plane: E from the endpoints in lexicographic
    (x', y') order, E = (v'_y - u'_y) u'_x - (v'_x - u'_x) u'_y; its sign, else sign(-(v'_y - u'_y)), else sign(v'_x - u'_x); side and
    value negated if the endpoints were swapped."""
    swapped = (vx < ux) | ((vx == ux) & (vy < uy))
    if planted == "stored_order":
        swapped = np.zeros_like(swapped)
    ax, ay, bx, by = np.where(swapped, vx, ux), np.where(swapped, vy, uy), np.where(swapped, ux, vx), np.where(swapped, uy, vy)
    dx, dy = bx - ax, by - ay
    e = dy * ax - dx * ay
    s = _sign(e)
    if planted != "no_fallback":
        s = np.where(s == 0, _sign(-dy), s)
        s = np.where(s == 0, _sign(dx), s)
    return np.where(swapped, -s, s), np.where(swapped, -e, e)


# ------------------------------------------------------------------ R3
def crossing(xa, ya, xb, yb, xc, yc, planted=None):
    """(sigma, U, V, W): sigma = the common side of a -> b, b -> c, c -> a (0 where they differ or are 0); sigma = -1 is front-facing
    (d . n < 0).  U, V, W: the values of the edges opposite a, b, c."""
    s_ab, W = edge_side(xa, ya, xb, yb, planted)
    s_bc, U = edge_side(xb, yb, xc, yc, planted)
    s_ca, V = edge_side(xc, yc, xa, ya, planted)
    return np.where((s_ab == s_bc) & (s_bc == s_ca), s_ab, 0), U, V, W


# ------------------------------------------------------------------ R4
def depth(U, V, W, za, zb, zc):
    """(t, det): det = (U + V) + W, t = ((U z'_a + V z'_b) + W z'_c) / det."""
    det = (U + V) + W
    return ((U * za + V * zb) + W * zc) / det, det


def counts(t, t_min, t_max, planted=None):
    """t_min < t < t_max, both strict; false for a NaN."""
    return ((t >= t_min) if planted == "tmin_le" else (t > t_min)) & (t < t_max)


def face_terms(fr, tri, t_min, t_max, planted=None):
    """R1 - R4 for every (ray, face) pair: tri (Q or 1, F, 3 corners, 3).  (sigma where the face counts else 0, t, U, V, W, det), (Q, F)."""
    with np.errstate(all="ignore"):
        x, y, z = project(fr, tri)
        sigma, U, V, W = crossing(x[..., 0], y[..., 0], x[..., 1], y[..., 1], x[..., 2], y[..., 2], planted)
        t, det = depth(U, V, W, z[..., 0], z[..., 1], z[..., 2])
        ok = (sigma != 0) & counts(t, t_min[:, None], t_max[:, None], planted) & fr["live"][:, None]
    return np.where(ok, sigma, 0), t, U, V, W, det


# ------------------------------------------------------------------ R5
def _inputs(verts, faces, o, d, t_min, t_max):
    v = np.asarray(verts, F32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    o = np.asarray(o, F32).reshape(-1, 3).astype(np.float64)
    d = np.asarray(d, F32).reshape(-1, 3).astype(np.float64)
    lo = np.broadcast_to(np.asarray(t_min, F32).astype(np.float64), (len(o),)).copy()
    hi = np.broadcast_to(np.asarray(t_max, F32).astype(np.float64), (len(o),)).copy()
    return v, f, o, d, lo, hi


def _empty(Q):
    return dict(face=np.full(Q, -1, np.int32), t=np.full(Q, INF), weights=np.zeros((Q, 3), F32), side=np.zeros(Q, np.int8),
                signed=np.zeros(Q, np.int32), total=np.zeros(Q, np.int32))


def _first(out, q, ids, sigma, t, U, V, W, det, cull, planted=None):
    """Take the faces ``ids`` with their terms (1-D) into the first hit of ray q: the smallest t, ties to the lowest face index."""
    keep = sigma != 0
    if cull == 1:
        keep &= sigma < 0                                              # back-facing faces (sigma = +1) are dropped
    elif cull == 2:
        keep &= sigma > 0
    for k in np.nonzero(keep)[0]:
        better = t[k] < out["t"][q] or (t[k] == out["t"][q] and (ids[k] > out["face"][q] if planted == "tie_high" else ids[k] < out["face"][q]))
        if better:
            with np.errstate(all="ignore"):
                w = np.array([U[k], V[k], W[k]]) / det[k]
            out["t"][q], out["face"][q], out["weights"][q], out["side"][q] = t[k], ids[k], w.astype(F32), -sigma[k]


def brute_force(verts, faces, o, d, t_min=0.0, t_max=INF, cull=0, planted=None):
    """R5 for one object, over all usable faces: dict(face (Q,) int32, t (Q,) float64, weights (Q, 3) fp32, side (Q,) int8, signed and
    total (Q,) int32).  ``cull`` bears on the first hit only."""
    v, f, o, d, lo, hi = _inputs(verts, faces, o, d, t_min, t_max)
    ids = np.nonzero(NR.usable_faces(verts, faces))[0]
    out = _empty(len(o))
    if not len(ids) or not len(o):
        return out
    tri = v[f[ids]][None]
    for q0 in range(0, len(o), 256):
        q = slice(q0, q0 + 256)
        fr = ray_frame(o[q], d[q], planted)
        sigma, t, U, V, W, det = face_terms(fr, tri, lo[q], hi[q], planted)
        out["signed"][q], out["total"][q] = sigma.sum(1), (sigma != 0).sum(1)
        for r in np.nonzero((sigma != 0).any(1))[0]:
            _first(out, q0 + r, ids, sigma[r], t[r], U[r], V[r], W[r], det[r], cull, planted)
    return out


def bad_flag(verts, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return bool(((f < 0) | (f >= np.asarray(verts).reshape(-1, 3).shape[0])).any())


# ------------------------------------------------------------------ R6
def clip(g, o, d, t_min, t_max):
    """(t_a, t_b, s) of one ray against the object's bounds widened by the slack s = 2^-40 (E + m), m the largest over the axes of
    lo - o, o - hi and 0; None where the ray misses them or t_min < t_max fails."""
    if not t_min < t_max:
        return None
    m = max(0.0, float((g["lo"] - o).max()), float((o - g["hi"]).max()))
    s = SLACK * (g["extent"] + m)
    ta, tb = t_min, t_max
    for a in range(3):
        if d[a] != 0:
            t1, t2 = ((g["lo"][a] - s) - o[a]) / d[a], ((g["hi"][a] + s) - o[a]) / d[a]
            if t1 > t2:
                t1, t2 = t2, t1
            ta, tb = max(ta, t1), min(tb, t2)
        elif o[a] < g["lo"][a] - s or o[a] > g["hi"][a] + s:
            return None
    return (ta, tb, s) if ta <= tb else None


def _cell1(g, a, x):
    p = np.zeros(3)
    p[a] = x
    return int(NR.cell_of(g, p)[a])


def walk(verts, faces, o, d, h, t_min=0.0, t_max=INF, cull=0, planted=None):
    """R6 for one object over the grid of edge ``h``: (the dict of ``brute_force``, faces looked at per ray (Q,), repeats counted).  The
    first hit and the crossings are walked separately, as the two kernels do: only the first walk cuts at the best t and stops early.
    (The terms of a (ray, face) pair do not depend on the cell it is met in, so they are formed once per ray.)"""
    v, f, o, d, lo, hi = _inputs(verts, faces, o, d, t_min, t_max)
    g = NR.grid(verts, h)
    lists = {c: np.asarray(ids, np.int64) for c, ids in NR.cell_lists(verts, faces, g).items()}
    n, hh = g["n"], g["h"]
    out, looked = _empty(len(o)), np.zeros(len(o), np.int64)
    if not lists:
        return out, looked
    tri = v[np.where(NR.usable_faces(verts, faces)[:, None], f, 0)]
    fl, fh = NR.cell_of(g, tri.min(1)), NR.cell_of(g, tri.max(1))
    for q in range(len(o)):
        fr = ray_frame(o[q:q + 1], d[q:q + 1], planted)
        c = clip(g, o[q], d[q], lo[q], hi[q]) if fr["live"][0] else None
        if c is None:
            continue
        ta, tb, s = c
        sigma, t, U, V, W, det = (x[0] for x in face_terms(fr, tri[None], lo[q:q + 1], hi[q:q + 1], planted))
        kx, ky, kz = int(fr["kx"][0]), int(fr["ky"][0]), int(fr["kz"][0])
        oz, dz = o[q, kz], d[q, kz]
        st = s / abs(dz)
        c_in, c_out, step = _cell1(g, kz, oz + ta * dz), _cell1(g, kz, oz + tb * dz), (1 if dz > 0 else -1)
        with np.errstate(all="ignore"):
            # crossings: the slab a face counts in -- that of its hit, clamped to the face's own slabs and to the walk's
            kh = np.clip(NR.cell_of(g, np.stack([np.where(sigma != 0, oz + t * dz, oz)] * 3, 1))[:, kz], fl[:, kz], fh[:, kz])
        kh = np.clip(kh, min(c_in, c_out), max(c_in, c_out))
        for first in (True, False):
            for k in range(c_in, c_out + step, step):
                tp = ((g["lo"][kz] + float(k + (step > 0)) * hh) - oz) / dz              # the slab's far plane
                tn = ((g["lo"][kz] + float(k + (step < 0)) * hh) - oz) / dz              # and its near plane
                t_near = ta if k == c_in else max(ta, tn - st)
                t_far = tb if k == c_out else min(tb, tp + st)
                if first:
                    t_far = min(t_far, out["t"][q] + st)
                if t_near <= t_far:
                    rect = []
                    for a in (kx, ky):
                        x0, x1 = o[q, a] + t_near * d[q, a], o[q, a] + t_far * d[q, a]
                        rect.append((_cell1(g, a, min(x0, x1) - s), _cell1(g, a, max(x0, x1) + s)))
                    for i in range(rect[0][0], rect[0][1] + 1):
                        for j in range(rect[1][0], rect[1][1] + 1):
                            cc = [0, 0, 0]
                            cc[kx], cc[ky], cc[kz] = i, j, k
                            ids = lists.get(int((cc[0] * n[1] + cc[1]) * n[2] + cc[2]))
                            if ids is None:
                                continue
                            if first:
                                looked[q] += len(ids)
                                _first(out, q, ids, sigma[ids], t[ids], U[ids], V[ids], W[ids], det[ids], cull, planted)
                                continue
                            sg = sigma[ids]
                            if planted != "every_cell":
                                # once: in slab kh, in the first cell of that slab's rectangle that lists the face
                                here = (kh[ids] == k) & (np.maximum(fl[ids, kx], rect[0][0]) == i) & (np.maximum(fl[ids, ky], rect[1][0]) == j)
                                sg = np.where(here, sg, 0)
                            out["signed"][q] += sg.sum()
                            out["total"][q] += (sg != 0).sum()
                if first and (out["t"][q] < tp - st or (planted == "stop_at_first_hit" and out["t"][q] < INF)):
                    break
    return out, looked


# ------------------------------------------------------------------ closed forms
def box_slab(o, d, half, t_min=0.0, t_max=INF):
    """The slab method in float64 for the axis-parallel box +-half: (t_enter, t_exit) per ray; t_enter > t_exit where the line misses."""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t1, t2 = (-np.asarray(half) - o) / d, (np.asarray(half) - o) / d
    near, far = np.minimum(t1, t2), np.maximum(t1, t2)
    par = d == 0
    inside = np.abs(o) < np.asarray(half)
    near, far = np.where(par, np.where(inside, -INF, INF), near), np.where(par, np.where(inside, INF, -INF), far)
    return near.max(1), far.min(1)


def plane_depth(o, d, a, b, c):
    """t = n . (a - o) / (n . d), n = (b - a) x (c - a): the closed form ``geometry.ray_mesh`` differentiates; and its gradients
    (dt/do, dt/dd, dt/da, dt/db, dt/dc), all float64."""
    o, d, a, b, c = (np.asarray(x, np.float64) for x in (o, d, a, b, c))
    n = np.cross(b - a, c - a)
    nd = n @ d
    t = n @ (a - o) / nd
    p = o + t * d
    # dt/dn = ((a - o) - t d) / nd = (a - p) / nd;  dn = d(b - a) x (c - a) + (b - a) x d(c - a)
    gn = (a - p) / nd
    ga = n / nd + (np.cross(b - a, gn) - np.cross(c - a, gn))
    gb = np.cross(c - a, gn)
    gc = -np.cross(b - a, gn)
    return t, (-n / nd, -t * n / nd, ga, gb, gc)


# ------------------------------------------------------------------ the cases the CPU and the GPU tests share
OBLIQUE = (0.25, 0.5, 1.0)                     # few bits: rays through few-bit targets stay exact, so they pass exactly through them
DOUBLED = (IR.TRI, np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0]], np.int32))       # one triangle three times: every hit is a tie
ROOF = (np.array([[0, 0, 0], [4, 0, 4], [0, 4, 4], [1, 1, 1], [2, 1, 1], [1, 2, 1]], F32), np.array([[0, 1, 2], [3, 4, 5]], np.int32))
DYADIC_HALF = (0.25, 0.125, 0.5)


def rays_through(targets, d, back=2.0):
    """Rays of direction d through the target points, starting ``back`` d before them."""
    targets = np.asarray(targets, np.float64).reshape(-1, 3)
    d = np.broadcast_to(np.asarray(d, np.float64), targets.shape)
    return (targets - back * d).astype(F32), d.astype(F32)


def shared_targets(verts, faces):
    """(points on interior edges and vertices -- shared by faces all around --, points on boundary edges and vertices) of a small open
    mesh: every vertex and every edge midpoint, sorted by whether all edges they lie on have two faces."""
    v = np.asarray(verts, np.float64)
    count = {}
    for f in np.asarray(faces):
        for k in range(3):
            e = tuple(sorted((int(f[k]), int(f[(k + 1) % 3]))))
            count[e] = count.get(e, 0) + 1
    inner, border = [], []
    for (i, j), c in count.items():
        (inner if c == 2 else border).append((v[i] + v[j]) / 2)
    for i in range(len(v)):
        edges = [c for e, c in count.items() if i in e]
        (inner if edges and min(edges) == 2 else border).append(v[i])
    return np.array(inner), np.array(border)


def hand_cases():
    """[(name, verts, faces, rays_o, rays_d, t_min, t_max, cull)]: small cases with results known by hand (tests/test_mesh_raycast_cpu.py
    says which); the GPU tests hold the kernels to the restatement on every one."""
    cases = [("triangle", IR.TRI, IR.ONE, F32([[.25, .25, -1], [.25, .25, 3], [.25, .25, -1], [.25, .25, 3]]),
              F32([[0, 0, 2], [0, 0, -1], [0, 0, 2], [0, 0, -1]]), 0.0, INF, c) for c in (0, 1, 2)]
    for name, (v, f) in (("square", IR.SQUARE), ("fan", IR.FAN)):
        inner, border = shared_targets(v, f)
        for d in ((0, 0, 1), OBLIQUE, (-0.5, 0.25, -1.0)):
            o, dd = rays_through(np.concatenate([inner, border]), d)
            cases.append((f"{name} {d}", v, f, o, dd, 0.0, INF, 0))
    cases.append(("in the plane", IR.TRI, IR.ONE, F32([[-1, .25, 0], [-1, 0, 0], [.25, -1, 0]]), F32([[1, 0, 0], [1, .25, 0], [0, 1, 0]]), 0.0, INF, 0))
    nv, nf, nq = IR.NEVER
    for d in ((0, 0, 1), (0, 0, -1), (1, 0, 0)):
        o, dd = rays_through(nq, d, 4.0)
        cases.append((f"never {d}", nv, nf, o, dd, 0.0, INF, 0))
    sv, sf, sq = IR.skew_mesh()
    cases.append(("skew", sv, sf, sq, F32([[0, 0, 1]]), 0.0, INF, 0))
    cases.append(("doubled", *DOUBLED, F32([[.25, .25, -1], [.5, .5, 1], [0, 0, -2]]), F32([[0, 0, 1], [0, 0, -1], [0, 0, 1]]), 0.0, INF, 0))
    bv, bf = IR.box12(DYADIC_HALF)
    o = F32([[-1, .0625, .125], [-1, .0625, .125], [-1, .0625, .125], [-1, .0625, .125], [-.25, .0625, .125], [-1, 0, 0], [.25, .0625, .125]])
    d = F32([[1, 0, 0]] * 6 + [[-1, 0, 0]])
    cases.append(("box strict", bv, bf, o, d, F32([0, .75, 0, .75, 0, 0, 0]), F32([INF, INF, .75, 1.25, INF, INF, .5]), 0))
    return cases


def aimed_rays(rng, origins, lo, hi, share=0.7):
    """fp32 rays from ``origins``: ``share`` of them aimed at uniform points of the box lo .. hi, the rest in random directions."""
    origins = np.asarray(origins, F32)
    d = rng.normal(size=origins.shape)
    aim = rng.uniform(size=len(origins)) < share
    d[aim] = rng.uniform(lo, hi, (int(aim.sum()), 3)) - origins[aim]
    return origins, d.astype(F32)


def walk_cases():
    """[(name, verts, faces, cell edge, rays_o, rays_d, t_min, t_max)]: where the pruned walk of R6 could go wrong."""
    v, f = IR.octahedron()
    rng = np.random.default_rng(11)
    o, d = aimed_rays(rng, IR.octa_queries(), -0.4, 0.4)                     # rays that start outside the grid, inside it, on its border
    cases = [("octahedron at 16 cells", v, f, 1 / 16, o, d, 0.0, INF), ("octahedron, one cell", v, f, 1.0, o, d, 0.0, INF)]
    cases.append(("octahedron, t_max inside", v, f, 1 / 16, o, d, F32(0.125), rng.uniform(0.2, 0.9, len(o)).astype(F32)))
    far = (rng.uniform(-0.4, 0.4, (24, 3)) + np.eye(3)[np.arange(24) % 3] * 3 * (-1) ** (np.arange(24) // 3)[:, None]).astype(F32)
    away = (far * F32(0.5)).astype(F32)                                      # leaving, and passing by
    cases.append(("octahedron, rays that miss the bounds", v, f, 1 / 16, np.concatenate([far, far]),
                  np.concatenate([away, np.roll(away, 1, axis=1)]), 0.0, INF))
    # axis-parallel rays lying exactly in cell planes and through cell corners, in both directions of every axis
    g = np.arange(0, 17, 2) / 16 - 0.5
    P, Q = np.meshgrid(g, g, indexing="ij")
    oo, dd = [], []
    for a in range(3):
        for sgn in (1, -1):
            p = np.zeros((P.size, 3))
            p[:, a], p[:, (a + 1) % 3], p[:, (a + 2) % 3] = -sgn, P.ravel(), Q.ravel()
            oo.append(p)
            dd.append(np.broadcast_to(np.eye(3)[a] * sgn, p.shape))
    cases.append(("octahedron, rays in cell planes", v, f, 1 / 16, np.concatenate(oo).astype(F32), np.concatenate(dd).astype(F32), 0.0, INF))
    tv = (v * IR.THIN).astype(F32)                                           # an axis clamped to 256 cells
    to, td = aimed_rays(np.random.default_rng(12), IR.octa_queries(IR.THIN), -0.4 * IR.THIN, 0.4 * IR.THIN)
    cases.append(("thin octahedron, a clamped axis", tv, f, 1e-3, to, td, 0.0, INF))
    cases.append(("roof", *ROOF, 0.5, F32([[1.25, 1.25, -1], [1.25, 1.25, 5], [-1, 1.25, 1.125]]), F32([[0, 0, 1], [0, 0, -1], [1, 0, .25]]), 0.0, INF))
    sv, sf, sq = IR.sphere_case()
    so, sd = aimed_rays(np.random.default_rng(13), sq[:96], -0.3, 0.3)
    cases.append(("sphere", sv, sf, 0.1, so, sd, 0.0, INF))
    return cases
