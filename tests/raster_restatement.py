"""The mesh rasteriser's rules (include/supnerf_hip.h, "Mesh rasteriser"), restated in numpy step by step: what the ``snr_raster_*`` kernels
are held to bit for bit.  Every fp32 step is one numpy float32 operation (one rounding); orientation and coverage are int64; a face is
evaluated over its whole candidate box at once.  Also the hand-made meshes the CPU and GPU tests share."""
import numpy as np

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_PIXEL = F32(2.0 ** 22)


def project(verts, n_verts, mats, cam):
    """Rule 1: screen (sum V, 3) fp32 = (u, v, camera z); ``mats`` (B, 3, 4) fp32, ``cam`` = (fx, fy, cx, cy)."""
    verts, mats = np.asarray(verts, F32), np.asarray(mats, F32)
    fx, fy, cx, cy = [F32(c) for c in cam]
    M = np.repeat(mats, np.asarray(n_verts, np.int64), axis=0)                      # (sum V, 3, 4): each vertex's object's matrix
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    with np.errstate(all="ignore"):
        c = [((M[:, k, 0] * x + M[:, k, 1] * y) + M[:, k, 2] * z) + M[:, k, 3] for k in range(3)]
        return np.stack([fx * (c[0] / c[2]) + cx, fy * (c[1] / c[2]) + cy, c[2]], axis=1).astype(F32)


def snap_all(tri, z_near):
    """Rule 2 for many faces at once: ``tri`` (F, 3, 3) their screen vertices -> (xs (F, 3) int64, ys (F, 3) int64, iz (F, 3) fp32,
    kept (F,) bool); the numbers of a dropped face mean nothing."""
    u, v, z = tri[..., 0], tri[..., 1], tri[..., 2]
    with np.errstate(all="ignore"):
        ok = (np.abs(u) < MAX_PIXEL) & (np.abs(v) < MAX_PIXEL) & (z >= F32(z_near)) & (z < F32(np.inf))    # (all false on a NaN)
        keep = ok.all(-1)
        safe = lambda a: np.where(keep[:, None], a, F32(0))                         # noqa: E731
        xs = np.rint(safe(u) * F32(256)).astype(np.int64)                           # (half to even)
        ys = np.rint(safe(v) * F32(256)).astype(np.int64)
        return xs, ys, (F32(1) / z).astype(F32), keep


def snap(sv, z_near):
    """Rule 2 for one face: ``sv`` (3, 3) its screen vertices -> (xs (3,) ints, ys (3,) ints, iz (3,) fp32), or None when dropped."""
    xs, ys, iz, keep = snap_all(np.asarray(sv, F32)[None], z_near)
    return ([int(a) for a in xs[0]], [int(a) for a in ys[0]], iz[0]) if keep[0] else None


def area(xs, ys):
    """Rule 3: A, an exact python integer."""
    return (xs[1] - xs[0]) * (ys[2] - ys[0]) - (xs[2] - xs[0]) * (ys[1] - ys[0])


def edges(xs, ys, A):
    """Rule 4's per-edge constants: [(dx, dy, owns ties, a_x, a_y)] for i = 0, 1, 2."""
    s = 1 if A > 0 else -1
    out = []
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = s * (xs[b] - xs[a]), s * (ys[b] - ys[a])
        out.append((dx, dy, dy > 0 or (dy == 0 and dx < 0), xs[a], ys[a]))
    return out


def box(xs, ys, H, W):
    """The candidate pixels (x0, x1, y0, y1), both ends included, or None."""
    x0, x1 = max((min(xs) + 255) >> 8, 0), min(max(xs) >> 8, W - 1)
    y0, y1 = max((min(ys) + 255) >> 8, 0), min(max(ys) >> 8, H - 1)
    return None if x1 < x0 or y1 < y0 else (x0, x1, y0, y1)


def cover(xs, ys, A, PX, PY):
    """Rule 4 at the pixel centres (PX, PY) (int64 arrays): (covered, [E_0, E_1, E_2])."""
    X, Y = PX.astype(np.int64) * 256, PY.astype(np.int64) * 256
    cov, E = np.ones(PX.shape, bool), []
    for dx, dy, owns, ax, ay in edges(xs, ys, A):
        e = np.int64(dx) * (Y - np.int64(ay)) - np.int64(dy) * (X - np.int64(ax))
        cov &= (e > 0) | ((e == 0) & owns)
        E.append(e)
    return cov, E


def depth_weights(E, iz, A):
    """Rules 5 and 7 from the edge functions: (depth, weights (..., 3)), fp32."""
    with np.errstate(all="ignore"):
        t = [E[i].astype(F32) * iz[i] for i in range(3)]
        q = (t[0] + t[1]) + t[2]
        depth = np.array(abs(A), np.int64).astype(F32) / q
        return depth.astype(F32), np.stack([t[i] / q for i in range(3)], axis=-1).astype(F32)


def rasterize(verts, faces, n_verts, n_faces, mats, cam, H, W, z_near=1e-3, image_of=None, n_images=1, cull_sign=None):
    """Rules 1 - 7 on a packed mesh: dict(face (n_images, H, W) int32, obj int32, depth fp32, weights (n_images, H, W, 3) fp32,
    keys uint64, screen).  ``image_of`` (B,): the image of each object (default all 0); ``cull_sign`` (B,) ints or None."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    B = len(n_verts)
    voff, foff = np.concatenate([[0], np.cumsum(n_verts)]).astype(np.int64), np.concatenate([[0], np.cumsum(n_faces)]).astype(np.int64)
    image_of = np.zeros(B, np.int64) if image_of is None else np.asarray(image_of, np.int64)
    screen = project(verts, n_verts, mats, cam)
    keys = np.full((n_images, H, W), EMPTY, np.uint64)
    weights = np.zeros((n_images, H, W, 3), F32)
    nF = faces.shape[0]
    obj_of = np.searchsorted(foff[1:], np.arange(nF), side="right")                  # the object of each face
    V = (voff[1:] - voff[:-1])[obj_of] if nF else np.zeros(0, np.int64)
    img = image_of[obj_of] if nF else np.zeros(0, np.int64)
    keep = ((faces >= 0) & (faces < V[:, None])).all(1) & (img >= 0) & (img < n_images)
    rows = np.where(keep[:, None], faces + voff[obj_of][:, None], 0)
    xs_all, ys_all, iz_all, ok = snap_all(screen[rows], z_near)
    A_all = area(xs_all.T, ys_all.T)                                                 # (int64: exact, every product is below 2^62)
    keep &= ok & (A_all != 0)
    if cull_sign is not None:
        keep &= ~(A_all * np.asarray(cull_sign, np.int64)[obj_of] > 0)
    x0s, x1s = np.maximum((xs_all.min(1) + 255) >> 8, 0), np.minimum(xs_all.max(1) >> 8, W - 1)
    y0s, y1s = np.maximum((ys_all.min(1) + 255) >> 8, 0), np.minimum(ys_all.max(1) >> 8, H - 1)
    keep &= (x1s >= x0s) & (y1s >= y0s)
    for f in np.nonzero(keep)[0]:
        xs, ys, iz, A = [int(a) for a in xs_all[f]], [int(a) for a in ys_all[f]], iz_all[f], int(A_all[f])
        x0, x1, y0, y1 = box(xs, ys, H, W)
        PY, PX = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        cov, E = cover(xs, ys, A, PX, PY)
        if not cov.any():
            continue
        depth, w = depth_weights(E, iz, A)
        key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)      # rule 6
        old = keys[img[f], y0:y1 + 1, x0:x1 + 1]
        win = cov & (key < old)
        old[win] = key[win]
        weights[img[f], y0:y1 + 1, x0:x1 + 1][win] = w[win]
    empty = keys == EMPTY
    face = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth = np.where(empty, F32(0), (keys >> np.uint64(32)).astype(np.uint32).view(F32)).astype(F32)
    obj = np.where(empty, -1, np.searchsorted(foff[1:], face, side="right")).astype(np.int32)
    return dict(face=face, obj=obj, depth=depth, weights=weights, keys=keys, screen=screen)


def interpolate(face, weights, faces, n_verts, n_faces, attributes, background=0.0):
    """Rule 8: (..., C) fp32 from packed per-vertex ``attributes`` (sum V, C)."""
    faces, att = np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(attributes, F32)
    voff = np.concatenate([[0], np.cumsum(n_verts)]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum(n_faces)]).astype(np.int64)
    out = np.full(face.shape + (att.shape[1],), F32(background), F32)
    hit = face >= 0
    f = face[hit].astype(np.int64)
    g = faces[f] + voff[np.searchsorted(foff[1:], f, side="right")][:, None]         # global vertex rows of each winning face
    w = weights[hit]
    out[hit] = (w[:, 0:1] * att[g[:, 0]] + w[:, 1:2] * att[g[:, 1]]) + w[:, 2:3] * att[g[:, 2]]
    return out


# ---- cameras and hand-made meshes
IDENTITY = np.concatenate([np.eye(3, dtype=F32), np.zeros((3, 1), F32)], axis=1)


def screen_mesh(points_px, depth=1.0):
    """Vertices that the camera (fx, fy, cx, cy) = (1, 1, 0, 0) with the identity matrix projects EXACTLY to the pixel coordinates
    ``points_px`` (n, 2) (multiples of 1/256 up to a few thousand, and a depth that is a power of two, keep every step exact)."""
    p = np.asarray(points_px, np.float64)
    z = np.broadcast_to(np.asarray(depth, np.float64), p.shape[:1])
    return np.stack([p[:, 0] * z, p[:, 1] * z, z], axis=1).astype(F32)


UNIT_CAM = (1.0, 1.0, 0.0, 0.0)


def fan(centre=(8.0, 8.0), radius=6.0, spokes=7, clockwise=False):
    """(points (n, 2) px, faces): a closed fan of triangles around a vertex exactly on a pixel centre; rim vertices on 1/256 pixel."""
    ang = 2 * np.pi * (np.arange(spokes) + 0.3) / spokes
    rim = np.round((np.stack([np.cos(ang), np.sin(ang)], 1) * radius + centre) * 256) / 256
    pts = np.concatenate([[centre], rim])
    f = np.array([[0, 1 + k, 1 + (k + 1) % spokes] for k in range(spokes)], np.int32)
    return pts, (f[:, ::-1].copy() if clockwise else f)


def lattice_sheet(nx=9, ny=7, pitch=2.25, origin=(1.25, 1.5), seed=3, clockwise=False):
    """(points, faces): a sheet of 2 (nx - 1)(ny - 1) triangles on a lattice of ``pitch`` pixels whose vertices are jittered on the
    quarter-pixel lattice (so many vertices and edges fall exactly on pixel centres), diagonals alternating."""
    rng = np.random.default_rng(seed)
    jx, jy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    pts = np.stack([jx, jy], -1).reshape(-1, 2) * pitch + origin + rng.integers(-2, 3, (nx * ny, 2)) * 0.25
    f = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            f += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    f = np.array(f, np.int32)
    return pts, (f[:, ::-1].copy() if clockwise else f)


def sphere(n_lat=24, n_lon=48, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """(verts (V, 3) fp32 ON the sphere up to fp32 rounding, faces int32 wound counter-clockwise seen from outside): a latitude /
    longitude tessellation with two pole vertices."""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    T, P = np.meshgrid(th, ph, indexing="ij")
    ring = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    f, south = [], 1 + (n_lat - 1) * n_lon
    for j in range(n_lon):
        k = (j + 1) % n_lon
        f.append([0, 1 + j, 1 + k])
        for i in range(n_lat - 2):
            a, b, c, d = 1 + i * n_lon + j, 1 + (i + 1) * n_lon + j, 1 + (i + 1) * n_lon + k, 1 + i * n_lon + k
            f += [[a, b, c], [a, c, d]]
        f.append([south, 1 + (n_lat - 2) * n_lon + k, 1 + (n_lat - 2) * n_lon + j])
    return v.astype(F32), np.array(f, np.int32)
