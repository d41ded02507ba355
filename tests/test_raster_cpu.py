"""The mesh rasteriser's rules without a GPU: tests/raster_restatement.py -- what the ``snr_raster_*`` kernels are held to bit for bit in
tests/test_raster_gpu.py -- checked against exact rational arithmetic (coverage), float64 (depth), an analytic sphere, and the properties
the header promises: every interior pixel of a mesh covered exactly once, the nearest face wins with ties to the lowest index, the image
does not depend on the order of the faces, culling by orientation, dropped faces.  Also the host side: ABI version, symbols, no CPU path."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import raster_restatement as RR
from oracle_bands import amd  # noqa: F401  (a fixture)

EPS = 2.0 ** -24          # one fp32 rounding, relative
RASTER_SYMBOLS = ["snr_raster_project", "snr_raster_faces", "snr_raster_resolve", "snr_raster_interpolate"]


def _draw(points_px, faces, H, W, depth=1.0, **kw):
    """The restatement on a mesh given in pixel coordinates (exact projection: ``RR.screen_mesh``)."""
    v = RR.screen_mesh(points_px, depth)
    return RR.rasterize(v, faces, [v.shape[0]], [len(faces)], RR.IDENTITY[None], RR.UNIT_CAM, H, W, **kw)


# ------------------------------------------------------------------------------------ coverage
def _exact_cover(xs, ys, px, py):
    """Rule 4 in exact rationals, arranged differently from the restatement: pixel coordinates as fractions of a pixel, the side of every
    edge from the cross product (b - a) x (p - a) taken relative to the triangle's own orientation.  Returns (strictly inside, covered)."""
    P = [(Fraction(x, 256), Fraction(y, 256)) for x, y in zip(xs, ys)]
    p = (Fraction(px), Fraction(py))
    A = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[2][0] - P[0][0]) * (P[1][1] - P[0][1])
    if A == 0:
        return False, False
    s = 1 if A > 0 else -1
    strict = covered = True
    for i in range(3):
        a, b = P[(i + 1) % 3], P[(i + 2) % 3]
        dx, dy = s * (b[0] - a[0]), s * (b[1] - a[1])
        side = dx * (p[1] - a[1]) - dy * (p[0] - a[0])
        strict = strict and side > 0
        covered = covered and (side > 0 or (side == 0 and (dy > 0 or (dy == 0 and dx < 0))))
    return strict, covered


def _coverage_cases():
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(40):                                      # random triangles around a 12 x 10 image, some reaching far outside
        cases.append(rng.integers(-3 * 256, 14 * 256, (3, 2)))
    for _ in range(10):                                      # vertices thousands of pixels away: products near 2^60
        far = rng.integers(-2 ** 29, 2 ** 29, (3, 2))
        far[0] = rng.integers(0, 10 * 256, 2)
        cases.append(far)
    for _ in range(20):                                      # smaller than a pixel: most cover no centre
        cases.append(rng.integers(0, 10 * 256, 2) + rng.integers(-100, 100, (3, 2)))
    for _ in range(30):                                      # vertices and edges exactly on pixel centres (multiples of 256)
        cases.append(rng.integers(0, 11, (3, 2)) * 256)
    cases.append(np.array([[0, 0], [8 * 256, 0], [0, 8 * 256]]))         # axis-parallel edges through centres, both windings
    cases.append(np.array([[0, 0], [0, 8 * 256], [8 * 256, 0]]))
    cases.append(np.array([[256, 256], [5 * 256, 5 * 256], [9 * 256, 9 * 256]]))      # A = 0
    return cases


def test_coverage_matches_exact_rationals():
    H, W = 10, 12
    PY, PX = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    n_cov = n_none = n_tie = 0
    for tri in _coverage_cases():
        xs, ys = [int(v) for v in tri[:, 0]], [int(v) for v in tri[:, 1]]
        A = RR.area(xs, ys)
        exact = np.array([[_exact_cover(xs, ys, px, py) for px in range(W)] for py in range(H)])
        if A == 0:
            assert not exact[..., 1].any()
            continue
        cov, E = RR.cover(xs, ys, A, PX, PY)
        assert np.array_equal(cov, exact[..., 1]), (xs, ys)
        assert (cov[exact[..., 0]]).all()                                         # strictly inside is always covered
        assert all((E[0] + E[1] + E[2] == abs(A)).ravel())                        # the edge functions sum to s A: rule 5's numerator
        bx = RR.box(xs, ys, H, W)                                                 # nothing is covered outside the candidate box
        inside_box = np.zeros((H, W), bool)
        if bx is not None:
            inside_box[bx[2]:bx[3] + 1, bx[0]:bx[1] + 1] = True
        assert not (cov & ~inside_box).any(), (xs, ys, bx)
        n_cov += int(cov.sum())
        n_none += int(not cov.any())
        n_tie += int((cov & ~exact[..., 0]).sum())
    print(f"coverage: {n_cov} covered centres, {n_none} triangles covering none, {n_tie} centres won on a tie")
    assert n_cov > 500 and n_none > 10 and n_tie > 20                             # the cases reach what they are meant to reach


def _cover_counts(points_px, faces, H, W):
    """(how many faces cover each pixel, interior mask, outside mask), all from exact integers.  Interior: in the closed triangle of some
    face and on no border edge (an edge only one face has); outside: in no closed triangle."""
    xs_all = np.rint(np.asarray(points_px, np.float64) * 256).astype(np.int64)
    assert np.array_equal(xs_all, np.asarray(points_px, np.float64) * 256)        # the meshes sit on the 1/256 lattice
    PY, PX = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    n_edge = {}
    for f in faces:
        for i in range(3):
            e = tuple(sorted((int(f[(i + 1) % 3]), int(f[(i + 2) % 3]))))
            n_edge[e] = n_edge.get(e, 0) + 1
    count, closed_any, on_border = np.zeros((H, W), int), np.zeros((H, W), bool), np.zeros((H, W), bool)
    for f in faces:
        xs, ys = [int(xs_all[i, 0]) for i in f], [int(xs_all[i, 1]) for i in f]
        A = RR.area(xs, ys)
        cov, E = RR.cover(xs, ys, A, PX, PY)
        closed = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
        count += cov
        closed_any |= closed
        for i in range(3):
            if n_edge[tuple(sorted((int(f[(i + 1) % 3]), int(f[(i + 2) % 3]))))] == 1:
                on_border |= closed & (E[i] == 0)
    return count, closed_any & ~on_border, ~closed_any


@pytest.mark.parametrize("clockwise", [False, True])
def test_fan_and_lattice_cover_every_interior_pixel_once(clockwise):
    for name, (pts, faces), (H, W) in (("fan", RR.fan(clockwise=clockwise), (17, 17)),
                                       ("fan12", RR.fan((9.0, 7.0), 6.5, 12, clockwise), (16, 18)),
                                       ("sheet", RR.lattice_sheet(clockwise=clockwise), (17, 23))):
        count, interior, outside = _cover_counts(pts, faces, H, W)
        assert interior.sum() > 60, name
        assert (count[interior] == 1).all(), (name, np.argwhere(interior & (count != 1))[:5])
        assert (count[outside] == 0).all(), name
        assert count.max() == 1, name                                             # and a border pixel at most once
        r = _draw(pts, faces, H, W)                                               # the whole pipeline agrees with the counts
        assert np.array_equal(r["face"][0] >= 0, count == 1), name


def test_vertex_on_a_pixel_centre_belongs_to_one_face():
    for cw in (False, True):
        pts, faces = RR.fan(clockwise=cw)
        count, _, _ = _cover_counts(pts, faces, 17, 17)
        assert count[8, 8] == 1                                                   # the fan's hub is the centre of pixel (8, 8)


# ------------------------------------------------------------------------------------ depth
# Rule 5, roundings on the way to one depth, all relative (every term is positive, nothing cancels): iz_i = 1 / z_i (1), float(E_i) (1),
# their product (1): each term carries (1 + e)^3; the first sum (1) and the second (1) put at most 2 more on a term: q within 5 e; float(s A)
# (1) and the division (1): 7 roundings on the longest path, (1 + e)^7 - 1 = 7 e + O(e^2).  The band is 8 e: one e for the second-order terms
# and the float64 reference's own error.
DEPTH_BAND = 8 * EPS


def _exact_depth(E, z, A):
    """Perspective-correct interpolation in float64 on the snapped vertices: 1 / sum(lambda_i / z_i), lambda_i = E_i / (s A)."""
    lam = [E[i].astype(np.float64) / float(abs(A)) for i in range(3)]
    return 1.0 / sum(lam[i] / np.float64(z[i]) for i in range(3))


def test_depth_against_float64():
    rng = np.random.default_rng(5)
    H, W = 24, 32
    PY, PX = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    worst, n = 0.0, 0
    for k in range(60):
        xs = [int(v) for v in rng.integers(-20 * 256, 50 * 256, 3)]
        ys = [int(v) for v in rng.integers(-20 * 256, 40 * 256, 3)]
        z = (10.0 ** rng.uniform(-1, 2, 3)).astype(np.float32)                    # 0.1 .. 100, up to 1000 : 1 across one face
        A = RR.area(xs, ys)
        if A == 0:
            continue
        cov, E = RR.cover(xs, ys, A, PX, PY)
        depth, w = RR.depth_weights(E, (np.float32(1) / z).astype(np.float32), A)
        ref = _exact_depth(E, z, A)
        err = np.abs(depth[cov].astype(np.float64) - ref[cov]) / ref[cov]
        worst, n = max(worst, err.max(initial=0.0)), n + int(cov.sum())
        assert (err <= DEPTH_BAND).all(), (k, err.max() / EPS)
        assert (depth[cov] >= z.min() * (1 - DEPTH_BAND)).all() and (depth[cov] <= z.max() * (1 + DEPTH_BAND)).all()
        assert (np.abs(w[cov].astype(np.float64).sum(-1) - 1) <= 8 * EPS).all()    # the weights are a partition of one, to rounding
    print(f"depth: worst relative error {worst / EPS:.2f} x 2^-24 over {n} pixels (band {DEPTH_BAND / EPS:.0f})")
    assert n > 5000


def test_interpolating_the_vertex_depths_gives_the_depth():
    """Perspective-correct weights: sum w_i z_i = sum (E_i / z_i) z_i / q = s A / q = depth.  In fp32: w_i within 3 + 2 + 1 roundings, the
    products and the two sums 3 more on positive terms -- 9 e; the depth itself 7 e away from the same real number."""
    pts = np.array([[1.5, 2.25], [20.0, 4.0], [7.75, 15.5]])
    z = np.array([2.0, 9.0, 0.5])
    v = RR.screen_mesh(pts, z)
    f = np.array([[0, 1, 2]], np.int32)
    r = RR.rasterize(v, f, [3], [1], RR.IDENTITY[None], RR.UNIT_CAM, 18, 22)
    out = RR.interpolate(r["face"], r["weights"], f, [3], [1], v[:, 2:3], background=-1.0)[..., 0]
    hit = r["face"][0] >= 0
    assert hit.sum() > 80 and (out[0][~hit] == -1.0).all()
    assert (np.abs(out[0][hit].astype(np.float64) - r["depth"][0][hit]) <= 16 * EPS * r["depth"][0][hit]).all()


# ------------------------------------------------------------------------------------ visibility
def test_coplanar_duplicates_go_to_the_lowest_index():
    pts = np.array([[1.0, 1.0], [14.0, 2.0], [6.0, 12.0]])
    r = _draw(pts, np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2]], np.int32), 14, 16, depth=np.array([1.0, 2.0, 4.0]))
    assert (r["face"] >= 0).sum() > 40 and set(np.unique(r["face"])) == {-1, 0}
    r = _draw(pts, np.array([[2, 1, 0], [0, 1, 2], [0, 1, 2]], np.int32), 14, 16, depth=np.array([1.0, 2.0, 4.0]), cull_sign=[-1])
    assert (r["face"] >= 0).sum() > 40 and set(np.unique(r["face"])) == {-1, 1}          # (face 0 faces the other way: culled)


def test_interpenetrating_triangles_switch_winner_along_their_intersection():
    pts = np.array([[0.5, 0.5], [30.5, 0.5], [0.5, 20.5], [30.5, 20.5]])
    za, zb = np.array([1.0, 3.0, 1.0, 3.0]), np.array([3.0, 1.0, 3.0, 1.0])          # two sheets that cross on the line x = 15.5
    v = np.concatenate([RR.screen_mesh(pts, za), RR.screen_mesh(pts, zb)])
    f = np.array([[0, 1, 2], [1, 3, 2], [4, 5, 6], [5, 7, 6]], np.int32)
    r = RR.rasterize(v, f, [8], [4], RR.IDENTITY[None], RR.UNIT_CAM, 22, 32)
    face, depth = r["face"][0], r["depth"][0]
    px = np.broadcast_to(np.arange(32), face.shape)
    inside = face >= 0
    assert inside[1:20, 1:30].all()
    assert np.isin(face[inside & (px < 15)], (0, 1)).all() and np.isin(face[inside & (px > 16)], (2, 3)).all()
    # per pixel the winner's depth is the smaller of the two sheets' float64 depths
    lam = (px - 0.5) / 30.0
    da, db = 1 / ((1 - lam) / 1.0 + lam / 3.0), 1 / ((1 - lam) / 3.0 + lam / 1.0)
    assert (np.abs(depth[inside] - np.minimum(da, db)[inside]) <= DEPTH_BAND * 3.0).all()


def _tie_free_scene():
    """A sphere in front of a big tilted triangle, with one exact duplicate face: ties only inside the duplicated pair."""
    v, f = RR.sphere(10, 16, 1.0, (0.1, -0.05, 4.0))
    back = np.array([[-3, -3, 5.0], [4, -2, 7.0], [-1, 4, 6.0]], np.float32)
    v2 = np.concatenate([v, back])
    f2 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]], f[5:6]]).astype(np.int32)
    return v2, f2, (60.0, 60.0, 23.5, 19.5), (40, 48)


def test_face_order_does_not_change_the_image():
    v, f, cam, (H, W) = _tie_free_scene()
    a = RR.rasterize(v, f, [len(v)], [len(f)], RR.IDENTITY[None], cam, H, W)
    perm = np.random.default_rng(2).permutation(len(f))                              # new face j is old face perm[j]
    b = RR.rasterize(v, f[perm], [len(v)], [len(f)], RR.IDENTITY[None], cam, H, W)
    assert (a["face"] >= 0).sum() > 600
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    assert np.array_equal(a["face"] >= 0, b["face"] >= 0)
    back = np.where(b["face"] >= 0, perm[np.maximum(b["face"], 0)], -1)
    twins = (5, len(f) - 1)                                                          # the duplicated pair: an exact tie
    differ = back != a["face"]
    assert np.isin(a["face"][differ], twins).all() and np.isin(back[differ], twins).all()
    assert np.array_equal(np.where(np.isin(back, twins), 5, back), np.where(np.isin(a["face"], twins), 5, a["face"]))


# ------------------------------------------------------------------------------------ the analytic sphere
SPHERE = dict(n_lat=24, n_lon=48, r=1.0, c=(0.13, -0.07, 4.0), cam=(250.0, 250.0, 79.5, 79.5), size=(160, 160))
_sphere_cache = {}


def _sphere_images():
    """The restatement's images of the sphere with both cull modes, under the identity and under a mirror: computed once."""
    if not _sphere_cache:
        s = SPHERE
        v, f = RR.sphere(s["n_lat"], s["n_lon"], s["r"], s["c"])
        H, W = s["size"]
        mirror = RR.IDENTITY.copy()
        mirror[0, 0] = -1.0                                                          # x -> -x: det < 0
        vm, fm = v * np.array([-1, 1, 1], np.float32), f[:, ::-1].copy()             # the mirror image, wound outward in its own frame
        args = ([len(v)], [len(f)])
        _sphere_cache.update(
            v=v, f=f,
            none=RR.rasterize(v, f, *args, RR.IDENTITY[None], s["cam"], H, W),
            back=RR.rasterize(v, f, *args, RR.IDENTITY[None], s["cam"], H, W, cull_sign=[1]),
            front=RR.rasterize(v, f, *args, RR.IDENTITY[None], s["cam"], H, W, cull_sign=[-1]),
            m_none=RR.rasterize(vm, fm, *args, mirror[None], s["cam"], H, W),
            m_back=RR.rasterize(vm, fm, *args, mirror[None], s["cam"], H, W, cull_sign=[-1]))
    return _sphere_cache


def _sphere_analytic(px, py):
    """Float64, per pixel: (camera z of the first hit of the sphere or NaN, impact parameter b of the pixel's ray, |(x, y, 1)|)."""
    fx, fy, cx, cy = SPHERE["cam"]
    d = np.stack([(px - cx) / fx, (py - cy) / fy, np.ones_like(px, dtype=np.float64)], -1)
    n = np.linalg.norm(d, axis=-1)
    u = d / n[..., None]
    c = np.asarray(SPHERE["c"], np.float64)
    tc = u @ c                                                                       # closest approach along the unit ray
    b = np.sqrt(np.maximum(c @ c - tc ** 2, 0.0))
    with np.errstate(invalid="ignore"):
        t = tc - np.sqrt(SPHERE["r"] ** 2 - b ** 2)
    return t / n, b, n, tc


def test_sphere_depth_within_sagitta_and_snapping():
    """|depth - analytic| on a sphere whose vertices lie ON the sphere.  Two terms, both derived here:

    Sagitta.  A point p = sum l_i v_i of a face with |v_i - c| = r has r^2 - |p - c|^2 = sum_{i<j} l_i l_j |v_i - v_j|^2 <= L^2 / 3 (L the
    longest edge; sum_{i<j} l_i l_j <= 1/3).  So the mesh lies between radius rho = sqrt(r^2 - L^2 / 3) and r.  A ray with impact
    parameter b meets radius R at tc - sqrt(R^2 - b^2) along its unit direction: the mesh is hit at most
    sqrt(r^2 - b^2) - sqrt(rho^2 - b^2) behind the sphere, never in front; in camera z that is divided by |(x, y, 1)|.

    Snapping.  Vertices move by at most 1/512 pixel per axis (plus the fp32 projection's few 2^-24 |u|, below 1e-4 pixel here): the
    drawn surface at a centre is the mesh's at a point within delta = sqrt(2) / 512 + 1e-4 pixel of it.  The analytic depth is convex in
    the pixel position, so over that distance it changes by at most delta times its largest difference G to the 8 neighbours; factor 2
    for the direction.  The sagitta term is taken as its largest over the same 3 x 3 neighbourhood.  Plus the fp32 band of rule 5.

    Excluded: pixels with a 3 x 3 neighbour that misses the sphere or has b > rho (within one pixel of the silhouette); the share is
    printed and capped at 10 %."""
    s, im = SPHERE, _sphere_images()
    H, W = s["size"]
    v, f = im["v"].astype(np.float64), im["f"]
    L = max(np.linalg.norm(v[f[:, i]] - v[f[:, (i + 1) % 3]], axis=1).max() for i in range(3))
    rho = np.sqrt(s["r"] ** 2 - L ** 2 / 3)
    PY, PX = np.meshgrid(np.arange(-1, H + 1, dtype=np.float64), np.arange(-1, W + 1, dtype=np.float64), indexing="ij")
    z, b, n, _ = _sphere_analytic(PX, PY)                                            # with a border of one pixel for the neighbourhoods
    with np.errstate(invalid="ignore"):
        sag = (np.sqrt(s["r"] ** 2 - b ** 2) - np.sqrt(rho ** 2 - b ** 2)) / n       # NaN where b > rho
    shifts = [(dy, dx) for dy in (0, 1, 2) for dx in (0, 1, 2)]
    nb = lambda a: np.stack([a[dy:dy + H, dx:dx + W] for dy, dx in shifts])          # noqa: E731  (9, H, W)
    zc = z[1:-1, 1:-1]
    core = np.isfinite(nb(sag)).all(0)
    hit = np.isfinite(zc)
    share = 1 - core.sum() / hit.sum()
    delta = np.sqrt(2) / 512 + 1e-4
    with np.errstate(invalid="ignore"):
        G = np.abs(nb(z) - zc).max(0)
        bound = nb(sag).max(0) + 2 * delta * G + DEPTH_BAND * zc
    depth = im["none"]["depth"][0].astype(np.float64)
    assert (im["none"]["face"][0][core] >= 0).all()                                  # every core pixel is hit
    err = depth[core] - zc[core]
    print(f"sphere: {hit.sum()} pixels on the sphere, {share:.1%} excluded near the silhouette; longest edge {L:.4f}, sagitta "
          f"{s['r'] - rho:.2e}; depth - analytic in [{err.min():.2e}, {err.max():.2e}], bound from {bound[core].min():.2e} to "
          f"{bound[core].max():.2e}")
    assert share <= 0.10
    assert (np.abs(err) <= bound[core]).all(), float((np.abs(err) / bound[core]).max())
    assert (err >= -(2 * delta * G + DEPTH_BAND * zc)[core]).all()                   # inscribed: never in front, but for snapping


def test_culling_a_closed_sphere_changes_nothing_and_follows_the_mirror():
    im = _sphere_images()
    for a, b in (("none", "back"), ("m_none", "m_back")):
        for k in ("face", "depth", "weights"):
            assert np.array_equal(im[a][k].view(np.uint32), im[b][k].view(np.uint32)), (a, b, k)
    hit = im["none"]["face"] >= 0
    assert hit.sum() > 10000
    # the opposite sign keeps the far hemisphere instead: same silhouette up to its rim, everything deeper
    far = im["front"]["face"] >= 0
    both = hit & far
    assert both.sum() > 0.95 * hit.sum() and (im["front"]["depth"][both] > im["none"]["depth"][both]).all()
    # the mirror image under the mirror matrix is the same camera-frame surface (its faces list their vertices in the opposite order)
    assert np.array_equal(im["m_none"]["face"], im["none"]["face"])
    assert np.abs(im["m_none"]["depth"] - im["none"]["depth"]).max() <= 1e-5
    # extract_mesh's convention: a face seen from outside under det > 0 has A < 0
    scr = im["none"]["screen"]
    f0 = im["none"]["face"][0][80, 80]
    xs, ys, _ = RR.snap(scr[im["f"][f0]], 1e-3)
    assert RR.area(xs, ys) < 0


# ------------------------------------------------------------------------------------ dropped faces
def test_dropped_faces():
    good = np.array([[2.0, 2.0], [12.0, 3.0], [5.0, 11.0]])
    base = RR.screen_mesh(good, 1.0)
    f = np.array([[0, 1, 2]], np.int32)
    draw = lambda v, **kw: RR.rasterize(v, f, [3], [1], RR.IDENTITY[None], RR.UNIT_CAM, 14, 16, **kw)       # noqa: E731
    assert (draw(base)["face"] >= 0).sum() > 30
    behind = base.copy()
    behind[1] *= np.float32(0.25)                                                    # the same pixel, depth 0.25
    assert (draw(behind, z_near=0.2)["face"] >= 0).sum() > 30
    assert (draw(behind, z_near=0.5)["face"] == -1).all()                            # one vertex nearer than z_near: the whole face goes
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            v = base.copy()
            v[2, col] = bad
            assert (draw(v)["face"] == -1).all(), (bad, col)
    far = base.copy()
    far[0, 0] = np.float32(2.0 ** 22)                                                # u = 2^22 exactly: dropped; just below: drawn
    assert (draw(far)["face"] == -1).all()
    far[0, 0] = np.nextafter(np.float32(2.0 ** 22), np.float32(0))
    assert (draw(far)["face"] >= 0).sum() > 0
    neg = base.copy()
    neg[0, 1] = np.float32(-2.0 ** 22)
    assert (draw(neg)["face"] == -1).all()
    out_of_range = RR.rasterize(base, np.array([[0, 1, 3]], np.int32), [3], [1], RR.IDENTITY[None], RR.UNIT_CAM, 14, 16)
    assert (out_of_range["face"] == -1).all()
    assert (out_of_range["depth"] == 0).all() and (out_of_range["weights"] == 0).all()


def test_images_per_object_and_instance_ids():
    a, fa = RR.fan((6.0, 6.0), 4.0, 5)
    va, vb = RR.screen_mesh(a, 2.0), RR.screen_mesh(a + 2.0, 1.0)
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fa])
    nv, nf = [len(va), 0, len(vb)], [len(fa), 0, len(fa)]                            # an empty object in the middle
    mats = np.repeat(RR.IDENTITY[None], 3, 0)
    one = RR.rasterize(v, f, nv, nf, mats, RR.UNIT_CAM, 14, 14)
    per = RR.rasterize(v, f, nv, nf, mats, RR.UNIT_CAM, 14, 14, image_of=[0, 1, 2], n_images=3)
    assert set(np.unique(one["obj"])) == {-1, 0, 2} and (per["face"][1] == -1).all()
    assert set(np.unique(per["obj"][0])) == {-1, 0} and set(np.unique(per["obj"][2])) == {-1, 2}
    overlap = (per["face"][0] >= 0) & (per["face"][2] >= 0)
    assert overlap.sum() > 10 and (one["obj"][0][overlap] == 2).all()                # the nearer object wins the scene image
    assert np.array_equal(one["face"][0][overlap], per["face"][2][overlap])


# ------------------------------------------------------------------------------------ the host side
def test_abi_and_symbols():
    from supnerf_amd import _lib
    assert _lib.header_abi_version() >= 15
    assert all(n in _lib.exported_symbols() for n in RASTER_SYMBOLS)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in RASTER_SYMBOLS)
    # argument checks that need no device: they return before anything is launched
    assert lib.snr_raster_faces(None, None, None, None, None, None, 1, 3, 1, 1, 4, 4, 0.0, None, None) == -1        # z_near <= 0
    assert lib.snr_raster_faces(None, None, None, None, None, None, 1, 3, 1, 1, 4, 4, 0.5, None, None) == -1        # null pointers
    assert lib.snr_raster_faces(None, None, None, None, None, None, 1, 3, 1, 2, 1 << 15, 1 << 15, 0.5, None, None) == -5
    assert lib.snr_raster_faces(None, None, None, None, None, None, 1, 3, 1 << 31, 1, 4, 4, 0.5, None, None) == -5
    assert lib.snr_raster_faces(None, None, None, None, None, None, 1, 3, 1, 1, -4, 4, 0.5, None, None) == -1
    assert lib.snr_raster_resolve(None, None, None, None, None, 1, 3, 1, 1, 1 << 16, 1 << 15, None, None, None, None) == -5
    for C in (0, 17):
        assert lib.snr_raster_interpolate(None, None, None, None, None, 1, 3, 1, None, C, 16, 0.0, None, None) == -1
    assert lib.snr_raster_interpolate(None, None, None, None, None, 1, 3, 1, None, 3, 16, 0.0, None, None) == -1
    assert lib.snr_raster_project(None, None, 1, 3, None, 1.0, 1.0, 0.0, 0.0, None, None) == -1


def test_cpu_tensors_raise(amd):  # noqa: F811
    from supnerf_amd import geometry as G
    v, f = RR.sphere(4, 6)
    mesh = (torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(amd.SnrError):
        G.rasterize(mesh, torch.from_numpy(RR.IDENTITY), (10.0, 10.0, 4.0, 4.0), (8, 8))
    with pytest.raises(amd.SnrError):
        G.mesh_view(mesh, torch.eye(4)[:3], 1.0, torch.eye(3), [0, 0, 8, 8])
    with pytest.raises(amd.SnrError):
        G.scene_view([mesh], torch.eye(4)[None, :3], [1.0], torch.eye(3), 8, 8)
    assert G.Raster._fields == ("face", "obj", "depth", "weights", "mesh")
