"""The mesh rasteriser on the MI355X: ``geometry.rasterize`` / ``interpolate`` (the ``snr_raster_*`` kernels) against
tests/raster_restatement.py -- face, depth, weights and interpolated attributes bit for bit, two runs bit for bit, dtypes and shapes -- on
hand-made meshes, an image wider than a wave with faces on both sides of the whole-wave threshold, the planted ball and the fog mesh
through ``extract_mesh``, several objects with an empty one; ``mesh_view`` against the rays of ``utils.get_rays`` (the camera convention end
to end) and against hand-composed matrices; ``scene_view``; argument errors."""
import numpy as np
import pytest
import torch

import mesh_restatement as MR
import raster_restatement as RR
from geometry_cases import codes as _codes, model as _model
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _np(t):
    return t.detach().cpu().numpy()


def _gpu_mesh(mesh, dev):  # noqa: F811
    v, f = mesh
    if torch.is_tensor(v):
        return v, f
    return (torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(G, dev, meshes, mats, cam, size, tag, cull=None, per_object=False, z_near=1e-3, channels=(1, 3, 16)):  # noqa: F811
    """``geometry.rasterize`` and ``interpolate`` on ``meshes`` (numpy or GPU pairs) against the restatement; returns (Raster, restated)."""
    ms = [_gpu_mesh(m, dev) for m in meshes]
    B, (H, W) = len(ms), size
    mats = np.asarray(mats, np.float32).reshape(B, 3, 4)
    r = G.rasterize(ms, torch.from_numpy(mats).to(dev), cam, size, cull=cull, z_near=z_near, per_object=per_object)
    again = G.rasterize(ms, torch.from_numpy(mats).to(dev), cam, size, cull=cull, z_near=z_near, per_object=per_object)
    nv, nf = [m[0].shape[0] for m in ms], [m[1].shape[0] for m in ms]
    verts = np.concatenate([_np(m[0]) for m in ms])
    faces = np.concatenate([_np(m[1]) for m in ms])
    sign = np.sign(np.linalg.det(mats[:, :, :3].astype(np.float64))).astype(np.int64) if cull == "back" else None
    n_images = B if per_object else 1
    ref = RR.rasterize(verts, faces, nv, nf, mats, cam, H, W, z_near=z_near, image_of=np.arange(B) if per_object else None,
                       n_images=n_images, cull_sign=sign)
    want = {"face": torch.int32, "obj": torch.int32, "depth": torch.float32, "weights": torch.float32}
    for name, dt in want.items():
        g = getattr(r, name)
        assert g.dtype == dt and tuple(g.shape) == ref[name].shape and g.is_contiguous(), (tag, name, g.dtype, tuple(g.shape))
        assert not g.requires_grad
        assert np.array_equal(_bits(_np(g)), _bits(ref[name])), (tag, name, int((_bits(_np(g)) != _bits(ref[name])).sum()))
        assert torch.equal(g, getattr(again, name)), (tag, name, "run to run")
    assert tuple(r.face.shape) == (n_images, H, W) and tuple(r.weights.shape) == (n_images, H, W, 3)
    rng = np.random.default_rng(7)
    for C in channels:
        att = rng.standard_normal((verts.shape[0], C)).astype(np.float32)
        packed = torch.from_numpy(att).to(dev)
        out = G.interpolate(r, packed, background=-2.5)
        assert out.dtype == torch.float32 and tuple(out.shape) == (n_images, H, W, C)
        assert np.array_equal(_bits(_np(out)), _bits(RR.interpolate(ref["face"], ref["weights"], faces, nv, nf, att, -2.5))), (tag, C)
        per = G.interpolate(r, list(torch.split(packed, nv)), background=-2.5)       # the per-object list is the same thing
        assert torch.equal(per, out) and torch.equal(G.interpolate(r, packed, background=-2.5), out)
    print(f"{tag}: {sum(nf)} faces, {int((ref['face'] >= 0).sum())} of {n_images * H * W} pixels covered, "
          f"{len(np.unique(ref['face'])) - 1} faces visible")
    return r, ref


def _px(points, faces, depth=1.0):
    return RR.screen_mesh(points, depth), np.asarray(faces, np.int32)


# ------------------------------------------------------------------------------------ hand-made meshes, 23 x 17
def test_hand_made_cases(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    size = (17, 23)
    for cw in (False, True):
        _check(G, dev, [_px(*RR.fan(clockwise=cw))], RR.IDENTITY, RR.UNIT_CAM, size, f"fan cw={cw}")
        r, ref = _check(G, dev, [_px(*RR.lattice_sheet(clockwise=cw))], RR.IDENTITY, RR.UNIT_CAM, size, f"lattice sheet cw={cw}")
        assert (ref["face"] >= 0).sum() > 150
    tri = np.array([[1.0, 1.0], [14.0, 2.0], [6.0, 12.0]])
    r, _ = _check(G, dev, [_px(tri, [[0, 1, 2]] * 3, np.array([1.0, 2.0, 4.0]))], RR.IDENTITY, RR.UNIT_CAM, size, "coplanar duplicates")
    assert set(_np(r.face).ravel().tolist()) == {-1, 0}
    quad = np.array([[0.5, 0.5], [20.5, 0.5], [0.5, 15.5], [20.5, 15.5]])
    v = np.concatenate([RR.screen_mesh(quad, np.array([1.0, 3.0, 1.0, 3.0])), RR.screen_mesh(quad, np.array([3.0, 1.0, 3.0, 1.0]))])
    r, _ = _check(G, dev, [(v, np.array([[0, 1, 2], [1, 3, 2], [4, 5, 6], [5, 7, 6]], np.int32))], RR.IDENTITY, RR.UNIT_CAM, size,
                  "interpenetrating sheets")
    assert set(_np(r.face).ravel().tolist()) == {-1, 0, 1, 2, 3}
    # dropped faces beside one that is drawn: behind z_near, NaN, infinite, 2^22 pixels away, an index outside the object
    base = RR.screen_mesh(tri, 1.0)
    bad = [base.copy() for _ in range(5)]
    bad[0][1] *= np.float32(0.25)
    bad[1][2, 0] = np.nan
    bad[2][0, 2] = np.inf
    bad[3][0, 0] = np.float32(2.0 ** 22)
    bad[4][0, 1] = np.float32(-2.0 ** 22)
    v = np.concatenate(bad + [RR.screen_mesh(tri + 3.0, 2.0)])
    f = np.array([[3 * k, 3 * k + 1, 3 * k + 2] for k in range(6)] + [[0, 1, 18], [-1, 1, 2]], np.int32)
    r, ref = _check(G, dev, [(v, f)], RR.IDENTITY, RR.UNIT_CAM, size, "dropped faces", z_near=0.5)
    assert set(_np(r.face).ravel().tolist()) == {-1, 5}
    r, _ = _check(G, dev, [(v, f)], RR.IDENTITY, RR.UNIT_CAM, size, "dropped faces, near plane closer", z_near=0.125)
    assert set(_np(r.face).ravel().tolist()) == {-1, 0, 5}


# ------------------------------------------------------------------------------------ wider than a wave: both sides of the threshold
def _box_triangle(x0, y0, w, h):
    """A triangle whose candidate box is exactly w x h pixels at (x0, y0)."""
    return [[x0 - 0.25, y0 - 0.25], [x0 + w - 0.75, y0 - 0.25], [x0 - 0.25, y0 + h - 0.75]]


BOXES = ((15, (5, 3)), (16, (4, 4)), (17, (17, 1)), (31, (31, 1)), (32, (8, 4)), (33, (11, 3)), (63, (9, 7)), (64, (8, 8)),
         (65, (13, 5)), (127, (127, 1)), (128, (16, 8)), (129, (43, 3)), (255, (17, 15)), (256, (16, 16)), (260, (20, 13)))


def mixed_scene():
    """(verts, faces, index of the first special face, how many special faces) of ``test_large_and_small_boxes_in_one_launch``."""
    pts, faces, depth = [], [], []

    def add(tri, z):
        faces.append([len(pts), len(pts) + 1, len(pts) + 2])
        pts.extend(tri)
        depth.extend(np.broadcast_to(z, 3))
    sheet_p, sheet_f = RR.lattice_sheet(40, 20, 2.25, (20.25, 10.5), seed=9)
    first = len(sheet_f) // 2
    for k, f in enumerate(sheet_f):                                                  # small faces before and after the special ones
        if k == first:
            add([[-20.0, -30.0], [400.0, -10.0], [-30.0, 200.0]], [4.0, 6.0, 5.0])                    # covers the whole image
            add([[-5000.25, -3000.5], [6000.0, 10.0], [-100.0, 4000.75]], [2.0, 32.0, 16.0])         # thousands of pixels off-screen
            add([[-10.5, 20.0], [8.0, 25.5], [-4.0, 40.0]], 1.0)                                     # across the left border
            add([[120.0, 30.0], [140.5, 35.0], [125.0, 50.5]], 1.0)                                  # right
            add([[50.0, -8.0], [70.0, -6.0], [60.5, 6.0]], 1.0)                                      # top
            add([[50.0, 64.0], [75.0, 80.0], [55.5, 90.0]], 1.0)                                     # bottom
            for j, (n, (w, h)) in enumerate(BOXES):
                assert w * h == n
                add(_box_triangle(1 + n % 3, 1 + 3 * j, w, h), 0.5 + n / 512)
        add(sheet_p[f].tolist(), 1.5)
    return RR.screen_mesh(np.array(pts), np.array(depth)), np.array(faces, np.int32), first, 6 + len(BOXES)


def test_large_and_small_boxes_in_one_launch(amd, dev):  # noqa: F811
    """A 130 x 70 image (wider than a wave, no multiple of 64): a triangle covering all of it, one with vertices thousands of pixels
    off-screen, one across each border, and boxes of 15 .. 260 candidates -- one below, at and above every power of two a whole-wave
    threshold could be (the kernel's is 64; 257 is prime, so 260) -- between the small faces of a lattice sheet, all in one launch."""
    from supnerf_amd import geometry as G
    v, f, first, n_special = mixed_scene()
    r, ref = _check(G, dev, [(v, f)], RR.IDENTITY, RR.UNIT_CAM, (70, 130), "130 x 70, mixed boxes")
    assert (ref["face"] >= 0).all()                                                  # the two big triangles are behind everything
    seen = set(np.unique(ref["face"]).tolist())
    assert all(first + k in seen for k in range(n_special))                          # every special face wins somewhere
    # the candidate boxes are the sizes they are meant to be
    for j, (n, _) in enumerate(BOXES):
        xs, ys, _ = RR.snap(ref["screen"][f[first + 6 + j]], 1e-3)
        x0, x1, y0, y1 = RR.box(xs, ys, 70, 130)
        assert (x1 - x0 + 1) * (y1 - y0 + 1) == n


# ------------------------------------------------------------------------------------ extracted meshes
BALL_CAM = (100.0, 100.0, 31.5, 23.5)


def _shift(z, x=0.0, y=0.0):
    m = RR.IDENTITY.copy()
    m[:, 3] = (x, y, z)
    return m


@pytest.fixture(scope="module")
def ball(amd, dev):  # noqa: F811
    """The planted ball of radius 0.2 at R = 24 through ``extract_mesh``, beside an all-outside grid (an empty mesh): B = 3."""
    from supnerf_amd import geometry as G
    field = MR.ball_field(24)[0]
    grid = torch.from_numpy(np.stack([field, np.full_like(field, -1.0), field])).to(dev)
    return G.extract_mesh(grid, level=0.0)


def test_planted_ball(amd, dev, ball):  # noqa: F811
    from supnerf_amd import geometry as G
    assert 1000 < ball[0][1].shape[0] < 10000 and ball[1][1].shape[0] == 0
    imgs = {}
    for cull in (None, "back"):
        imgs[cull], ref = _check(G, dev, ball[:1], _shift(1.0), BALL_CAM, (48, 64), f"ball R=24 cull={cull}", cull=cull)
        assert 1000 < (ref["face"] >= 0).sum() < 1500                                # a disc of radius 20 pixels
    for a, b in zip(imgs[None][:4], imgs["back"][:4]):                               # a closed outward-wound surface: culling changes nothing
        assert torch.equal(a, b)
    mirror = _shift(1.0)
    mirror[0, 0] = -1.0
    _check(G, dev, ball[:1], mirror, BALL_CAM, (48, 64), "ball under a mirror", cull="back")
    one = G.rasterize(ball[0], torch.from_numpy(_shift(1.0)).to(dev), BALL_CAM, (48, 64))          # one pair, a (3, 4) matrix
    assert all(torch.equal(a, b) for a, b in zip(one[:4], imgs[None][:4]))


def test_several_objects_with_an_empty_one(amd, dev, ball):  # noqa: F811
    from supnerf_amd import geometry as G
    mats = [_shift(1.0, -0.08), _shift(1.0), _shift(0.8, 0.08, 0.03)]
    r, ref = _check(G, dev, ball, mats, BALL_CAM, (48, 64), "B=3, one scene image", cull="back")
    assert set(np.unique(ref["obj"]).tolist()) == {-1, 0, 2}
    r, ref = _check(G, dev, ball, mats, BALL_CAM, (48, 64), "B=3, one image each", cull="back", per_object=True, channels=(3,))
    assert (ref["face"][1] == -1).all() and (ref["obj"][0].max(), ref["obj"][2].max()) == (0, 2)


def test_fog_mesh(amd, dev):  # noqa: F811
    """Many overlapping tiny faces: dozens of faces contend for every pixel's atomic min."""
    from supnerf_amd import geometry as G
    model = _model(amd, dev, 3, 1, seed=0)
    grid = G.density_grid(model, _codes(2, 5, dev), 24)
    meshes = G.extract_mesh(grid, level=float(grid.median()))
    assert min(m[1].shape[0] for m in meshes) > 2000
    mats = [_shift(1.6, -0.1), _shift(1.5, 0.1, 0.05)]
    for per_object in (False, True):
        _check(G, dev, meshes, mats, (60.0, 60.0, 31.5, 23.5), (48, 64), f"fog R=24 B=2 per_object={per_object}", per_object=per_object,
               channels=(3,))


# ------------------------------------------------------------------------------------ the camera convention, end to end
def _look_at(eye, up=(0.0, 0.0, 1.0)):
    """(3, 4) float32 camera pose in the object's frame: at ``eye``, looking at the origin; columns x right, y down, z forward."""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(np.float32)


def _view_matrices(pose, scale, K, roi, im_sz):
    """What ``mesh_view`` composes, by hand in float64: (M (3, 4) float32, (fx, fy, cx, cy), (ny, nx))."""
    P = pose.astype(np.float64)
    r_inv = np.linalg.inv(P[:, :3])
    M = np.concatenate([r_inv * scale, -(r_inv @ P[:, 3:4])], 1)
    x0, y0, x1, y1 = roi
    nx, ny = (im_sz, im_sz) if im_sz else (x1 - x0, y1 - y0)
    sx, sy = (x1 - 1 - x0) / (nx - 1), (y1 - 1 - y0) / (ny - 1)
    return M.astype(np.float32), (K[0, 0] / sx, K[1, 1] / sy, (K[0, 2] - x0) / sx, (K[1, 2] - y0) / sy), (ny, nx)


VIEW_K = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1]])
VIEW_ROI = [118, 82, 202, 158]
VIEW_DIAG = 1.5


@pytest.mark.parametrize("im_sz", [None, 40])
def test_mesh_view_lies_on_the_rays_of_get_rays(amd, dev, ball, im_sz):  # noqa: F811
    """The point rays_o + depth viewdir of ``utils.get_rays`` at the same pixel lies on the winning face.

    Reference: the float64 plane through the winning face's SNAPPED vertices (xs / 256, ys / 256, z_i), un-projected with the effective
    camera and moved to the object's frame with ``cam_pose``; depth_ref = n . (a - o) / (n . d) along the ray (o, d) of ``get_rays``.
    Band, relative to the depth: rule 5's 7 roundings, the length factor (its cast to fp32 and the product: 2), |d| = 1 within 2 e:
    11 e, taken as 12; the direction of ``get_rays`` (fp32 camera table, rotation, normalisation: each component within about 4 e, and
    the fp32 ``linspace`` of the pixel grid) moves the point sideways by up to 8 e depth, which changes the depth along the ray by that
    over |n . d|.  So |depth - depth_ref| <= depth e (12 + 8 / |n . d|), for faces with |n . d| >= 0.2.  Inside the face: the point's
    signed distance to every edge line, in the plane, is at least -8 e depth."""
    from supnerf_amd import geometry as G, utils as U
    pose = _look_at((2.1, -1.3, 0.9))
    K = torch.from_numpy(VIEW_K).float()
    cam_pose = torch.from_numpy(pose).to(dev)
    mesh = ball[0]
    view = G.mesh_view(mesh, cam_pose, VIEW_DIAG, K, VIEW_ROI, im_sz=im_sz, cull="back")
    M, cam, (ny, nx) = _view_matrices(pose, VIEW_DIAG, VIEW_K, VIEW_ROI, im_sz)
    assert tuple(view.depth.shape) == (ny, nx) and view.mask.dtype == torch.bool and view.face.dtype == torch.int32
    assert view.normal is None and view.color is None and not view.depth.requires_grad
    # the same image from rasterize with the hand-composed matrix, bit for bit
    r = G.rasterize(mesh, torch.from_numpy(M).to(dev), cam, (ny, nx), cull="back")
    assert torch.equal(r.face[0], view.face) and torch.equal(r.face[0] >= 0, view.mask)
    px, py = (np.arange(nx) - cam[2]) / cam[0], (np.arange(ny) - cam[3]) / cam[1]
    length = np.sqrt(px[None, :] ** 2 + py[:, None] ** 2 + 1.0).astype(np.float32)
    assert np.array_equal(_bits(_np(view.depth)), _bits(_np(r.depth[0]) * length))
    # the rays of get_rays, float64 from here on
    steps = None if im_sz is None else [im_sz, im_sz]
    rays_o, viewdir = U.get_rays(K, cam_pose, VIEW_ROI, uv_steps=steps)
    o, d = _np(rays_o).astype(np.float64).reshape(ny, nx, 3), _np(viewdir).astype(np.float64).reshape(ny, nx, 3)
    face, depth = _np(view.face), _np(view.depth).astype(np.float64)
    v, f = _np(mesh[0]), _np(mesh[1])
    screen = RR.project(v, [v.shape[0]], M[None], cam)
    hit = face >= 0
    assert 1500 < hit.sum() if im_sz is None else 300 < hit.sum()
    tri = screen[f[face[hit]]]                                                       # (n, 3, 3) screen vertices of each pixel's winner
    xs, ys, _, keep = RR.snap_all(tri, 1e-3)
    assert keep.all()
    z = tri[..., 2].astype(np.float64)
    cam_pts = np.stack([(xs / 256.0 - cam[2]) / cam[0] * z, (ys / 256.0 - cam[3]) / cam[1] * z, z], -1)        # (n, 3, 3) camera frame
    P = pose.astype(np.float64)
    obj_pts = cam_pts @ P[:, :3].T + P[:, 3]
    a, e1, e2 = obj_pts[:, 0], obj_pts[:, 1] - obj_pts[:, 0], obj_pts[:, 2] - obj_pts[:, 0]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    oh, dh, depth_h = o[hit], d[hit], depth[hit]
    nd = np.einsum("ij,ij->i", n, dh)
    steep = np.abs(nd) >= 0.2
    assert steep.mean() > 0.8
    ref = np.einsum("ij,ij->i", n, a - oh) / nd
    err = np.abs(depth_h - ref)[steep]
    band = (depth_h * EPS * (12 + 8 / np.abs(nd)))[steep]
    print(f"mesh_view im_sz={im_sz}: {hit.sum()} pixels, {steep.sum()} with |n.d| >= 0.2; worst |depth - plane| / band {np.max(err / band):.3f}, "
          f"depth {depth_h.min():.3f} .. {depth_h.max():.3f} m")
    assert (err <= band).all()
    # inside the face: signed distance of the point to each edge line, within the plane
    p = oh + depth_h[:, None] * dh
    worst = np.inf
    for i in range(3):
        va, vb, vc = obj_pts[:, (i + 1) % 3], obj_pts[:, (i + 2) % 3], obj_pts[:, i]
        edge = vb - va
        inward = np.cross(n, edge)
        inward *= np.sign(np.einsum("ij,ij->i", inward, vc - va))[:, None] / np.linalg.norm(inward, axis=1, keepdims=True)
        dist = np.einsum("ij,ij->i", p - va, inward)
        worst = min(worst, float((dist / depth_h)[steep].min()))
        assert (dist[steep] >= -8 * EPS * depth_h[steep]).all(), i
    print(f"  smallest signed distance to an edge / depth: {worst:.3e} (allowed {-8 * EPS:.3e})")
    # and the depth is the one surface_depth speaks of: the ball of radius 0.2 VIEW_DIAG around the origin, seen from |eye| away
    centre = depth[ny // 2, nx // 2]
    assert abs(centre - (np.linalg.norm(pose[:, 3]) - 0.2 * VIEW_DIAG)) < 0.02 * VIEW_DIAG


def test_mesh_view_attributes(amd, dev, ball):  # noqa: F811
    from supnerf_amd import geometry as G, utils as U
    pose = _look_at((2.1, -1.3, 0.9))
    K, cam_pose = torch.from_numpy(VIEW_K).float(), torch.from_numpy(pose).to(dev)
    v, f = ball[0]
    normals = torch.nn.functional.normalize(v, dim=1)                                # a ball about the origin: radial
    colors = (v * 2.0 + 0.5).contiguous()
    view = G.mesh_view((v, f), cam_pose, VIEW_DIAG, K, VIEW_ROI, normals=normals, colors=colors, shapenet_obj_cood=True)
    plain = G.mesh_view([(v, f)], cam_pose, VIEW_DIAG, K, VIEW_ROI, shapenet_obj_cood=True)
    assert torch.equal(view.depth, plain.depth) and tuple(view.normal.shape) == tuple(view.color.shape) == tuple(view.depth.shape) + (3,)
    m = view.mask
    assert (view.normal[~m] == 0).all() and (view.color[~m] == 0).all()
    assert float((view.normal[m].norm(dim=1) - 1).abs().max()) < 1e-5
    # the hit point in the object's frame, from the rays; the normal there is radial up to the tessellation
    rays_o, viewdir = U.get_rays(K, cam_pose, VIEW_ROI)
    p = (rays_o + view.depth.reshape(-1, 1) * viewdir).view(*view.depth.shape, 3)
    radial = torch.nn.functional.normalize(p, dim=-1)
    assert float((view.normal[m] * radial[m]).sum(1).min()) > 0.98
    # colours are affine in the decoder-frame position: the interpolated colour is the colour of the hit point
    back = G.to_decoder_frame(p, VIEW_DIAG, shapenet_obj_cood=True) * 2.0 + 0.5
    assert float((view.color[m] - back[m]).abs().max()) < 1e-4


def test_scene_view(amd, dev, ball):  # noqa: F811
    from supnerf_amd import geometry as G
    H, W = 60, 80
    K = np.array([[80.0, 0, 39.5], [0, 80.0, 29.5], [0, 0, 1]])
    poses = np.stack([_shift(6.0, -0.3), _shift(4.0, 0.3, 0.1)])                     # object -> camera: the second is nearer
    diags = [4.0, 3.0]
    meshes = [ball[0], ball[2]]
    normals = [torch.nn.functional.normalize(m[0], dim=1) for m in meshes]
    s = G.scene_view(meshes, torch.from_numpy(poses).to(dev), diags, torch.from_numpy(K), H, W, normals=normals)
    mats = poses.astype(np.float64).copy()
    mats[:, :, :3] *= np.array(diags)[:, None, None]
    nv, nf = [m[0].shape[0] for m in meshes], [m[1].shape[0] for m in meshes]
    ref = RR.rasterize(np.concatenate([_np(m[0]) for m in meshes]), np.concatenate([_np(m[1]) for m in meshes]), nv, nf,
                       mats.astype(np.float32), (80.0, 80.0, 39.5, 29.5), H, W, cull_sign=[1, 1])
    assert s.obj.dtype == torch.int32 and tuple(s.obj.shape) == (H, W)
    assert np.array_equal(_np(s.obj), ref["obj"][0]) and np.array_equal(_np(s.face), ref["face"][0])
    assert np.array_equal(_bits(_np(s.depth)), _bits(ref["depth"][0]))
    alone = [G.scene_view(meshes[b:b + 1], torch.from_numpy(poses[b:b + 1]).to(dev), diags[b:b + 1], K, H, W) for b in range(2)]
    overlap = (alone[0].obj >= 0) & (alone[1].obj >= 0)
    assert int(overlap.sum()) > 100 and (s.obj[overlap] == 1).all()                  # the nearer object wins where they overlap
    assert (s.depth[overlap] == alone[1].depth[overlap]).all()
    assert set(_np(s.obj).ravel().tolist()) == {-1, 0, 1}
    hit = s.obj >= 0
    assert float((s.normal[hit].norm(dim=1) - 1).abs().max()) < 1e-5 and float(s.normal[hit][:, 2].mean()) < -0.5        # they face the camera


def test_argument_errors(amd, dev, ball):  # noqa: F811
    from supnerf_amd import geometry as G, ops
    mesh, m, cam = ball[0], torch.from_numpy(_shift(1.0)).to(dev), BALL_CAM
    for kw in (dict(cull="front"), dict(z_near=0.0), dict(z_near=-1.0)):
        with pytest.raises(amd.SnrError):
            G.rasterize(mesh, m, cam, (8, 8), **kw)
    for bad in (dict(size=(0, 8)), dict(obj_to_cam=m[:2]), dict(obj_to_cam=torch.stack([m, m])), dict(K=torch.eye(2)),
                dict(meshes=(mesh[0], mesh[1].long())), dict(size=(1 << 16, 1 << 15))):
        args = dict(meshes=mesh, obj_to_cam=m, K=cam, size=(8, 8))
        args.update(bad)
        with pytest.raises(amd.SnrError):
            G.rasterize(args["meshes"], args["obj_to_cam"], args["K"], args["size"])
    r = G.rasterize(mesh, m, cam, (8, 8))
    V = mesh[0].shape[0]
    for att in (torch.zeros(V, 17, device=dev), torch.zeros(V, 0, device=dev), torch.zeros(V + 1, 3, device=dev), torch.zeros(V, 3),
                [torch.zeros(V, 3, device=dev)] * 2):
        with pytest.raises(amd.SnrError):
            G.interpolate(r, att)
    with pytest.raises(amd.SnrError):                                                # straight at the C ABI: z_near <= 0
        ops.raster_faces(r.mesh, torch.zeros(V, 3, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), 1, 8, 8, 0.0)
    with pytest.raises(amd.SnrError):
        G.scene_view([mesh], torch.from_numpy(_shift(1.0)[None]).to(dev), [1.0, 2.0], cam, 8, 8)
    with pytest.raises(amd.SnrError):
        G.mesh_view(mesh, torch.eye(3, device=dev), 1.0, torch.eye(3), [0, 0, 8, 8])
