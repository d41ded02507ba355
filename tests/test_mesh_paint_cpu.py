"""Mesh painting on the host: the rules of include/supnerf_hip.h ("Mesh painting") as tests/paint_restatement.py restates them, held against
results that can be worked out by hand -- an affine image (where bilinear sampling is exact), a tessellated box seen from the front and
from the back, an occluder, a mask, a strip filled from one end -- with planted mistakes that the same checks reject; and the parts of
the API that need no GPU (symbols, the argument checks of the C ABI and of the Python layer).

Depth buffers and screen positions come from tests/raster_restatement.py, so the whole chain is numpy."""
import inspect

import numpy as np
import pytest
import torch

import paint_restatement as PR
import raster_restatement as RR
import smooth_restatement as MS
from segment_sum_restatement import same_bits

F32 = np.float32
EPS = 2.0 ** -24
QUAD = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _quad(x0, y0, x1, y1, z):
    """Four vertices that ``RR.UNIT_CAM`` projects exactly to the corners of a pixel rectangle at camera depth z (a power of two)."""
    return RR.screen_mesh([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], z)


def _view(verts, faces, H, W, image, mask=None, tol=0.0, mats=RR.IDENTITY[None], cam=RR.UNIT_CAM, centre=(0.0, 0.0, 0.0), cull_sign=None):
    r = RR.rasterize(verts, faces, [len(verts)], [len(faces)], mats, cam, H, W, cull_sign=cull_sign)
    return dict(screen=r["screen"], depth=r["depth"][0], image=np.ascontiguousarray(image, F32), mask=mask, centre=centre, tol=tol)


# ------------------------------------------------------------------ the affine image
ALPHA, BETA, GAMMA = (0.5, 0.25, 1.0), (0.125, -0.25, 0.0625), (0.0625, 0.5, -0.125)


def _affine(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.stack([a + b * x + g * y for a, b, g in zip(ALPHA, BETA, GAMMA)], axis=-1)


def _affine_case():
    """A quad at depth 2 that covers a 9 x 7 image and more, and loose vertices on its plane: on a pixel centre, between centres, on the
    first and last column and row exactly, and one ulp outside either."""
    H, W = 7, 9
    up, down = np.nextafter(F32(8), F32(9)), np.nextafter(F32(0), F32(-1))
    pts = [(3, 2), (3.25, 2.5), (0.5, 5.75), (7.875, 0.125), (8, 3.5), (up, 3.5), (0, 0), (down, 1), (4.5, 6), (4.5, np.nextafter(F32(6), F32(7))),
           (2.0, 6.0), (7.5, 5.5), (8, 6)]
    verts = np.concatenate([_quad(-2, -2, 12, 10, 2.0), RR.screen_mesh(np.array(pts, np.float64), 2.0)])
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    image = _affine(xx, yy).astype(F32)                       # (dyadic coefficients, small integers: exact in fp32)
    assert np.array_equal(image.astype(np.float64), _affine(xx, yy))
    inside = np.array([True] * 5 + [False, True, False, True, False, True, True, True])
    return verts, np.array(pts, np.float64), image, inside, (H, W)


def _affine_failures(planted=None):
    """The checks of the affine case; a list of the ones that fail.

    The bound.  a and b are exact (u - x0 with 0 <= u - x0 <= 1 is exact in fp32).  1 - a rounds once (e = 2^-24 relative), so a weight,
    two such factors and one product, carries at most 3 e; a term w_t I_t 4 e; the numerator adds four terms with three additions,
    each of which adds at most e to what is summed so far: 7 e sum_t w_t |I_t| <= 7 e max|I| (the exact weights add up to 1).  s carries
    3 e per weight and 3 e of additions: 6 e.  The division adds e.  To first order |c - exact| <= (7 + 6 + 1) e max|I|; 16 e max|I|
    covers the second-order terms."""
    verts, pts, image, inside, (H, W) = _affine_case()
    view = _view(verts, QUAD, H, W, image)
    state = PR.new_state(len(verts))
    got = PR.paint_view(view["screen"], verts, None, view["image"], None, view["depth"], (0, 0, 0), 0.0, 1e-3, 0, state, planted)
    loose = slice(4, None)
    failed = []
    if not np.array_equal(view["screen"][loose, :2].astype(np.float64), pts):
        failed.append("the case itself: projection is not exact")
    if not np.array_equal(got["sees"][loose], inside):
        failed.append("footprint")
    want = _affine(pts[:, 0], pts[:, 1])[inside]
    seen64, c64 = PR.colour64(view["screen"], image, None, view["depth"], 0.0)
    if not (np.array_equal(seen64[loose], inside) and np.abs(c64[loose][inside] - want).max() < 1e-12):
        failed.append("the float64 evaluator")
    both = got["sees"][loose] & inside
    err = np.abs(got["c"][loose][both].astype(np.float64) - _affine(pts[:, 0], pts[:, 1])[both])
    if err.size == 0 or err.max() > 16 * EPS * np.abs(image).max():
        failed.append("colour")
    colors, filled = PR.finish(state, "weighted")
    if not (np.array_equal(filled[loose] == 0, got["sees"][loose]) and same_bits(colors[got["sees"]], got["c"][got["sees"]]).all()):
        failed.append("finish")                              # (one view without normals: sum = 1 c, weight 1, c / 1 = c)
    return failed


def test_affine_image_is_reproduced():
    assert _affine_failures() == []


def test_exact_corner_values():
    """On a pixel centre the colour is the pixel, bit for bit; on the last column u = W - 1, x0 = W - 2 and a = 1."""
    verts, pts, image, inside, (H, W) = _affine_case()
    fp = PR.footprint(RR.project(verts, [len(verts)], RR.IDENTITY[None], RR.UNIT_CAM), H, W, 1e-3)
    assert fp["tap"][4].tolist() == [2 * W + 3, 2 * W + 4, 3 * W + 3, 3 * W + 4] and fp["weight"][4].tolist() == [1, 0, 0, 0]
    assert fp["tap"][8].tolist() == [3 * W + 7, 3 * W + 8, 4 * W + 7, 4 * W + 8] and fp["weight"][8].tolist() == [0, 0.5, 0, 0.5]
    assert fp["tap"][16].tolist() == [5 * W + 7, 5 * W + 8, 6 * W + 7, 6 * W + 8] and fp["weight"][16].tolist() == [0, 0, 0, 1]
    assert (fp["tap"][9] == -1).all() and (fp["tap"][11] == -1).all() and not fp["inside"][13]
    view = _view(verts, QUAD, H, W, image)
    got = PR.paint_view(view["screen"], verts, None, image, None, view["depth"], (0, 0, 0), 0.0, 1e-3, 0, PR.new_state(len(verts)))
    assert same_bits(got["c"][4], image[2, 3]).all() and same_bits(got["c"][16], image[6, 8]).all() and same_bits(got["c"][10], image[0, 0]).all()


def test_images_of_one_row_or_column():
    """W = 1 or H = 1: the taps that would repeat their neighbour are not taps."""
    for H, W in ((1, 1), (1, 7), (5, 1)):
        pts = np.array([(0, 0), (W - 1, H - 1), ((W - 1) / 2 + 0.25 * (W > 1), (H - 1) / 2 + 0.25 * (H > 1))], np.float64)
        verts = np.concatenate([_quad(-2, -2, 12, 10, 2.0), RR.screen_mesh(pts, 2.0)])
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        image = _affine(xx, yy).astype(F32)
        view = _view(verts, QUAD, H, W, image)
        fp = PR.footprint(view["screen"], H, W, 1e-3)
        assert (fp["tap"][:, 1] == -1).all() == (W == 1) and (fp["tap"][:, 2] == -1).all() == (H == 1)
        got = PR.paint_view(view["screen"], verts, None, image, None, view["depth"], (0, 0, 0), 0.0, 1e-3, 0, PR.new_state(len(verts)))
        assert got["sees"][4:].all()
        assert np.abs(got["c"][4:].astype(np.float64) - _affine(pts[:, 0], pts[:, 1])).max() <= 16 * EPS * np.abs(image).max()


# ------------------------------------------------------------------ the tessellated box
HALF, N_BOX, DIST = (0.5, 0.5, 0.25), 4, 2.25


def _box_case():
    """The box +-(0.5, 0.5, 0.25), 4 x 4 quads per side (98 vertices), seen along its z axis from both sides by cameras 2 in front of the
    nearer side: fx = 16 puts that side's 25 vertices 2 pixels apart, at 4.25, 6.25 .. 12.25 (cx = 8.25: no vertex and no edge of the
    outline on a pixel centre, so no tie rule enters the count).  Normals: the normalised sum of the adjacent faces' normals."""
    verts, faces = MS.box_mesh(HALF, N_BOX)
    assert verts.shape == (98, 3)
    fn = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]).astype(np.float64)
    normals = np.zeros((98, 3))
    for k in range(3):
        np.add.at(normals, faces[:, k], fn)
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    cam = (16.0, 16.0, 8.25, 8.25)
    mats = [np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, DIST]], F32), np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, DIST]], F32)]
    centres = [(0.0, 0.0, -DIST), (0.0, 0.0, DIST)]
    images = [np.full((17, 17, 3), 0.25, F32), np.full((17, 17, 3), 0.75, F32)]
    views = [_view(verts, faces, 17, 17, images[k], tol=0.01, mats=mats[k][None], cam=cam, centre=centres[k], cull_sign=[1]) for k in range(2)]
    return verts, faces, normals, views


def _box_failures(planted=None):
    verts, faces, normals, views = _box_case()
    front, back = verts[:, 2] == -HALF[2], verts[:, 2] == HALF[2]
    assert front.sum() == 25 and back.sum() == 25                 # (n + 1)^2 each; the other 98 - 50 = 48 lie on the four sides only
    failed = []
    for use_normals in (True, False):
        p = PR.paint(verts, normals if use_normals else None, views, planted=planted)
        want_seen = (front | back).astype(np.int32)
        want_best = np.where(front, 0, np.where(back, 1, -1)).astype(np.int32)
        if not (np.array_equal(p["seen"], want_seen) and np.array_equal(p["best"], want_best)):
            failed.append(f"seen / best, normals {use_normals}")
        if not np.array_equal(p["filled"], np.where(front | back, 0, -1)):
            failed.append(f"filled, normals {use_normals}")
        # a constant image: every seen vertex has that colour within the bound of test_mesh_paint_gpu.py's constant-colour test
        want = np.where(front[:, None], 0.25, 0.75)
        hit = p["seen"] > 0
        if not (np.abs(p["colors"][hit].astype(np.float64) - want[hit]).max() <= 16 * EPS):
            failed.append(f"colour, normals {use_normals}")
        if use_normals:
            # the weight of a vertex inside the front side, normal (0, 0, -1), d = (-x, -y, -2): cos^2 = 4 / (x^2 + y^2 + 4)
            inner = front & (np.abs(verts[:, 0]) < HALF[0]) & (np.abs(verts[:, 1]) < HALF[1])
            x, y = verts[inner, 0].astype(np.float64), verts[inner, 1].astype(np.float64)
            if not (inner.sum() == 9 and np.abs(p["weight"][inner] - 4 / (x * x + y * y + 4)).max() < 8 * EPS):
                failed.append("weights")
    return failed


def test_box_from_front_and_back():
    assert _box_failures() == []


def test_side_faces_get_cos_squared():
    """P3 alone, at the centres of the four side faces and the two ends, from a camera off the axis: cos^2 in float64 where the face looks
    towards the camera, 0 where it looks away.  Bound: d has one rounding per component, each of the three sums of three products five
    more, dot dot, nn dd and the division one each -- under 16 e relative for these well-conditioned sums."""
    centre = (2.0, 0.75, -2.0)
    x = np.array([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, -0.25], [0, 0, 0.25]], F32)
    n = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1]], F32)
    g = PR.facing(x, n, centre)
    d = np.asarray(centre, np.float64) - x
    cos = (d * n).sum(1) / np.linalg.norm(d, axis=1)
    want = np.where(cos > 0, cos * cos, 0.0)
    assert (want > 0).tolist() == [True, False, True, False, True, False]
    assert np.abs(g - want).max() <= 16 * EPS and (g[want == 0] == 0).all()
    # a zero normal, a vertex at the camera and a non-finite normal weigh nothing
    assert PR.facing(x[:3], np.array([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], F32), centre).tolist() == [0, 0, 0]
    assert PR.facing(np.array([centre], F32), n[:1], centre).tolist() == [0]
    assert PR.facing(x, None, centre).tolist() == [1] * 6


# ------------------------------------------------------------------ the occluder
def _occluder_failures(planted=None):
    """A large quad at depth 2.5 behind a small one at depth 2 (gap 0.5); loose vertices on the far plane, two behind the near quad and two
    beside it.  The image is 0.5 everywhere."""
    H, W = 12, 16
    far_pts = np.array([(6.5, 5.5), (7.25, 6.0), (2.5, 3.5), (13.0, 9.25)])
    verts = np.concatenate([_quad(-2, -2, 20, 16, 2.5 * np.ones(4)), _quad(4, 3, 10, 8, 2.0), RR.screen_mesh(far_pts, 2.5 * np.ones(4))])
    faces = np.concatenate([QUAD, QUAD + 4])
    image = np.full((H, W, 3), 0.5, F32)
    failed = []
    for tol, want in ((0.25, [False, False, True, True]), (1.0, [True, True, True, True])):
        view = _view(verts, faces, H, W, image, tol=tol)
        p = PR.paint(verts, None, [view], planted=planted)
        if (p["seen"][8:] > 0).tolist() != want:
            failed.append(f"tol {tol}")
        if not (p["colors"][8:][p["seen"][8:] > 0] == 0.5).all():
            failed.append(f"colour at tol {tol}")
    return failed


def test_occluder():
    assert _occluder_failures() == []


# ------------------------------------------------------------------ the mask
RED, WHITE = (1.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _mask_failures(planted=None):
    """Columns 0..4 are the object (mask 1, red); column 5 is background (mask 0, white); column 6 is another object (mask -1, white);
    column 7 is the object again."""
    H, W = 6, 8
    mask = np.ones((H, W), F32)
    mask[:, 5], mask[:, 6] = 0.0, -1.0
    image = np.where((mask > 0)[:, :, None], np.array(RED, F32), np.array(WHITE, F32)).astype(F32)
    pts = np.array([(4.5, 2.25), (5.5, 2.0), (6.5, 3.5), (5.0, 1.0), (2.75, 4.5)])
    verts = np.concatenate([_quad(-2, -2, 12, 10, 2.0), RR.screen_mesh(pts, 2.0)])
    p = PR.paint(verts, None, [_view(verts, QUAD, H, W, image, mask=mask)], planted=planted)
    failed = []
    if (p["seen"][4:] > 0).tolist() != [True, False, True, False, True]:
        failed.append("seen")                                  # (5.5: both columns masked; 5.0: the only tap with weight is masked)
    hit = p["seen"][4:] > 0
    if not (p["colors"][4:][hit] == np.array(RED, F32)).all():
        failed.append("exactly red")
    return failed


def test_mask():
    assert _mask_failures() == []


# ------------------------------------------------------------------ fill
def _strip_views(n, W=3):
    """n vertices at the pixel centres (i, 0) of a depth-1 plane; the image has W pixels, so the view sees the first W of them."""
    screen = np.stack([np.arange(n), np.zeros(n), np.ones(n)], axis=1).astype(F32)
    image = (np.arange(W)[None, :, None] + np.array([1.0, 10.0, 100.0])).astype(F32)
    return [dict(screen=screen, depth=np.ones((1, W), F32), image=image, mask=None, centre=(0, 0, 0), tol=0.0)]


def test_fill_on_a_strip():
    """A strip of 12 vertices (vertex i's neighbours are i - 2, i - 1, i + 1, i + 2) of which a view sees 0, 1, 2."""
    n = 12
    verts, faces = MS.strip(n)
    adj = MS.adjacency(faces, n)
    assert adj["nbr"][adj["nbr_start"][5]:adj["nbr_start"][6]].tolist() == [3, 4, 6, 7]
    views = _strip_views(n)
    p0 = PR.paint(verts, None, views)
    assert p0["filled"].tolist() == [0, 0, 0] + [-1] * 9 and p0["colors"][:3, 0].tolist() == [1, 2, 3] and (p0["colors"][3:] == 0).all()
    for R in (1, 2, 20):
        p = PR.paint(verts, None, views, rounds=R, adj=adj, background=-1.0)
        dist = np.maximum((np.arange(n) - 2 + 1) // 2, 0)            # graph distance to {0, 1, 2}: two vertices per step
        assert p["filled"].tolist() == np.where(dist <= R, dist, -1).tolist(), R
        assert (p["colors"][dist > R] == -1.0).all() and same_bits(p["colors"][:3], p0["colors"][:3]).all()
        c = p["colors"].astype(np.float64)
        # round 1: vertex 3 has the seen neighbours 1 and 2, vertex 4 only 2
        assert c[3, 0] == (2 + 3) / 2 and c[4, 0] == 3 and c[3, 2] == (101 + 102) / 2
        if R >= 2:      # round 2: vertex 5 has 3 and 4 (filled in round 1), vertex 6 only 4
            assert p["colors"][5, 0] == F32((c[3, 0] + c[4, 0]) / 2) and p["colors"][6, 0] == p["colors"][4, 0]
    fallback = np.full((n, 3), 7.0, F32)
    p = PR.paint(verts, None, views, rounds=2, adj=adj, fallback=fallback, background=-1.0)
    assert (p["colors"][7:] == 7.0).all() and p["filled"][7:].tolist() == [-1] * 5 and (p["colors"][:7] != 7.0).all()
    # an ascending float64 sum: three terms whose fp32 sum would depend on the order
    colors = np.array([[1, 0, 0], [2.0 ** -24, 0, 0], [2.0 ** -24, 0, 0], [0, 0, 0]], F32)
    star = dict(nbr_start=np.array([0, 1, 2, 3, 6]), nbr=np.array([3, 3, 3, 0, 1, 2], np.int32), degree=np.array([1, 1, 1, 3], np.int32))
    out, f = PR.fill_round(colors, np.array([0, 0, 0, -1], np.int32), star, 1)
    assert f.tolist() == [0, 0, 0, 1] and out[3, 0] == F32((1.0 + 2.0 ** -23) / 3.0)
    # a Jacobi round: vertex 3 must not see what vertex 4 takes in the same round
    out, f = PR.fill_round(p0["colors"], p0["filled"], adj, 1)
    assert f.tolist() == [0, 0, 0, 1, 1] + [-1] * 7


# ------------------------------------------------------------------ order and ties
def _order_case():
    """One vertex on a pixel centre, three views without normals (g = 1) whose images are 1, 2^-24 and 2^-24: in fp32
    (1 + 2^-24) + 2^-24 = 1 (two ties to even) but (2^-24 + 2^-24) + 1 = 1 + 2^-23."""
    screen = np.array([[0, 0, 1]], F32)
    return [dict(screen=screen, depth=np.ones((1, 1), F32), image=np.full((1, 1, 3), v, F32), mask=None, centre=(0, 0, 0), tol=0.0)
            for v in (1.0, 2.0 ** -24, 2.0 ** -24)]


def _order_failures(planted=None):
    views = _order_case()
    p = PR.paint(np.zeros((1, 3), F32), None, views, planted=planted)
    failed = []
    if not (p["state"]["sum_rgb"][0, 0] == F32(1.0) and p["state"]["sum_w"][0] == 3 and p["colors"][0, 0] == F32(1.0) / F32(3.0)):
        failed.append("ascending sums")
    b = PR.paint(np.zeros((1, 3), F32), None, views, blend="best", planted=planted)
    if not (b["best"].tolist() == [0] and b["colors"][0, 0] == 1.0 and b["weight"].tolist() == [1.0] and b["seen"].tolist() == [3]):
        failed.append("ties keep the lower view")
    return failed


def test_view_order_and_ties():
    assert _order_failures() == []
    up = PR.paint(np.zeros((1, 3), F32), None, _order_case())["state"]["sum_rgb"][0, 0]
    down = PR.paint(np.zeros((1, 3), F32), None, _order_case(), planted="descending")["state"]["sum_rgb"][0, 0]
    assert up == F32(1.0) and down == np.nextafter(F32(1.0), F32(2.0)) and not same_bits(np.array([up]), np.array([down])).all()


# ------------------------------------------------------------------ planted mistakes
CHECKS = {"affine": _affine_failures, "box": _box_failures, "occluder": _occluder_failures, "mask": _mask_failures, "order": _order_failures}
REJECTED_BY = {"no_depth_test": "occluder", "all_taps": "mask", "half_pixel": "affine", "nearest": "affine", "descending": "order",
               "tie_high": "order"}


@pytest.mark.parametrize("planted", PR.PLANTED)
def test_planted_mistakes_are_rejected(planted):
    assert set(REJECTED_BY) == set(PR.PLANTED)
    failed = {name: check(planted) for name, check in CHECKS.items()}
    print(planted, {k: v for k, v in failed.items() if v})
    assert failed[REJECTED_BY[planted]], (planted, failed)
    if planted == "no_depth_test":
        assert failed["box"]                                  # (without normals the far side shows through)


# ------------------------------------------------------------------ the API without a GPU
PAINT_SYMBOLS = ("snr_paint_view", "snr_paint_finish", "snr_paint_fill")


def test_symbols_and_c_abi_checks():
    import os
    import re
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, geometry as G, ops
    assert all(n in _lib.exported_symbols() for n in PAINT_SYMBOLS)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in PAINT_SYMBOLS)
    assert _lib.header_abi_version() >= 24 and lib.snr_abi_version() == _lib.header_abi_version()
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    hdr = open(os.path.join(here, "..", "include", "supnerf_hip.h")).read()
    assert all(re.search(r"\b" + n + r"\(", hdr) for n in PAINT_SYMBOLS) and "Mesh painting" in hdr
    assert "snr_paint.hip" in open(os.path.join(here, "build.py")).read()
    assert G.Painted._fields == ("colors", "weight", "seen", "best", "filled")
    assert ops.PaintState._fields == ("sum_rgb", "sum_w", "seen", "best_w", "best", "best_rgb") and ops.PAINT_BLENDS == ("weighted", "best")
    sig = inspect.signature(G.paint_mesh)
    assert list(sig.parameters) == ["meshes", "views", "normals", "blend", "facing", "tol", "fill", "adjacency", "fallback", "background",
                                    "cull", "family", "shapenet_obj_cood", "kitti2nusc", "z_near"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    d = {n: p.default for n, p in sig.parameters.items()}
    assert (d["blend"], d["facing"], d["tol"], d["fill"], d["background"], d["cull"], d["z_near"]) == ("weighted", True, None, 0, 0.0, "back", 1e-3)
    assert list(inspect.signature(ops.paint_view).parameters) == ["mesh", "screen", "normals", "image", "mask", "depth", "centre", "tol",
                                                                  "z_near", "k", "state"]
    # the C ABI validates before it launches: these return without touching a device
    big, p = 1 << 39, 64                                      # (p: a pointer that is not null and is never followed)
    view = lambda nV=4, H=2, W=2, tol=0.0, zn=1e-3, k=0, screen=p, image=p, depth=p, st=(p,) * 6: lib.snr_paint_view(  # noqa: E731
        screen, None, None, nV, image, None, depth, H, W, 0.0, 0.0, 0.0, tol, zn, k, *st, None)
    assert view(nV=0) == 0 and view(H=0) == 0 and view(W=0) == 0
    assert view(nV=-1) == -1 and view(H=-1) == -1 and view(W=-2) == -1 and view(k=-1) == -1
    assert view(zn=0.0) == -1 and view(zn=float("nan")) == -1 and view(tol=-1.0) == -1 and view(tol=float("nan")) == -1
    assert view(tol=float("inf")) == -1
    assert view(screen=None) == -1 and view(image=None) == -1 and view(depth=None) == -1
    for i in range(6):
        assert view(st=(p,) * i + (None,) + (p,) * (5 - i)) == -1
    assert lib.snr_paint_view(p, None, p, 4, p, None, p, 2, 2, 0.0, 0.0, 0.0, 0.0, 1e-3, 0, p, p, p, p, p, p, None) == -1   # normals without verts
    assert view(nV=big) == -5 and view(H=1 << 16, W=1 << 16) == -5
    fin = lambda nV=4, blend=0, a=p, b=p, seen=p, best=p, out=p, filled=p: lib.snr_paint_finish(a, b, seen, best, nV, blend, 0.0, out, filled,  # noqa: E731
                                                                                                  None)
    assert fin(nV=0) == 0 and fin(nV=-1) == -1 and fin(blend=2) == -1 and fin(blend=-1) == -1 and fin(nV=big) == -5
    assert fin(seen=None) == -1 and fin(out=None) == -1 and fin(filled=None) == -1 and fin(a=None) == -1 and fin(b=None) == -1
    assert fin(blend=1, best=None) == -1
    fill = lambda nV=4, nE=6, B=1, r=1, cin=p, fin_=p, start=p, nbr=p, voff=p, cout=1 << 20, fout=1 << 21: lib.snr_paint_fill(  # noqa: E731
        cin, fin_, start, nbr, voff, B, nV, nE, r, cout, fout, None)
    assert fill(nV=0) == 0 and fill(nV=-1) == -1 and fill(nE=-1) == -1 and fill(B=-1) == -1 and fill(B=0) == -1
    assert fill(r=0) == -1 and fill(r=-3) == -1 and fill(nV=big) == -5 and fill(nE=big) == -5
    for name in ("cin", "fin_", "start", "nbr", "voff", "cout", "fout"):
        assert fill(**{name: None}) == -1, name
    assert fill(cout=p) == -1 and fill(cout=p + 44) == -1 and fill(fout=p + 12) == -1            # a Jacobi round: not in place, no overlap


def test_python_argument_errors_without_a_device():
    import supnerf_amd as A
    from supnerf_amd import geometry as G, ops
    verts, faces = MS.box_mesh(HALF, 2)
    mesh = (torch.from_numpy(verts), torch.from_numpy(faces))
    view = dict(img=torch.zeros(4, 6, 3), mask=torch.ones(24), cam_pose=torch.eye(4)[:3], obj_diag=1.0, K=np.eye(3), roi=(10, 20, 16, 24))
    normals = torch.zeros(verts.shape[0], 3)
    with pytest.raises(A.SnrError, match="GPU|gpu|CPU|device"):
        G.paint_mesh(mesh, [view], normals=normals)                                  # CPU tensors: no fallback
    with pytest.raises(A.SnrError, match="GPU|gpu|CPU|device"):
        G.paint_mesh([mesh], [view], facing=False)
    with pytest.raises(A.SnrError, match="blend"):
        G.paint_mesh(mesh, [view], normals=normals, blend="median")
    with pytest.raises(A.SnrError, match="normals"):
        G.paint_mesh(mesh, [view])                                                   # facing=True needs them
    with pytest.raises(A.SnrError, match="fill"):
        G.paint_mesh(mesh, [view], facing=False, fill=-1)
    for tol in (-0.1, float("nan"), float("inf")):
        with pytest.raises(A.SnrError, match="tol"):
            G.paint_mesh(mesh, [view], facing=False, tol=tol)
    with pytest.raises(A.SnrError, match="cull"):
        G.paint_mesh(mesh, [view], facing=False, cull="front")
    with pytest.raises(A.SnrError, match="z_near"):
        G.paint_mesh(mesh, [view], facing=False, z_near=0.0)
    with pytest.raises(A.SnrError, match="family"):
        G.paint_mesh(mesh, [view], facing=False, family="c")
    for views in ([], view, None):
        with pytest.raises(A.SnrError, match="views"):
            G.paint_mesh(mesh, views, facing=False)
    with pytest.raises(A.SnrError, match="cam_pose"):
        G.paint_mesh(mesh, [{k: v for k, v in view.items() if k != "cam_pose"}], facing=False)
    for bad in (dict(view, img=torch.zeros(6, 4, 3)), dict(view, mask=torch.ones(23)), dict(view, roi=(10, 20, 10, 24)),
                dict(view, img=torch.zeros(4, 6))):
        with pytest.raises(A.SnrError, match="not the native"):
            G.paint_mesh(mesh, [view, bad], facing=False)
    assert G.paint_mesh([], [view], facing=False) == []
    with pytest.raises(A.SnrError, match="GPU|gpu"):
        ops.paint_state(4, "cpu")
    with pytest.raises(A.SnrError, match="negative"):
        ops.paint_state(-1, "cuda")
    with pytest.raises(A.SnrError, match="blend"):
        ops.paint_finish(None, "median")
    with pytest.raises(A.SnrError, match="state"):
        ops.paint_finish(None, "best")
