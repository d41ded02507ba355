"""Mesh painting on the MI355X: ``ops.paint_view`` / ``paint_finish`` / ``paint_fill`` and ``geometry.paint_mesh`` (the ``snr_paint_*``
kernels) against tests/paint_restatement.py.

Every float output is compared BIT FOR BIT with the restatement: every operation of rules P1 to P6 is one correctly rounded IEEE operation
in a fixed order, so there is no tolerance.  The paint kernels are judged alone: the screen positions and depth buffers the restatement
reads are the GPU rasteriser's own (or drawn at random where no mesh is needed).  Every integer output is compared exactly.  The end-to-end
test restates the whole chain, the raster half with tests/raster_restatement.py."""
import numpy as np
import pytest
import torch

import geometry_cases as GC
import paint_restatement as PR
import raster_restatement as RR
import smooth_restatement as MS
from segment_sum_restatement import banded as _banded, bands_intact as _bands_intact, same_bits
from oracle_bands import amd, dev  # noqa: F401  (fixtures)
from planted_decoder import WOBBLE
from test_mesh_smooth_gpu import HAND

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS = 2.0 ** -24
Z_NEAR = 0.25
STATE = (("sum_rgb", 3, torch.float32), ("sum_w", 1, torch.float32), ("seen", 1, torch.int32), ("best_w", 1, torch.float32),
         ("best", 1, torch.int32), ("best_rgb", 3, torch.float32))


def _np(t):
    return t.detach().cpu().numpy()


def _up(a, dev, dtype=None):  # noqa: F811
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _same(got, want, tag):
    got = _np(got) if torch.is_tensor(got) else got
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32:
        bad = ~same_bits(got, want)
        assert not bad.any(), (tag, int(bad.sum()), got[bad][:4], want[bad][:4])
    else:
        assert np.array_equal(got, want), (tag, int((got != want).sum()))


def _same_state(state, want, tag):
    for name, _, _ in STATE:
        _same(getattr(state, name), want[name], (tag, name))


# ------------------------------------------------------------------ drawn cases: no mesh, every edge of rule P1 planted
def _special_rows(H, W):
    """Screen rows (u, v, z) on every edge of P1: not finite, nearer than z_near, exactly 0 and W - 1 / H - 1, one ulp beyond either."""
    w1, h1 = F32(W - 1), F32(H - 1)
    below, inf, nan = np.nextafter(F32(0), F32(-1)), F32(np.inf), F32(np.nan)
    return np.array([(nan, 0, 1), (0, inf, 1), (0, 0, nan), (0, 0, inf), (-inf, 0, 1), (0, 0, Z_NEAR / 2), (0, 0, Z_NEAR), (0, 0, 1), (w1, h1, 1),
                     (w1, 0, 1), (0, h1, 1), (np.nextafter(w1, inf), 0, 1), (0, np.nextafter(h1, inf), 1), (below, 0, 1), (0, below, 1),
                     (w1 / 2, h1 / 2, 1), (0, 0, -1)], F32)


def _drawn_view(V, H, W, seed, with_mask, centre):
    """Screen positions on a 1/8-pixel lattice reaching one pixel outside the image (the special rows first, as far as V allows), a
    depth buffer with holes, an image, a mask of 1, 0.5, 0 and -1."""
    rng = np.random.default_rng(seed)
    screen = np.stack([rng.integers(-8, 8 * W + 1, V) / 8.0, rng.integers(-8, 8 * H + 1, V) / 8.0, rng.uniform(0.5, 2.5, V)], 1).astype(F32)
    special = _special_rows(H, W)[:V]
    screen[:special.shape[0]] = special
    depth = np.where(rng.random((H, W)) < 0.2, 0.0, rng.uniform(1.0, 2.5, (H, W))).astype(F32)
    depth.reshape(-1)[0] = 2.0                                                          # (the special rows at (0, 0) have something to see)
    image = rng.standard_normal((H, W, 3)).astype(F32)
    mask = rng.choice(np.array([1.0, 1.0, 0.5, 0.0, -1.0], F32), (H, W)) if with_mask else None
    return dict(screen=screen, depth=depth, image=image, mask=mask, centre=centre, tol=0.25)


def _drawn_case(V, sizes, seed, with_mask, with_normals):
    """(verts, normals or None, views): views 0 and 1 share a camera centre, so with normals their weights tie exactly."""
    rng = np.random.default_rng(1000 + seed)
    verts = rng.uniform(-0.5, 0.5, (V, 3)).astype(F32)
    normals = None
    if with_normals:
        normals = rng.standard_normal((V, 3)).astype(F32)
        normals[1::7] = 0.0                                                             # zero normals
        if V > 3:
            normals[3] = (np.nan, 0, 0)
    centres = [(0.3, -0.2, -3.0), (0.3, -0.2, -3.0), (2.0, 1.0, -1.0), (-2.5, 0.5, 0.25), (0.0, 3.0, 0.0)]
    views = [_drawn_view(V, H, W, 10 * seed + k, with_mask, centres[k]) for k, (H, W) in enumerate(sizes)]
    return verts, normals, views


def _run_views(ops, dev, verts, normals, views, state=None):  # noqa: F811
    V = verts.shape[0]
    mesh = ops.pack_mesh(_up(verts, dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), [V], [0])
    state = ops.paint_state(V, dev) if state is None else state
    n = None if normals is None else _up(normals, dev)
    for k, v in enumerate(views):
        out = ops.paint_view(mesh, _up(v["screen"], dev), n, _up(v["image"], dev), None if v["mask"] is None else _up(v["mask"], dev),
                             _up(v["depth"], dev), v["centre"], v["tol"], Z_NEAR, k, state)
        assert out is state
    return state


def _check_drawn(amd, dev, V, sizes, seed, with_mask, with_normals):  # noqa: F811
    ops = amd.ops
    verts, normals, views = _drawn_case(V, sizes, seed, with_mask, with_normals)
    state = _run_views(ops, dev, verts, normals, views)
    tag = (V, sizes, with_mask, with_normals)
    want = {}
    for blend in ops.PAINT_BLENDS:
        want[blend] = PR.paint(verts, normals, views, blend=blend, background=-2.0, z_near=Z_NEAR)
        colors, filled = ops.paint_finish(state, blend, -2.0)
        _same(colors, want[blend]["colors"], (tag, blend, "colors"))
        _same(filled, want[blend]["filled"], (tag, blend, "filled"))
    _same_state(state, want["best"]["state"], tag)
    again = _run_views(ops, dev, verts, normals, views)                                # two runs, the same bits
    for name, _, _ in STATE:
        assert torch.equal(getattr(state, name).view(torch.int32), getattr(again, name).view(torch.int32)), (tag, name)
    return want["weighted"]


SIZES = [(1, 1), (1, 7), (5, 1), (3, 5), (64, 48)]


@pytest.mark.parametrize("V", [0, 1, 63, 64, 65, 257])
def test_drawn_views_at_every_size(amd, dev, V):  # noqa: F811
    """1, 2 and 5 views of different crop sizes, with and without a mask, with and without normals; both blends."""
    seen = 0
    for n_views in (1, 2, 5):
        for with_mask in (False, True):
            for with_normals in (False, True):
                sizes = (SIZES[-n_views:] if V % 2 else SIZES[:n_views])
                p = _check_drawn(amd, dev, V, sizes, 3 * n_views + V, with_mask, with_normals)
                seen += int((p["seen"] > 0).sum())
                if n_views > 1 and V >= 257 and not with_mask:
                    assert (p["seen"] > 1).any()                                     # (ties in g are met: views 0 and 1 share the centre)
    assert seen > 0 or V < 63                                                         # (the first rows are the special ones)


@pytest.mark.parametrize("size", SIZES)
def test_every_image_size_alone(amd, dev, size):  # noqa: F811
    p = _check_drawn(amd, dev, 300, [size], 77, True, True)
    q = _check_drawn(amd, dev, 300, [size], 78, False, False)
    H, W = size
    assert (q["seen"] > 0).sum() > (20 if min(H, W) > 1 else 0) and p["seen"].shape == (300,)
    # the special rows: 0..5 are skipped by P1; z = z_near, (0, 0), (W - 1, H - 1) and the other corners are inside; one ulp beyond is outside
    view = _drawn_case(300, [size], 78, False, False)[2][0]
    fp = PR.footprint(view["screen"], H, W, Z_NEAR)
    assert fp["inside"][:17].tolist() == [False] * 6 + [True] * 5 + [False] * 4 + [True, False]


def test_more_vertices_than_one_pass_of_the_grid(amd, dev):  # noqa: F811
    V = amd.ops.PAINT_GRID_THREADS + 257
    p = _check_drawn(amd, dev, V, [(64, 48), (3, 5)], 5, True, True)
    tail = slice(amd.ops.PAINT_GRID_THREADS, None)
    assert (p["seen"][tail] > 0).any() and (p["seen"][tail] == 0).any()


def test_ties_keep_the_lower_view(amd, dev):  # noqa: F811
    """Two views from one centre: equal weights, with normals too; best is 0 wherever both see the vertex."""
    for with_normals in (False, True):
        verts, normals, views = _drawn_case(257, [(64, 48), (64, 48)], 9, False, with_normals)
        views[1] = dict(views[0], image=views[1]["image"])
        state = _run_views(amd.ops, dev, verts, normals, views)
        both = _np(state.seen) == 2
        assert both.sum() > 20 and (_np(state.best)[both] == 0).all()
        want = PR.paint(verts, normals, views, blend="best", z_near=Z_NEAR)
        _same_state(state, want["state"], with_normals)
        colors, _ = amd.ops.paint_finish(state, "best")
        assert same_bits(_np(colors)[both], want["state"]["best_rgb"][both]).all()


# ------------------------------------------------------------------ the rasteriser's own screen and depth
def _box_views(ops, dev, verts, faces):  # noqa: F811
    """The tessellated box of tests/test_mesh_paint_cpu.py from the front, the back and a corner, crops of three sizes: the GPU
    rasteriser's (screen, depth) per view."""
    mesh = ops.pack_mesh(_up(verts, dev), _up(faces, dev), [len(verts)], [len(faces)])
    c, s = np.cos(0.7), np.sin(0.7)
    mats = [np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.25]], F32), np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 2.25]], F32),
            np.array([[c, 0, s, 0.1], [0, 1, 0, -0.05], [-s, 0, c, 2.5]], F32)]
    cams, sizes = [(16.0, 16.0, 8.25, 8.25), (40.0, 40.0, 31.5, 23.5), (24.0, 20.0, 12.0, 9.5)], [(17, 17), (48, 64), (19, 25)]
    rng = np.random.default_rng(2)
    zero, sign = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    views = []
    for M, cam, (H, W) in zip(mats, cams, sizes):
        _, depth, _, screen = ops.rasterize(mesh, _up(M[None], dev), cam, zero, 1, H, W, 1e-3, sign)
        R, t = M[:, :3].astype(np.float64), M[:, 3].astype(np.float64)
        views.append(dict(screen=_np(screen), depth=_np(depth[0]), image=rng.uniform(0, 1, (H, W, 3)).astype(F32),
                          mask=(rng.random((H, W)) < 0.9).astype(F32), centre=tuple(-(R.T @ t)), tol=0.01))
    return mesh, views


def test_box_with_the_rasterisers_own_depth(amd, dev):  # noqa: F811
    ops = amd.ops
    verts, faces = MS.box_mesh((0.5, 0.5, 0.25), 4)
    fn = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]).astype(np.float64)
    normals = np.zeros((98, 3))
    for k in range(3):
        np.add.at(normals, faces[:, k], fn)
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    mesh, views = _box_views(ops, dev, verts, faces)
    front, back = verts[:, 2] == -0.25, verts[:, 2] == 0.25
    for n in (normals, None):
        state = ops.paint_state(98, dev)
        for k, v in enumerate(views):
            ops.paint_view(mesh, _up(v["screen"], dev), None if n is None else _up(n, dev), _up(v["image"], dev), _up(v["mask"], dev),
                           _up(v["depth"], dev), v["centre"], v["tol"], 1e-3, k, state)
        want = PR.paint(verts, n, views, blend="weighted")
        _same_state(state, want["state"], "box")
        for blend in ops.PAINT_BLENDS:
            colors, filled = ops.paint_finish(state, blend)
            _same(colors, PR.finish(want["state"], blend)[0], ("box", blend))
            _same(filled, want["filled"], ("box", blend, "filled"))
    # without the mask: the hand counts of the CPU test, on the device's numbers
    state = ops.paint_state(98, dev)
    for k, v in enumerate(views[:2]):
        ops.paint_view(mesh, _up(v["screen"], dev), _up(normals, dev), _up(v["image"], dev), None, _up(v["depth"], dev), v["centre"], 0.01, 1e-3,
                       k, state)
    assert np.array_equal(_np(state.seen), (front | back).astype(np.int32))
    assert np.array_equal(_np(state.best), np.where(front, 0, np.where(back, 1, -1)).astype(np.int32))


def test_constant_image_gives_its_colour(amd, dev):  # noqa: F811
    """An image of one colour C gives every seen vertex C.  The bound: with valid taps of weights w_t, the numerator is the sum of the
    products fl(w_t C) -- one rounding each -- added with at most three additions, each of which adds at most e = 2^-24 to what is summed
    so far: C sum_t w_t (1 + d_t), |d_t| <= 4 e.  s is the same sum without the products: sum_t w_t (1 + d'_t), |d'_t| <= 3 e; the
    roundings inside the w_t themselves are common to both and cancel.  The division adds e: |c - C| <= 8 e |C| to first order (four
    products, three additions, one division), (1 + 2^-20) of it with the second-order terms.  One view without normals: sum_rgb = 1 c,
    sum_w = 1, and c / 1 = c adds nothing."""
    ops = amd.ops
    verts, faces = MS.box_mesh((0.5, 0.5, 0.25), 4)
    mesh, views = _box_views(ops, dev, verts, faces)
    C = np.array([0.3, 0.7, 1.1], F32)
    worst = 0.0
    for k, v in enumerate(views):
        H, W = v["depth"].shape
        state = ops.paint_state(98, dev)
        ops.paint_view(mesh, _up(v["screen"], dev), None, _up(np.broadcast_to(C, (H, W, 3)), dev), None, _up(v["depth"], dev), v["centre"], 0.01,
                       1e-3, 0, state)
        colors, filled = ops.paint_finish(state, "weighted", 0.0)
        hit = _np(filled) == 0
        assert hit.sum() >= 20
        err = np.abs(_np(colors)[hit].astype(np.float64) - C.astype(np.float64)) / C.astype(np.float64)
        worst = max(worst, float(err.max()) / EPS)
        assert (err <= 8 * EPS * (1 + 2.0 ** -20)).all(), (k, err.max() / EPS)
        assert (_np(colors)[~hit] == 0).all()
    print(f"constant image: worst |c - C| / |C| = {worst:.2f} x 2^-24 (8 allowed)")


# ------------------------------------------------------------------ fill
def _fill_case(amd, dev, verts, faces, seeds, rounds_list, tag):  # noqa: F811
    from supnerf_amd import geometry as G
    ops = amd.ops
    V = verts.shape[0]
    mesh = (_up(verts, dev, torch.float32), _up(np.asarray(faces, np.int32).reshape(-1, 3), dev))
    adj = MS.adjacency(np.asarray(faces).reshape(-1, 3), V)
    packed = G._pack_adjacency([G.mesh_adjacency(mesh)], [V], dev)
    rng = np.random.default_rng(V)
    colors = rng.standard_normal((V, 3)).astype(F32)
    filled = np.full(V, -1, np.int32)
    filled[np.asarray(seeds, np.int64)] = 0
    for rounds in rounds_list:
        got_c, got_f = ops.paint_fill(_up(colors, dev), _up(filled, dev), packed, rounds)
        want_c, want_f = PR.fill(colors, filled, adj, rounds)
        _same(got_c, want_c, (tag, rounds, "colors"))
        _same(got_f, want_f, (tag, rounds, "filled"))
        again_c, again_f = ops.paint_fill(_up(colors, dev), _up(filled, dev), packed, rounds)
        assert torch.equal(again_c.view(torch.int32), got_c.view(torch.int32)) and torch.equal(again_f, got_f)
    return want_f


def test_fill_on_hand_meshes(amd, dev):  # noqa: F811
    for name, (n, faces) in HAND.items():
        verts = np.random.default_rng(n).standard_normal((n, 3)).astype(F32)
        for seeds in ([0], [n - 1], [], list(range(n))):
            _fill_case(amd, dev, verts, np.asarray(faces, np.int32).reshape(-1, 3), seeds, (0, 1, 2, 5), (name, tuple(seeds)))
    # the isolated vertex of "repeated indices" stays unfilled for ever; "no faces" fills nothing
    n, faces = HAND["repeated indices, an isolated vertex"]
    f = _fill_case(amd, dev, np.zeros((n, 3), F32), np.asarray(faces, np.int32), [0], (5,), "isolated")
    assert f[4] == -1 and f[1] == 1


def test_fill_on_a_strip(amd, dev):  # noqa: F811
    verts, faces = MS.strip(300)
    f = _fill_case(amd, dev, verts, faces, [0, 1], (0, 1, 299), "strip 300")
    assert f.tolist() == [0, 0] + [(i - 1 + 1) // 2 for i in range(2, 300)] and f.max() == 149
    f = _fill_case(amd, dev, verts, faces, [150], (1, 40), "strip 300 from the middle")
    assert (f >= 0).sum() == 1 + 4 * 40 and f[150 + 80] == 40 and f[150 + 81] == -1


def test_canaries_through_the_c_abi(amd, dev):  # noqa: F811
    """Every state and output buffer between guard bands: the outputs are the restatement's and the bands are intact; the fill refuses
    to run in place."""
    ops, lib = amd.ops, amd._lib.lib()
    P, st = ops._ptr, ops._stream(dev)
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    V = 257
    verts, normals, views = _drawn_case(V, [(3, 5), (64, 48)], 21, True, True)
    nan = float("nan")
    full, part = {}, {}
    for name, width, dt in STATE:
        fill = -7 if dt == i32 else nan
        full[name], part[name] = _banded(V * width, dt, dev, fill)
        part[name].fill_(-1 if name == "best" else 0)
    state = ops.PaintState(*[part[name].view(V, 3) if width == 3 else part[name] for name, width, _ in STATE])
    _run_views(ops, dev, verts, normals, views, state)
    want = PR.paint(verts, normals, views, z_near=Z_NEAR)
    _same_state(state, want["state"], "banded")
    checks = [(full[name], V * width, -7 if dt == i32 else nan) for name, width, dt in STATE]
    outs = {}
    for blend in (0, 1):
        c_full, c = _banded(V * 3, f32, dev, nan)
        f_full, f = _banded(V, i32, dev, -7)
        assert lib.snr_paint_finish(P(state.sum_rgb), P(state.sum_w), P(state.seen, i32), P(state.best_rgb), V, blend, 0.5, P(c), P(f, i32), st) == 0
        wc, wf = PR.finish(want["state"], blend, 0.5)
        _same(c.view(V, 3), wc, ("finish", blend))
        _same(f, wf, ("finish filled", blend))
        checks += [(c_full, V * 3, nan), (f_full, V, -7)]
        outs[blend] = (c, f, wc, wf)
    # fill over a fan of 255 triangles (257 vertices): the hub joins everything in two rounds
    fan_v, fan_f = MS.fan(256)
    assert fan_v.shape[0] == V
    adj = MS.adjacency(fan_f, V)
    start, nbr, voff = _up(adj["nbr_start"], dev, i64), _up(adj["nbr"], dev, i32), _up(np.array([0, V]), dev, i64)
    nE = adj["nbr"].shape[0]
    c, f, wc, wf = outs[0]
    for r in (1, 2):
        o_full, o = _banded(V * 3, f32, dev, nan)
        g_full, g = _banded(V, i32, dev, -7)
        assert lib.snr_paint_fill(P(c), P(f, i32), P(start, i64), P(nbr, i32), P(voff, i64), 1, V, nE, r, P(o), P(g, i32), st) == 0
        wc, wf = PR.fill_round(wc, wf, adj, r)
        _same(o.view(V, 3), wc, ("fill", r))
        _same(g, wf, ("fill filled", r))
        checks += [(o_full, V * 3, nan), (g_full, V, -7)]
        before = (c.clone(), f.clone())
        assert lib.snr_paint_fill(P(c), P(f, i32), P(start, i64), P(nbr, i32), P(voff, i64), 1, V, nE, r, P(c), P(g, i32), st) == -1
        assert lib.snr_paint_fill(P(c), P(f, i32), P(start, i64), P(nbr, i32), P(voff, i64), 1, V, nE, r, P(o), P(f, i32), st) == -1
        assert torch.equal(c.view(i32), before[0].view(i32)) and torch.equal(f, before[1])
        c, f = o, g
    torch.cuda.synchronize()
    for buf, n, fill in checks:
        assert _bands_intact(buf, n, fill), (n, fill)


def test_wrapper_errors(amd, dev):  # noqa: F811
    ops = amd.ops
    V, H, W = 10, 4, 6
    mesh = ops.pack_mesh(torch.zeros(V, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), [V], [0])
    ok = dict(mesh=mesh, screen=torch.zeros(V, 3, device=dev), normals=torch.zeros(V, 3, device=dev), image=torch.zeros(H, W, 3, device=dev),
              mask=torch.ones(H, W, device=dev), depth=torch.ones(H, W, device=dev), centre=(0, 0, 0), tol=0.0, z_near=1e-3, k=0,
              state=ops.paint_state(V, dev))
    ops.paint_view(**ok)
    bad = [("screen", torch.zeros(V + 1, 3, device=dev)), ("screen", torch.zeros(V, 3, device=dev).double()),
           ("screen", torch.zeros(3, V, device=dev).T), ("normals", torch.zeros(V, 2, device=dev)), ("image", torch.zeros(H, W, device=dev)),
           ("image", torch.zeros(H, W, 3, device=dev).half()), ("image", torch.zeros(H, W, 4, device=dev)[:, :, :3]),
           ("mask", torch.ones(W, H, device=dev)), ("depth", torch.ones(H, W + 1, device=dev)), ("depth", torch.ones(H * W, device=dev)),
           ("image", torch.zeros(H, W, 3)), ("centre", (0, 0)), ("tol", -1.0), ("tol", float("nan")), ("z_near", 0.0), ("k", -1),
           ("state", ops.paint_state(V + 1, dev)), ("state", None)]
    for name, value in bad:
        with pytest.raises(amd.SnrError):
            ops.paint_view(**dict(ok, **{name: value}))
    with pytest.raises(amd.SnrError, match="blend"):
        ops.paint_finish(ok["state"], "mean")
    from supnerf_amd import geometry as G
    adj = G._pack_adjacency([G.mesh_adjacency((torch.zeros(V, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev)))], [V], dev)
    colors, filled = ops.paint_finish(ok["state"], "best")
    for c, f, r in ((colors[:-1], filled, 1), (colors, filled.long(), 1), (colors, filled, -1), (colors.double(), filled, 1)):
        with pytest.raises(amd.SnrError):
            ops.paint_fill(c, f, adj, r)
    c2, f2 = ops.paint_fill(colors, filled, adj, 0)
    assert torch.equal(c2, colors) and c2.data_ptr() != colors.data_ptr() and torch.equal(f2, filled)


# ------------------------------------------------------------------ end to end
def _look_at(eye, up=(0.0, 0.0, 1.0)):
    """(3, 4) float32 camera pose in the object's frame: at ``eye``, looking at the origin; columns x right, y down, z forward."""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(F32)


def _restated_view(pose, scale, K, roi):
    """What ``paint_mesh`` composes per view, by hand in float64: (M (3, 4) float32, (fx, fy, cx, cy), (h, w), the camera centre in the
    decoder frame)."""
    P = pose.astype(np.float64)
    r_inv = np.linalg.inv(P[:, :3])
    M = np.concatenate([r_inv * scale, -(r_inv @ P[:, 3:4])], 1)
    x0, y0, x1, y1 = roi
    return M.astype(F32), (K[0, 0], K[1, 1], K[0, 2] - x0, K[1, 2] - y0), (y1 - y0, x1 - x0), tuple((P[:, 3] / scale).tolist())


VIEW_K = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1]])
DIAG = 1.5
POSES = [((2.1, -1.3, 0.9), [112, 80, 208, 160]), ((-1.9, -1.2, 1.4), [118, 84, 199, 159]), ((0.4, 2.4, -0.7), [110, 78, 210, 163])]


@pytest.fixture(scope="module")
def planted(amd, dev):  # noqa: F811
    """The planted box decoder's mesh at resolution 24, its normals and the decoder's own colours."""
    from supnerf_amd import geometry as G
    model, sc = GC.box(amd, dev, 3, 1, seed=4, wobble=WOBBLE), GC.codes(1, 31, dev)
    tc = GC.codes(1, 32, dev)
    mesh = G.extract_mesh(model, sc, level=GC.LEVEL_BOX, resolution=24, bound=GC.BOUND_BOX, keep="largest")[0]
    normals = G.vertex_normals(model, [mesh], sc)[0]
    colors = G.vertex_colors(model, [mesh], [normals], sc, tc)[0]
    return mesh, normals.contiguous(), colors.contiguous()


def test_paint_mesh_end_to_end(amd, dev, planted):  # noqa: F811
    """Render the coloured mesh from three poses with ``mesh_view``, paint a second copy from those images, and restate the whole chain:
    tests/raster_restatement.py for the raster half, tests/paint_restatement.py for the rest."""
    from supnerf_amd import geometry as G
    (v, f), normals, colors = planted
    V, F = v.shape[0], f.shape[0]
    assert 100 < V < 5000
    K = torch.from_numpy(VIEW_K).float()
    views, restated = [], []
    vn, fnp = _np(v), _np(f)
    for eye, roi in POSES:
        pose = _look_at(eye)
        shot = G.mesh_view((v, f), torch.from_numpy(pose).to(dev), DIAG, K, roi, colors=colors)
        assert int(shot.mask.sum()) > 500
        views.append(dict(img=shot.color, mask=shot.mask.float().reshape(-1), cam_pose=torch.from_numpy(pose), obj_diag=DIAG, K=K, roi=roi))
        M, cam, (h, w), centre = _restated_view(pose, DIAG, VIEW_K, roi)
        ref = RR.rasterize(vn, fnp, [V], [F], M[None], cam, h, w, cull_sign=[int(np.sign(np.linalg.det(M[:, :3].astype(np.float64))))])
        assert tuple(shot.color.shape) == (h, w, 3) and np.array_equal(ref["face"][0] >= 0, _np(shot.mask))
        restated.append(dict(screen=ref["screen"], depth=ref["depth"][0], image=_np(shot.color), mask=_np(shot.mask).astype(F32),
                             centre=centre, tol=0.01 * DIAG))
    copy = (v.clone(), f.clone())
    adjacency = G.mesh_adjacency(copy)
    adj = MS.adjacency(fnp, V)
    for blend, facing, fill in (("weighted", True, 0), ("best", True, 3), ("weighted", False, 2)):
        got = G.paint_mesh(copy, views, normals=normals if facing else None, blend=blend, facing=facing, fill=fill,
                           adjacency=adjacency if fill == 3 else None, fallback=colors if fill else None, background=-1.0)
        assert isinstance(got, G.Painted) and not got.colors.requires_grad
        want = PR.paint(vn, _np(normals) if facing else None, restated, blend=blend, background=-1.0, rounds=fill, adj=adj,
                        fallback=_np(colors) if fill else None)
        for name in G.Painted._fields:
            _same(getattr(got, name), want[name], (blend, facing, fill, name))
        again = G.paint_mesh(copy, views, normals=normals if facing else None, blend=blend, facing=facing, fill=fill, fallback=colors if fill else None,
                             background=-1.0)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))
        seen, unseen = int((want["seen"] > 0).sum()), int((want["seen"] == 0).sum())
        assert int((got.seen > 0).sum()) == seen and int((got.seen == 0).sum()) == unseen and seen > 0
        per_view = [int(PR.paint(vn, _np(normals) if facing else None, [r], z_near=1e-3)["seen"].sum()) for r in restated]
        print(f"{blend}, facing {facing}, fill {fill}: {seen} of {V} vertices seen by some view, per view {per_view}; "
              f"{int((want['filled'] < 0).sum())} left uncoloured")
        if fill == 0:
            assert bool((got.colors[got.seen == 0] == -1.0).all()) and bool((got.filled == torch.where(got.seen > 0, 0, -1)).all())
            # what the views show is what was painted: the images are the mesh's own colours, so a seen vertex gets its colour back up
            # to the interpolation across the faces around it
            hit = got.seen > 0
            err = (got.colors[hit] - colors[hit]).abs().max(1).values
            print(f"{blend}: {seen} of {V} vertices seen ({unseen} by no view, {unseen / V:.1%}); |painted - own colour| median "
                  f"{float(err.median()):.2e} max {float(err.max()):.2e}")
        else:
            left = got.filled < 0
            assert torch.equal(got.colors[left], colors[left])


def test_paint_mesh_pieces_and_defaults(amd, dev):  # noqa: F811
    """Two pieces that share the pose give per-piece lists, equal to the restatement of the packed mesh; a view without a mask; the
    default tol is 0.01 obj_diag."""
    from supnerf_amd import geometry as G
    a_v, a_f = MS.box_mesh((0.25, 0.2, 0.15), 6)
    b_v, b_f = MS.noisy_sphere(level=2, radius=0.06)
    b_v = (b_v + np.array([0.0, -0.3, 0.1], F32)).astype(F32)
    pieces = [(_up(a_v, dev), _up(a_f, dev)), (_up(b_v, dev), _up(b_f, dev))]
    nv, nf = [len(a_v), len(b_v)], [len(a_f), len(b_f)]
    verts, faces = np.concatenate([a_v, b_v]), np.concatenate([a_f, b_f])
    rng = np.random.default_rng(8)
    views, restated = [], []
    for (eye, _), roi in zip(POSES[:2], ([80, 50, 240, 190], [85, 48, 236, 187])):
        pose = _look_at(eye)
        M, cam, (h, w), centre = _restated_view(pose, DIAG, VIEW_K, roi)
        img = rng.uniform(0, 1, (h, w, 3)).astype(F32)
        views.append(dict(img=torch.from_numpy(img), cam_pose=pose, obj_diag=DIAG, K=VIEW_K, roi=roi))
        ref = RR.rasterize(verts, faces, nv, nf, np.stack([M, M]), cam, h, w, cull_sign=[1, 1])
        restated.append(dict(screen=ref["screen"], depth=ref["depth"][0], image=img, mask=None, centre=centre, tol=0.01 * DIAG))
    got = G.paint_mesh(pieces, views, facing=False, fill=2, background=0.5)
    assert isinstance(got, list) and len(got) == 2 and all(isinstance(p, G.Painted) for p in got)
    want = PR.paint(verts, None, restated, background=0.5)
    start = 0
    for b, (p, n, fb) in enumerate(zip(got, nv, (a_f, b_f))):
        part = slice(start, start + n)
        c, fl = PR.fill(want["colors"][part], want["filled"][part], MS.adjacency(fb, n), 2)
        _same(p.colors, c, (b, "colors"))
        _same(p.filled, fl, (b, "filled"))
        for name in ("weight", "seen", "best"):
            _same(getattr(p, name), want[name][part], (b, name))
        start += n
    assert int((got[1].seen > 0).sum()) > 10 and int((got[0].seen == 2).sum()) > 10
    one = G.paint_mesh(pieces[0], views, facing=False, tol=0.01 * DIAG)
    assert isinstance(one, G.Painted) and one.colors.shape == (nv[0], 3)
    with pytest.raises(amd.SnrError, match="normals"):
        G.paint_mesh(pieces, views, normals=[torch.zeros(nv[0], 3, device=dev)])
    with pytest.raises(amd.SnrError):
        G.paint_mesh(pieces, views, facing=False, fallback=torch.zeros(nv[0], 3, device=dev))
