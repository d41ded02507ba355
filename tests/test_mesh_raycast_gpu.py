"""Mesh ray casting on the MI355X: ``snr_raycast_first`` / ``snr_raycast_crossings`` and ``geometry.ray_mesh`` / ``ray_crossings`` /
``visible`` / ``mesh_depth`` against tests/raycast_restatement.py.  The kernels run the restatement's float64 operations in its order:
integers are compared exactly, t bit for bit in float64, the weights bit for bit in fp32.

Every hand case and every walk case of the CPU tests, a packed launch of four objects with ragged ray counts into canary-filled outputs
with guard bands, an index of one cell against the default cell on 4096 rays, two runs bit for bit, a bad face index, non-finite vertices
and rays, an object without a usable grid; the autograd of ``ray_mesh`` on a tilted plane against the float64 closed form; ``visible`` on
the box; ``mesh_depth`` against ``rasterize`` on the same box, camera and image."""
import functools

import numpy as np
import pytest
import torch

import inside_restatement as IR
import raycast_restatement as RR
from segment_sum_restatement import banded, bands_intact
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = np.inf
NAN = float("nan")
EPS = 2.0 ** -24
HALF = (0.25, 0.2, 0.15)
CANARY = -7
KEYS = ("face", "t", "weights", "side", "signed", "total")


def _np(t):
    return t.detach().cpu().numpy()


def _t(x, dev, dtype=F32):  # noqa: F811
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)


def _to_gpu(mesh, dev):  # noqa: F811
    return _t(np.reshape(mesh[0], (-1, 3)), dev), _t(np.reshape(mesh[1], (-1, 3)), dev, np.int32)


def _bounds(v, n):
    return np.broadcast_to(np.asarray(v, F32), (n,)).copy()


def _same(got, want, keys=KEYS):
    """The keys on which two result dicts differ in any bit."""
    bits = {"t": np.int64, "weights": np.int32}
    return [k for k in keys if not np.array_equal(got[k].view(bits.get(k, got[k].dtype)), want[k].view(bits.get(k, want[k].dtype)))]


def _kernels(G, ops, mesh, o, d, lo, hi, cull, cell, dev):  # noqa: F811
    """Both kernels on one object through ``ops``, over the index of ``cell``: the dict of ``RR.brute_force``."""
    index = G.mesh_index(_to_gpu(mesh, dev), cell)
    n = len(o)
    args = (index.mesh, index.grid, _t(o, dev), _t(d, dev), _t(_bounds(lo, n), dev), _t(_bounds(hi, n), dev), [n])
    face, t, w, side = ops.mesh_raycast_first(*args, cull)
    signed, total = ops.mesh_raycast_crossings(*args)
    assert (face.dtype, t.dtype, w.dtype, side.dtype, signed.dtype, total.dtype) == \
        (torch.int32, torch.float64, torch.float32, torch.int8, torch.int32, torch.int32)
    return dict(face=_np(face), t=_np(t), weights=_np(w), side=_np(side), signed=_np(signed), total=_np(total))


def test_hand_cases(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G, ops
    for name, v, f, o, d, lo, hi, cull in RR.hand_cases():
        want = RR.brute_force(v, f, o, d, lo, hi, cull)
        extent = float(np.ptp(np.asarray(v, np.float64), axis=0).max())
        for cell in (None, extent / 3, extent * 4):
            got = _kernels(G, ops, (v, f), o, d, lo, hi, cull, cell, dev)
            assert _same(got, want) == [], (name, cell, _same(got, want))


def test_walk_cases(amd, dev):  # noqa: F811
    """Faces that span eight cells, rays from outside the grid, in cell planes, that miss the bounds, with t_max inside the object, one
    cell and the 256 clamp: the restatement's brute force, bit for bit, with culling too."""
    from supnerf_amd import geometry as G, ops
    for name, v, f, h, o, d, lo, hi in RR.walk_cases():
        for cull in (0, 1, 2) if name == "octahedron at 16 cells" else (0,):
            want = RR.brute_force(v, f, o, d, lo, hi, cull)
            got = _kernels(G, ops, (v, f), o, d, lo, hi, cull, h, dev)
            assert _same(got, want) == [], (name, cull, _same(got, want), np.nonzero(got["face"] != want["face"])[0][:8])


# ------------------------------------------------------------------ raw launches: packed objects, guard bands, bad inputs
def _raw(ops, lib, index, o, d, lo, hi, n_rays, dev, cull=0, verts=None, faces=None, cell=None):  # noqa: F811
    """Both entry points into canary-filled outputs with guard bands: (the result dict, the two flags, whether every band held)."""
    m, g = index.mesh, index.grid
    i32, i64 = torch.int32, torch.int64
    verts, faces, cell = m.verts if verts is None else verts, m.faces if faces is None else faces, g.cell if cell is None else cell
    nR = o.shape[0]
    roff = torch.tensor(np.concatenate([[0], np.cumsum(n_rays)]), dtype=i64).to(dev)
    shared = (ops._ptr(verts), ops._ptr(faces, i32), ops._ptr(m.vert_offset, i64), ops._ptr(m.face_offset, i64), ops._ptr(o), ops._ptr(d),
              ops._ptr(roff, i64), ops._ptr(lo), ops._ptr(hi), ops._ptr(cell), ops._ptr(g.grid_lo), ops._ptr(g.grid_hi),
              ops._ptr(g.cell_offset, i64), ops._ptr(g.cell_start, i64), ops._ptr(g.pair_face, i32), len(m.n_verts), verts.shape[0],
              faces.shape[0], nR, g.n_cells, g.n_pairs)
    bufs = {"face": banded(nR, i32, dev, CANARY), "t": banded(nR, torch.float64, dev, CANARY), "weights": banded(nR * 3, torch.float32, dev, CANARY),
            "side": banded(nR, torch.int8, dev, CANARY), "signed": banded(nR, i32, dev, CANARY), "total": banded(nR, i32, dev, CANARY),
            "bad1": banded(1, i32, dev, CANARY), "bad2": banded(1, i32, dev, CANARY)}
    bufs["bad1"][1].zero_(), bufs["bad2"][1].zero_()
    rc = lib.snr_raycast_first(*shared, cull, ops._ptr(bufs["face"][1], i32), ops._ptr(bufs["t"][1], torch.float64), ops._ptr(bufs["weights"][1]),
                               ops._ptr(bufs["side"][1], torch.int8), ops._ptr(bufs["bad1"][1], i32), ops._stream(dev))
    assert rc == 0
    rc = lib.snr_raycast_crossings(*shared, ops._ptr(bufs["signed"][1], i32), ops._ptr(bufs["total"][1], i32), ops._ptr(bufs["bad2"][1], i32),
                                   ops._stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    intact = all(bands_intact(full, mid.numel(), CANARY) for full, mid in bufs.values())
    out = {k: _np(bufs[k][1]) for k in KEYS}
    out["weights"] = out["weights"].reshape(-1, 3)
    return out, (int(bufs["bad1"][1].item()), int(bufs["bad2"][1].item())), intact


def _packed_want(meshes, rays, cull=0):
    parts = [RR.brute_force(m[0], m[1], o, d, lo, hi, cull) for m, (o, d, lo, hi) in zip(meshes, rays)]
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}


@functools.lru_cache(maxsize=None)
def _packed_case(counts=(255, 0, 257, 256)):
    """Box, octahedron, sphere and an object without faces, overlapping in space; ragged ray counts with a 0 among them: every block edge
    is straddled by two objects' rays, and every ray must see its own object only."""
    sv, sf, sq = IR.sphere_case()
    meshes = [IR.box12(HALF), IR.octahedron(0.3), (sv, sf), (sv[:5], np.zeros((0, 3), np.int32))]
    rng = np.random.default_rng(31)
    o, d = RR.aimed_rays(rng, sq[:768], -0.2, 0.2)
    o[:4] = [[NAN, 0, 0], [0, INF, 0], [0, 0, -1], [0, 0, -1]]
    d[2:6] = [[0, 0, 0], [0, NAN, 1], [0, 0, 0], [INF, 0, 0]]
    lo, hi = _bounds(0.0, 768), _bounds(INF, 768)
    lo[8:12], hi[8:12] = [NAN, 0.5, 2.0, 0.0], [INF, NAN, 1.0, 0.0]
    counts = list(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    assert off[-1] == 768
    rays = [(o[a:b], d[a:b], lo[a:b], hi[a:b]) for a, b in zip(off[:-1], off[1:])]
    return meshes, rays, counts, (o, d, lo, hi)


def test_packed_launch_ragged_counts_and_guard_bands(amd, dev):  # noqa: F811
    from supnerf_amd import _lib, geometry as G, ops
    meshes, rays, counts, (o, d, lo, hi) = _packed_case()
    index = G.mesh_index([_to_gpu(m, dev) for m in meshes], [0.1, 0.08, 0.05, 1.0])
    for cull in (0, 1):
        want = _packed_want(meshes, rays, cull)
        got, bad, intact = _raw(ops, _lib.lib(), index, _t(o, dev), _t(d, dev), _t(lo, dev), _t(hi, dev), counts, dev, cull)
        assert intact and bad == (0, 0)
        assert _same(got, want) == [], (cull, _same(got, want))                       # (every entry is written: no canary is left)
    assert (want["face"][:255] >= 0).sum() > 50 and (want["face"][255:512] >= 0).sum() > 50 and not (want["face"][512:] >= 0).any()
    dead = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]                                           # rays and bounds that are not finite, d = 0, t_min >= t_max
    assert not want["total"][dead].any() and (want["face"][dead] == -1).all() and want["total"][6] == 2
    # other counts: the octahedron is cast too, the object without faces at a block edge
    m2, rays2, counts2, _ = _packed_case((1, 256, 255, 256))
    want2 = _packed_want(m2, rays2)
    got2, bad, intact = _raw(ops, _lib.lib(), index, _t(o, dev), _t(d, dev), _t(lo, dev), _t(hi, dev), counts2, dev)
    assert intact and bad == (0, 0) and _same(got2, want2) == [] and (want2["face"][1:257] >= 0).sum() > 50
    # and through ops and the public API: the same
    a = ops.mesh_raycast_first(index.mesh, index.grid, _t(o, dev), _t(d, dev), _t(lo, dev), _t(hi, dev), counts, 1)
    assert np.array_equal(_np(a[0]), got["face"]) and np.array_equal(_np(a[1]).view(np.int64), got["t"].view(np.int64))
    ms = [_to_gpu(m, dev) for m in meshes]
    off = np.concatenate([[0], np.cumsum(counts)])
    cut = lambda x: [_t(x[a:b], dev) for a, b in zip(off[:-1], off[1:])]              # noqa: E731
    hits = G.ray_mesh(ms, cut(o), cut(d), t_min=cut(lo), t_max=cut(hi), cull="back", index=index)
    assert np.array_equal(np.concatenate([_np(h.face) for h in hits]), got["face"])
    assert np.array_equal(np.concatenate([_np(h.t) for h in hits]), got["t"].astype(F32))
    crossings = G.ray_crossings(ms, cut(o), cut(d), t_min=cut(lo), t_max=cut(hi), index=index)
    assert np.array_equal(np.concatenate([_np(c[0]) for c in crossings]), got["signed"])
    assert np.array_equal(np.concatenate([_np(c[1]) for c in crossings]), got["total"])


@pytest.mark.parametrize("n_rays", [0, 1, 63, 64, 65, 255, 256, 257])
def test_ray_counts_and_guard_bands(amd, dev, n_rays):  # noqa: F811
    from supnerf_amd import _lib, geometry as G, ops
    meshes, _, _, (o, d, lo, hi) = _packed_case()
    index = G.mesh_index(_to_gpu(meshes[2], dev), 0.06)
    s = slice(300, 300 + n_rays)
    got, bad, intact = _raw(ops, _lib.lib(), index, _t(o[s].reshape(-1, 3), dev), _t(d[s].reshape(-1, 3), dev), _t(lo[s], dev), _t(hi[s], dev),
                            [n_rays], dev)
    assert intact and bad == (0, 0) and _same(got, RR.brute_force(*meshes[2], o[s], d[s], lo[s], hi[s])) == []


def test_one_cell_against_the_default_cell_and_two_runs(amd, dev):  # noqa: F811
    """One cell per object is the brute force run through the same kernel: 4096 rays on the sphere give the same bits at the default
    cell, at a fine one, and again on a second run; the restatement's brute force agrees on the first 512."""
    from supnerf_amd import geometry as G, ops
    sv, sf, sq = IR.sphere_case()
    rng = np.random.default_rng(41)
    origins = np.concatenate([sq, rng.uniform(-0.6, 0.6, (4096 - len(sq), 3)).astype(F32)])
    o, d = RR.aimed_rays(rng, origins, -0.35, 0.35)
    assert len(o) == 4096
    runs = {cell: _kernels(G, ops, (sv, sf), o, d, 0.0, INF, 0, cell, dev) for cell in (4.0, None, 0.03)}
    assert G.mesh_index(_to_gpu((sv, sf), dev), 4.0).grid.n_cells == 1 and G.mesh_index(_to_gpu((sv, sf), dev)).grid.n_cells > 100
    for cell in (None, 0.03):
        assert _same(runs[cell], runs[4.0]) == [], cell
    assert _same(_kernels(G, ops, (sv, sf), o, d, 0.0, INF, 0, None, dev), runs[None]) == []
    want = RR.brute_force(sv, sf, o[:512], d[:512])
    assert _same({k: runs[None][k][:512] for k in KEYS}, want) == [] and (want["face"] >= 0).sum() > 300
    assert (runs[None]["face"] >= 0).sum() > 2500 and set(runs[None]["total"].tolist()) == {0, 1, 2}


def test_bad_index_non_finite_vertex_and_an_unusable_grid(amd, dev):  # noqa: F811
    """R5: a face index that goes bad after the index was built is skipped and flagged by the rays that meet it; a vertex that stops
    being finite has its faces skipped without a flag; an object whose cell is not positive gets nothing, and the flag."""
    from supnerf_amd import _lib, geometry as G, ops
    lib = _lib.lib()
    meshes, rays, counts, (o, d, lo, hi) = _packed_case()
    index = G.mesh_index([_to_gpu(m, dev) for m in meshes], [0.1, 0.08, 0.05, 1.0])
    want = _packed_want(meshes, rays)
    sv, sf = meshes[2]
    f0, v0 = len(meshes[0][1]) + len(meshes[1][1]), len(meshes[0][0]) + len(meshes[1][0])
    k = int(np.nonzero(want["face"][255:512] >= 0)[0][3])                              # a ray of the sphere that hits
    hit = int(want["face"][255 + k])
    broken = np.concatenate([m[1] for m in meshes]).astype(np.int32)
    broken[f0 + hit, 1] = 10 ** 6
    broken[f0 + (hit + 1) % 320, 2] = -1
    args = (_t(o, dev), _t(d, dev), _t(lo, dev), _t(hi, dev), counts, dev)
    got, bad, intact = _raw(ops, lib, index, *args, faces=torch.from_numpy(broken).to(dev))
    ref = RR.brute_force(sv, broken[f0:f0 + 320], *rays[2])
    assert intact and bad == (1, 1) and RR.bad_flag(sv, broken[f0:f0 + 320]) and ref["face"][k] != hit
    assert _same({k: got[k][255:512] for k in KEYS}, ref) == []
    assert _same({k: np.concatenate([got[k][:255], got[k][512:]]) for k in KEYS}, {k: np.concatenate([want[k][:255], want[k][512:]]) for k in KEYS}) == []
    nan = np.concatenate([m[0] for m in meshes]).astype(F32)
    nan[v0 + sf[hit, 0], 1] = NAN
    nan[v0 + sf[(hit + 7) % 320, 2], 2] = INF
    got, bad, intact = _raw(ops, lib, index, *args, verts=torch.from_numpy(nan).to(dev))
    ref = RR.brute_force(nan[v0:v0 + len(sv)], sf, *rays[2])
    assert intact and bad == (0, 0) and ref["face"][k] != hit and _same({k: got[k][255:512] for k in KEYS}, ref) == []
    cell = index.grid.cell.clone()
    cell[2] = 0.0
    got, bad, intact = _raw(ops, lib, index, *args, cell=cell)
    assert intact and bad == (1, 1) and (got["face"][255:512] == -1).all() and not got["total"][255:512].any() and np.isinf(got["t"][255:512]).all()
    assert _same({k: got[k][:255] for k in KEYS}, {k: want[k][:255] for k in KEYS}) == []


# ------------------------------------------------------------------ ray_mesh: autograd
PLANE = (np.array([[-1, -1, -0.4], [1, -1, 0.2], [1, 1, 0.6], [-1, 1, 0.0]], F32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))     # z = 0.3 x + 0.2 y + 0.1


def _abs_plane_grads(o, d, a, b, c):
    """``RR.plane_depth``'s gradients with every difference of products replaced by the sum of their magnitudes: what one relative
    rounding of every operation can move each gradient by, to first order, is a small multiple of e times this."""
    o, d, a, b, c = (np.asarray(x, np.float64) for x in (o, d, a, b, c))
    cross = lambda x, y: np.array([x[1] * y[2] + x[2] * y[1], x[2] * y[0] + x[0] * y[2], x[0] * y[1] + x[1] * y[0]])      # noqa: E731
    e1, e2, am, da = np.abs(b - a), np.abs(c - a), np.abs(a - o), np.abs(d)
    n = cross(e1, e2)
    nd = abs(np.cross(b - a, c - a) @ d)
    kappa = (n @ da) / nd                                                              # how much the denominator cancels
    t = n @ am / nd
    gn = (am + t * da) / nd
    return kappa, (n / nd, t * n / nd, n / nd + cross(e1, gn) + cross(e2, gn), cross(e2, gn), cross(e1, gn))


def test_ray_mesh_autograd_on_a_tilted_plane(amd, dev):  # noqa: F811
    """dt/do, dt/dd and dt/dverts of ``ray_mesh`` on a plane of two triangles against the float64 closed form of a ray-plane depth
    (``RR.plane_depth``, checked against differences on the CPU).  torch forms t = n . (a - o) / (n . d) and its backward in fp32: about
    16 operations on the way to t and as many on the way back, each one relative rounding e = 2^-24 of its own result.  To first order
    such a rounding moves a gradient by at most e times the gradient formula evaluated on magnitudes (``_abs_plane_grads``), and by kappa
    times that where it goes through the cancelling denominator n . d.  Band: 32 e kappa |formula|.  Misses get exact zeros."""
    from supnerf_amd import geometry as G
    v, f = PLANE
    rng = np.random.default_rng(51)
    o = np.c_[rng.uniform(-0.6, 0.6, (24, 2)), rng.uniform(1.0, 2.0, 24)].astype(F32)
    d = np.c_[rng.uniform(-0.1, 0.1, (24, 2)), -rng.uniform(0.8, 1.5, 24)].astype(F32)
    o[20:], d[20:] = [[3, 0, 1], [0, 3, 1], [0, 0, 1], [0, 0, -1]], [[0, 0, -1], [0, 0, -1], [0, 0, 1], [1, 0, 0]]            # misses
    want = RR.brute_force(v, f, o, d)
    assert (want["face"][:20] >= 0).all() and (want["face"][20:] == -1).all() and set(want["face"][:20].tolist()) == {0, 1}
    to, td, tv = _t(o, dev).requires_grad_(), _t(d, dev).requires_grad_(), _t(v, dev).requires_grad_()
    hits = G.ray_mesh((tv, _t(f, dev, np.int32)), to, td)
    assert hits.t.requires_grad and not hits.weights.requires_grad and hits.face.dtype == torch.int32 and hits.side.dtype == torch.int8
    assert np.array_equal(_np(hits.face), want["face"]) and np.array_equal(_np(hits.side), want["side"])
    assert np.array_equal(_np(hits.weights).view(np.int32), want["weights"].view(np.int32))
    t = _np(hits.t).astype(np.float64)
    assert np.isinf(t[20:]).all() and np.abs(t[:20] - want["t"][:20]).max() <= 16 * EPS * np.abs(want["t"][:20]).max()
    coef = rng.uniform(0.5, 1.5, 24)
    go, gd, gv = (_np(x).astype(np.float64) for x in torch.autograd.grad(hits.t, (to, td, tv), grad_outputs=_t(coef, dev)))
    assert not go[20:].any() and not gd[20:].any() and np.isfinite(gv).all()          # misses: exact zeros
    want_v, band_v, worst = np.zeros((4, 3)), np.zeros((4, 3)), 0.0
    v64 = v.astype(np.float64)
    for r in range(20):
        idx = f[want["face"][r]]
        _, grads = RR.plane_depth(o[r], d[r], *v64[idx])
        kappa, mags = _abs_plane_grads(o[r], d[r], *v64[idx])
        for got, g, mag in ((go[r], grads[0], mags[0]), (gd[r], grads[1], mags[1])):
            band = 32 * EPS * kappa * mag * coef[r]
            worst = max(worst, float((np.abs(got - coef[r] * g) / band).max()))
            assert (np.abs(got - coef[r] * g) <= band).all(), (r, got, coef[r] * g, band)
        for k in range(3):
            want_v[idx[k]] += coef[r] * grads[2 + k]
            band_v[idx[k]] += 32 * EPS * kappa * mags[2 + k] * coef[r]
    worst_v = float((np.abs(gv - want_v) / band_v).max())
    print(f"ray_mesh autograd: worst |gradient - closed form| / band: rays {worst:.3f}, vertices {worst_v:.3f}")
    assert (np.abs(gv - want_v) <= band_v).all() and np.abs(want_v).max() > 0.1
    # without grad: the kernel's float64 t rounded once; point and normal; face_forward
    with torch.no_grad():
        plain = G.ray_mesh((tv, _t(f, dev, np.int32)), to, td, face_forward=True)
    assert np.array_equal(_np(plain.t), want["t"].astype(F32)) and not plain.t.requires_grad
    p = _np(plain.point).astype(np.float64)
    assert np.abs(p[:20] - (o[:20] + want["t"][:20, None] * d[:20])).max() < 1e-6 and np.isinf(p[20:]).all()
    n = np.array([-0.3, -0.2, 1.0]) / np.linalg.norm([-0.3, -0.2, 1.0])               # both faces wind counter-clockwise seen from +z
    assert np.abs(_np(plain.normal)[:20] - n).max() < 1e-6 and not _np(plain.normal)[20:].any()
    below = G.ray_mesh((tv.detach(), _t(f, dev, np.int32)), _t([[0, 0, -1.0]], dev), _t([[0, 0, 1.0]], dev))
    flipped = G.ray_mesh((tv.detach(), _t(f, dev, np.int32)), _t([[0, 0, -1.0]], dev), _t([[0, 0, 1.0]], dev), face_forward=True)
    assert int(below.side) == -1 and np.abs(_np(below.normal)[0] - n).max() < 1e-6 and np.abs(_np(flipped.normal)[0] + n).max() < 1e-6


# ------------------------------------------------------------------ visible
def test_visible_on_the_box(amd, dev):  # noqa: F811
    """From an eye in front of the +x face: the centre of that face is visible, the centre of the back face is not; of the eight
    vertices -- all on the silhouette or in front, none hidden by their own faces at offset 0 (R4) -- only those whose segment runs
    through the box are hidden; and points placed so that their segment passes through a silhouette vertex or edge midpoint (up to the
    rounding of the frame's two quotients) get what R2 gives the restatement."""
    from supnerf_amd import geometry as G
    bv, bf = IR.box12(RR.DYADIC_HALF)
    mesh = _to_gpu((bv, bf), dev)
    eye = np.array([2.0, 0.0, 0.0])
    centres = np.array([[0.25, 0, 0], [-0.25, 0, 0], [0.25, 0.0625, -0.25]], F32)
    assert _np(G.visible(mesh, _t(centres, dev), _t(eye, dev))).tolist() == [True, False, True]
    corners = bv.astype(np.float64)
    edges = np.array([(corners[i] + corners[j]) / 2 for i in range(8) for j in range(i + 1, 8) if bin(i ^ j).count("1") == 1])
    through = np.concatenate([corners, edges])
    behind = (through - 0.5 * (eye - through)).astype(F32)                            # (few-bit numbers: exact)
    assert np.array_equal(behind.astype(np.float64), 1.5 * through - 0.5 * eye)
    pts = np.concatenate([bv, behind])
    want = RR.brute_force(bv, bf, pts, (eye - pts.astype(np.float64)).astype(F32), 0.0, 1.0)["face"] < 0
    got = _np(G.visible(mesh, _t(pts, dev), _t(eye, dev)))
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert got[:8].tolist() == (bv[:, 0] > 0).tolist()                                # the vertices of the +x face see the eye, the others do not
    assert 0 < got[8:].sum() < len(got[8:])
    # one eye per point, an offset that skips the whole box, and several meshes
    eyes = np.broadcast_to(eye, pts.shape).astype(F32)
    assert np.array_equal(_np(G.visible(mesh, _t(pts, dev), _t(eyes, dev))), want)
    assert _np(G.visible(mesh, _t(pts, dev), _t(eye, dev), offset=0.999)).all()
    both = G.visible([mesh, mesh], [_t(pts, dev), _t(centres, dev)], _t(eye, dev))
    assert np.array_equal(_np(both[0]), want) and _np(both[1]).tolist() == [True, False, True]


# ------------------------------------------------------------------ mesh_depth against rasterize
DEPTH_DIAG = 1.5
DEPTH_ROI = [0, 0, 64, 64]


def _look_at(eye, up=(0.0, 0.0, 1.0)):
    """(3, 4) float32 camera pose in the object's frame: at ``eye``, looking at the origin; columns x right, y down, z forward."""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(F32)


def _segment_distance(P, A, B):
    ab = B - A
    s = np.clip(((P - A) @ ab) / (ab @ ab), 0, 1)
    return np.linalg.norm(P - (A + s[:, None] * ab), axis=1)


def _depth_geometry(pose, K):
    """From the vertices alone, in float64: per pixel of the 64 x 64 image whether a projected face covers its centre, whether the centre
    lies within 1/8 pixel of a projected edge (of any face, hidden ones too), and the camera-frame vertices."""
    P = pose.astype(np.float64)
    v, f = IR.box12(HALF)
    cam = (v.astype(np.float64) * DEPTH_DIAG - P[:, 3]) @ P[:, :3]                   # R^T (x - c): the pose is a rotation
    uv = np.stack([K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]], 1)
    ys, xs = np.mgrid[0:64, 0:64]
    px = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    covered, near = np.zeros(len(px), bool), np.zeros(len(px), bool)
    for tri in f:
        a, b, c = uv[tri]
        side = np.stack([(q[0] - p[0]) * (px[:, 1] - p[1]) - (q[1] - p[1]) * (px[:, 0] - p[0]) for p, q in ((a, b), (b, c), (c, a))])
        covered |= (side > 0).all(0) | (side < 0).all(0)
        for p, q in ((a, b), (b, c), (c, a)):
            near |= _segment_distance(px, p, q) <= 0.125
    return covered.reshape(64, 64), near.reshape(64, 64), cam


@pytest.mark.parametrize("eye,focal", [((1.5, 0.0, 0.0), 105.0), ((2.1, -1.3, 0.9), 150.0)])
def test_mesh_depth_against_rasterize(amd, dev, eye, focal):  # noqa: F811
    """The same box, camera and 64 x 64 image through ``mesh_depth`` (exact rays) and ``rasterize`` (vertices snapped to 1/256 pixel).
    On the covered pixels whose centre lies more than 1/8 pixel -- 32 snaps -- from every projected edge (more than 90 % of them, counted
    from the geometry alone) both name the same face, and ``mesh_depth``'s depth along the unit view direction, divided in float64 by
    |((px - cx) / fx, (py - cy) / fy, 1)|, is ``Raster.depth``.

    Band.  Frontal view (the eye on the +x axis: one face is seen and its camera z is one number, so where the snapped vertices lie
    does not matter): the fp32 roundings alone -- the rasteriser's rule 1 (4) and rule 5 (7), ``get_rays``' direction (each component
    within about 4 e, which moves the hit sideways by 8 e depth and the depth by that times the slope, below 1 here), the origin's
    division by obj_diag, t's one rounding and the product with obj_diag: 24 e z.  Oblique view (three faces seen): the rasteriser's
    depth is the exact camera z at a point up to 1/512 pixel away in u and in v (a convex combination of vertices that each moved by
    at most that), so the band grows by (|dz/du| + |dz/dv|) / 512, the slopes taken from the face's plane at the pixel."""
    from supnerf_amd import geometry as G
    pose = _look_at(eye)
    K = np.array([[focal, 0, 31.3], [0, focal, 31.7], [0, 0, 1]])
    covered, near, cam = _depth_geometry(pose, K)
    keep = covered & ~near
    assert covered.sum() > 1700 and keep.sum() >= 0.9 * covered.sum(), (covered.sum(), keep.sum())
    v, f = IR.box12(HALF)
    mesh = _to_gpu((v, f), dev)
    cam_pose = torch.from_numpy(pose).to(dev)
    depth, hits = G.mesh_depth(mesh, cam_pose, DEPTH_DIAG, torch.from_numpy(K).float(), DEPTH_ROI)
    assert tuple(depth.shape) == (64, 64) and tuple(hits.point.shape) == (64, 64, 3) and hits.face.dtype == torch.int32
    P = pose.astype(np.float64)
    r_inv = np.linalg.inv(P[:, :3])
    M = np.concatenate([r_inv * DEPTH_DIAG, -(r_inv @ P[:, 3:4])], 1).astype(F32)
    raster = G.rasterize(mesh, torch.from_numpy(M).to(dev), (focal, focal, 31.3, 31.7), (64, 64), cull="back")
    face_r, face_m = _np(raster.face[0]), _np(hits.face)
    assert np.array_equal(face_m[keep], face_r[keep]) and (face_r[keep] >= 0).all()
    print(f"eye {eye}: {covered.sum()} covered pixels, {keep.sum()} compared; faces differ on {(face_m != face_r).sum()} of all pixels")
    assert (_np(hits.side)[keep] == 1).all() and np.isinf(_np(depth)[~covered & ~near]).all()
    ys, xs = np.mgrid[0:64, 0:64]
    du, dv = (xs - 31.3) / focal, (ys - 31.7) / focal
    z_m = _np(depth).astype(np.float64) / np.sqrt(du ** 2 + dv ** 2 + 1.0)
    z_r = _np(raster.depth[0]).astype(np.float64)
    band = 24 * EPS * z_r
    if eye[1] != 0.0:
        tri = cam[f[np.maximum(face_r, 0)]]                                          # (64, 64, 3 corners, 3): the face's plane n . X = c
        n = np.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])
        c = (n * tri[..., 0, :]).sum(-1)
        q = n[..., 0] * du + n[..., 1] * dv + n[..., 2]                               # z = c / q
        band = band + (np.abs(c * n[..., 0] / q ** 2) + np.abs(c * n[..., 1] / q ** 2)) / focal / 512
    err = np.abs(z_m - z_r)
    print(f"  worst |camera z of mesh_depth - Raster.depth| / band on the compared pixels: {(err / band)[keep].max():.3f}")
    assert (err[keep] <= band[keep]).all()
    # listed pixels: the same depths; gradients reach the pose and the vertices
    pix = (np.array([20, 31, 40]), np.array([25, 31, 38]))
    tv = mesh[0].clone().requires_grad_()
    tp = cam_pose.clone().requires_grad_()
    d3, h3 = G.mesh_depth((tv, mesh[1]), tp, DEPTH_DIAG, torch.from_numpy(K).float(), DEPTH_ROI, pixels=pix)
    assert tuple(d3.shape) == (3,) and np.abs(_np(d3) - _np(depth)[pix[1], pix[0]]).max() <= 16 * EPS * 3
    d3.sum().backward()
    assert tv.grad is not None and tp.grad is not None and float(tv.grad.abs().sum()) > 0 and float(tp.grad.abs().sum()) > 0
