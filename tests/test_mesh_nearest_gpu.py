"""Mesh distance on the MI355X: the ``snr_nearest_*`` / ``snr_surface_sample`` kernels and ``geometry.closest_point`` / ``sample_surface``
/ ``mesh_distance`` against tests/nearest_restatement.py.  The kernels run the restatement's float64 operations in its order, so ``face``,
``dist2``, the weights and the sample points are compared bit for bit; ``distance`` (a float64 square root rounded to fp32) within one
fp32 ulp; the per-object sums of ``mesh_distance`` bit for bit against the fixed-order segmented sum.

Hand cases, the box at one cell and at several cell sizes, a packed launch of three objects (one empty), faces without area, a bad
face index and non-finite queries, guard bands around every output of the C ABI, two runs bit for bit, the gradient of the distance,
``mesh_distance`` on two offset boxes and ``sample_surface`` from the device's own cumulative areas.  The largest mesh has 768 faces."""
import functools

import numpy as np
import pytest
import torch

import nearest_restatement as NR
import segment_sum_restatement as SS
import simplify_restatement as SR
from segment_sum_restatement import banded, bands_intact, same_bits
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
HALF = (0.25, 0.2, 0.15)
DELTA = 2.0 ** -6
NAN = float("nan")


def _np(t):
    return t.detach().cpu().numpy()


def _to_gpu(mesh, dev):  # noqa: F811
    return (torch.from_numpy(np.ascontiguousarray(mesh[0], F32).reshape(-1, 3)).to(dev),
            torch.from_numpy(np.ascontiguousarray(mesh[1], np.int32).reshape(-1, 3)).to(dev))


@functools.lru_cache(maxsize=None)
def _box():
    """The box, the 450 shared queries and their brute-force answer, computed once."""
    verts, faces = SR.box_mesh(HALF, 8)
    queries = NR.box_queries(HALF)
    return verts, faces, queries, NR.brute_force(verts, faces, queries)


def _kernel(G, ops, meshes, points, cell):
    """(face, weights, dist2) as numpy lists per object, straight from ``snr_nearest_query`` over the index of ``cell``."""
    index = G.mesh_index(meshes, cell)
    nqs = [p.shape[0] for p in points]
    face, weights, dist2 = ops.mesh_nearest_query(index.mesh, index.grid, torch.cat(points), nqs)
    off = np.concatenate([[0], np.cumsum(nqs)])
    return [dict(face=_np(face)[a:b], weights=_np(weights)[a:b], dist2=_np(dist2)[a:b]) for a, b in zip(off[:-1], off[1:])], index


def _assert_same(got, ref, tag):
    assert got["face"].dtype == np.int32 and got["weights"].dtype == F32 and got["dist2"].dtype == np.float64, tag
    assert np.array_equal(got["face"], ref["face"]), (tag, np.nonzero(got["face"] != ref["face"])[0][:10])
    assert same_bits(got["dist2"], ref["dist2"]).all(), (tag, "dist2")
    assert same_bits(got["weights"], ref["weights"]).all(), (tag, "weights")


def _ulps(got, want64):
    want = np.asarray(want64, np.float64).astype(F32)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
    return np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) / np.spacing(np.maximum(np.abs(want[fin]), np.finfo(F32).tiny))


def test_hand_cases(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G, ops
    tri = _to_gpu((NR.TRI, [[0, 1, 2]]), dev)
    pts = np.array([p for p, _, _, _ in NR.REGIONS], F32)
    for cell in (8.0, 0.25, None):
        (got,), _ = _kernel(G, ops, [tri], [torch.from_numpy(pts).to(dev)], cell)
        _assert_same(got, NR.brute_force(NR.TRI, [[0, 1, 2]], pts), f"triangle at cell {cell}")
        assert got["dist2"].tolist() == [d2 for _, _, _, d2 in NR.REGIONS]
        assert got["weights"].tolist() == [list(map(float, w)) for _, _, w, _ in NR.REGIONS]
    # a face exactly in a cell plane and an exact tie behind it; two faces that share an edge, the query above it
    sv, sf, sq = NR.sheets_mesh()
    (got,), _ = _kernel(G, ops, [_to_gpu((sv, sf), dev)], [torch.from_numpy(sq).to(dev)], 0.25)
    _assert_same(got, NR.brute_force(sv, sf, sq), "sheets")
    assert got["face"].tolist() == [0] and got["dist2"].tolist() == [2.0 ** -8]
    rv, rf = NR.roof_mesh()
    rq = np.array([[0.5, 0.0, 1.0], [0.25, 0.0, 0.5]], F32)
    for cell in (4.0, 0.5):
        (got,), _ = _kernel(G, ops, [_to_gpu((rv, rf), dev)], [torch.from_numpy(rq).to(dev)], cell)
        _assert_same(got, NR.brute_force(rv, rf, rq), f"roof at {cell}")
        assert got["face"].tolist() == [0, 0]


def test_box_at_every_grid_size(amd, dev):  # noqa: F811
    """One cell is the brute force of the same kernel; every other grid gives its bits, and the restatement's.  Run twice: same bits."""
    from supnerf_amd import geometry as G, ops
    verts, faces, queries, brute = _box()
    mesh, pts = _to_gpu((verts, faces), dev), torch.from_numpy(queries).to(dev)
    (one,), index = _kernel(G, ops, [mesh], [pts], 1.0)
    assert index.grid.n_cells == 1 and index.grid.n_pairs == 768
    _assert_same(one, brute, "one cell")
    for cell in (0.5 / 4, float(F32(0.5 / 9)), 0.03, 0.011, None):
        (got,), index = _kernel(G, ops, [mesh], [pts], cell)
        g = NR.grid(verts, _np(index.grid.cell)[0])
        assert index.grid.n_cells == int(g["n"].prod()) and index.grid.n_pairs == int(NR.cell_counts(verts, faces, g).sum()), cell
        _assert_same(got, one, f"cell {cell} against one cell")
        _assert_same(got, brute, f"cell {cell}")
        (again,), _ = _kernel(G, ops, [mesh], [pts], cell)
        _assert_same(again, got, f"cell {cell}, second run")
    # the lists themselves: sorted by cell, faces ascending within a cell
    index = G.mesh_index(mesh, 0.125)
    g = NR.grid(verts, 0.125)
    lists = NR.cell_lists(verts, faces, g)
    start, pf = _np(index.grid.cell_start), _np(index.grid.pair_face)
    assert start.dtype == np.int64 and pf.dtype == np.int32 and start[0] == 0 and start[-1] == len(pf)
    for c in range(index.grid.n_cells):
        assert pf[start[c]:start[c + 1]].tolist() == lists.get(c, []), c


def test_closest_point_values(amd, dev):  # noqa: F811
    """``geometry.closest_point`` without autograd: the kernel's face and weights, the point from them, the distance within one ulp."""
    from supnerf_amd import geometry as G
    verts, faces, queries, brute = _box()
    mesh, pts = _to_gpu((verts, faces), dev), torch.from_numpy(queries).to(dev)
    got = G.closest_point(mesh, pts)
    assert isinstance(got, G.Closest) and got.distance.dtype == torch.float32 and not got.distance.requires_grad
    assert np.array_equal(_np(got.face), brute["face"]) and same_bits(_np(got.weights), brute["weights"]).all()
    ulps = _ulps(_np(got.distance), np.sqrt(brute["dist2"]))
    print("distance: worst", ulps.max(), "ulp")
    assert ulps.max() <= 1.0
    # the point: three fp32 products and two adds of coordinates below 1/2: 3 ulp of 1/2 at the most
    assert np.abs(_np(got.point).astype(np.float64) - NR.closest_points(verts, faces, brute)).max() <= 3 * 2.0 ** -25
    many = G.closest_point([mesh, mesh], [pts[:50], pts[50:120]], index=G.mesh_index([mesh, mesh], [0.1, 0.07]))
    assert np.array_equal(_np(many[0].face), brute["face"][:50]) and np.array_equal(_np(many[1].face), brute["face"][50:120])
    assert torch.equal(many[1].distance, got.distance[50:120])


def test_packed_launch(amd, dev):  # noqa: F811
    """Three objects with different scales and cells, one of them empty, overlapping in space: every query sees its own object only."""
    from supnerf_amd import geometry as G, ops
    verts, faces, queries, brute = _box()
    big = ((verts * F32(8.0) + F32(0.05)).astype(F32), faces)
    rv, rf = NR.roof_mesh()
    roof = ((rv * F32(0.25)).astype(F32), rf)                                    # inside the region the box's queries cover
    empty = (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32))
    meshes = [(verts, faces), empty, big, roof]
    points = [queries[:200], queries[200:230], (queries[230:] * F32(8.0)).astype(F32), queries[:200]]
    cells = [0.06, 1.0, 0.9, 0.2]
    got, index = _kernel(G, ops, [_to_gpu(m, dev) for m in meshes], [torch.from_numpy(p).to(dev) for p in points], cells)
    assert index.grid.cell_offset.tolist()[:3] == [0, int(NR.grid(verts, 0.06)["n"].prod()), int(NR.grid(verts, 0.06)["n"].prod()) + 1]
    for b, (m, p) in enumerate(zip(meshes, points)):
        ref = brute if b == 0 else NR.brute_force(m[0], m[1], p)
        _assert_same(got[b], {k: (v[:200] if b == 0 else v) for k, v in ref.items()}, f"object {b}")
    assert (got[1]["face"] == -1).all() and np.isinf(got[1]["dist2"]).all() and (got[1]["weights"] == 0).all()
    assert (got[3]["face"] >= 0).all() and not np.array_equal(got[3]["dist2"], got[0]["dist2"])
    out = G.closest_point([_to_gpu(m, dev) for m in meshes], [torch.from_numpy(p).to(dev) for p in points])
    assert (out[1].face == -1).all() and torch.isinf(out[1].distance).all() and (out[1].point == 0).all()
    assert np.array_equal(_np(out[2].face), got[2]["face"])


def test_faces_without_area_and_non_finite_input(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G, ops
    verts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [0.5, 0.5, 0.5], [3, 3, 3], [0, 0, 2], [1, 0, 2], [0, 1, 2]], F32)
    faces = np.array([[0, 0, 1], [4, 4, 4], [0, 1, 2], [2, 0, 1], [1, 2, 0], [5, 5, 3], [6, 7, 8]], np.int32)
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.integers(-16, 33, (150, 3)) / 8.0, rng.uniform(-1, 4, (50, 3))]).astype(F32)
    pts[:6] = [[NAN, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.5, 0.5, 0.5], [1.5, 2, 0], [3, 3, 3]]
    ref = NR.brute_force(verts, faces, pts)
    assert ref["face"][:3].tolist() == [-1, -1, -1] and np.isfinite(ref["dist2"][3:]).all() and ref["dist2"][3] == 0.0
    for cell in (8.0, 0.5, None):
        (got,), _ = _kernel(G, ops, [_to_gpu((verts, faces), dev)], [torch.from_numpy(pts).to(dev)], cell)
        _assert_same(got, ref, f"degenerate faces at cell {cell}")
    out = G.closest_point(_to_gpu((verts, faces), dev), torch.from_numpy(pts).to(dev))
    assert out.face[:3].tolist() == [-1, -1, -1] and torch.isinf(out.distance[:3]).all() and (out.weights[:3] == 0).all()
    # a mesh of faces without area only still answers (the default cell falls back to one cell)
    (got,), index = _kernel(G, ops, [_to_gpu((verts, faces[:5]), dev)], [torch.from_numpy(pts).to(dev)], None)
    _assert_same(got, NR.brute_force(verts, faces[:5], pts), "no area at all")


def _raw(ops, lib, index, points, nqs, dev, faces=None):  # noqa: F811
    """``snr_nearest_query`` with guard bands around every output; returns the outputs, the flag and whether the bands held."""
    m, g = index.mesh, index.grid
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    faces = m.faces if faces is None else faces
    nQ = points.shape[0]
    qoff = torch.tensor(np.concatenate([[0], np.cumsum(nqs)]), dtype=i64).to(dev)
    (ff, face), (wf, w), (df, d2), (bf, bad) = banded(nQ, i32, dev, -7), banded(nQ * 3, torch.float32, dev, NAN), banded(nQ, f64, dev, NAN), \
        banded(1, i32, dev, -7)
    bad.zero_()
    rc = lib.snr_nearest_query(ops._ptr(m.verts), ops._ptr(faces, i32), ops._ptr(m.vert_offset, i64), ops._ptr(m.face_offset, i64),
                               ops._ptr(points), ops._ptr(qoff, i64), ops._ptr(g.cell), ops._ptr(g.grid_lo), ops._ptr(g.grid_hi),
                               ops._ptr(g.cell_offset, i64), ops._ptr(g.cell_start, i64), ops._ptr(g.pair_face, i32), len(m.n_verts),
                               m.verts.shape[0], faces.shape[0], nQ, g.n_cells, g.n_pairs, ops._ptr(face, i32), ops._ptr(w), ops._ptr(d2, f64),
                               ops._ptr(bad, i32), ops._stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    intact = bands_intact(ff, nQ, -7) and bands_intact(wf, nQ * 3, NAN) and bands_intact(df, nQ, NAN) and bands_intact(bf, 1, -7)
    return dict(face=_np(face), weights=_np(w).reshape(-1, 3), dist2=_np(d2)), int(bad.item()), intact


def test_bad_index_and_guard_bands(amd, dev, monkeypatch):  # noqa: F811
    from supnerf_amd import _lib, geometry as G, ops
    lib = _lib.lib()
    verts, faces, queries, brute = _box()
    mesh, pts = _to_gpu((verts, faces), dev), torch.from_numpy(queries[:257]).to(dev)            # (one block and one thread)
    index = G.mesh_index(mesh, 0.09)
    got, bad, intact = _raw(ops, lib, index, pts, [257], dev)
    assert intact and bad == 0
    _assert_same(got, {k: v[:257] for k, v in brute.items()}, "guard bands")
    # a face index that goes bad after the index was built: skipped, flagged, the other faces unaffected
    broken = faces.copy()
    broken[brute["face"][0], 1] = 10 ** 6
    broken[brute["face"][5], 2] = -1
    got, bad, intact = _raw(ops, lib, index, pts, [257], dev, faces=torch.from_numpy(broken).to(dev))
    ref = NR.brute_force(verts, broken, queries[:257])
    assert intact and bad == 1 and ref["face"][0] != brute["face"][0]
    _assert_same(got, ref, "a bad face index")
    with pytest.raises(amd.SnrError, match="face index"):
        G.mesh_index((mesh[0], torch.from_numpy(broken).to(dev)), 0.09)
    nan = verts.copy()
    nan[3, 1] = NAN
    with pytest.raises(amd.SnrError, match="not finite"):
        G.mesh_index(_to_gpu((nan, faces), dev), 0.09)
    for cell in (0.0, -1.0, NAN, float("inf")):
        with pytest.raises(amd.SnrError, match="cell"):
            G.mesh_index(mesh, cell)
        with pytest.raises(amd.SnrError, match="cell"):
            G.mesh_index(mesh, torch.tensor([cell], device=dev))
    # the count and emit passes, banded: counts of the restatement, 0 and the flag for the bad faces
    i32, i64 = torch.int32, torch.int64
    g = NR.grid(verts, 0.09)
    m, gr = index.mesh, index.grid
    for f_np, want_bad in ((faces, 0), (broken, 1)):
        f_t = torch.from_numpy(f_np).to(dev)
        (cf, count), flag = banded(768, i32, dev, -7), torch.zeros(1, dtype=i32, device=dev)
        args = (ops._ptr(m.verts), ops._ptr(f_t, i32), ops._ptr(m.vert_offset, i64), ops._ptr(m.face_offset, i64), ops._ptr(gr.cell),
                ops._ptr(gr.grid_lo), ops._ptr(gr.grid_hi), ops._ptr(gr.cell_offset, i64))
        assert lib.snr_nearest_count(*args, 1, m.verts.shape[0], 768, gr.n_cells, ops._ptr(count, i32), ops._ptr(flag, i32), ops._stream(dev)) == 0
        want = NR.cell_counts(verts, f_np, g)
        assert bands_intact(cf, 768, -7) and int(flag.item()) == want_bad and np.array_equal(_np(count), want)
        n_pairs = int(want.sum())
        scan = torch.from_numpy(np.concatenate([[0], np.cumsum(want)[:-1]]).astype(np.int64)).to(dev)
        (pcf, pc), (pff, pf) = banded(n_pairs, i64, dev, -7), banded(n_pairs, i32, dev, -7)
        assert lib.snr_nearest_emit(*args, ops._ptr(scan, i64), 1, m.verts.shape[0], 768, gr.n_cells, n_pairs, ops._ptr(pc, i64), ops._ptr(pf, i32),
                                    ops._stream(dev)) == 0
        cells, fs = NR.pairs(verts, f_np, g)
        assert bands_intact(pcf, n_pairs, -7) and bands_intact(pff, n_pairs, -7)
        assert np.array_equal(_np(pc), cells) and np.array_equal(_np(pf), fs)
    # the pair limit: the error names a cell size, and that size fits
    monkeypatch.setattr(ops, "NEAREST_MAX_PAIRS", 2000)
    with pytest.raises(amd.SnrError, match="times as large") as err:
        G.mesh_index(mesh, 0.02)
    factor = float(str(err.value).split("cells ")[1].split(" times")[0])
    assert factor > 1 and G.mesh_index(mesh, 0.02 * factor * 1.001).grid.n_pairs <= 2000


def test_distance_gradient(amd, dev):  # noqa: F811
    """Autograd through ``closest_point``: d distance / d point = (p - c) / d, and the vertices get -w_k times it.  Queries are taken
    where the closest point lies inside a face (every weight in [0.05, 0.95]) at a distance of 0.01 or more: there c moves on a plane and
    the formula holds.  fp32: p - c carries 3 ulp of 1/2 (1e-7) against d >= 0.01, a relative 1e-5; 1e-4 leaves room for the norm."""
    from supnerf_amd import geometry as G
    verts, faces, queries, brute = _box()
    w, d = brute["weights"], np.sqrt(brute["dist2"])
    pick = np.nonzero((w.min(1) >= 0.05) & (w.max(1) <= 0.95) & (d >= 0.01))[0]
    assert len(pick) >= 40
    v, f = _to_gpu((verts, faces), dev)
    v.requires_grad_()
    p = torch.from_numpy(queries[pick]).to(dev).requires_grad_()
    got = G.closest_point((v, f), p)
    assert got.distance.requires_grad and np.array_equal(_np(got.face), brute["face"][pick])
    assert np.abs(_np(got.distance).astype(np.float64) - d[pick]).max() <= 1e-6
    got.distance.sum().backward()
    c = NR.closest_points(verts, faces, {k: x[pick] for k, x in brute.items()})
    unit = (queries[pick].astype(np.float64) - c) / d[pick, None]
    assert np.abs(_np(p.grad).astype(np.float64) - unit).max() <= 1e-4
    want = np.zeros((len(verts), 3))
    for k in range(3):
        np.add.at(want, faces[brute["face"][pick], k], -w[pick, k:k + 1].astype(np.float64) * unit)
    assert np.abs(_np(v.grad).astype(np.float64) - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    # only the points: the vertices of a plain mesh stay out of the graph
    p2 = torch.from_numpy(queries[pick]).to(dev).requires_grad_()
    G.closest_point(_to_gpu((verts, faces), dev), p2).distance.sum().backward()
    assert torch.equal(p2.grad, p.grad)


def test_surface_samples(amd, dev):  # noqa: F811
    """``snr_surface_sample`` against the restatement, bit for bit, with the device's own cumulative areas as the restatement's input."""
    from supnerf_amd import _lib, geometry as G, ops
    verts, faces = SR.box_mesh(HALF, 4)
    flat = np.array([[0, 0, 1], [2, 2, 2], [0, 1, 0]], np.int32)
    faces = np.concatenate([flat[:1], faces[:50], flat[1:2], faces[50:], flat[2:], flat[:1]])
    rv, rf = NR.roof_mesh()
    meshes = [(verts, faces), (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)), (rv, rf), (verts, flat)]
    mesh = ops.pack_mesh(*G._packed([_to_gpu(m, dev) for m in meshes]))
    areas = _np(ops.mesh_face_areas(mesh))
    assert same_bits(areas, np.concatenate([NR.face_areas(*m) for m in meshes])).all()
    cum_t = ops.mesh_cumulative_area(mesh)
    cum = _np(cum_t)
    off = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])])
    assert np.abs(cum[:off[1]] - np.cumsum(areas[:off[1]])).max() <= 1e-12 and cum[off[3] - 1] > 0 and (cum[off[3]:] == 0).all()
    counts = [1000, 5, 257, 9]
    u = np.random.default_rng(4).random((sum(counts), 3))
    u[0], u[999] = [0.0, 0.25, 0.5], [1.0 - 2.0 ** -53, 0.25, 0.5]               # the first and the last stratum
    points, face, weights = ops.mesh_surface_sample(mesh, cum_t, torch.from_numpy(u).to(dev), counts)
    so = np.concatenate([[0], np.cumsum(counts)])
    for b, m in enumerate(meshes):
        ref = NR.sample(m[0], m[1], cum[off[b]:off[b + 1]], u[so[b]:so[b + 1]])
        s = slice(so[b], so[b + 1])
        assert np.array_equal(_np(face)[s], ref["face"]), b
        assert same_bits(_np(points)[s], ref["points"]).all() and same_bits(_np(weights)[s], ref["weights"]).all(), b
    f0 = _np(face)[:1000]
    assert f0[0] == 1 and f0[999] == len(faces) - 3 and (areas[:off[1]][f0] > 0).all()
    assert (np.abs(np.bincount(f0, minlength=len(faces)) - 1000 * areas[:off[1]] / areas[:off[1]].sum()) < 2).all()
    assert (_np(face)[so[1]:so[2]] == -1).all() and (_np(face)[so[3]:] == -1).all() and (_np(points)[so[3]:] == 0).all()
    # guard bands and the flag, through the C ABI; a face index that is bad sets the flag and gives -1
    lib, i32, i64, f64 = _lib.lib(), torch.int32, torch.int64, torch.float64
    nS = sum(counts)
    soff = torch.from_numpy(so.astype(np.int64)).to(dev)
    u_t = torch.from_numpy(u).to(dev)
    for f_t, want_bad in ((mesh.faces, 0), (torch.where(mesh.faces == 7, torch.full_like(mesh.faces, 10 ** 6), mesh.faces), 1)):
        (pf, p), (ff, fa), (wf, w), flag = banded(nS * 3, torch.float32, dev, NAN), banded(nS, i32, dev, -7), banded(nS * 3, torch.float32, dev, NAN), \
            torch.zeros(1, dtype=i32, device=dev)
        assert lib.snr_surface_sample(ops._ptr(mesh.verts), ops._ptr(f_t.contiguous(), i32), ops._ptr(mesh.vert_offset, i64),
                                      ops._ptr(mesh.face_offset, i64), ops._ptr(cum_t, f64), ops._ptr(u_t, f64), ops._ptr(soff, i64), 4,
                                      mesh.verts.shape[0], mesh.faces.shape[0], nS, ops._ptr(p), ops._ptr(fa, i32), ops._ptr(w), ops._ptr(flag, i32),
                                      ops._stream(dev)) == 0
        assert bands_intact(pf, nS * 3, NAN) and bands_intact(ff, nS, -7) and bands_intact(wf, nS * 3, NAN) and int(flag.item()) == want_bad
        if not want_bad:
            assert torch.equal(p.view(-1, 3), points) and torch.equal(fa, face) and torch.equal(w.view(-1, 3), weights)
        else:
            hit = (mesh.faces[:off[1]][face[:1000].long()] == 7).any(1)
            assert bool(hit.any()) and bool((fa[:1000][hit] == -1).all()) and torch.equal(fa[:1000][~hit], face[:1000][~hit])
    # geometry.sample_surface: torch.rand of (B n, 3) float64 from the generator, then the same kernel
    gen = torch.Generator(device=dev).manual_seed(12)
    got = G.sample_surface([_to_gpu(m, dev) for m in meshes[:3]], 64, generator=gen)
    u2 = torch.rand(3 * 64, 3, dtype=f64, device=dev, generator=torch.Generator(device=dev).manual_seed(12))
    sub = ops.pack_mesh(*G._packed([_to_gpu(m, dev) for m in meshes[:3]]))
    p2, f2, w2 = ops.mesh_surface_sample(sub, ops.mesh_cumulative_area(sub), u2, [64] * 3)
    assert all(isinstance(s, G.SurfaceSamples) and s.points.shape == (64, 3) for s in got)
    assert torch.equal(torch.cat([s.points for s in got]), p2) and torch.equal(torch.cat([s.face for s in got]), f2)
    cpu = G.sample_surface(_to_gpu(meshes[0], dev), 32, generator=torch.Generator().manual_seed(1))
    assert cpu.points.shape == (32, 3) and bool((cpu.face >= 0).all())


def test_mesh_distance_on_offset_boxes(amd, dev):  # noqa: F811
    """Two boxes DELTA apart: every figure against the restatement on the device's own samples -- the means and the RMS from the
    fixed-order sums bit for bit, the maxima and the counts exactly -- and against DELTA (bounds: test_mesh_nearest_cpu.py)."""
    from supnerf_amd import geometry as G
    inner = SR.box_mesh(HALF, 8)
    outer = SR.box_mesh(tuple(h + DELTA for h in HALF), 8)
    a, b = _to_gpu(inner, dev), _to_gpu(outer, dev)
    n, thr = 600, DELTA * 1.25
    gen = torch.Generator(device=dev).manual_seed(21)
    sa, sb = G.sample_surface(a, n, generator=gen), G.sample_surface(b, n, generator=gen)
    md = G.mesh_distance(a, b, n=n, generator=torch.Generator(device=dev).manual_seed(21), threshold=thr)
    assert isinstance(md, G.MeshDistance) and md.chamfer.dim() == 0 and md.chamfer.dtype == torch.float64
    want = []
    for samples, mesh in ((sa, outer), (sb, inner)):
        d2 = NR.brute_force(mesh[0], mesh[1], _np(samples.points))["dist2"]
        d = np.sqrt(d2)
        sums = SS.segment_sum(np.stack([d, d2], 1), np.array([0, n]))[0]
        want.append((sums[0] / n, np.sqrt(sums[1] / n), d.max(), (d <= thr).sum() / n))
    got = [(md.forward_mean, md.forward_rms, md.forward_max, md.precision), (md.backward_mean, md.backward_rms, md.backward_max, md.recall)]
    for g, w in zip(got, want):
        for x, y in zip(g, w):
            assert same_bits(np.array([float(x)]), np.array([float(y)])).all(), (float(x), float(y))
    (fm, fr, fx, p), (bm, br, bx, r) = want
    assert float(md.chamfer) == fm + bm and float(md.hausdorff) == max(fx, bx) and float(md.fscore) == 2 * p * r / (p + r)
    assert abs(fm - DELTA) <= 1e-7 and abs(fr - DELTA) <= 1e-7 and abs(fx - DELTA) <= 1e-7 and p == 1.0
    assert DELTA - 1e-7 <= bm <= DELTA * np.sqrt(3.0) + 1e-7 and bx <= DELTA * np.sqrt(3.0) + 1e-7 and 0 < r < 1
    # lists of meshes: (B,) values, each object its own; a mesh against itself is at distance 0 (up to the rounding of the samples)
    both = G.mesh_distance([a, b], [b, b], n=200, generator=torch.Generator(device=dev).manual_seed(3))
    assert both.chamfer.shape == (2,) and both.precision is None
    assert abs(float(both.forward_mean[0]) - DELTA) <= 1e-7 and float(both.hausdorff[1]) <= 1e-7
    again = G.mesh_distance([a, b], [b, b], n=200, generator=torch.Generator(device=dev).manual_seed(3))
    assert all(torch.equal(x, y) for x, y in zip(both[:8], again[:8]))
