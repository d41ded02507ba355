"""Mesh containment on the MI355X: ``snr_inside_query`` / ``snr_inside_lattice`` and ``geometry.winding_number`` / ``contains`` /
``signed_distance`` / ``voxelize`` / ``mesh_iou`` against tests/inside_restatement.py.  The kernels run the restatement's float64 operations
in its order and the results are integers: every comparison is exact.

The hand meshes, the box with every tie, the octahedron at one cell, 16 cells and a clamped axis, the 320-face icosphere, a packed launch
of five objects (one without faces, one without vertices), a bad face index, non-finite vertices and queries, query counts around the
wave and the block into canary-filled outputs with guard bands, the lattice kernel against the point kernel on the same points, two
runs bit for bit, and the public API down to an extracted mesh against the density grid it came from."""
import functools

import numpy as np
import pytest
import torch

import geometry_cases as GC
import inside_restatement as IR
import nearest_restatement as NR
from segment_sum_restatement import banded, bands_intact
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
HALF = (0.25, 0.2, 0.15)
HALF32 = np.asarray(HALF, F32).astype(np.float64)
NAN = float("nan")
CANARY = -7


def _np(t):
    return t.detach().cpu().numpy()


def _to_gpu(mesh, dev):  # noqa: F811
    return (torch.from_numpy(np.ascontiguousarray(mesh[0], F32).reshape(-1, 3)).to(dev),
            torch.from_numpy(np.ascontiguousarray(mesh[1], np.int32).reshape(-1, 3)).to(dev))


def _t(x, dev):  # noqa: F811
    return torch.from_numpy(np.ascontiguousarray(x, F32)).to(dev)


def _kernel(G, ops, meshes, points, cell):
    """The winding numbers per object as numpy, straight from ``snr_inside_query`` over the index of ``cell``."""
    index = G.mesh_index([_to_gpu(m, points[0].device) for m in meshes], cell)
    nqs = [p.shape[0] for p in points]
    w = _np(ops.mesh_inside_query(index.mesh, index.grid, torch.cat(points), nqs))
    assert w.dtype == np.int32
    off = np.concatenate([[0], np.cumsum(nqs)])
    return [w[a:b] for a, b in zip(off[:-1], off[1:])], index


@functools.lru_cache(maxsize=None)
def _sphere_brute():
    verts, faces, q = IR.sphere_case()
    return IR.brute_force(verts, faces, q)


def _hand_cases():
    """(name, verts, faces, queries, cells)"""
    below = np.array([[x, y, -1] for (x, y), _ in IR.UNDER], F32)
    tri_q = np.concatenate([below, below * F32([1, 1, 0]), below * F32([1, 1, -1])])
    shared = np.array([[0.5, 0.5, -1], [0.25, 0.25, -1], [0, 0, -1], [1, 1, -1], [0.5, 0.25, -1], [0.25, 0.5, -1]], F32)
    fan = IR.FAN[0]
    spokes = np.concatenate([[[0, 0, -1]], np.c_[fan[1:, :2] / 2, -np.ones(6)], np.c_[fan[1:, :2] / 4, -np.ones(6)]]).astype(F32)
    sv, sf, sq = IR.skew_mesh()
    return [("triangle", IR.TRI, IR.ONE, tri_q, (8.0, 0.25, None)), ("reversed", IR.TRI, IR.ONE[:, ::-1], tri_q, (0.25,)),
            ("tilted", IR.TILTED, IR.ONE, np.array([[0.25, 0.25, 0.25], [0.25, 0.25, 0.5], [0.25, 0.25, 0.75], [0.5, 0.25, 0.75]], F32), (0.3, None)),
            ("two triangles", *IR.SQUARE, shared, (4.0, 0.25)), ("fan", *IR.FAN, spokes, (0.5, None)),
            ("never", *IR.NEVER, (0.5, None)), ("skew", sv, sf, sq, (2.0 ** 41, 2.0 ** 34)),
            ("highest corner", IR.GUARD_TRI, IR.ONE, IR.GUARD_TRI.copy(), (1.0, 0.1)),
            ("box", *IR.box12(HALF), IR.box_tie_queries(), (1.0, 0.1, None))]


def test_hand_meshes_and_the_box(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G, ops
    for name, verts, faces, q, cells in _hand_cases():
        want = IR.brute_force(verts, faces, q)
        for cell in cells:
            (got,), _ = _kernel(G, ops, [(verts, faces)], [_t(q, dev)], cell)
            assert np.array_equal(got, want), (name, cell, np.nonzero(got != want)[0][:10])
    (got,), _ = _kernel(G, ops, [(IR.TRI, IR.ONE)], [_t([[x, y, -1] for (x, y), _ in IR.UNDER], dev)], 0.25)
    assert got.tolist() == [w for _, w in IR.UNDER]
    p = IR.box_tie_queries().astype(np.float64)
    (got,), _ = _kernel(G, ops, [IR.box12(HALF)], [_t(IR.box_tie_queries(), dev)], 0.07)
    assert np.array_equal(got, ((p >= -HALF32) & (p < HALF32)).all(1).astype(np.int32))


def test_octahedron_at_three_cell_sizes_and_the_sphere(amd, dev):  # noqa: F811
    """One cell is the brute force of the same kernel; 16 cells make every face span eight cells of a column; 256 is the clamp."""
    from supnerf_amd import geometry as G, ops
    v, f = IR.octahedron()
    q = IR.octa_queries()
    want = IR.brute_force(v, f, q)
    for cell, n in ((1.0, [1, 1, 1]), (1 / 16, [16, 16, 16])):
        (got,), index = _kernel(G, ops, [(v, f)], [_t(q, dev)], cell)
        assert index.grid.n_cells == int(np.prod(n)) and NR.grid(v, cell)["n"].tolist() == n
        assert np.array_equal(got, want), cell
    tv, tq = (v * IR.THIN).astype(F32), IR.octa_queries(IR.THIN)
    (got,), index = _kernel(G, ops, [(tv, f)], [_t(tq, dev)], 1e-3)
    assert index.grid.n_cells == 16 * 16 * 256 and np.array_equal(got, IR.brute_force(tv, f, tq))
    verts, faces, sq = IR.sphere_case()
    for cell in (None, 0.05, 2.0):
        (got,), _ = _kernel(G, ops, [(verts, faces)], [_t(sq, dev)], cell)
        assert np.array_equal(got, _sphere_brute()), cell
        (again,), _ = _kernel(G, ops, [(verts, faces)], [_t(sq, dev)], cell)
        assert np.array_equal(again, got)
    r = np.linalg.norm(sq.astype(np.float64), axis=1)
    assert (got[r < 0.4 * 0.96] == 1).all() and (got[r > 0.4] == 0).all()


def _raw_query(ops, lib, index, points, nqs, dev, verts=None, faces=None):  # noqa: F811
    """``snr_inside_query`` into a canary-filled output with guard bands; (winding, the flag, whether the bands held)."""
    m, g = index.mesh, index.grid
    i32, i64 = torch.int32, torch.int64
    verts, faces = m.verts if verts is None else verts, m.faces if faces is None else faces
    nQ = points.shape[0]
    qoff = torch.tensor(np.concatenate([[0], np.cumsum(nqs)]), dtype=i64).to(dev)
    (wf, w), (bf, bad) = banded(nQ, i32, dev, CANARY), banded(1, i32, dev, CANARY)
    bad.zero_()
    rc = lib.snr_inside_query(ops._ptr(verts), ops._ptr(faces, i32), ops._ptr(m.vert_offset, i64), ops._ptr(m.face_offset, i64),
                              ops._ptr(points), ops._ptr(qoff, i64), ops._ptr(g.cell), ops._ptr(g.grid_lo), ops._ptr(g.grid_hi),
                              ops._ptr(g.cell_offset, i64), ops._ptr(g.cell_start, i64), ops._ptr(g.pair_face, i32), len(m.n_verts),
                              verts.shape[0], faces.shape[0], nQ, g.n_cells, g.n_pairs, ops._ptr(w, i32), ops._ptr(bad, i32), ops._stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    return _np(w), int(bad.item()), bands_intact(wf, nQ, CANARY) and bands_intact(bf, 1, CANARY)


def test_packed_launch_bad_index_and_non_finite_input(amd, dev):  # noqa: F811
    """Five objects that overlap in space, one without faces and one without vertices: every query sees its own object only.  Then a face
    index that goes bad after the index was built (skipped, flagged), a vertex that is not finite (its faces skipped) and queries that
    are not finite (0)."""
    from supnerf_amd import _lib, geometry as G, ops
    lib = _lib.lib()
    sv, sf, sq = IR.sphere_case()
    ov, of = IR.octahedron(0.3)
    meshes = [IR.box12(HALF), (sv[:5], np.zeros((0, 3), np.int32)), (sv, sf), (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)), (ov, of)]
    q = sq[:300].copy()
    q[:6] = [[NAN, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0, 0, 0], [0.01, 0.02, -0.1], [0.01, 0.02, 0.39]]
    points = [q[:200], q[:50], q, q[:30], q[:257]]
    index = G.mesh_index([_to_gpu(m, dev) for m in meshes], [0.1, 1.0, 0.05, 1.0, 0.07])
    nqs = [len(p) for p in points]
    off = np.concatenate([[0], np.cumsum(nqs)])
    packed = _t(np.concatenate(points), dev)
    got, bad, intact = _raw_query(ops, lib, index, packed, nqs, dev)
    assert intact and bad == 0
    want = [IR.brute_force(m[0], m[1], p) for m, p in zip(meshes, points)]
    for b in range(5):
        assert np.array_equal(got[off[b]:off[b + 1]], want[b]), b
    assert not got[off[1]:off[2]].any() and not got[off[3]:off[4]].any() and want[2][:3].tolist() == [0, 0, 0] and want[2][3:5].tolist() == [1, 1]
    assert want[0].any() and want[4].any() and not np.array_equal(want[2][:200], want[0])
    assert np.array_equal(_np(ops.mesh_inside_query(index.mesh, index.grid, packed, nqs)), got)
    # the sphere's faces above the query (0.01, 0.02, *): one gets a bad index, so the query loses its crossing
    tri = sv[sf].astype(np.float64)
    above = np.nonzero(IR.contributions(q[4].astype(np.float64), tri[:, 0], tri[:, 1], tri[:, 2]) != 0)[0]
    assert len(above) == 1
    f0 = sum(len(m[1]) for m in meshes[:2])
    broken = np.concatenate([m[1] for m in meshes]).astype(np.int32)
    broken[f0 + above[0], 1] = 10 ** 6
    broken[f0 + 7, 2] = -1
    got, bad, intact = _raw_query(ops, lib, index, packed, nqs, dev, faces=torch.from_numpy(broken).to(dev))
    ref = IR.brute_force(sv, broken[f0:f0 + 320], q)
    assert intact and bad == 1 and IR.bad_flag(sv, broken[f0:f0 + 320]) and ref[4] == 0 and want[2][4] == 1
    assert np.array_equal(got[off[2]:off[3]], ref) and np.array_equal(got[:off[2]], np.concatenate(want[:2])) and np.array_equal(got[off[3]:], np.concatenate(want[3:]))
    # a vertex that stops being finite: its faces are skipped, no flag
    v0 = sum(len(m[0]) for m in meshes[:2])
    nan = np.concatenate([m[0] for m in meshes]).astype(F32)
    nan[v0 + sf[above[0], 0], 1] = NAN
    nan[v0 + 11, 2] = np.inf
    got, bad, intact = _raw_query(ops, lib, index, packed, nqs, dev, verts=torch.from_numpy(nan).to(dev))
    ref = IR.brute_force(nan[v0:v0 + len(sv)], sf, q)
    assert intact and bad == 0 and ref[4] == 0 and np.array_equal(got[off[2]:off[3]], ref)


@pytest.mark.parametrize("n_queries", [0, 1, 63, 64, 65, 257])
def test_query_counts_and_guard_bands(amd, dev, n_queries):  # noqa: F811
    from supnerf_amd import _lib, geometry as G, ops
    sv, sf, sq = IR.sphere_case()
    index = G.mesh_index(_to_gpu((sv, sf), dev), 0.06)
    got, bad, intact = _raw_query(ops, _lib.lib(), index, _t(sq[700:700 + n_queries].reshape(-1, 3), dev), [n_queries], dev)
    assert intact and bad == 0 and np.array_equal(got, _sphere_brute()[700:700 + n_queries])


def _raw_lattice(ops, lib, index, lo, h, n, dev):  # noqa: F811
    m, g = index.mesh, index.grid
    i32, i64 = torch.int32, torch.int64
    B, total = len(m.n_verts), len(m.n_verts) * int(np.prod(n))
    (wf, w), (bf, bad) = banded(total, i32, dev, CANARY), banded(1, i32, dev, CANARY)
    bad.zero_()
    lo_t, h_t = _t(lo, dev), _t(h, dev)
    rc = lib.snr_inside_lattice(ops._ptr(m.verts), ops._ptr(m.faces, i32), ops._ptr(m.vert_offset, i64), ops._ptr(m.face_offset, i64),
                                ops._ptr(g.cell), ops._ptr(g.grid_lo), ops._ptr(g.grid_hi), ops._ptr(g.cell_offset, i64),
                                ops._ptr(g.cell_start, i64), ops._ptr(g.pair_face, i32), ops._ptr(lo_t), ops._ptr(h_t), B, m.verts.shape[0],
                                m.faces.shape[0], g.n_cells, g.n_pairs, n[0], n[1], n[2], ops._ptr(w, i32), ops._ptr(bad, i32), ops._stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    return _np(w).reshape((B,) + tuple(n)), int(bad.item()), bands_intact(wf, total, CANARY) and bands_intact(bf, 1, CANARY)


# per object (lat_lo, lat_h): lattices that reach outside the grid on every side, steps that differ, one step below 0 and one of 0
LATTICES = [([-0.7, -0.6, -0.9], [0.2, 0.3, 0.1]), ([0.45, -0.33, 0.62], [-0.06, 0.011, -0.04]), ([-0.31, 0.02, -0.2], [0.04, 0.0, 0.023])]


@pytest.mark.parametrize("n", [(1, 1, 1), (2, 3, 5), (16, 16, 16), (7, 64, 3), (3, 2, 17), (2, 2, 33)])
def test_lattice_kernel_equals_query_kernel(amd, dev, n):  # noqa: F811
    """``snr_inside_lattice`` gives the integers of ``snr_inside_query`` on ``lattice_points`` of the same lattice, and the
    restatement's.  The kernel takes 16 z-points per thread: n_z = 17 and 33 are one past its tile."""
    from supnerf_amd import _lib, geometry as G, ops
    sv, sf, _ = IR.sphere_case()
    meshes = [IR.octahedron(), IR.box12(HALF, (0.05, -0.1, 0.02)), (sv, sf)]
    index = G.mesh_index([_to_gpu(m, dev) for m in meshes], [1 / 16, 0.09, 0.05])
    lo, h = np.array([x[0] for x in LATTICES], F32), np.array([x[1] for x in LATTICES], F32)
    got, bad, intact = _raw_lattice(ops, _lib.lib(), index, lo, h, n, dev)
    assert intact and bad == 0 and got.dtype == np.int32
    pts = [IR.lattice_points(lo[b], h[b], n) for b in range(3)]
    per = int(np.prod(n))
    by_query = _np(ops.mesh_inside_query(index.mesh, index.grid, _t(np.concatenate(pts), dev), [per] * 3))
    assert np.array_equal(got.reshape(-1), by_query)
    for b in range(3):
        assert np.array_equal(got[b].reshape(-1), IR.brute_force(meshes[b][0], meshes[b][1], pts[b])), b
    if per >= 4096:
        assert all(got[b].any() for b in range(3))
    again = ops.mesh_inside_lattice(index.mesh, index.grid, lo, h, n)
    assert again.shape == (3,) + tuple(n) and again.dtype == torch.int32 and np.array_equal(_np(again), got)
    assert np.array_equal(_np(ops.mesh_inside_lattice(index.mesh, index.grid, lo, h, n)), got)              # two runs, the same bits


def test_public_api_on_spheres_and_boxes(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    sv, sf, sq = IR.sphere_case()
    two = IR.merged((sv, sf), ((sv + F32([0.1, 0, 0])).astype(F32), sf))
    back = (sv, sf[:, ::-1])
    meshes, pts = [_to_gpu(two, dev), _to_gpu(back, dev)], [_t(sq, dev), _t(sq[:500], dev)]
    want = [IR.brute_force(*two, sq), IR.brute_force(*back, sq[:500])]
    assert sorted(set(want[0].tolist())) == [0, 1, 2] and sorted(set(want[1].tolist())) == [-1, 0]
    index = G.mesh_index(meshes)
    w = G.winding_number(meshes, pts, index=index)
    assert all(x.dtype == torch.int32 and np.array_equal(_np(x), y) for x, y in zip(w, want))
    one = G.winding_number(meshes[0], pts[0])
    assert torch.is_tensor(one) and torch.equal(one, w[0])
    for rule in IR.RULES:
        c = G.contains(meshes, pts, index=index, rule=rule)
        assert all(x.dtype == torch.bool and np.array_equal(_np(x), IR.contained(y, rule)) for x, y in zip(c, want)), rule
    assert int(G.contains(meshes[0], pts[0], rule="odd").sum()) < int(G.contains(meshes[0], pts[0]).sum())
    assert not bool(G.contains(meshes[1], pts[1], rule="positive").any()) and bool(G.contains(meshes[1], pts[1]).any())
    # voxelize: the box on a lattice of (16, 12, 9) points is the half-open box
    box = _to_gpu(IR.box12(HALF), dev)
    vox = G.voxelize(box, (16, 12, 9))
    assert vox.shape == (16, 12, 9) and vox.dtype == torch.bool
    lat = G.lattice((16, 12, 9))
    axes = IR.lattice_axes([lat.lo[a] for a in range(3)], [lat.h[a] for a in range(3)], (16, 12, 9))
    inside = [(x.astype(np.float64) >= -hh) & (x.astype(np.float64) < hh) for x, hh in zip(axes, HALF32)]
    assert int(vox.sum()) == int(np.prod([i.sum() for i in inside])) > 0
    assert np.array_equal(_np(vox), inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :])
    both = G.voxelize([box, box], 8, bound=[(-0.5, 0.5), ((-0.3, -0.3, -0.2), (0.3, 0.3, 0.2))])
    assert both.shape == (2, 8, 8, 8) and torch.equal(both[0], G.voxelize(box, 8)) and int(both[1].sum()) > int(both[0].sum())
    assert torch.equal(both[1], G.voxelize(box, 8, bound=((-0.3, -0.3, -0.2), (0.3, 0.3, 0.2))))
    # mesh_iou on two boxes a whole number of lattice steps apart: all integers by closed form
    a, b = _to_gpu(IR.box12(*IR.IOU_A), dev), _to_gpu(IR.box12(*IR.IOU_B), dev)
    got = G.mesh_iou(a, b, resolution=IR.IOU_R)
    assert isinstance(got, G.IoU) and got.iou.dim() == 0 and got.iou.dtype == torch.float64 and got.union.dtype == torch.int64
    assert (float(got.iou), *[int(x) for x in got[1:]]) == (0.6, *IR.IOU_WANT)
    many = G.mesh_iou([a, b, a], [b, b, box], resolution=IR.IOU_R, index_a=G.mesh_index([a, b, a]))
    assert many.iou.shape == (3,) and many.intersection.tolist()[:2] == [4800, 8000] and many.iou.tolist()[:2] == [0.6, 1.0]
    fixed = G.mesh_iou(a, b, resolution=32, bound=(-0.5, 0.5))          # steps of 1/32: 16^3 voxels each, 4 apart
    assert [int(x) for x in fixed[1:]] == [12 * 256, 20 * 256, 4096, 4096]
    # errors
    other = G.mesh_index(meshes[1])
    for call in (lambda: G.winding_number(meshes[0], pts[0], index=other), lambda: G.voxelize(box, 8, index=other),
                 lambda: G.signed_distance(box, pts[0], index=other), lambda: G.winding_number(meshes[0], pts[0], index=index.grid)):
        with pytest.raises(amd.SnrError, match="index"):
            call()
    with pytest.raises(amd.SnrError, match="GPU|gpu"):
        G.winding_number(meshes[0], pts[0].cpu())
    with pytest.raises(amd.SnrError, match="GPU|gpu"):
        G.voxelize((box[0].cpu(), box[1].cpu()), 8)
    with pytest.raises(amd.SnrError, match="rule"):
        G.contains(meshes[0], pts[0], rule="even")


def test_signed_distance(amd, dev):  # noqa: F811
    """The magnitude is ``closest_point``'s distance bit for bit, the sign is the box's, and the gradient to the points is +-
    ``closest_point``'s."""
    from supnerf_amd import geometry as G
    import simplify_restatement as SR
    verts, faces = SR.box_mesh(HALF, 8)
    q = NR.box_queries(HALF)
    want = IR.box_signed_distance(q, HALF32)
    mesh, pts = _to_gpu((verts, faces), dev), _t(q, dev)
    index = G.mesh_index(mesh)
    sd, cp = G.signed_distance(mesh, pts, index=index), G.closest_point(mesh, pts, index=index)
    assert isinstance(sd, G.SignedDistance) and sd.distance.dtype == torch.float32 and sd.winding.dtype == torch.int32
    assert torch.equal(sd.distance.abs(), cp.distance) and torch.equal(sd.closest.face, cp.face) and torch.equal(sd.closest.weights, cp.weights)
    assert np.array_equal(_np(sd.winding), IR.brute_force(verts, faces, q))
    clear = np.abs(want) > 1e-6
    assert clear.sum() >= 400 and (want[clear] < 0).sum() >= 100
    assert np.array_equal(np.sign(_np(sd.distance)[clear]), np.sign(want[clear]))
    # the float64 distance is within 2e-7 of the closed form (the box's bound in test_mesh_nearest_cpu.py); its rounding to fp32 adds
    # half an ulp, at most 2^-24 of the distance (the far queries lie 10 away)
    assert (np.abs(_np(sd.distance).astype(np.float64) - want) <= 2e-7 + 2.0 ** -24 * np.abs(want)).all()
    # a query without an answer keeps +inf
    odd = torch.tensor([[NAN, 0, 0], [0, 0, 0]], device=dev)
    assert G.signed_distance(mesh, odd).distance.tolist() == [float("inf"), -float(F32(0.15))]
    empty = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))
    out = G.signed_distance([mesh, empty], [pts[:10], pts[:10]])
    assert torch.equal(out[0].distance, sd.distance[:10]) and bool(torch.isinf(out[1].distance).all()) and bool((out[1].distance > 0).all())
    # autograd: through closest_point's graph, the sign a constant
    pick = np.nonzero(np.abs(want) >= 0.01)[0]
    p1, p2 = _t(q[pick], dev).requires_grad_(), _t(q[pick], dev).requires_grad_()
    s = G.signed_distance(mesh, p1, index=index)
    (g1,) = torch.autograd.grad(s.distance.sum(), p1)
    (g2,) = torch.autograd.grad(G.closest_point(mesh, p2, index=index).distance.sum(), p2)
    inside = torch.from_numpy(want[pick] < 0).to(dev)
    assert bool(inside.any()) and bool((~inside).any()) and torch.equal(g1, torch.where(inside[:, None], -g2, g2))
    v = mesh[0].clone().requires_grad_()
    s = G.signed_distance((v, mesh[1]), _t(q[pick], dev))
    s.distance.sum().backward()
    assert v.grad is not None and bool((v.grad != 0).any())


def test_extracted_mesh_against_its_density_grid(amd, dev):  # noqa: F811
    """``voxelize(extract_mesh(grid), R)`` against ``grid > level`` at R = 32 on the planted box decoder: the two may differ only at
    lattice points within one lattice diagonal of the surface (by ``closest_point``), and count h^3 is the mesh's volume within
    area h sqrt(3): a voxel can be miscounted only if the surface passes within h sqrt(3) / 2 of its lattice point, and the points
    that close to the surface stand for a volume of at most area h sqrt(3) (both sides of it)."""
    from supnerf_amd import geometry as G
    R = 32
    model, sc = GC.box(amd, dev, 3, 1, seed=4), GC.codes(1, 31, dev)
    grid = G.density_grid(model, sc, R, GC.BOUND_BOX)
    mesh = G.extract_mesh(grid, level=GC.LEVEL_BOX, bound=GC.BOUND_BOX)[0]
    assert mesh[1].shape[0] > 500 and G.mesh_adjacency(mesh).closed
    index = G.mesh_index(mesh)
    vox = G.voxelize(mesh, R, GC.BOUND_BOX, index=index)
    occ = grid[0] > GC.LEVEL_BOX
    lat = G.lattice(R, GC.BOUND_BOX)
    h = float(lat.h[0])
    d = G.closest_point(mesh, G.lattice_points(lat, dev), index=index).distance.view(R, R, R)
    differ = vox != occ
    iou = G.occupancy_iou(vox, occ)
    print(f"voxelize against density_grid > level at R = {R}: {int(differ.sum())} voxels differ, IoU {float(iou.iou):.6f}, "
          f"largest distance of a differing voxel {float(d[differ].max()) if bool(differ.any()) else 0.0:.3g} (h = {h:.3g})")
    assert int(vox.sum()) > 1000 and bool((d[differ] <= h * 3 ** 0.5).all())
    comps = G.mesh_components(mesh)
    volume, area = float(comps.volume.sum()), float(comps.area.sum())
    print(f"count h^3 = {int(vox.sum()) * h ** 3:.6f}, signed volume {volume:.6f}, bound {area * h * 3 ** 0.5:.6f}")
    assert abs(int(vox.sum()) * h ** 3 - volume) <= area * h * 3 ** 0.5
