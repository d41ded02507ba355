"""Mesh containment on the host: the rules of include/supnerf_hip.h ("Mesh containment") as tests/inside_restatement.py restates them, held
against results known by hand or in closed form -- one triangle with queries above, below, on its plane and under each edge and vertex,
two triangles on one edge, a fan around a vertex, the axis-parallel box as a half-open box with every tie, the voxel count of a box, a
sphere with a cavity, two overlapping spheres, faces that can never count, the pruned walk against the brute force (bit for bit, with
faces that span many cells, queries outside the grid, one cell and a clamped axis), the signed distance to a box, the IoU of two offset
boxes -- with planted mistakes that the same checks reject; and the parts of the API that need no GPU (symbols, the argument checks of
the C ABI and of the Python layer)."""
import functools
import inspect

import numpy as np
import pytest
import torch

import inside_restatement as IR
import nearest_restatement as NR

F32 = np.float32
HALF = (0.25, 0.2, 0.15)
HALF32 = np.asarray(HALF, F32).astype(np.float64)            # the box the fp32 vertices really span
TRI, UNDER, TILTED, SQUARE, FAN, GUARD_TRI, ONE, NEVER = IR.TRI, IR.UNDER, IR.TILTED, IR.SQUARE, IR.FAN, IR.GUARD_TRI, IR.ONE, IR.NEVER


def _hand_failures(planted=None):
    """The hand cases; a list of the ones that fail."""
    failed = []
    bf = functools.partial(IR.brute_force, planted=planted)
    # one triangle
    below = np.array([[x, y, -1] for (x, y), _ in UNDER], F32)
    want = [w for _, w in UNDER]
    if bf(TRI, ONE, below).tolist() != want:
        failed.append(f"triangle, from below: {bf(TRI, ONE, below).tolist()}")
    if bf(TRI, ONE[:, ::-1], below).tolist() != [-w for w in want]:
        failed.append("triangle, reversed")
    if bf(TRI, ONE, below * F32([1, 1, -1])).any() or bf(TRI, ONE, below * F32([1, 1, 0])).any():
        failed.append("triangle: a query above it or on its plane")
    got = bf(TILTED, ONE, np.array([[0.25, 0.25, 0.25], [0.25, 0.25, 0.5], [0.25, 0.25, 0.75], [0.5, 0.25, 0.75]], F32)).tolist()
    if got != [1, 0, 0, 0]:
        failed.append(f"tilted triangle, below / on its plane / above: {got}")
    # two triangles on one edge, a fan around a vertex: a query under what they share counts once
    shared = np.array([[0.5, 0.5, -1], [0.25, 0.25, -1], [0, 0, -1], [1, 1, -1], [0.5, 0.25, -1], [0.25, 0.5, -1]], F32)
    if bf(*SQUARE, shared).tolist() != [1, 1, 1, 0, 1, 1]:
        failed.append(f"two triangles: {bf(*SQUARE, shared).tolist()}")
    spokes = np.concatenate([[[0, 0, -1]], np.c_[FAN[0][1:, :2] / 2, -np.ones(6)], np.c_[FAN[0][1:, :2] / 4, -np.ones(6)]]).astype(F32)
    if bf(*FAN, spokes).tolist() != [1] * 13:
        failed.append(f"fan: {bf(*FAN, spokes).tolist()}")
    # the box is the half-open box, every tie included
    q = IR.box_tie_queries()
    assert q.shape == (336, 3)
    p = q.astype(np.float64)
    half_open = ((p >= -HALF32) & (p < HALF32)).all(1).astype(np.int32)
    if not np.array_equal(bf(*IR.box12(HALF), q), half_open):
        failed.append("box: not the half-open box")
    on_tie = (np.abs(p) == HALF32).any(1) & (np.abs(p) <= HALF32).all(1)
    assert on_tie.sum() >= 60 and half_open[on_tie].any() and not half_open[on_tie].all()
    # 16^3 voxel centres
    pts = IR.lattice_points([-0.5 + 1 / 32] * 3, [1 / 16] * 3, (16, 16, 16))
    c = pts[:16, 2].astype(np.float64)
    closed = int(np.prod([((c >= -h) & (c < h)).sum() for h in HALF32]))
    assert closed == 192
    if int((bf(*IR.box12(HALF), pts) != 0).sum()) != closed:
        failed.append("box: voxel count")
    # spheres: solid, with a cavity, two overlapping
    verts, faces, q = IR.sphere_case()
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    inner, mid, outer = r < 0.19, (r > 0.21) & (r < 0.4 * 0.96), r > 0.4                # (the shells between hold chords of the faces)
    assert inner.sum() > 40 and mid.sum() > 350 and outer.sum() > 500 and (inner | mid)[2000:].sum() >= 60
    w = bf(verts, faces, q)
    if not ((w[mid | inner] == 1).all() and (w[outer] == 0).all() and set(w.tolist()) == {0, 1}):
        failed.append("sphere")
    cavity = IR.merged((verts, faces), (verts * F32(0.5), faces[:, ::-1]))
    w = bf(*cavity, q)
    if not ((w[inner] == 0).all() and (w[mid] == 1).all() and (w[outer] == 0).all()):
        failed.append(f"cavity: inside it {sorted(set(w[inner].tolist()))}")
    two = IR.merged((verts, faces), ((verts + F32([0.1, 0, 0])).astype(F32), faces))
    w = bf(*two, q)
    if sorted(set(w.tolist())) != [0, 1, 2] or not (w[np.abs(q.astype(np.float64) - [0.05, 0, 0]).max(1) < 0.15] == 2).all():
        failed.append(f"two spheres: {sorted(set(w.tolist()))}")
    counts = [int(IR.contained(w, rule).sum()) for rule in IR.RULES]
    if not (counts[0] == counts[1] == (w != 0).sum() and counts[2] == (w == 1).sum() < counts[0]):
        failed.append(f"rules on two spheres: {counts}")
    # faces that never count: without area, collinear, vertical; queries under their corners and edges among them
    if bf(*NEVER).any():
        failed.append("a face without projected area counted")
    # the canonical endpoint order, and the guard as part of the rule
    sv, sf, sq = IR.skew_mesh()
    if bf(sv, sf, sq).tolist() != [1]:
        failed.append(f"skew: {bf(sv, sf, sq).tolist()}")
    top = GUARD_TRI[1:2]
    assert GUARD_TRI[1, 2] == GUARD_TRI[:, 2].max()
    if bf(GUARD_TRI, ONE, top).tolist() != [0] or bf(GUARD_TRI, ONE[:, ::-1], top).tolist() != [0]:
        failed.append(f"a query at the face's highest corner: {bf(GUARD_TRI, ONE, top).tolist()}")
    return failed


def test_hand_cases_and_closed_forms():
    assert _hand_failures() == []


def test_rules_of_contains():
    w = np.array([-2, -1, 0, 1, 2, 3], np.int32)
    assert IR.contained(w, "nonzero").tolist() == [True, True, False, True, True, True]
    assert IR.contained(w, "positive").tolist() == [False, False, False, True, True, True]
    assert IR.contained(w, "odd").tolist() == [False, True, False, True, False, True]
    verts, faces, q = IR.sphere_case()
    w = IR.brute_force(verts, faces[:, ::-1], q[:300])
    assert set(w.tolist()) == {0, -1} and not IR.contained(w, "positive").any() and IR.contained(w, "odd").sum() == (w != 0).sum()


# ------------------------------------------------------------------ W5: the walk is the brute force
def _walk_failures(planted=None):
    failed = []
    v, f = IR.octahedron()
    q = IR.octa_queries()
    want = IR.brute_force(v, f, q)
    assert set(want.tolist()) == {0, 1} and want.sum() > 20
    g = NR.grid(v, 1 / 16)
    lo, hi, _ = NR.face_boxes(v, f, g)
    assert g["n"].tolist() == [16, 16, 16] and (hi[:, 2] - lo[:, 2] + 1).min() >= 8           # every face spans eight z-cells
    got, looked = IR.walk(v, f, q, 1 / 16, planted)
    if not np.array_equal(got, want):
        failed.append(f"octahedron at 16 cells: {int((got != want).sum())} queries differ")
    if planted is None:
        print("octahedron at 16 cells: faces looked at per query: mean", looked.mean(), "of 8")
        one, looked1 = IR.walk(v, f, q, 1.0)
        assert NR.grid(v, 1.0)["n"].tolist() == [1, 1, 1] and np.array_equal(one, want) and (looked1 == 8).all()
        # an axis clamped to 256 cells: border cells reach outwards without end
        tv, tq = (v * IR.THIN).astype(F32), IR.octa_queries(IR.THIN)
        assert NR.grid(tv, 1e-3)["n"].tolist() == [16, 16, 256]
        assert np.array_equal(IR.walk(tv, f, tq, 1e-3)[0], IR.brute_force(tv, f, tq))
        # W6: runs of z-points from the cell of their lowest point; lattices that reach outside the grid, an h below 0, one point
        for lo3, h3, n in (([-0.7, -0.6, -0.9], [0.2, 0.3, 0.1], (8, 5, 19)), ([0.1, -0.2, 0.8], [0.05, 0.0, -0.09], (3, 1, 17)),
                           ([0.05, 0.05, -0.2], [0, 0, 0], (1, 1, 1))):
            pts = IR.lattice_points(lo3, h3, n)
            assert np.array_equal(IR.column_walk(v, f, lo3, h3, n, 1 / 16, 16).reshape(-1), IR.brute_force(v, f, pts)), n
    return failed


def test_walk_equals_brute_force():
    assert _walk_failures() == []


# ------------------------------------------------------------------ planted mistakes
REJECTED_BY = {"no_eps_both": "two triangles", "no_eps_neither": "two triangles", "stored_anchor": "skew", "guard_le": "highest corner",
               "t_ge": "tilted triangle", "sigma_dropped": "cavity", "every_cell": "octahedron"}


@pytest.mark.parametrize("planted", IR.PLANTED)
def test_planted_mistakes_are_rejected(planted):
    assert set(REJECTED_BY) == set(IR.PLANTED)
    failed = _walk_failures(planted) if planted == "every_cell" else _hand_failures(planted)
    print(planted, failed)
    assert any(REJECTED_BY[planted] in f for f in failed), (planted, failed)


# ------------------------------------------------------------------ signed distance and IoU in closed form
def test_box_signed_distance_closed_form():
    verts, faces = IR.box12(HALF)
    q = NR.box_queries(HALF)
    d = np.sqrt(NR.brute_force(verts, faces, q)["dist2"])
    sd = np.where(IR.contained(IR.brute_force(verts, faces, q), "nonzero"), -d, d)
    want = IR.box_signed_distance(q, HALF32)
    assert (want < -1e-3).sum() >= 100 and (want > 1e-3).sum() >= 200
    assert np.abs(sd - want).max() <= 2e-7                                         # (the bound of test_mesh_nearest_cpu.py's box)


IOU_A, IOU_B, IOU_R, IOU_WANT = IR.IOU_A, IR.IOU_B, IR.IOU_R, IR.IOU_WANT


def test_iou_of_offset_boxes():
    from supnerf_amd import geometry as G
    a, b = IR.box12(*IOU_A), IR.box12(*IOU_B)
    lo, h = IR.iou_lattice(np.minimum(a[0].min(0), b[0].min(0)), np.maximum(a[0].max(0), b[0].max(0)), IOU_R)
    assert h.tolist() == [F32(1 / 32), F32(0.5) / F32(20), F32(0.5) / F32(20)] and lo[0] == F32(-0.25 + 1 / 64)
    pts = IR.lattice_points(lo, h, (IOU_R,) * 3)
    ga, gb = (IR.contained(IR.brute_force(*m, pts), "nonzero").reshape((IOU_R,) * 3) for m in (a, b))
    assert IR.iou_counts(ga, gb) == (0.6, *IOU_WANT)
    got = G.occupancy_iou(torch.from_numpy(ga), torch.from_numpy(gb))
    assert isinstance(got, G.IoU) and got.iou.dtype == torch.float64 and got.intersection.dtype == torch.int64 and got.iou.dim() == 0
    assert (float(got.iou), *[int(x) for x in got[1:]]) == (0.6, *IOU_WANT)
    both = G.occupancy_iou(torch.from_numpy(np.stack([ga, gb, np.zeros_like(ga)])), torch.from_numpy(np.stack([gb, gb, np.zeros_like(ga)])))
    assert both.iou.tolist() == [0.6, 1.0, 0.0] and both.union.tolist() == [8000, 6400, 0] and both.count_a.tolist() == [6400, 6400, 0]
    for x, y in ((ga, gb[:10]), (ga.astype(np.int32), gb.astype(np.int32)), (ga[0, 0], gb[0, 0])):
        with pytest.raises(G.SnrError, match="bool grids"):
            G.occupancy_iou(torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(y)))


# ------------------------------------------------------------------ the API without a GPU
INSIDE_SYMBOLS = ("snr_inside_query", "snr_inside_lattice")


def test_symbols_and_c_abi_checks():
    import importlib.util
    import os
    import re
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, geometry as G, ops
    assert all(n in _lib.exported_symbols() for n in INSIDE_SYMBOLS)
    assert sum(n.startswith("snr_inside") for n in _lib.exported_symbols()) == 2
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in INSIDE_SYMBOLS)
    assert _lib.header_abi_version() >= 26 and lib.snr_abi_version() == _lib.header_abi_version()
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    hdr = open(os.path.join(here, "..", "include", "supnerf_hip.h")).read()
    assert all(re.search(r"\b" + n + r"\(", hdr) for n in INSIDE_SYMBOLS) and "Mesh containment" in hdr
    assert all(f"W{i}." in hdr for i in range(1, 7))
    spec = importlib.util.spec_from_file_location("snr_build_probe", os.path.join(here, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "snr_inside.hip" in mod.SOURCES and "snr_nearest_grid.hpp" in mod.HEADERS and "-ffp-contract=off" in mod.FLAGS
    assert "snr_inside.hip" in open(os.path.join(here, "..", "INTEGRATION.md")).read()
    # D3's device functions live in the shared header only
    for name in ("snr_nearest.hip", "snr_inside.hip"):
        src = open(os.path.join(here, "csrc", name)).read()
        assert '#include "snr_nearest_grid.hpp"' in src and "nearest_cell_of(const" not in src and "struct NearestGrid" not in src, name
    assert G.SignedDistance._fields == ("distance", "closest", "winding")
    assert G.IoU._fields == ("iou", "intersection", "union", "count_a", "count_b") and G.CONTAIN_RULES == IR.RULES
    assert list(inspect.signature(G.winding_number).parameters) == ["meshes", "points", "index"]
    assert list(inspect.signature(G.contains).parameters) == ["meshes", "points", "index", "rule"]
    assert list(inspect.signature(G.signed_distance).parameters) == ["meshes", "points", "index", "rule"]
    assert list(inspect.signature(G.voxelize).parameters) == ["meshes", "resolution", "bound", "index", "rule"]
    assert list(inspect.signature(G.occupancy_iou).parameters) == ["a", "b"]
    assert list(inspect.signature(G.mesh_iou).parameters) == ["a", "b", "resolution", "bound", "rule", "index_a", "index_b"]
    assert inspect.signature(G.mesh_iou).parameters["resolution"].default == 64 and inspect.signature(G.voxelize).parameters["bound"].default == (-0.5, 0.5)
    assert list(inspect.signature(ops.mesh_inside_query).parameters) == ["mesh", "index", "points", "n_queries"]
    assert list(inspect.signature(ops.mesh_inside_lattice).parameters) == ["mesh", "index", "lat_lo", "lat_h", "n"]
    for name in ("winding_number", "contains", "signed_distance", "voxelize", "occupancy_iou", "mesh_iou"):
        assert name in G.__doc__, name
        assert name == "occupancy_iou" or "open" in getattr(G, name).__doc__.lower(), name      # what an open mesh gets is said
    # the C ABI validates before it launches: these return without touching a device
    big, p = 1 << 39, 64                                      # (p: a pointer that is not null and is never followed)

    def query(B=1, nV=4, nF=2, nQ=3, nC=8, nP=5, ptrs=(p,) * 12, out=p, bad=p):
        return lib.snr_inside_query(*ptrs, B, nV, nF, nQ, nC, nP, out, bad, None)

    def lattice(B=1, nV=4, nF=2, nC=8, nP=5, nx=2, ny=3, nz=4, ptrs=(p,) * 12, out=p, bad=p):
        return lib.snr_inside_lattice(*ptrs, B, nV, nF, nC, nP, nx, ny, nz, out, bad, None)

    assert query(nQ=0) == 0 and lattice(nx=0) == 0 and lattice(ny=0) == 0 and lattice(nz=0) == 0 and lattice(B=0) == 0
    assert query(nQ=0, ptrs=(None,) * 12, out=None) == 0 and lattice(nz=0, ptrs=(None,) * 12, out=None) == 0
    for fn, sizes in ((query, ("B", "nV", "nF", "nQ", "nC", "nP")), (lattice, ("B", "nV", "nF", "nC", "nP", "nx", "ny", "nz"))):
        for name in sizes:
            assert fn(**{name: -1}) == -1, (fn.__name__, name)
            assert fn(**{name: big}) == -5, (fn.__name__, name)
        for i in range(12):
            assert fn(ptrs=(p,) * i + (None,) + (p,) * (11 - i)) == -1, (fn.__name__, i)
        assert fn(out=None) == -1 and fn(bad=None) == -1, fn.__name__
    assert query(B=0) == -1                                                          # rows but no objects
    assert lattice(nx=1 << 20, ny=1 << 20, nz=1) == -5 and lattice(B=1 << 10, nx=1 << 10, ny=1 << 10, nz=1 << 10) == -5   # 2^40 points
    # without faces and pairs the mesh and the lists may be null
    none = (None, None) + (p,) * 9 + (None,)
    assert query(nF=0, nP=0, nQ=0, ptrs=none) == 0


def test_python_argument_errors_without_a_device():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    verts, faces = IR.box12(HALF)
    mesh = (torch.from_numpy(verts), torch.from_numpy(faces))
    pts = torch.zeros(5, 3)
    for call in (lambda: G.winding_number(mesh, pts), lambda: G.contains([mesh, mesh], [pts, pts]), lambda: G.signed_distance(mesh, pts),
                 lambda: G.voxelize(mesh, 8), lambda: G.mesh_iou(mesh, mesh, 8), lambda: G.mesh_iou([mesh], [mesh], 8, bound=(-0.5, 0.5))):
        with pytest.raises(A.SnrError, match="GPU|gpu|CPU|device"):
            call()                                                                   # CPU tensors: no fallback
    for call in (lambda: G.contains(mesh, pts, rule="even"), lambda: G.signed_distance(mesh, pts, rule=""), lambda: G.voxelize(mesh, 8, rule="any"),
                 lambda: G.mesh_iou(mesh, mesh, rule="evenodd")):
        with pytest.raises(A.SnrError, match="rule"):
            call()
    with pytest.raises(A.SnrError, match="resolution"):
        G.mesh_iou(mesh, mesh, resolution=0)
    with pytest.raises(A.SnrError, match="object by object"):
        G.mesh_iou([mesh, mesh], [mesh])
    with pytest.raises(A.SnrError, match="object by object"):
        G.mesh_iou(mesh, [mesh])
    with pytest.raises(A.SnrError, match="no meshes"):
        G.mesh_iou([], [])
    assert G.winding_number([], []) == [] and G.contains([], []) == [] and G.signed_distance([], []) == [] and G.voxelize([], 8) == []
