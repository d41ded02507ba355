"""Mesh distance on the host: the rules of include/supnerf_hip.h ("Mesh distance") as tests/nearest_restatement.py restates them, held
against results known by hand or in closed form -- one triangle with a query in each region, faces without area, the distance to an
axis-parallel box, two boxes a fixed offset apart, the ring search of D4 against the brute force of D2 (bit for bit, at 1, 4 and 9
cells per axis, with queries outside the grid, a float64 ulp from cell planes, faces lying exactly in cell planes and an exact tie), the
stratified sample counts -- with planted mistakes that the same checks reject; and the parts of the API that need no GPU (symbols, the
argument checks of the C ABI and of the Python layer)."""
import functools
import inspect

import numpy as np
import pytest
import torch

import nearest_restatement as NR
import simplify_restatement as SR
from segment_sum_restatement import same_bits

F32 = np.float32
HALF = (0.25, 0.2, 0.15)
HALF32 = np.asarray(HALF, F32).astype(np.float64)            # the box the fp32 vertices really span
TRI, REGIONS = NR.TRI, NR.REGIONS


@functools.lru_cache(maxsize=None)
def _box():
    verts, faces = SR.box_mesh(HALF, 8)
    assert faces.shape == (768, 3)
    queries = NR.box_queries(HALF)
    assert queries.shape == (450, 3)
    return verts, faces, queries, NR.brute_force(verts, faces, queries)


def _same(a, b):
    return bool(np.array_equal(a["face"], b["face"]) and same_bits(a["dist2"], b["dist2"]).all() and
                same_bits(a["weights64"], b["weights64"]).all())


# ------------------------------------------------------------------ D1
def _triangle_failures(planted=None):
    failed = []
    for p, region, w, d2 in REGIONS:
        gw, gd = NR.point_triangle(np.asarray(p, np.float64), TRI[0], TRI[1], TRI[2], planted)
        if NR.region_of(p, *TRI) != region:
            failed.append(f"region of {p}")
        if gw.tolist() != list(map(float, w)) or float(gd) != d2:
            failed.append(f"{p}: weights {gw.tolist()} d2 {float(gd)}")
    return failed


def test_one_triangle_each_region():
    assert {r for _, r, _, _ in REGIONS} == {"a", "b", "ab", "c", "ac", "bc", "interior"}
    assert _triangle_failures() == []


def _segment_distance2(p, s0, s1):
    d = s1 - s0
    t = 0.0 if not d.any() else float(np.clip(((p - s0) * d).sum() / (d * d).sum(), 0.0, 1.0))
    return float(((p - (s0 + t * d)) ** 2).sum())


def test_faces_without_area():
    """Coincident corners and exactly collinear corners in every order give the distance to the segment or the point, never a NaN."""
    z, x1, x2 = np.zeros(3), np.array([1.0, 0, 0]), np.array([2.0, 0, 0])
    for tri in ((z, z, x1), (z, x1, z), (x1, z, z), (z, z, z), (z, x1, x2), (z, x2, x1), (x1, z, x2), (x2, x1, z)):
        lo, hi = min(t[0] for t in tri), max(t[0] for t in tri)
        for p in ((0.5, 1, 0), (1.5, 2, 0), (3, 0, 4), (-1, 0, 0), (0, 0, 0), (1, 0, 0), (0.75, 0, 0), (2, 0, -0.5)):
            w, d2 = NR.point_triangle(np.asarray(p, np.float64), *tri)
            want = _segment_distance2(np.asarray(p, np.float64), np.array([lo, 0, 0]), np.array([hi, 0, 0]))
            assert np.isfinite(d2) and float(d2) == want and abs(w.sum() - 1.0) < 1e-15 and (w >= 0).all(), (tri, p, float(d2), want)
    # segments in general position (dyadic coordinates, so collinear exactly): the third corner anywhere on the line through the two
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(300):
        s0, d = rng.integers(-8, 9, 3) / 8.0, rng.integers(-8, 9, 3) / 8.0
        ts = np.array([0.0, 1.0, rng.integers(0, 9) / 8.0])
        corners = [s0 + t * d for t in ts[rng.permutation(3)]]
        p = rng.integers(-16, 17, 3) / 8.0
        _, d2 = NR.point_triangle(p, *corners)
        assert np.isfinite(d2)
        worst = max(worst, abs(float(d2) - _segment_distance2(p, s0, s0 + d)))
    assert worst <= 1e-12, worst


# ------------------------------------------------------------------ D2 against closed forms
def test_box_distance_closed_form():
    verts, faces, queries, brute = _box()
    err = np.abs(np.sqrt(brute["dist2"]) - NR.box_distance(queries, HALF32))
    print("box: largest error", err.max())
    assert (brute["face"] >= 0).all() and err.max() <= 2e-7
    # the closest point, from the fp32 weights, lies on the box and at that distance
    c = NR.closest_points(verts, faces, brute)
    assert np.abs(NR.box_distance(c, HALF32)).max() <= 2e-7
    assert np.abs(np.linalg.norm(queries.astype(np.float64) - c, axis=1) - np.sqrt(brute["dist2"])).max() <= 2e-7


DELTA = 2.0 ** -6


@functools.lru_cache(maxsize=None)
def _offset_case(n=600):
    """The box and the same box with every half-extent larger by DELTA; n samples of each from default_rng(9), cum = numpy's cumsum."""
    inner = SR.box_mesh(HALF, 8)
    outer = SR.box_mesh(tuple(h + DELTA for h in HALF), 8)
    rng = np.random.default_rng(9)
    out = []
    for mesh in (inner, outer):
        u = rng.random((n, 3))
        out.append((mesh, u, np.cumsum(NR.face_areas(*mesh))))
    return out


def _offset_failures(planted=None):
    """Bounds.  A coordinate of a sample, and a half-extent of either box, is rounded to fp32 once: 2^-26 (half an ulp below 1/2) each.
    The distance from an inner sample to the outer box is DELTA plus at most three such roundings on one axis, and on the other two axes
    nothing (the sample projects inside the outer side): 1e-7 covers 3 x 1.5e-8 with room for float64.  The closed form of the other
    direction reads the same rounded numbers on up to three axes: sqrt(3) x 3 x 1.5e-8 < 1e-7 too."""
    (inner, ui, cumi), (outer, uo, cumo) = _offset_case()
    si, so = NR.sample(*inner, cumi, ui, planted), NR.sample(*outer, cumo, uo, planted)
    failed = []
    d = np.sqrt(NR.brute_force(*outer, si["points"])["dist2"])
    if not (abs(d.mean() - DELTA) <= 1e-7 and abs(np.sqrt((d * d).mean()) - DELTA) <= 1e-7 and abs(d.max() - DELTA) <= 1e-7 and
            abs(d.min() - DELTA) <= 1e-7):
        failed.append(f"inner to outer: mean {d.mean()}, max {d.max()}, min {d.min()}")
    back = np.sqrt(NR.brute_force(*inner, so["points"])["dist2"])
    want = NR.box_distance(so["points"], HALF32)
    if not (np.abs(back - want).max() <= 1e-7 and back.min() >= DELTA - 1e-7 and back.max() <= DELTA * np.sqrt(3.0) + 1e-7):
        failed.append(f"outer to inner: error {np.abs(back - want).max()}, range {back.min()} .. {back.max()}")
    if not (back.max() > DELTA * 1.2):
        failed.append("outer to inner: no sample near an edge or corner")          # (the case itself)
    # the samples lie on their surface, and within their face the way a uniform draw does: E[w] = (1/3, 1/3, 1/3); a draw that is
    # linear in u1 has E[w0] = 1/2.  n = 600: the standard error of a mean weight is 0.236 / sqrt(600) < 0.01
    for s, half in ((si, HALF32), (so, HALF32 + DELTA)):
        if np.abs(NR.box_distance(s["points"], half)).max() > 1e-7:
            failed.append("samples off the surface")
        if np.abs(s["weights"].astype(np.float64).mean(0) - 1.0 / 3.0).max() > 0.04:
            failed.append(f"weights are not uniform: mean {s['weights'].mean(0)}")
    return failed


def test_offset_boxes():
    assert _offset_failures() == []


# ------------------------------------------------------------------ D3 and D4
def _cell(k):
    return float(F32(0.5 / k))


def _plane_queries(verts, h, rng):
    """float64 queries 0 to 3 float64 ulps on either side of every interior cell plane of the grid, elsewhere random around the box."""
    g = NR.grid(verts, h)
    out = []
    for a in range(3):
        for j in range(1, int(g["n"][a])):
            plane = g["lo"][a] + j * g["h"]
            for steps in range(-3, 4):
                x = plane
                for _ in range(abs(steps)):
                    x = np.nextafter(x, np.inf if steps > 0 else -np.inf)
                p = rng.uniform(-1.3, 1.3, 3) * np.asarray(HALF)
                p[a] = x
                out.append(p)
    return np.asarray(out, np.float64)


@pytest.mark.parametrize("k", [1, 4, 9])
def test_ring_search_equals_brute_force(k):
    verts, faces, queries, brute = _box()
    ring = NR.ring_search(verts, faces, queries, _cell(k))
    assert _same(ring, brute), np.nonzero(ring["face"] != brute["face"])[0][:10]
    g = NR.grid(verts, _cell(k))
    outside = ((queries < g["lo"]) | (queries > g["hi"])).any(1)
    assert outside.sum() >= 100                                                     # queries outside the grid are among them
    if k == 1:
        assert g["n"].tolist() == [1, 1, 1] and (ring["tested"] == 768).all()
    else:
        print(f"{k} cells: {g['n'].tolist()}, faces tested per query: mean {ring['tested'].mean():.0f}, max {ring['tested'].max()}")
        # the grid prunes: a query on the surface (the last 30) finds it in its own cell and stops after the ring around it, 27 cells of
        # the k^3; repeats are counted, so queries deep inside or far away may test more than 768
        assert g["n"][0] in (k, k + 1) and np.median(ring["tested"][-30:]) < 768 / 2 and ring["rings"][-30:].max() <= 2
        near = _plane_queries(verts, _cell(k), np.random.default_rng(k))
        assert _same(NR.ring_search(verts, faces, near, _cell(k)), NR.brute_force(verts, faces, near))


def _ring_failures(planted=None):
    """The ring search with a planted mistake against the brute force without one: the box at 4 cells (x planes at multiples of 1/8:
    every fourth column of vertices, and the faces of the sides x = +-1/4, lie exactly in cell planes), the sheets and the roof."""
    verts, faces, queries, brute = _box()
    failed = []
    sub = slice(0, 450, 3)
    ring = NR.ring_search(verts, faces, queries[sub], _cell(4), planted)
    if not _same(ring, {k: v[sub] for k, v in brute.items()}):
        failed.append("box at 4 cells")
    sv, sf, sq = NR.sheets_mesh()
    g = NR.grid(sv, 0.25)
    lists = NR.cell_lists(sv, sf, g)
    want = NR.brute_force(sv, sf, sq)
    got = NR.ring_search(sv, sf, sq, 0.25, planted)
    in_plane = all(0 in lists.get((2 * 4 + y) * 4 + z, []) and 0 not in lists.get((1 * 4 + y) * 4 + z, []) for y in range(2) for z in range(2))
    if not (g["n"].tolist() == [4, 4, 4] and in_plane and want["face"].tolist() == [0] and want["dist2"].tolist() == [2.0 ** -8]):
        failed.append("the sheets case itself")
    if not (_same(got, want) and got["rings"].tolist() == [2]):
        failed.append(f"sheets: face {got['face'].tolist()} after {got['rings'].tolist()} rings")
    rv, rf = NR.roof_mesh()
    rq = np.array([[0.5, 0.0, 1.0], [0.25, 0.0, 0.5]], F32)
    d2 = [NR.point_triangle(rq.astype(np.float64), *rv[rf[i]].astype(np.float64))[1] for i in range(2)]
    if not (same_bits(d2[0], d2[1]).all() and d2[0].tolist() == [1.0, 0.25]):
        failed.append("the roof case itself")
    for h in (4.0, 0.5):
        got = NR.ring_search(rv, rf, rq, h, planted)
        if got["face"].tolist() != [0, 0] or not _same(got, NR.brute_force(rv, rf, rq)):
            failed.append(f"roof at cell {h}: face {got['face'].tolist()}")
    if NR.brute_force(rv, rf, rq, planted)["face"].tolist() != [0, 0]:
        failed.append("roof, brute force")
    return failed


def test_planes_sheets_and_ties():
    assert _ring_failures() == []


def test_grid_and_lists():
    """D3 on the box: the anchor, the cell counts, clamping, and a face on a plane belongs to the upper cell."""
    verts, faces, _, _ = _box()
    g = NR.grid(verts, 0.125)
    assert g["lo"].tolist() == (-HALF32).tolist() and g["n"].tolist() == [4, 4, 3] and g["extent"] == 0.5
    assert NR.cell_of(g, np.array([[-9.0, 9.0, np.nan], [-0.25, -0.125, 0.0], [0.25, 0.0, 0.15]])).tolist() == [[0, 3, 0], [0, 0, 1], [3, 1, 2]]
    assert NR.grid(verts, 1e-4)["n"].tolist() == [256, 256, 256] and NR.grid(np.zeros((0, 3)), 1.0)["n"].tolist() == [1, 1, 1]
    counts = NR.cell_counts(verts, faces, g)
    cells, fs = NR.pairs(verts, faces, g)
    assert counts.sum() == len(cells) and np.array_equal(np.bincount(fs, minlength=768), counts) and counts.min() >= 1
    lists = NR.cell_lists(verts, faces, g)
    assert sum(len(v) for v in lists.values()) == len(cells) and all(v == sorted(v) for v in lists.values())
    bad = faces.copy()
    bad[5, 1] = 10 ** 6
    nan = verts.copy()
    nan[faces[7, 2], 0] = np.nan
    assert NR.cell_counts(verts, bad, g)[5] == 0 and (NR.cell_counts(nan, faces, NR.grid(verts, 0.125)) == 0).sum() >= 1


# ------------------------------------------------------------------ D5
def _strata_failures(planted=None):
    verts, faces = SR.box_mesh(HALF, 4)
    flat = np.array([[0, 0, 1], [2, 2, 2], [0, 1, 0]], np.int32)                     # faces without area: in front, inside and at the end
    faces = np.concatenate([flat[:1], faces[:50], flat[1:2], faces[50:], flat[2:], flat[:1]])
    area = NR.face_areas(verts, faces)
    cum = np.cumsum(area)
    failed = []
    for n in (1, 7, 1000, 4093):
        s = NR.sample(verts, faces, cum, np.random.default_rng(n).random((n, 3)), planted)
        count = np.bincount(s["face"], minlength=len(faces))
        if not (np.abs(count - n * area / area.sum()) < 2).all():
            failed.append(f"n = {n}: counts off by {np.abs(count - n * area / area.sum()).max()}")
        if count[area == 0].any() or (s["face"] < 0).any():
            failed.append(f"n = {n}: a sample on a face without area")
    # u0 so close to 1 that the target rounds to the whole area: the last face WITH area, not the last face
    s = NR.sample(verts, faces, cum, np.array([[1.0 - 2.0 ** -53, 0.25, 0.5]]))
    if not (s["face"].tolist() == [len(faces) - 3] and area[-3] > 0 and area[-2] == 0 and area[-1] == 0):
        failed.append(f"the last stratum: face {s['face'].tolist()}")
    s = NR.sample(verts, faces, cum, np.array([[0.0, 0.25, 0.5]]))
    if s["face"].tolist() != [1]:
        failed.append(f"the first stratum: face {s['face'].tolist()}")
    w = NR.sample(verts, faces, cum, np.array([[0.5, 0.25, 0.5]]), planted)["weights"]
    if w.tolist() != [[0.5, 0.25, 0.25]]:
        failed.append(f"weights {w.tolist()}")                                   # s = sqrt(1/4) = 1/2: (1/2, 1/4, 1/4)
    none = NR.sample(verts, flat, np.zeros(3), np.random.default_rng(0).random((5, 3)))
    if not ((none["face"] == -1).all() and (none["points"] == 0).all() and (none["weights"] == 0).all()):
        failed.append("a mesh without area")
    return failed


def test_stratified_samples():
    assert _strata_failures() == []


# ------------------------------------------------------------------ planted mistakes
CHECKS = {"triangle": _triangle_failures, "ring": _ring_failures, "offset": _offset_failures, "strata": _strata_failures}
REJECTED_BY = {"stop_ge_no_slack": "ring", "centroid_cell_only": "ring", "tie_high": "ring", "edge_to_vertex": "triangle", "s_linear": "offset"}


@pytest.mark.parametrize("planted", NR.PLANTED)
def test_planted_mistakes_are_rejected(planted):
    assert set(REJECTED_BY) == set(NR.PLANTED)
    failed = CHECKS[REJECTED_BY[planted]](planted)
    print(planted, failed)
    assert failed, planted
    if planted == "stop_ge_no_slack":
        assert any(f.startswith("sheets") for f in failed)
    if planted == "tie_high":
        assert any(f.startswith("roof") for f in failed)
    if planted == "s_linear":
        assert _strata_failures(planted) != []                                   # (the weights (1/2, 1/4, 1/4) of s = sqrt(1/4) too)


# ------------------------------------------------------------------ the API without a GPU
NEAREST_SYMBOLS = ("snr_nearest_count", "snr_nearest_emit", "snr_nearest_query", "snr_surface_sample")


def test_symbols_and_c_abi_checks():
    import importlib.util
    import os
    import re
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, geometry as G, ops
    assert all(n in _lib.exported_symbols() for n in NEAREST_SYMBOLS)
    assert sum(n.startswith(("snr_nearest", "snr_surface")) for n in _lib.exported_symbols()) == 4
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in NEAREST_SYMBOLS)
    assert _lib.header_abi_version() >= 25 and lib.snr_abi_version() == _lib.header_abi_version()
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    hdr = open(os.path.join(here, "..", "include", "supnerf_hip.h")).read()
    assert all(re.search(r"\b" + n + r"\(", hdr) for n in NEAREST_SYMBOLS) and "Mesh distance" in hdr
    assert all(f"D{i}." in hdr for i in range(1, 6))
    spec = importlib.util.spec_from_file_location("snr_build_probe", os.path.join(here, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "snr_nearest.hip" in mod.SOURCES and "-ffp-contract=off" in mod.FLAGS
    assert "snr_nearest.hip" in open(os.path.join(here, "..", "INTEGRATION.md")).read()
    assert G.Closest._fields == ("point", "face", "weights", "distance") and G.SurfaceSamples._fields == ("points", "face", "weights")
    assert G.MeshIndex._fields == ("mesh", "grid") and {"chamfer", "hausdorff", "precision", "recall", "fscore"} <= set(G.MeshDistance._fields)
    assert list(inspect.signature(G.mesh_index).parameters) == ["meshes", "cell"]
    assert list(inspect.signature(G.closest_point).parameters) == ["meshes", "points", "index"]
    assert list(inspect.signature(G.sample_surface).parameters) == ["meshes", "n", "generator"]
    assert list(inspect.signature(G.mesh_distance).parameters)[:5] == ["a", "b", "n", "generator", "threshold"]
    assert ops.NEAREST_MAX_CELLS == NR.MAX_CELLS and ops.NEAREST_MAX_PAIRS > 0 and ops.NEAREST_CELL_FACTOR > 0
    for name in ("closest_point", "mesh_index", "sample_surface", "mesh_distance"):
        assert name in G.__doc__
    # the C ABI validates before it launches: these return without touching a device
    big, p = 1 << 39, 64                                      # (p: a pointer that is not null and is never followed)

    def count(B=1, nV=4, nF=2, nC=8, ptrs=(p,) * 8, out=p, bad=p):
        return lib.snr_nearest_count(*ptrs, B, nV, nF, nC, out, bad, None)

    def emit(B=1, nV=4, nF=2, nC=8, nP=5, ptrs=(p,) * 9, cells=p, faces=p):
        return lib.snr_nearest_emit(*ptrs, B, nV, nF, nC, nP, cells, faces, None)

    def query(B=1, nV=4, nF=2, nQ=3, nC=8, nP=5, ptrs=(p,) * 12, outs=(p,) * 3, bad=p):
        return lib.snr_nearest_query(*ptrs, B, nV, nF, nQ, nC, nP, *outs, bad, None)

    def sample(B=1, nV=4, nF=2, nS=3, ptrs=(p,) * 7, outs=(p,) * 3, bad=p):
        return lib.snr_surface_sample(*ptrs, B, nV, nF, nS, *outs, bad, None)

    assert count(nF=0) == 0 and emit(nF=0) == 0 and emit(nP=0) == 0 and query(nQ=0) == 0 and sample(nS=0) == 0
    for fn, sizes in ((count, ("B", "nV", "nF", "nC")), (emit, ("B", "nV", "nF", "nC", "nP")), (query, ("B", "nV", "nF", "nQ", "nC", "nP")),
                      (sample, ("B", "nV", "nF", "nS"))):
        for name in sizes:
            assert fn(**{name: -1}) == -1, (fn.__name__, name)
            assert fn(**{name: big}) == -5, (fn.__name__, name)
        assert fn(B=0) == -1, fn.__name__                                            # rows but no objects
        n = len(inspect.signature(fn).parameters["ptrs"].default)
        for i in range(n):
            assert fn(ptrs=(p,) * i + (None,) + (p,) * (n - 1 - i)) == -1, (fn.__name__, i)
    assert count(out=None) == -1 and count(bad=None) == -1 and emit(cells=None) == -1 and emit(faces=None) == -1
    assert query(bad=None) == -1 and sample(bad=None) == -1
    for i in range(3):
        outs = (p,) * i + (None,) + (p,) * (2 - i)
        assert query(outs=outs) == -1 and sample(outs=outs) == -1


def test_python_argument_errors_without_a_device():
    import supnerf_amd as A
    from supnerf_amd import geometry as G, ops
    verts, faces = SR.box_mesh(HALF, 2)
    mesh = (torch.from_numpy(verts), torch.from_numpy(faces))
    pts = torch.zeros(5, 3)
    for call in (lambda: G.mesh_index(mesh), lambda: G.mesh_index([mesh], 0.1), lambda: G.closest_point(mesh, pts),
                 lambda: G.closest_point([mesh, mesh], [pts, pts]), lambda: G.sample_surface(mesh, 10), lambda: G.mesh_distance(mesh, mesh, n=10)):
        with pytest.raises(A.SnrError, match="GPU|gpu|CPU|device"):
            call()                                                                   # CPU tensors: no fallback
    with pytest.raises(A.SnrError, match="negative"):
        G.sample_surface(mesh, -1)
    with pytest.raises(A.SnrError, match="positive"):
        G.mesh_distance(mesh, mesh, n=0)
    with pytest.raises(A.SnrError, match="threshold"):
        G.mesh_distance(mesh, mesh, threshold=-1.0)
    with pytest.raises(A.SnrError, match="object by object"):
        G.mesh_distance([mesh, mesh], [mesh])
    with pytest.raises(A.SnrError, match="object by object"):
        G.mesh_distance(mesh, [mesh])
    assert G.closest_point([], []) == [] and G.sample_surface([], 5) == []
    with pytest.raises(A.SnrError, match="no meshes"):
        G.mesh_index([])
    with pytest.raises(A.SnrError, match="GPU|gpu"):
        ops.object_sums(torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), [3])
