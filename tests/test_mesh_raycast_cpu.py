"""Mesh ray casting on the host: the rules of include/supnerf_hip.h ("Mesh ray casting", R1 - R6) as tests/raycast_restatement.py restates
them, held against results known by hand or in closed form -- one triangle hit from both sides, rays through every shared edge and vertex
of two triangles and of a fan, rays in the plane of a face and at faces that never count, the axis-parallel box against the slab method,
strict bounds exactly at a hit, crossings against the winding numbers of "Mesh containment", the pruned walk against the brute force
(bit for bit: faces that span many cells, rays outside the grid, in cell planes, one cell, a clamped axis, a t_max inside the object)
-- with planted mistakes that the same checks reject; and the parts of the API that need no GPU (symbols, the argument checks of the C
ABI and of the Python layer)."""
import functools
import inspect

import numpy as np
import pytest
import torch

import inside_restatement as IR
import nearest_restatement as NR
import raycast_restatement as RR

F32 = np.float32
INF = np.inf
HALF = (0.25, 0.2, 0.15)
HALF32 = np.asarray(HALF, F32).astype(np.float64)            # the box the fp32 vertices really span
# crossings against winding numbers: +z and two more directions.  A query that lies ON the surface (sphere_case puts some on vertices of
# the equator) has no direction-free answer; W gives those 0, and a ray from them that stays within the facets' slope of the vertical
# stays outside as well.  So the fixed directions are generic but steep; the strongly oblique ones below run on the random queries.
WINDING_DIRECTIONS = ((0.0, 0.0, 1.0), (0.013, -0.021, 1.0), (-0.017, 0.011, -1.0))
OBLIQUE_DIRECTIONS = ((0.3, -0.5, 0.8), (-0.7, 0.2, -0.4), (1.0, 0.25, 0.125))


def _case(cases, name):
    return next(c for c in cases if c[0] == name)


def _hand_failures(planted=None):
    """The hand cases; a list of the ones that fail."""
    failed = []
    bf = functools.partial(RR.brute_force, planted=planted)
    cases = RR.hand_cases()

    def run(name, cull=None):
        c = [c for c in cases if c[0] == name and (cull is None or c[7] == cull)][0]
        return bf(*c[1:])

    # one triangle, counter-clockwise seen from +z (n = +z): from below the ray leaves through it (back, sigma = +1), from above it
    # enters (front, sigma = -1); t in units of |d|; the weights of (0.25, 0.25) in (a, b, c)
    r = run("triangle", 0)
    if not (r["face"].tolist() == [0, 0, 0, 0] and r["t"].tolist() == [0.5, 3.0, 0.5, 3.0] and r["side"].tolist() == [-1, 1, -1, 1]
            and r["signed"].tolist() == [1, -1, 1, -1] and r["total"].tolist() == [1] * 4
            and r["weights"].tolist() == [[0.5, 0.25, 0.25]] * 4):
        failed.append(f"triangle from both sides: side {r['side'].tolist()} t {r['t'].tolist()}")
    if run("triangle", 1)["face"].tolist() != [-1, 0, -1, 0] or run("triangle", 2)["face"].tolist() != [0, -1, 0, -1]:
        failed.append("triangle: cull")
    # rays through what faces share hit exactly one of them; through what lies on the border of an open mesh, one or none
    for name, mesh in (("square", IR.SQUARE), ("fan", IR.FAN)):
        inner = len(RR.shared_targets(*mesh)[0])
        assert inner == (1 if name == "square" else 7)
        for c in cases:
            if c[0].startswith(name + " "):
                r = bf(*c[1:])
                if not ((r["total"][:inner] == 1).all() and (r["face"][:inner] >= 0).all() and (r["total"] <= 1).all()
                        and (r["t"][r["face"] >= 0] == 2.0).all()):
                    failed.append(f"{c[0]}: shared edges and vertices: {r['total'].tolist()}")
    r = run("in the plane")
    if r["total"].any() or (r["face"] >= 0).any():
        failed.append("a ray in the plane of a face")
    for c in cases:
        if c[0].startswith("never"):
            r = bf(*c[1:])
            if r["total"].any() or (r["face"] >= 0).any() or not np.isinf(r["t"]).all():
                failed.append(f"{c[0]}: a face without projected area counted")
    r = run("skew")
    if r["total"].tolist() != [1]:
        failed.append(f"skew: {r['total'].tolist()}")
    r = run("doubled")
    if r["face"].tolist() != [0, -1, 0] or r["total"].tolist() != [3, 0, 3]:
        failed.append(f"doubled triangle, ties to the lowest face: {r['face'].tolist()}")
    # strict bounds exactly at a hit; a ray that starts on a face
    r = run("box strict")
    if r["t"].tolist() != [0.75, 1.25, INF, INF, 0.5, 0.75, INF] or r["total"].tolist() != [2, 1, 0, 0, 1, 2, 0]:
        failed.append(f"box, strict bounds and a start on a face: t {r['t'].tolist()} total {r['total'].tolist()}")
    failed += _box_failures(bf)
    return failed


def _box_failures(bf):
    failed = []
    verts, faces = IR.box12(HALF)
    rng = np.random.default_rng(21)
    outside = rng.uniform(-1, 1, (600, 3))
    outside = outside[(np.abs(outside) > HALF32 * 1.05).any(1)][:300]
    o, d = RR.aimed_rays(rng, outside, -0.9 * HALF32, 0.9 * HALF32, share=1.0)
    axis = np.concatenate([np.eye(3), -np.eye(3)])
    o = np.concatenate([o, (-2 * axis + rng.uniform(-0.9, 0.9, (6, 3)) * HALF32 * (axis == 0)).astype(F32)])
    d = np.concatenate([d, axis.astype(F32)])
    r = bf(verts, faces, o, d)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    enter, leave = RR.box_slab(o64, d64, HALF32)
    assert (enter < leave).all() and (enter > 0).all()
    # both are float64 evaluations on the same inputs; R6's proof needs every counted t within the slack of the exact one, so the
    # closed form is held to the slack itself: 2^-40 (E + m) / |d[kz]|
    m = np.maximum(np.abs(o64) - HALF32, 0).max(1)
    band = RR.SLACK * (2 * HALF32.max() + m) / np.abs(d64).max(1)
    err = np.abs(r["t"] - enter)
    print("box: t against the slab method: max error / band", (err / band).max())
    if not ((err <= band).all() and (r["side"] == 1).all() and (r["signed"] == 0).all() and (r["total"] == 2).all()):
        failed.append(f"box from outside against the slab method: {(err / band).max()} of the band")
    p = o64 + r["t"][:, None] * d64
    w = r["weights"].astype(np.float64)
    v64 = verts.astype(np.float64)
    if np.abs((w[:, :, None] * v64[faces[np.maximum(r["face"], 0)]]).sum(1) - p).max() > 1e-6:
        failed.append("box: the weights do not give the hit point")
    if np.abs(bf(verts, faces, o, d, cull=2)["t"] - leave).max() > band.max():
        failed.append("box: with the front faces culled the hit is the exit")
    # from inside
    inside = (rng.uniform(-0.9, 0.9, (200, 3)) * HALF32).astype(F32)
    di = rng.normal(size=(200, 3)).astype(F32)
    r = bf(verts, faces, inside, di)
    leave = RR.box_slab(inside.astype(np.float64), di.astype(np.float64), HALF32)[1]
    if not ((r["signed"] == 1).all() and (r["total"] == 1).all() and (r["side"] == -1).all() and np.abs(r["t"] - leave).max() < 1e-12):
        failed.append("box from inside")
    # through corners and edges, exactly (a box of few-bit numbers) and as nearly as fp32 origins allow
    for half in (RR.DYADIC_HALF, HALF):
        bv, bfaces = IR.box12(half)
        corners = bv.astype(np.float64)
        edges = np.array([(corners[i] + corners[j]) / 2 for i in range(8) for j in range(i + 1, 8) if bin(i ^ j).count("1") == 1])
        targets = np.concatenate([corners, edges])
        for dd in ((0.5, 0.25, 1.0), (-1.0, 0.5, 0.5), (0.25, -1.0, -0.5), (1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, -1.0, 1.0)):
            oo, dv = RR.rays_through(targets, dd)
            r = bf(bv, bfaces, oo, dv)
            if not (np.isin(r["total"], (0, 2)).all() and (r["signed"] == 0).all()):
                failed.append(f"box {half}: rays through corners and edges from outside, direction {dd}: {sorted(set(r['total'].tolist()))}")
            r = bf(bv, bfaces, np.zeros_like(oo), (targets - 0.0).astype(F32))
            if not ((r["total"] == 1).all() and (r["signed"] == 1).all()):
                failed.append(f"box {half}: rays to corners and edges from inside: {sorted(set(r['total'].tolist()))}")
    return failed


def test_hand_cases_and_closed_forms():
    assert _hand_failures() == []


def test_plane_depth_gradients_by_differences():
    """The closed-form gradients the autograd test uses as its yardstick, checked against central differences in float64."""
    rng = np.random.default_rng(5)
    x = [rng.normal(size=3) for _ in range(5)]
    t, grads = RR.plane_depth(*x)
    for k in range(5):
        for a in range(3):
            hi, lo = [v.copy() for v in x], [v.copy() for v in x]
            hi[k][a] += 1e-6
            lo[k][a] -= 1e-6
            num = (RR.plane_depth(*hi)[0] - RR.plane_depth(*lo)[0]) / 2e-6
            assert abs(num - grads[k][a]) <= 1e-6 * max(1.0, abs(num)), (k, a, num, grads[k][a])


# ------------------------------------------------------------------ crossings against winding numbers
@functools.lru_cache(maxsize=None)
def _winding_meshes():
    verts, faces, q = IR.sphere_case()
    cavity = IR.merged((verts, faces), (verts * F32(0.5), faces[:, ::-1]))
    two = IR.merged((verts, faces), ((verts + F32([0.1, 0, 0])).astype(F32), faces))
    return (("sphere", (verts, faces)), ("cavity", cavity), ("two spheres", two)), q


def _winding_failures(planted=None):
    failed = []
    meshes, q = _winding_meshes()
    for name, mesh in meshes:
        want = IR.brute_force(*mesh, q)
        assert len(set(want.tolist())) >= 2
        for d in WINDING_DIRECTIONS:
            r = RR.brute_force(*mesh, q, np.broadcast_to(F32(d), q.shape), planted=planted)
            if not np.array_equal(r["signed"], want):                                     # every query, no exclusions
                failed.append(f"{name}: signed crossings along {d} are not the winding numbers: {int((r['signed'] != want).sum())} differ")
            if not ((r["total"] - np.abs(want)) % 2 == 0).all():
                failed.append(f"{name}: parity of the crossings along {d}")
        if planted is None:
            for d in OBLIQUE_DIRECTIONS:                                                  # the random queries: none lies on the surface
                r = RR.brute_force(*mesh, q[:2000], np.broadcast_to(F32(d), (2000, 3)))
                assert np.array_equal(r["signed"], want[:2000]), (name, d)
    return failed


def test_signed_crossings_are_winding_numbers():
    assert _winding_failures() == []


# ------------------------------------------------------------------ R6: the walk is the brute force
def _walk_failures(planted=None):
    failed = []
    for name, v, f, h, o, d, lo, hi in RR.walk_cases():
        want = RR.brute_force(v, f, o, d, lo, hi)
        got, looked = RR.walk(v, f, o, d, h, lo, hi, planted=planted)
        diff = {k: int((got[k].view(np.int64 if k == "t" else got[k].dtype) != want[k].view(np.int64 if k == "t" else want[k].dtype)).sum())
                for k in want}
        diff["weights"] = int((got["weights"].view(np.int32) != want["weights"].view(np.int32)).sum())
        if any(diff.values()):
            failed.append(f"{name}: {diff}")
        if planted is None:
            print(name, ": rays", len(o), "hits", int((want["face"] >= 0).sum()), "faces looked at per ray", looked.mean(), "of", len(f))
            g = NR.grid(v, h)
            if name == "octahedron at 16 cells":
                flo, fhi, _ = NR.face_boxes(v, f, g)
                assert g["n"].tolist() == [16, 16, 16] and (fhi - flo + 1).min() >= 8       # every face spans eight cells each way
                assert (want["face"] >= 0).sum() > 100 and (want["total"] == 1).sum() > 20 and (want["total"] == 2).sum() > 50
            if name == "octahedron, one cell":
                assert g["n"].tolist() == [1, 1, 1]
            if name == "thin octahedron, a clamped axis":
                assert g["n"].tolist() == [16, 16, 256]
            if name == "octahedron, rays that miss the bounds":
                assert looked.sum() == 0 and not (want["face"] >= 0).any()
            if name == "octahedron, t_max inside":
                full = RR.brute_force(v, f, o, d)
                assert ((want["face"] < 0) & (full["face"] >= 0)).sum() > 20 and (want["face"] >= 0).sum() > 20
            if name == "octahedron, rays in cell planes":
                assert (want["face"] >= 0).sum() > 150
            if name == "sphere":
                assert looked.sum() < len(f) * len(o) / 8, "the walk does not prune"
    return failed


def test_walk_equals_brute_force():
    assert _walk_failures() == []


# ------------------------------------------------------------------ planted mistakes
REJECTED_BY = {"stored_order": "skew", "no_fallback": "square", "tmin_le": "start on a face", "tie_high": "doubled triangle",
               "stop_at_first_hit": "roof", "every_cell": "octahedron at 16 cells", "unswapped": "triangle from both sides"}


@pytest.mark.parametrize("planted", RR.PLANTED)
def test_planted_mistakes_are_rejected(planted):
    assert set(REJECTED_BY) == set(RR.PLANTED) and len(RR.PLANTED) >= 6
    failed = _walk_failures(planted) if planted in ("stop_at_first_hit", "every_cell") else _hand_failures(planted)
    print(planted, failed)
    assert any(REJECTED_BY[planted] in f for f in failed), (planted, failed)


def test_unswapped_frame_breaks_the_winding_number():
    failed = _winding_failures("unswapped")
    assert any("-1.0)" in f for f in failed), failed


# ------------------------------------------------------------------ the API without a GPU
RAYCAST_SYMBOLS = ("snr_raycast_first", "snr_raycast_crossings")


def test_symbols_and_c_abi_checks():
    import importlib.util
    import os
    import re
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, geometry as G, ops
    assert all(n in _lib.exported_symbols() for n in RAYCAST_SYMBOLS)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in RAYCAST_SYMBOLS)
    assert _lib.header_abi_version() >= 27 and lib.snr_abi_version() == _lib.header_abi_version()
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    hdr = open(os.path.join(here, "..", "include", "supnerf_hip.h")).read()
    assert all(re.search(r"\b" + n + r"\(", hdr) for n in RAYCAST_SYMBOLS) and "Mesh ray casting" in hdr
    assert all(f"R{i}." in hdr for i in range(1, 7)) and "Why this cannot change the result" in hdr[hdr.index("Mesh ray casting"):]
    spec = importlib.util.spec_from_file_location("snr_build_probe", os.path.join(here, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "snr_raycast.hip" in mod.SOURCES and "-ffp-contract=off" in mod.FLAGS
    assert "snr_raycast.hip" in open(os.path.join(here, "..", "INTEGRATION.md")).read()
    src = open(os.path.join(here, "csrc", "snr_raycast.hip")).read()
    assert '#include "snr_nearest_grid.hpp"' in src and "nearest_cell_of(const" not in src and "struct NearestGrid" not in src
    assert G.MeshHits._fields == ("t", "face", "weights", "side", "point", "normal")
    sig = {n: inspect.signature(getattr(G, n)) for n in ("ray_mesh", "ray_crossings", "visible", "mesh_depth")}
    assert list(sig["ray_mesh"].parameters) == ["meshes", "rays_o", "rays_d", "t_min", "t_max", "cull", "index", "face_forward"]
    assert list(sig["ray_crossings"].parameters) == ["meshes", "rays_o", "rays_d", "t_min", "t_max", "index"]
    assert list(sig["visible"].parameters) == ["meshes", "points", "eye", "offset", "index"]
    assert list(sig["mesh_depth"].parameters) == ["meshes", "cam_pose", "obj_diag", "K", "roi", "im_sz", "pixels", "cull", "family",
                                                  "shapenet_obj_cood", "kitti2nusc", "index"]
    for name, first_keyword in (("ray_mesh", "t_min"), ("ray_crossings", "t_min"), ("visible", "offset"), ("mesh_depth", "im_sz")):
        kinds = [p.kind for p in sig[name].parameters.values()]
        at = list(sig[name].parameters).index(first_keyword)
        assert all(k == inspect.Parameter.POSITIONAL_OR_KEYWORD for k in kinds[:at]) and all(k == inspect.Parameter.KEYWORD_ONLY for k in kinds[at:])
    p = sig["ray_mesh"].parameters
    assert (p["t_min"].default, p["t_max"].default, p["cull"].default, p["index"].default, p["face_forward"].default) == (0.0, INF, None, None, False)
    assert sig["mesh_depth"].parameters["cull"].default == "back" and sig["visible"].parameters["offset"].default == 0.0
    assert list(inspect.signature(ops.mesh_raycast_first).parameters) == ["mesh", "index", "rays_o", "rays_d", "t_min", "t_max", "n_rays", "cull"]
    assert list(inspect.signature(ops.mesh_raycast_crossings).parameters) == ["mesh", "index", "rays_o", "rays_d", "t_min", "t_max", "n_rays"]
    for name in ("MeshHits", "ray_mesh", "ray_crossings", "visible", "mesh_depth"):
        assert name in G.__doc__, name
    assert "open" in G.ray_mesh.__doc__ and "offset" in G.visible.__doc__ and "R4" in G.visible.__doc__
    # the C ABI validates before it launches: these return without touching a device
    big, p = 1 << 39, 64                                      # (p: a pointer that is not null and is never followed)

    def first(B=1, nV=4, nF=2, nR=3, nC=8, nP=5, ptrs=(p,) * 15, cull=0, out=(p,) * 4, bad=p):
        return lib.snr_raycast_first(*ptrs, B, nV, nF, nR, nC, nP, cull, *out, bad, None)

    def crossings(B=1, nV=4, nF=2, nR=3, nC=8, nP=5, ptrs=(p,) * 15, out=(p,) * 2, bad=p):
        return lib.snr_raycast_crossings(*ptrs, B, nV, nF, nR, nC, nP, *out, bad, None)

    for fn, n_out in ((first, 4), (crossings, 2)):
        assert fn(nR=0) == 0 and fn(nR=0, ptrs=(None,) * 15, out=(None,) * n_out) == 0
        for name in ("B", "nV", "nF", "nR", "nC", "nP"):
            assert fn(**{name: -1}) == -1, (fn.__name__, name)
            assert fn(**{name: big}) == -5, (fn.__name__, name)
        for i in range(15):
            assert fn(ptrs=(p,) * i + (None,) + (p,) * (14 - i)) == -1, (fn.__name__, i)
        for i in range(n_out):
            assert fn(out=(p,) * i + (None,) + (p,) * (n_out - 1 - i)) == -1, (fn.__name__, i)
        assert fn(bad=None) == -1 and fn(B=0) == -1                                  # rays but no objects
        # without faces and pairs the mesh and the lists may be null
        assert fn(nF=0, nP=0, nR=0, ptrs=(None, None) + (p,) * 12 + (None,)) == 0
    assert first(cull=3) == -1 and first(cull=-1) == -1 and first(cull=3, nR=0) == -1 and first(cull=2, nR=0) == 0


def test_python_argument_errors_without_a_device():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    verts, faces = IR.box12(HALF)
    mesh = (torch.from_numpy(verts), torch.from_numpy(faces))
    o, d = torch.zeros(5, 3), torch.ones(5, 3)
    pose = torch.eye(4)[:3]
    K = np.array([[100.0, 0, 32], [0, 100.0, 32], [0, 0, 1]])
    for call in (lambda: G.ray_mesh(mesh, o, d), lambda: G.ray_mesh([mesh, mesh], [o, o], [d, d]), lambda: G.ray_crossings(mesh, o, d),
                 lambda: G.visible(mesh, o, torch.ones(3)), lambda: G.mesh_depth(mesh, pose, 1.0, K, (0, 0, 64, 64))):
        with pytest.raises(A.SnrError, match="GPU|gpu|CPU|device"):
            call()                                                                   # CPU tensors: no fallback
    for call in (lambda: G.ray_mesh(mesh, o, d, cull="both"), lambda: G.ray_mesh(mesh, o, d, cull=1),
                 lambda: G.mesh_depth(mesh, pose, 1.0, K, (0, 0, 64, 64), cull="none")):
        with pytest.raises(A.SnrError, match="cull"):
            call()
    for call in (lambda: G.ray_mesh([mesh, mesh], [o], [d]), lambda: G.ray_mesh([mesh, mesh], o, d), lambda: G.ray_mesh(mesh, [o, o], [d, d]),
                 lambda: G.ray_crossings([mesh, mesh], [o, o], [d]), lambda: G.ray_mesh(mesh, o, [d])):
        with pytest.raises(A.SnrError, match="meshes|one per object|both"):
            call()                                                                   # ray lists that do not match the meshes
    with pytest.raises(A.SnrError, match=r"\(N, 3\)"):
        G.ray_mesh(mesh, o, torch.ones(4, 3))
    with pytest.raises(A.SnrError, match="one .verts, faces. pair"):
        G.mesh_depth([mesh, mesh], pose, 1.0, K, (0, 0, 64, 64))
    assert G.ray_mesh([], [], []) == [] and G.ray_crossings([], [], []) == [] and G.visible([], [], torch.ones(3)) == []
