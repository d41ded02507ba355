"""Mesh smoothing on the host: the rules of include/supnerf_hip.h ("Mesh smoothing") as tests/smooth_restatement.py restates them, held
against hand results (a regular tetrahedron, two and three triangles on one edge, a duplicated face, a repeated index, an isolated
vertex), against what smoothing must do to a noisy sphere, and against the dense matrix of the operator -- with planted mistakes that
the same checks reject; and the parts of the new API that need no GPU (symbols, signatures, the argument checks of the C ABI and of the
Python layer).

The sphere's bounds were fixed before any code ran: after 10 plain Laplacian iterations the signed volume is below 0.90 of the start; after 10 Taubin
iterations it is within 2 % of the start and the standard deviation of the radii is below half of the start.  Measured here on the
restatement: volume ratios 0.8425 (Laplacian) and 1.0088 (Taubin), radial std 0.00999 -> 0.00403."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import smooth_restatement as MS

REGULAR = [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]
QUAD = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
TWO = np.array([[0, 1, 2], [1, 3, 2]], np.int32)


def _ring(adj, i):
    s, e = adj["nbr_start"][i], adj["nbr_start"][i + 1]
    return adj["nbr"][s:e].tolist(), adj["edge_faces"][s:e].tolist()


def test_hand_adjacencies():
    a = MS.adjacency(TWO, 4)
    c = MS.classes(a, 2)
    assert a["degree"].tolist() == [2, 3, 3, 2] and a["nbr_start"].tolist() == [0, 2, 5, 8, 10]
    assert a["nbr"].dtype == np.int32 and a["edge_faces"].dtype == np.int32 and a["nbr_start"].dtype == np.int64
    assert _ring(a, 1) == ([0, 2, 3], [1, 2, 1]) and _ring(a, 2) == ([0, 1, 3], [1, 2, 1])            # all but the shared edge: boundary
    assert (c["boundary_edges"], c["nonmanifold_edges"], c["closed"]) == (4, 0, False) and c["boundary"].all() and not c["nonmanifold"].any()
    # a third triangle on the shared edge
    a = MS.adjacency(np.concatenate([TWO, [[1, 2, 4]]]), 5)
    c = MS.classes(a, 3)
    assert a["degree"].tolist() == [2, 4, 4, 2, 2] and _ring(a, 1) == ([0, 2, 3, 4], [1, 3, 1, 1])
    assert (c["boundary_edges"], c["nonmanifold_edges"]) == (6, 1) and c["nonmanifold"].tolist() == [False, True, True, False, False]
    # a duplicated face: the same degrees, its edges count 2 (and the shared one 3)
    a = MS.adjacency(np.concatenate([TWO, TWO[:1]]), 4)
    c = MS.classes(a, 3)
    assert a["degree"].tolist() == [2, 3, 3, 2] and _ring(a, 0) == ([1, 2], [2, 2]) and _ring(a, 1) == ([0, 2, 3], [2, 3, 1])
    assert (c["boundary_edges"], c["nonmanifold_edges"]) == (2, 1) and c["boundary"].tolist() == [False, True, True, True]
    # a repeated index gives the pair of its distinct indices, once; vertex 4 is named by no face
    a = MS.adjacency([[0, 0, 1], [2, 3, 2], [1, 1, 1]], 5)
    assert a["degree"].tolist() == [1, 1, 1, 1, 0] and a["nbr"].tolist() == [1, 0, 3, 2] and a["edge_faces"].tolist() == [1, 1, 1, 1]
    x = np.arange(15, dtype=np.float32).reshape(5, 3) ** 2
    u = MS.umbrella(x, a)
    assert np.array_equal(u[4], [0, 0, 0]) and np.array_equal(u[0], x[1].astype(np.float64) - x[0])
    moved = MS.step(x, a, 0.5)
    assert np.array_equal(moved[4], x[4]) and np.array_equal(moved[0], ((x[0].astype(np.float64) + x[1]) / 2).astype(np.float32))
    for bad in ([[0, 1, 5]], [[0, -1, 2]]):
        with pytest.raises(MS.Rejected):
            MS.adjacency(bad, 5)
    # a closed mesh
    verts, faces = MS.tetrahedron(REGULAR)
    a = MS.adjacency(faces, 4)
    c = MS.classes(a, 4)
    assert a["degree"].tolist() == [3, 3, 3, 3] and set(a["edge_faces"].tolist()) == {2} and c["closed"] and not c["boundary"].any()
    assert not MS.classes(MS.adjacency(np.zeros((0, 3), np.int32), 3), 0)["closed"]


@pytest.fixture(scope="module")
def sphere():
    verts, faces = MS.noisy_sphere()
    assert verts.shape == (642, 3) and faces.shape == (1280, 3) and verts.dtype == np.float32
    adj = MS.adjacency(faces, 642)
    assert MS.classes(adj, 1280)["closed"] and sorted(set(adj["degree"].tolist())) == [5, 6] and MS.signed_volume(verts, faces) > 0
    return verts, faces, adj


def _checks(sphere, planted=None, report=None):
    """Every check the rules have to pass; a list of the ones that fail."""
    failed = []
    # a regular tetrahedron centred at 0: U_i = -4/3 x_i, so a step scales it by 1 - 4 f / 3 and an iteration by the product of the two
    x, faces = MS.tetrahedron(REGULAR)
    adj = MS.adjacency(faces, 4)
    if np.abs(MS.umbrella(x, adj, planted) + 4.0 / 3.0 * x.astype(np.float64)).max() > 1e-12:
        failed.append("tetrahedron: U")
    if np.abs(MS.step(x, adj, 0.5, planted=planted) - x / 3.0).max() > 1e-6:
        failed.append("tetrahedron: step")
    want = x * (1 - 4 * MS.LAMBDA / 3) * (1 - 4 * MS.MU / 3)
    if np.abs(MS.taubin(x, adj, 1, planted=planted) - want).max() > 1e-6:
        failed.append("tetrahedron: iteration")
    # two triangles on one edge: every neighbour counts once
    u = MS.umbrella(QUAD, MS.adjacency(TWO, 4), planted)
    if np.abs(u[1] - [1.0 / 3 - 1, 2.0 / 3, 0]).max() > 1e-12 or np.abs(u[0] - [0.5, 0.5, 0]).max() > 1e-12:
        failed.append("two triangles: U")
    # the noisy sphere
    verts, faces, adj = sphere
    v0, s0 = MS.signed_volume(verts, faces), MS.radii(verts).std()
    lap = MS.taubin(verts, adj, 10, mu=None, planted=planted)
    tau = MS.taubin(verts, adj, 10, planted=planted)
    r_lap, r_tau, s_tau = MS.signed_volume(lap, faces) / v0, MS.signed_volume(tau, faces) / v0, MS.radii(tau).std()
    if report is not None:
        report(f"{planted}: volume ratio {r_lap:.4f} (Laplacian) {r_tau:.4f} (Taubin); radial std {s0:.5f} -> {s_tau:.5f}")
    if not r_lap < 0.90:
        failed.append("sphere: Laplacian shrinks")
    if not abs(r_tau - 1.0) < 0.02:
        failed.append("sphere: Taubin keeps the volume")
    if not s_tau < 0.5 * s0:
        failed.append("sphere: Taubin smooths")
    return failed


def test_rules_pass_every_check(sphere):
    assert _checks(sphere, report=print) == []


@pytest.mark.parametrize("planted", MS.PLANTED)
def test_planted_mistakes_are_rejected(sphere, planted):
    failed = _checks(sphere, planted, report=print)
    print(planted, "->", failed)
    assert failed != []
    assert {"multiplicity": "two triangles: U", "gauss_seidel": "tetrahedron: step", "stale_mu": "tetrahedron: iteration"}[planted] in failed


def test_steps_pins_and_copies(sphere):
    verts, faces, adj = sphere
    assert np.array_equal(MS.taubin(verts, adj, 0), verts)
    pinned = np.zeros(642, bool)
    pinned[::5] = True
    out = MS.taubin(verts, adj, 3, pinned=pinned)
    assert np.array_equal(out[pinned], verts[pinned]) and (out[~pinned] != verts[~pinned]).any(1).all()
    free = MS.taubin(verts, adj, 3)
    assert not np.array_equal(free[~pinned], out[~pinned])                      # a pinned vertex still serves as a neighbour
    # a NaN vertex poisons exactly its 1-ring per step
    x = verts.copy()
    x[17] = np.nan
    after = MS.step(x, adj, 0.5)
    ring = adj["nbr"][adj["nbr_start"][17]:adj["nbr_start"][18]]
    hit = np.isnan(after).any(1)
    assert sorted(np.nonzero(hit)[0].tolist()) == sorted(ring.tolist() + [17])
    assert np.array_equal(after[~hit], MS.step(verts, adj, 0.5)[~hit])
    # attributes of 1 and 16 channels: each channel on its own
    a = np.random.default_rng(1).uniform(0.5, 1.5, (642, 16)).astype(np.float32)
    assert np.array_equal(MS.taubin(a, adj, 2)[:, 3:4], MS.taubin(a[:, 3:4], adj, 2))


def test_transpose_is_the_dense_transpose():
    verts, faces = MS.box_mesh((0.25, 0.2, 0.15), 24)
    adj = MS.adjacency(faces, verts.shape[0])
    L = MS.dense_operator(adj)
    x = (verts + np.random.default_rng(2).normal(0, 1e-3, verts.shape)).astype(np.float32)
    g = np.random.default_rng(3).standard_normal(verts.shape)
    u, t = MS.umbrella(x, adj), MS.transpose64(g, adj)
    assert np.abs(u - L @ x.astype(np.float64)).max() <= 1e-15
    assert np.abs(t - L.T @ g).max() <= 4e-15 * np.abs(g).max()
    e, grad, bound = MS.energy_and_gradient(x, adj)
    assert abs(e - ((L @ x.astype(np.float64)) ** 2).sum() / verts.shape[0]) <= 1e-9 * e
    assert np.abs(grad - L.T @ (2.0 / verts.shape[0] * (L @ x.astype(np.float64)))).max() <= 1e-9 * bound.max() and (bound >= np.abs(grad)).all()
    # an isolated vertex: the bracket of rule 7
    a = MS.adjacency([[0, 1, 2]], 4)
    gg = np.array([[1.0], [2.0], [4.0], [8.0]])
    assert MS.transpose64(gg, a)[:, 0].tolist() == [2.0, 0.5, -2.5, 0.0]
    assert np.array_equal(MS.dense_operator(a).T @ gg, MS.transpose64(gg, a))


# ------------------------------------------------------------------ the API without a GPU
SMOOTH_SYMBOLS = ("snr_smooth_edge_keys", "snr_smooth_vertex_flags", "snr_smooth_step", "snr_smooth_laplacian")


def test_symbols_and_signatures():
    import os
    import re
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, geometry as G, ops
    assert all(n in _lib.exported_symbols() for n in SMOOTH_SYMBOLS)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in SMOOTH_SYMBOLS)
    assert _lib.header_abi_version() >= 23 and lib.snr_abi_version() == _lib.header_abi_version()
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    hdr = open(os.path.join(here, "..", "include", "supnerf_hip.h")).read()
    assert all(re.search(r"\b" + n + r"\(", hdr) for n in SMOOTH_SYMBOLS) and "Mesh smoothing" in hdr
    assert "ASCENDING" in hdr[hdr.index("Mesh smoothing"):] and "tests/smooth_restatement.py" in hdr
    import importlib.util
    build = importlib.util.spec_from_file_location("snr_build", os.path.join(here, "build.py"))
    mod = importlib.util.module_from_spec(build)
    build.loader.exec_module(mod)
    assert "snr_smooth.hip" in mod.SOURCES
    assert ops.MeshAdjacency._fields[:8] == ("nbr_start", "nbr", "edge_faces", "degree", "boundary", "nonmanifold", "boundary_edges",
                                             "nonmanifold_edges")
    assert list(inspect.signature(ops.mesh_adjacency).parameters) == ["verts", "faces", "n_verts", "n_faces"]
    assert issubclass(ops.MeshLaplacian, torch.autograd.Function) and callable(ops.mesh_smooth)
    assert G.Adjacency._fields == ("nbr_start", "nbr", "edge_faces", "degree", "boundary", "nonmanifold", "boundary_edges",
                                   "nonmanifold_edges", "closed")
    assert G.Smoothed._fields == ("verts", "attributes")
    assert list(inspect.signature(G.mesh_adjacency).parameters) == ["meshes"]
    sig = inspect.signature(G.smooth_mesh)
    assert list(sig.parameters) == ["meshes", "iterations", "lam", "mu", "pin", "attributes", "adjacency"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    assert [sig.parameters[n].default for n in list(sig.parameters)[1:]] == [10, 0.5, -0.53, "boundary", None, None]
    for fn in (G.mesh_laplacian, G.laplacian_energy):
        s = inspect.signature(fn)
        assert list(s.parameters) == ["meshes", "adjacency"] and s.parameters["adjacency"].default is None
    # the C ABI validates before it launches: these return without touching a device
    big = 1 << 39
    flag = ctypes.c_int32(0)
    host_flag = ctypes.addressof(flag)                                          # (never read: nothing is launched for zero faces)
    keys = lambda B, nV, nF, bad=None: lib.snr_smooth_edge_keys(None, None, None, B, nV, nF, None, bad, None)  # noqa: E731
    assert keys(1, 4, 4) == -1 and keys(1, -1, 4) == -1 and keys(-1, 4, 4) == -1 and keys(1, 4, -4) == -1
    assert keys(1, big, 4) == -5 and keys(1, 4, big) == -5 and keys(1, 4, (1 << 38) // 6 + 1) == -5
    assert keys(1, 1 << 32, 4, host_flag) == -5 and keys(1, (1 << 32) - 1, 0, host_flag) == 0                # sum V < 2^32
    assert keys(1, 4, 4, host_flag) == -1 and keys(1, 4, 0, host_flag) == 0 and flag.value == 0
    vflags = lambda nV, nE: lib.snr_smooth_vertex_flags(None, None, nV, nE, None, None, None)  # noqa: E731
    assert vflags(4, 4) == -1 and vflags(0, 0) == 0 and vflags(-1, 0) == -1 and vflags(4, -1) == -1
    assert vflags(big, 4) == -5 and vflags(4, big) == -5
    step = lambda C_, B, nV, nE: lib.snr_smooth_step(None, C_, None, None, None, B, nV, nE, None, 0.5, None, None)  # noqa: E731
    lap = lambda C_, B, nV, nE, tr=0: lib.snr_smooth_laplacian(None, C_, None, None, None, B, nV, nE, tr, None, None)  # noqa: E731
    for call in (step, lap):
        assert call(3, 1, 4, 4) == -1 and call(0, 1, 0, 0) == -1 and call(17, 1, 0, 0) == -1 and call(-3, 1, 0, 0) == -1
        assert call(3, 1, 0, 0) == 0 and call(16, 0, 0, 0) == 0 and call(1, 1, 0, 0) == 0
        assert call(3, -1, 4, 4) == -1 and call(3, 1, -4, 4) == -1 and call(3, 1, 4, -4) == -1
        assert call(3, 1, big, 4) == -5 and call(3, 1, 4, big) == -5
    assert lap(3, 1, 0, 0, 2) == -1 and lap(3, 1, 0, 0, -1) == -1 and lap(3, 1, 0, 0, 1) == 0


def test_cpu_tensors_and_bad_arguments_raise():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    verts, faces = MS.tetrahedron(REGULAR)
    v, f = torch.from_numpy(verts), torch.from_numpy(faces)
    for call in (G.mesh_adjacency, G.smooth_mesh, G.mesh_laplacian, G.laplacian_energy):
        with pytest.raises(A.SnrError, match="GPU|gpu|CPU|device"):
            call([(v, f)])                                                       # CPU tensors: no fallback
        with pytest.raises(A.SnrError):
            call((v, f))
        with pytest.raises(A.SnrError):
            call((v, f.long()))
    with pytest.raises(A.SnrError):
        A.ops.mesh_adjacency(v, f, [4], [4])
    with pytest.raises(A.SnrError, match="int32"):
        A.ops.mesh_adjacency(v, f.long(), [4], [4])
    for kw in (dict(lam=float("nan")), dict(lam=float("inf")), dict(mu=float("-inf")), dict(mu=float("nan")), dict(lam=float("nan"), mu=None)):
        with pytest.raises(A.SnrError, match="finite"):
            G.smooth_mesh([(v, f)], **kw)
    with pytest.raises(A.SnrError, match="iterations"):
        G.smooth_mesh([(v, f)], -1)
    with pytest.raises(A.SnrError, match="pin"):
        G.smooth_mesh([(v, f)], pin="rim")
    assert G.smooth_mesh([]) == [] and G.mesh_adjacency([]) == [] and G.mesh_laplacian([]) == [] and G.laplacian_energy([]).shape == (0,)
