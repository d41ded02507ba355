"""Mesh smoothing on the MI355X: ``geometry.mesh_adjacency`` / ``smooth_mesh`` / ``mesh_laplacian`` / ``laplacian_energy`` (the
``snr_smooth_*`` kernels) against tests/smooth_restatement.py.

Every integer output equals the restatement exactly.  Steps, operator and transpose are compared BIT FOR BIT with the restatement rounded
to fp32: every operation of rules 4 to 7 is one correctly rounded IEEE operation in a fixed order, so there is no tolerance.  The autograd
gradient of the energy is held, per entry, to 8 * 2^-24 * (sum_{j in N(i)} |g_j| / d_j + |g_i|) around the restatement's float64
gradient (``smooth_restatement.energy_and_gradient``): the fp32 roundings of U, of torch's square / mean and of the final store, derived
and not measured.  The energy itself, an fp32 sum of 3 V non-negative terms whose terms carry two roundings each, is held to
(3 V + 4) 2^-24 relative, the bound of a sum in any order."""
import numpy as np
import pytest
import torch

import geometry_cases as GC
import smooth_restatement as MS
from segment_sum_restatement import banded as _banded, bands_intact as _bands_intact, same_bits
from oracle_bands import amd, dev  # noqa: F401  (fixtures)
from planted_decoder import WOBBLE

pytestmark = pytest.mark.gpu

HALF = (0.25, 0.2, 0.15)
EPS = 2.0 ** -24
TWO = [[0, 1, 2], [1, 3, 2]]
HAND = {"two triangles": (4, TWO), "three on an edge": (5, TWO + [[1, 2, 4]]), "a duplicated face": (4, TWO + TWO[:1]),
        "repeated indices, an isolated vertex": (5, [[0, 0, 1], [2, 3, 2], [1, 1, 1]]), "no faces": (3, [])}


def _np(t):
    return t.detach().cpu().numpy()


def _to_gpu(mesh, dev):  # noqa: F811
    return (torch.from_numpy(np.ascontiguousarray(mesh[0], np.float32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(mesh[1], np.int32).reshape(-1, 3)).to(dev))


def _bits(got, want):
    got = _np(got) if torch.is_tensor(got) else got
    return got.dtype == np.float32 and got.shape == want.shape and bool(same_bits(got, np.ascontiguousarray(want, np.float32)).all())


def _hand(name, dev):  # noqa: F811
    n, faces = HAND[name]
    verts = np.random.default_rng(n).standard_normal((n, 3)).astype(np.float32)
    return _to_gpu((verts, np.asarray(faces, np.int32).reshape(-1, 3)), dev)


def _perturbed(mesh, scale=1e-3, seed=0):
    verts, faces = mesh
    return (verts + scale * np.random.default_rng(seed).standard_normal(verts.shape)).astype(np.float32), faces


def _attributes(n, channels, seed=0):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (n, channels)).astype(np.float32)


def _ref(mesh):
    """(verts, faces, adjacency, classes) of a GPU mesh, from the restatement."""
    v, f = _np(mesh[0]), _np(mesh[1])
    adj = MS.adjacency(f, v.shape[0])
    return v, f, adj, MS.classes(adj, f.shape[0])


def _check_adjacency(G, mesh, tag):
    v, f, adj, cls = _ref(mesh)
    got = G.mesh_adjacency(mesh)
    assert isinstance(got, G.Adjacency), tag
    for name, dtype in (("nbr_start", np.int64), ("nbr", np.int32), ("edge_faces", np.int32), ("degree", np.int32)):
        g = _np(getattr(got, name))
        assert g.dtype == dtype and g.shape == adj[name].shape and np.array_equal(g, adj[name]), (tag, name)
    for name in ("boundary", "nonmanifold"):
        g = _np(getattr(got, name))
        assert g.dtype == np.bool_ and np.array_equal(g, cls[name]), (tag, name)
    assert (got.boundary_edges, got.nonmanifold_edges, got.closed) == (cls["boundary_edges"], cls["nonmanifold_edges"], cls["closed"]), tag
    assert type(got.closed) is bool and type(got.boundary_edges) is int
    print(f"{tag}: V {v.shape[0]} F {f.shape[0]} E2 {adj['nbr'].shape[0]} max degree {adj['degree'].max(initial=0)} boundary edges "
          f"{got.boundary_edges} non-manifold {got.nonmanifold_edges} closed {got.closed}")
    return got, adj, cls


@pytest.fixture(scope="module")
def box(dev):  # noqa: F811
    return _to_gpu(_perturbed(MS.box_mesh(HALF, 24)), dev)


@pytest.fixture(scope="module")
def open_box(dev):  # noqa: F811
    return _to_gpu(_perturbed(MS.open_box(HALF, 24), seed=1), dev)


@pytest.fixture(scope="module")
def extracted(amd, dev):  # noqa: F811
    """``extract_mesh`` of the planted box decoder at resolution 24: (model, codes, the two meshes)."""
    from supnerf_amd import geometry as G
    model, sc = GC.box(amd, dev, 3, 1, seed=4, wobble=WOBBLE), GC.codes(2, 31, dev)      # (the wobble makes the surface depend on the code)
    return model, sc, G.extract_mesh(model, sc, level=GC.LEVEL_BOX, resolution=24, bound=GC.BOUND_BOX)


# ------------------------------------------------------------------ adjacency: integers, exactly
def test_adjacency_of_hand_meshes(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    for name in HAND:
        _check_adjacency(G, _hand(name, dev), name)
    got, _, _ = _check_adjacency(G, _hand("two triangles", dev), "two triangles")
    assert got.degree.tolist() == [2, 3, 3, 2] and got.boundary_edges == 4 and got.edge_faces.tolist() == [1, 1, 1, 2, 1, 1, 2, 1, 1, 1]
    got, _, _ = _check_adjacency(G, _hand("three on an edge", dev), "three on an edge")
    assert got.nonmanifold_edges == 1 and got.nonmanifold.tolist() == [False, True, True, False, False]
    got, _, _ = _check_adjacency(G, _hand("a duplicated face", dev), "a duplicated face")
    assert got.degree.tolist() == [2, 3, 3, 2] and got.edge_faces.tolist() == [2, 2, 2, 3, 1, 2, 3, 1, 1, 1]
    got, _, _ = _check_adjacency(G, _to_gpu(MS.tetrahedron([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]), dev), "tetrahedron")
    assert got.closed and got.degree.tolist() == [3, 3, 3, 3]
    u = G.mesh_laplacian(_to_gpu(MS.tetrahedron([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]), dev))
    assert float((u + 4.0 / 3.0 * torch.tensor([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1.0]], device=dev)).abs().max()) < 1e-6


@pytest.mark.parametrize("n", [63, 64, 65, 300])
def test_adjacency_of_fans(amd, dev, n):  # noqa: F811
    from supnerf_amd import geometry as G
    got, adj, _ = _check_adjacency(G, _to_gpu(MS.fan(n), dev), f"fan {n}")
    assert int(got.degree[0]) == n and got.nbr[:n].tolist() == list(range(1, n + 1)) and got.boundary_edges == n + 1


@pytest.mark.parametrize("n", [255, 256, 257])
def test_adjacency_of_strips(amd, dev, n):  # noqa: F811
    from supnerf_amd import geometry as G
    got, _, _ = _check_adjacency(G, _to_gpu(MS.strip(n), dev), f"strip {n}")
    assert got.boundary_edges == n and bool(got.boundary.all())


def test_adjacency_of_boxes_and_an_extracted_mesh(amd, dev, box, open_box, extracted):  # noqa: F811
    from supnerf_amd import geometry as G
    got, _, _ = _check_adjacency(G, box, "box")
    assert got.closed and got.nbr.shape[0] == 2 * 3 * 6912 // 2 and set(got.edge_faces.tolist()) == {2}
    got, _, _ = _check_adjacency(G, open_box, "open box")                        # the outline of the removed side, 4 n = 96 each
    assert not got.closed and got.boundary_edges == 96 and int(got.boundary.sum()) == 96 and got.nonmanifold_edges == 0
    assert int((got.degree == 0).sum()) == 23 * 23
    rim = _np(got.boundary)
    v = _np(open_box[0])
    assert (np.abs(v[rim][:, 2] - HALF[2]) < 0.01).all() and ((np.abs(np.abs(v[rim][:, 0]) - HALF[0]) < 0.01) |
                                                               (np.abs(np.abs(v[rim][:, 1]) - HALF[1]) < 0.01)).all()
    for b, mesh in enumerate(extracted[2]):
        assert mesh[1].shape[0] > 0
        _check_adjacency(G, mesh, f"extracted {b}")


# ------------------------------------------------------------------ steps and operator: bit for bit
def _smooth_cases(G, mesh, tag, pins, channels=(1, 3, 16)):
    """One lam step, one mu step, 10 Taubin iterations and none, positions and attributes, under every pin of ``pins``."""
    from supnerf_amd import ops
    dev = mesh[0].device  # noqa: F811
    v, f, adj, cls = _ref(mesh)
    nV = v.shape[0]
    adjacency = G.mesh_adjacency(mesh)
    for pin_name, pin in pins.items():
        mask = cls["boundary"] if pin_name == "boundary" else pin
        pin_arg = pin if pin is None or isinstance(pin, str) else torch.from_numpy(pin).to(dev)
        for iters, lam, mu in ((1, 0.5, None), (1, -0.53, None), (10, 0.5, -0.53), (0, 0.5, -0.53)):
            for C in channels:
                att = _attributes(nV, C, C)
                got = G.smooth_mesh(mesh, iters, lam=lam, mu=mu, pin=pin_arg, attributes=torch.from_numpy(att).to(dev),
                                    adjacency=adjacency if C == 3 else None)
                assert isinstance(got, G.Smoothed) and got.verts.grad_fn is None and not got.verts.requires_grad
                assert _bits(got.verts, MS.taubin(v, adj, iters, lam, mu, mask)), (tag, pin_name, iters, lam, mu, "verts")
                assert _bits(got.attributes, MS.taubin(att, adj, iters, lam, mu, mask)), (tag, pin_name, iters, lam, mu, C)
                if mask is not None:
                    assert torch.equal(got.verts[torch.from_numpy(mask).to(dev)], mesh[0][torch.from_numpy(mask).to(dev)])
        one, two = (G.smooth_mesh(mesh, 10, pin=pin_arg, attributes=torch.from_numpy(att).to(dev)) for _ in range(2))
        assert torch.equal(one.verts, two.verts) and torch.equal(one.attributes, two.attributes)             # two runs, the same bits
    copy = G.smooth_mesh(mesh, 0)
    assert copy.attributes is None and torch.equal(copy.verts, mesh[0]) and copy.verts.data_ptr() != mesh[0].data_ptr()
    # operator and transpose
    u = G.mesh_laplacian(mesh, adjacency)
    assert _bits(u, MS.laplacian(v, adj)), (tag, "laplacian")
    for C in channels:
        g = np.random.default_rng(10 + C).standard_normal((nV, C)).astype(np.float32)
        t = torch.from_numpy(g).to(dev)
        packed = G._pack_adjacency([adjacency], [nV], dev)
        assert _bits(ops.mesh_laplacian_values(t, packed, transpose=True), MS.transpose(g, adj)), (tag, "transpose", C)
        assert _bits(ops.mesh_laplacian_values(t, packed), MS.laplacian(g, adj)), (tag, "laplacian", C)


def test_steps_on_the_open_box(amd, dev, open_box):  # noqa: F811
    from supnerf_amd import geometry as G
    mask = np.zeros(open_box[0].shape[0], bool)
    mask[::7] = True
    _smooth_cases(G, open_box, "open box", {"none": None, "boundary": "boundary", "mask": mask})


@pytest.mark.parametrize("name", ["fan 300", "fan 64", "strip 257", "sphere", "hand"])
def test_steps_on_small_meshes(amd, dev, name):  # noqa: F811
    from supnerf_amd import geometry as G
    if name == "hand":
        for hand in HAND:
            _smooth_cases(G, _hand(hand, dev), hand, {"none": None, "boundary": "boundary"}, channels=(3,))
        return
    mesh = {"fan": lambda: MS.fan(int(name.split()[1])), "strip": lambda: MS.strip(257), "sphere": MS.noisy_sphere}[name.split()[0]]()
    mask = np.zeros(mesh[0].shape[0], bool)
    mask[1::3] = True
    _smooth_cases(G, _to_gpu(mesh, dev), name, {"none": None, "boundary": "boundary", "mask": mask}, channels=(1, 3, 16) if name == "sphere" else (3,))


def test_sphere_behaviour_on_the_device(amd, dev):  # noqa: F811
    """What smoothing is for, on the device's numbers: the three bounds of tests/test_mesh_smooth_cpu.py on the noisy sphere."""
    from supnerf_amd import geometry as G
    verts, faces = MS.noisy_sphere()
    mesh = _to_gpu((verts, faces), dev)
    lap, tau = _np(G.smooth_mesh(mesh, 10, mu=None, pin=None).verts), _np(G.smooth_mesh(mesh, 10, pin=None).verts)
    v0, s0 = MS.signed_volume(verts, faces), MS.radii(verts).std()
    r_lap, r_tau, s_tau = MS.signed_volume(lap, faces) / v0, MS.signed_volume(tau, faces) / v0, MS.radii(tau).std()
    print(f"volume ratio {r_lap:.4f} (Laplacian) {r_tau:.4f} (Taubin); radial std {s0:.5f} -> {s_tau:.5f}")
    assert r_lap < 0.90 and abs(r_tau - 1.0) < 0.02 and s_tau < 0.5 * s0


def test_a_nan_vertex_poisons_its_ring_and_nothing_else(amd, dev, box):  # noqa: F811
    from supnerf_amd import geometry as G
    v, f, adj, _ = _ref(box)
    x = box[0].clone()
    x[1234] = float("nan")
    got = G.smooth_mesh((x, box[1]), 1, mu=None, pin=None).verts
    clean = G.smooth_mesh(box, 1, mu=None, pin=None).verts
    ring = adj["nbr"][adj["nbr_start"][1234]:adj["nbr_start"][1235]].tolist()
    hit = torch.isnan(got).any(1)
    assert sorted(torch.nonzero(hit).view(-1).tolist()) == sorted(ring + [1234])
    assert torch.equal(got[~hit], clean[~hit])
    assert _bits(got[~hit], MS.step(_np(x), adj, 0.5)[_np(~hit)])


def test_packed_launch_equals_per_object_calls(amd, dev, open_box):  # noqa: F811
    """B = 4 in one call -- the open box, a fan, an empty mesh, the sphere -- bit for bit what four calls give."""
    from supnerf_amd import geometry as G
    empty = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))
    meshes = [open_box, _to_gpu(MS.fan(65), dev), empty, _to_gpu(MS.noisy_sphere(), dev)]
    atts = [torch.from_numpy(_attributes(m[0].shape[0], 3, 5 + i)).to(dev) for i, m in enumerate(meshes)]
    adjs = G.mesh_adjacency(meshes)
    assert len(adjs) == 4 and [a.closed for a in adjs] == [False, False, False, True]
    singles = [G.mesh_adjacency(m) for m in meshes]
    for b, (a, s) in enumerate(zip(adjs, singles)):
        for name, x, y in zip(G.Adjacency._fields, a, s):
            assert (torch.equal(x, y) and x.dtype == y.dtype) if torch.is_tensor(x) else x == y, (b, name)
    assert adjs[2].nbr_start.tolist() == [0] and adjs[2].nbr.shape == (0,) and adjs[2].boundary_edges == 0
    for pin in (None, "boundary"):
        for adjacency in (None, adjs):
            packed = G.smooth_mesh(meshes, 3, pin=pin, attributes=atts, adjacency=adjacency)
            assert len(packed) == 4
            for b in range(4):
                one = G.smooth_mesh(meshes[b], 3, pin=pin, attributes=atts[b])
                assert torch.equal(packed[b].verts, one.verts) and torch.equal(packed[b].attributes, one.attributes), (b, pin)
                assert _bits(packed[b].verts, one.verts.cpu().numpy())
    masks = [torch.zeros(m[0].shape[0], dtype=torch.bool, device=dev) for m in meshes]
    masks[0][::2] = True
    packed = G.smooth_mesh(meshes, 2, pin=masks)
    assert torch.equal(packed[0].verts, G.smooth_mesh(meshes[0], 2, pin=masks[0]).verts)
    assert torch.equal(packed[3].verts, G.smooth_mesh(meshes[3], 2, pin=None).verts) and packed[2].verts.shape == (0, 3)
    us = G.mesh_laplacian(meshes, adjs)
    for b in range(4):
        assert torch.equal(us[b], G.mesh_laplacian(meshes[b])), b
    e = G.laplacian_energy(meshes)
    assert e.shape == (4,) and float(e[2]) == 0.0
    for b in (0, 1, 3):
        v, f, adj, _ = _ref(meshes[b])
        want = MS.energy_and_gradient(v, adj)[0]
        assert abs(float(e[b]) - want) <= (3 * v.shape[0] + 4) * EPS * want, (b, float(e[b]), want)


def test_canaries_through_the_c_abi(amd, dev, open_box):  # noqa: F811
    """Every output buffer of every entry point between guard bands: the outputs are the restatement's and the bands are intact; and
    the step refuses to run in place."""
    ops, lib = amd.ops, amd._lib.lib()
    P, st = ops._ptr, ops._stream(dev)
    i32, i64, u8, f32 = torch.int32, torch.int64, torch.uint8, torch.float32
    verts, faces = open_box
    v, f, adj, cls = _ref(open_box)
    nV, nF, nE = v.shape[0], f.shape[0], adj["nbr"].shape[0]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)  # noqa: E731
    voff, foff = up(np.array([0, nV]), i64), up(np.array([0, nF]), i64)
    nan = float("nan")
    bad = torch.zeros(1, dtype=i32, device=dev)
    key_full, key = _banded(6 * nF, i64, dev, -1)
    assert lib.snr_smooth_edge_keys(P(faces, i32), P(voff, i64), P(foff, i64), 1, nV, nF, P(key, i64), P(bad, i32), st) == 0
    keys, counts = np.unique(_np(key[key != 2 ** 63 - 1]), return_counts=True)                 # (no pair of this mesh is discarded)
    owner = np.repeat(np.arange(nV, dtype=np.int64), adj["degree"])
    assert np.array_equal(keys, (owner << 31) | adj["nbr"]) and np.array_equal(counts, adj["edge_faces"]) and bad.tolist() == [0]
    start, nbr, edge_faces = up(adj["nbr_start"], i64), up(adj["nbr"], i32), up(adj["edge_faces"], i32)
    bd_full, bd = _banded(nV, u8, dev, 255)
    nm_full, nm = _banded(nV, u8, dev, 255)
    assert lib.snr_smooth_vertex_flags(P(start, i64), P(edge_faces, i32), nV, nE, P(bd, u8), P(nm, u8), st) == 0
    assert np.array_equal(_np(bd).astype(bool), cls["boundary"]) and np.array_equal(_np(nm).astype(bool), cls["nonmanifold"])
    checks = [(key_full, 6 * nF, -1), (bd_full, nV, 255), (nm_full, nV, 255)]
    pinned = up(cls["boundary"], u8)
    for C in (1, 3, 16):
        x = _attributes(nV, C, 20 + C) if C != 3 else v
        xin = up(x, f32)
        so_full, sout = _banded(nV * C, f32, dev, nan)
        assert lib.snr_smooth_step(P(xin), C, P(start, i64), P(nbr, i32), P(voff, i64), 1, nV, nE, P(pinned, u8), -0.53, P(sout), st) == 0
        assert _bits(sout.view(nV, C), MS.step(x, adj, -0.53, cls["boundary"]))
        checks.append((so_full, nV * C, nan))
        for transpose, want in ((0, MS.laplacian(x, adj)), (1, MS.transpose(x, adj))):
            lo_full, lout = _banded(nV * C, f32, dev, nan)
            assert lib.snr_smooth_laplacian(P(xin), C, P(start, i64), P(nbr, i32), P(voff, i64), 1, nV, nE, transpose, P(lout), st) == 0
            assert _bits(lout.view(nV, C), want), (C, transpose)
            checks.append((lo_full, nV * C, nan))
        # a Jacobi step: in place, or into a buffer that overlaps the input, is refused before anything is launched
        before = xin.clone()
        assert lib.snr_smooth_step(P(xin), C, P(start, i64), P(nbr, i32), P(voff, i64), 1, nV, nE, None, 0.5, P(xin), st) == -1
        assert lib.snr_smooth_laplacian(P(xin), C, P(start, i64), P(nbr, i32), P(voff, i64), 1, nV, nE, 0, P(xin), st) == -1
        both = torch.zeros(2 * nV * C - 1, device=dev)
        assert lib.snr_smooth_step(P(both[:nV * C]), C, P(start, i64), P(nbr, i32), P(voff, i64), 1, nV, nE, None, 0.5,
                                   P(both[nV * C - 1:]), st) == -1
        assert torch.equal(xin, before)
    torch.cuda.synchronize()
    for full, n, fill in checks:
        assert _bands_intact(full, n, fill), (n, fill)


def test_a_bad_face_index_raises(amd, dev, box):  # noqa: F811
    """A face index out of range sets the device flag -- nothing is dereferenced with it -- and every entry raises; the next call is
    sound."""
    from supnerf_amd import geometry as G
    verts, faces = box
    for index in (verts.shape[0], verts.shape[0] + 12345, -1, 2 ** 31 - 1):
        f2 = faces.clone()
        f2[faces.shape[0] // 2, 1] = index
        for call in (G.mesh_adjacency, G.smooth_mesh, G.mesh_laplacian, G.laplacian_energy):
            with pytest.raises(amd.SnrError, match="face index"):
                call([box, (verts, f2)])
    with pytest.raises(amd.SnrError, match="int32"):
        G.smooth_mesh((verts, faces.long()))
    with pytest.raises(amd.SnrError):
        G.smooth_mesh(box, adjacency=G.mesh_adjacency(_to_gpu(MS.fan(10), dev)))  # another mesh's adjacency
    with pytest.raises(amd.SnrError):
        G.smooth_mesh(box, attributes=torch.zeros(verts.shape[0], 17, device=dev))
    with pytest.raises(amd.SnrError):
        G.smooth_mesh(box, pin=torch.zeros(verts.shape[0] - 1, dtype=torch.bool, device=dev))
    assert G.mesh_adjacency(box).closed


# ------------------------------------------------------------------ autograd
def test_energy_gradient_against_float64(amd, dev, box):  # noqa: F811
    from supnerf_amd import geometry as G
    v, f, adj, _ = _ref(box)
    x = box[0].clone().requires_grad_()
    e = G.laplacian_energy((x, box[1]))
    assert e.shape == (1,) and e.dtype == torch.float32
    (grad,) = torch.autograd.grad(e.sum(), x)
    want_e, want, bound = MS.energy_and_gradient(v, adj)
    err = np.abs(_np(grad).astype(np.float64) - want)
    ratio = (err / (EPS * bound)).max()
    print(f"energy {float(e.detach()[0]):.6e} (float64 {want_e:.6e}); gradient error at most {ratio:.2f} x 2^-24 x bound (8 allowed), "
          f"largest |gradient| {np.abs(want).max():.3e}")
    assert abs(float(e.detach()[0]) - want_e) <= (3 * v.shape[0] + 4) * EPS * want_e
    assert np.isfinite(_np(grad)).all() and np.abs(want).max() > 0 and (err <= 8 * EPS * bound).all()
    # the operator alone: U with autograd equals the plain call, and its backward is the transpose
    u = G.mesh_laplacian((x, box[1]))
    assert u.grad_fn is not None and _bits(u, MS.laplacian(v, adj))
    g = np.random.default_rng(5).standard_normal(v.shape).astype(np.float32)
    (t,) = torch.autograd.grad(u, x, torch.from_numpy(g).to(dev))
    assert _bits(t, MS.transpose(g, adj))


def test_energy_reaches_the_shape_codes(amd, dev, extracted):  # noqa: F811
    from supnerf_amd import geometry as G
    model, sc0, plain = extracted

    def run():
        sc = sc0.clone().requires_grad_()
        meshes = G.extract_mesh(model, sc, level=GC.LEVEL_BOX, resolution=24, bound=GC.BOUND_BOX, differentiable=True)
        return sc, meshes, G.laplacian_energy(meshes)

    sc, meshes, e = run()
    assert GC.same_meshes(meshes, plain) and e.shape == (2,) and bool((e > 0).all())
    e.sum().backward()
    assert sc.grad is not None and bool(torch.isfinite(sc.grad).all()) and bool((sc.grad != 0).any(1).all())
    # a second identical run, cut at the vertices: the same bits
    sc2, meshes2, e2 = run()
    assert torch.equal(e2, e)
    verts2 = [v for v, _ in meshes2]
    g = torch.autograd.grad(e2.sum(), verts2, retain_graph=True)
    torch.autograd.backward(verts2, list(g))
    assert torch.equal(sc2.grad, sc.grad)
    print(f"energy {e.tolist()}, |d energy / d code| max {float(sc.grad.abs().max()):.3e}")


def test_smoothing_an_extracted_mesh(amd, dev, extracted):  # noqa: F811
    from supnerf_amd import geometry as G
    model, sc, _ = extracted
    mesh = G.extract_mesh(model, sc[:1], level=GC.LEVEL_BOX, resolution=24, bound=GC.BOUND_BOX, keep="largest")[0]
    assert G.mesh_components(mesh).n_verts.shape[0] == 1
    adjacency = G.mesh_adjacency(mesh)
    s = G.smooth_mesh(mesh)
    after = (s.verts, mesh[1])
    comps = G.mesh_components(after)
    assert comps.n_verts.tolist() == [mesh[0].shape[0]] and comps.n_faces.tolist() == [mesh[1].shape[0]]          # still one component
    rim = adjacency.boundary
    assert torch.equal(s.verts[rim], mesh[0][rim]) and not torch.equal(s.verts[~rim], mesh[0][~rim])
    e0, e1 = float(G.laplacian_energy(mesh, adjacency)[0]), float(G.laplacian_energy(after, adjacency)[0])
    print(f"extracted: V {mesh[0].shape[0]} F {mesh[1].shape[0]} rim {int(rim.sum())} closed {adjacency.closed}; energy {e0:.4e} -> {e1:.4e}")
    assert e1 < e0
    v, f, adj, cls = _ref(mesh)
    assert _bits(s.verts, MS.taubin(v, adj, 10, MS.LAMBDA, MS.MU, cls["boundary"]))
