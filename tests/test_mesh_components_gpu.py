"""Mesh components on the MI355X: ``geometry.mesh_components`` (the ``snr_mesh_*`` kernels) against tests/mesh_restatement.py, object by
object -- labels, counts and bounding boxes bit for bit, area and volume bit for bit the fixed order restated
(``mesh_restatement.components_fixed_order``: the terms, the stable sort by component and the two sums all have one order) and, beside
that, within the bound any float64 summation order keeps of the plain restatement (``mesh_restatement.sum_bounds``: (F + 16) 2^-52 S,
derived, not measured), two runs bit for bit -- on the planted five-piece grid, the fog decoder cut at its median density, renumbered and
shuffled meshes, a long thin helix, the small hard meshes of tests/mesh_cases.py and its B = 67 objects in one call; the selection
functions against the restated sub-meshes; the gradient pass-through of a differentiable mesh; and the bad-index flag."""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_restatement as MR
from segment_sum_restatement import same_bits
from geometry_cases import codes as _codes, model as _model
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FIELDS = ("vert_label", "face_label", "n_verts", "n_faces", "bbox_lo", "bbox_hi")


def _np(t):
    return t.detach().cpu().numpy()


def _to_gpu(mesh, dev):  # noqa: F811
    return torch.from_numpy(np.ascontiguousarray(mesh[0])).to(dev), torch.from_numpy(np.ascontiguousarray(mesh[1])).to(dev)


def _check(G, meshes, tag):
    """Every object of ``meshes`` against the restatement; returns (components, restated components)."""
    got = G.mesh_components(meshes)
    again = G.mesh_components(meshes)
    assert len(got) == len(meshes)
    refs = []
    for b, ((v, f), c, c2) in enumerate(zip(meshes, got, again)):
        ref = MR.components(_np(v), _np(f))
        refs.append(ref)
        for name in FIELDS:
            g = _np(getattr(c, name))
            assert g.dtype == ref[name].dtype and g.shape == ref[name].shape, (tag, b, name, g.dtype, g.shape, ref[name].shape)
            assert np.array_equal(g, ref[name]), (tag, b, name)
        ba, bv = MR.sum_bounds(ref)
        ea = np.abs(_np(c.area) - ref["area"]).max(initial=0.0)
        ev = np.abs(_np(c.volume) - ref["volume"]).max(initial=0.0)
        print(f"{tag}[{b}]: V {v.shape[0]} F {f.shape[0]} C {ref['n_verts'].shape[0]} (largest {int(ref['n_verts'].max(initial=0))} vertices); "
              f"|area - ref| {ea:.3e} (bound {ba:.3e}), |volume - ref| {ev:.3e} (bound {bv:.3e})")
        assert c.area.dtype == torch.float64 and c.volume.dtype == torch.float64
        assert c.area.shape == ref["area"].shape and c.volume.shape == ref["volume"].shape
        assert ea <= ba and ev <= bv, (tag, b, ea, ba, ev, bv)
        fixed = MR.components_fixed_order(_np(v), _np(f), comp=ref)               # the order is fixed end to end: the same bits
        for name in ("area", "volume"):
            differ = ~same_bits(_np(getattr(c, name)), fixed[name])
            assert not differ.any(), (tag, b, name, int(differ.sum()), "of", differ.shape[0])
        for x, y in zip(c, c2):                                                    # two runs: the same bits, the float64 sums included
            assert torch.equal(x, y), (tag, b, "run to run")
    return got, refs


def _check_selection(G, meshes, comps, refs, tag):
    for by in ("area", "volume", "faces"):
        for drop in (True, False):
            subs = G.largest_component(meshes, by=by, drop_cavities=drop)
            assert len(subs) == len(meshes)
            for b, ((v, f), sub, ref) in enumerate(zip(meshes, subs, refs)):
                want = MR.select(_np(v), _np(f), ref, MR.largest(ref, by, drop))
                assert sub[1].dtype == torch.int32 and sub[2].dtype == torch.int64 and sub[3].dtype == torch.int64
                for g, w in zip(sub, want):
                    assert g.shape == w.shape and np.array_equal(_np(g), w), (tag, b, by, drop)
    all_at_once = G.largest_component(meshes)
    for b, ((v, f), c, ref) in enumerate(zip(meshes, comps, refs)):
        C = ref["n_verts"].shape[0]
        ids = list(range(0, C, 2))[:50]
        want = MR.select(_np(v), _np(f), ref, ids)
        mask = torch.zeros(C, dtype=torch.bool, device=v.device)
        if ids:
            mask[ids] = True
        for keep in (ids, mask, torch.tensor(ids, dtype=torch.int64)):
            sub = G.select_components((v, f), c, keep)
            assert all(g.shape == w.shape and np.array_equal(_np(g), w) for g, w in zip(sub, want)), (tag, b)
        one = G.largest_component((v, f))                                          # one pair in, one tuple out
        assert torch.equal(one[0], all_at_once[b][0])


@pytest.fixture(scope="module")
def planted(amd, dev):  # noqa: F811
    """(a): the five-piece grid, an all-outside grid (an empty mesh) and a single ball, B = 3, through ``extract_mesh``."""
    from supnerf_amd import geometry as G
    grid = torch.from_numpy(np.stack([MR.planted_field(48)[0], np.full((48, 48, 48), -1.0, np.float32), MR.ball_field(48)[0]])).to(dev)
    return grid, G.extract_mesh(grid, level=0.0)


@pytest.fixture(scope="module")
def fog(amd, dev):  # noqa: F811
    """(b): the fog decoder cut at its median density, R = 64, B = 2: one giant tangled component beside thousands of small ones."""
    from supnerf_amd import geometry as G
    model = _model(amd, dev, 3, 1, seed=0)
    sc = _codes(2, 5, dev)
    grid = G.density_grid(model, sc, 64)
    level = float(grid.median())
    return model, sc, level, G.extract_mesh(grid, level=level)


def test_planted_grid(amd, dev, planted):  # noqa: F811
    from supnerf_amd import geometry as G
    _, meshes = planted
    assert [m[0].shape[0] for m in meshes][:2] == [14074, 0] and meshes[0][1].shape[0] == 28076
    comps, refs = _check(G, meshes, "planted")
    assert [c.n_verts.shape[0] for c in comps] == [5, 0, 1]
    assert comps[0].n_verts.tolist() == [284, 11138, 1778, 446, 428]
    assert (torch.sign(comps[0].volume[:4]).tolist() == [1, 1, -1, 1]) and float(comps[2].volume[0]) > 0
    # the packed form straight from ops, and a single pair
    m = amd.ops.iso_extract(planted[0], G.lattice(48), 0.0)
    p = amd.ops.mesh_components(m.verts, m.faces, m.n_verts, m.n_faces)
    assert p.n_comps == [5, 0, 1] and p.comp_offset == [0, 5, 5, 6]
    assert torch.equal(p.vert_label, torch.cat([c.vert_label for c in comps])) and torch.equal(p.area, torch.cat([c.area for c in comps]))
    one = G.mesh_components(meshes[0])
    assert isinstance(one, G.Components) and all(torch.equal(x, y) for x, y in zip(one, comps[0]))
    _check_selection(G, meshes, comps, refs, "planted")
    kept = G.extract_mesh(planted[0], level=0.0, keep="largest")
    assert [k[0].shape[0] for k in kept] == [11138, 0, meshes[2][0].shape[0]]
    for k, sub in zip(kept, G.largest_component(meshes)):
        assert torch.equal(k[0], sub[0]) and torch.equal(k[1], sub[1])


def test_fog_mesh(amd, dev, fog):  # noqa: F811
    from supnerf_amd import geometry as G
    model, sc, level, meshes = fog
    comps, refs = _check(G, meshes, "fog 64^3 at its median")
    for ref in refs:
        assert ref["n_verts"].shape[0] > 10
    _check_selection(G, meshes, comps, refs, "fog")
    kept = G.extract_mesh(model, sc, level=level, resolution=64, keep="largest")
    for k, sub in zip(kept, G.largest_component(meshes)):
        assert torch.equal(k[0], sub[0]) and torch.equal(k[1], sub[1])
    # vert_index gathers per-vertex data of the full mesh onto the sub-mesh
    normals = G.vertex_normals(model, meshes, sc)
    subs = G.largest_component(meshes)
    again = G.vertex_normals(model, [(s[0], s[1]) for s in subs], sc)
    for (v, f), n, sub, ref, n_sub in zip(meshes, normals, subs, refs, again):
        want = MR.select(_np(v), _np(f), ref, MR.largest(ref))
        gathered = n[sub[2]]
        assert np.array_equal(_np(gathered), _np(n)[want[2]]) and gathered.shape == sub[0].shape
        assert torch.allclose(gathered, n_sub, atol=1e-4)                           # the normals the sub-mesh's own vertices get


def test_renumbered_and_shuffled_meshes(amd, dev, planted):  # noqa: F811
    """(c): the vertices renumbered by a seeded random permutation and by the reversal, the faces shuffled: the labels follow the
    restatement on the permuted mesh (the kernels may not lean on the order ``extract_mesh`` emits); plus a caller's mesh with unreferenced
    and duplicated vertices."""
    from supnerf_amd import geometry as G
    _, meshes = planted
    g = np.random.default_rng(11)
    for name in ("random", "reversed"):
        perm_meshes = []
        for v, f in meshes:
            V, F = v.shape[0], f.shape[0]
            perm = g.permutation(V) if name == "random" else np.arange(V)[::-1].copy()
            perm_meshes.append(_to_gpu(MR.permuted(_np(v), _np(f), perm, g.permutation(F)), dev))
        comps, refs = _check(G, perm_meshes, f"planted, {name} numbering")
        assert sorted(comps[0].n_verts.tolist()) == [284, 428, 446, 1778, 11138]
        _check_selection(G, perm_meshes, comps, refs, name)
    v, f = _np(meshes[0][0]), _np(meshes[0][1])
    f = f[(f < 300).all(1)]
    v = np.concatenate([v[:600], v[:3]])
    comps, refs = _check(G, [_to_gpu((v, f), dev), _to_gpu((v[:5], f[:0]), dev)], "unreferenced vertices")
    assert int((comps[0].n_faces == 0).sum()) >= 303 and comps[1].n_verts.tolist() == [1] * 5 and not comps[1].area.any()


def test_helix(amd, dev):  # noqa: F811
    """(d): a one-voxel-thick tube wound 6.5 turns through a 96^3 grid: one component, long parent chains."""
    from supnerf_amd import geometry as G
    grid = torch.from_numpy(MR.helix_field(96, turns=6.5)[0]).to(dev)
    meshes = G.extract_mesh(grid, level=0.0)
    comps, refs = _check(G, meshes, "helix")
    assert comps[0].n_verts.tolist() == [meshes[0][0].shape[0]] and meshes[0][0].shape[0] > 15000
    assert float(comps[0].volume[0]) > 0


@pytest.mark.parametrize("numbering", MC.NUMBERINGS)
def test_small_hard_meshes(amd, dev, numbering):  # noqa: F811
    """The corpus of tests/mesh_cases.py -- chains, stars, interleaved combs, repeated faces and indices, singletons beside a fan, a
    binary-tree merge order -- nine meshes of one numbering in one packed call."""
    from supnerf_amd import geometry as G
    cases = [c for c in MC.corpus() if c[0].endswith(", " + numbering)]
    assert len(cases) == len(MC.SHAPES)
    comps, _ = _check(G, [_to_gpu((v, f), dev) for _, v, f, _ in cases], f"small hard meshes, {numbering}")
    assert [c.n_verts.shape[0] for c in comps] == [n for _, _, _, n in cases]


def test_many_objects_in_one_call(amd, dev):  # noqa: F811
    """B = 67 in one packed call (``mesh_cases.many_objects``): runs of empty objects at the start, in the middle and at the end, lone
    points, small closed and open pieces, a fan and an edge path whose borders fall inside waves and blocks."""
    from supnerf_amd import geometry as G
    objects = MC.many_objects()
    meshes = [_to_gpu((v, f), dev) for _, v, f, _ in objects]
    comps, refs = _check(G, meshes, "B = 67")
    assert [c.n_verts.shape[0] for c in comps] == [n for _, _, _, n in objects]
    tetra = [b for b, (kind, _, _, _) in enumerate(objects) if kind == "tetrahedron"]
    assert len(tetra) >= 10 and all(comps[b].n_faces.tolist() == [4] for b in tetra)
    _check_selection(G, meshes, comps, refs, "B = 67")


def test_gradients_pass_through_the_selection(amd, dev, planted):  # noqa: F811
    from supnerf_amd import geometry as G
    grid, _ = planted
    g1 = grid.clone().requires_grad_()
    subs = G.largest_component(G.extract_mesh(g1, level=0.0, differentiable=True))
    assert all(s[0].grad_fn is not None for s in subs if s[0].shape[0])
    sum(s[0].sum() for s in subs).backward()
    g2 = grid.clone().requires_grad_()
    meshes = G.extract_mesh(g2, level=0.0, differentiable=True)
    sum(v[s[2]].sum() for (v, _), s in zip(meshes, subs)).backward()
    assert bool(g1.grad.any()) and torch.equal(g1.grad, g2.grad)
    g3 = grid.clone().requires_grad_()
    kept = G.extract_mesh(g3, level=0.0, differentiable=True, keep="largest")
    sum(v.sum() for v, _ in kept).backward()
    assert torch.equal(g3.grad, g1.grad)
    # nothing of the dropped pieces: the floaters' grid points get no gradient
    assert not bool(g1.grad[0, 40:, 40:, 40:].any()) and not bool(g1.grad[1].any())


def test_a_bad_face_index_raises(amd, dev, planted):  # noqa: F811
    """An index >= V (or < 0) sets the device flag -- checked before anything is dereferenced -- and the call raises."""
    from supnerf_amd import geometry as G
    _, meshes = planted
    v, f = meshes[2]
    for bad in (v.shape[0], v.shape[0] + 12345, -1, 2 ** 31 - 1):
        f2 = f.clone()
        f2[f.shape[0] // 2, 1] = bad
        with pytest.raises(amd.SnrError, match="face index"):
            G.mesh_components([meshes[0], (v, f2)])
    # an index that belongs to another object's range is out of range too: indices are local
    f3 = meshes[2][1].clone()
    f3[0, 0] = meshes[2][0].shape[0] + 5
    with pytest.raises(amd.SnrError):
        G.mesh_components([(v, f3), meshes[0]])
    assert G.mesh_components(meshes)[0].n_verts.shape[0] == 5                       # and the next call is sound
