"""Mesh simplification on the MI355X: ``geometry.simplify_mesh`` / ``ops.mesh_simplify`` (the ``snr_simplify_*`` kernels) against
tests/simplify_restatement.py, object by object -- ``vert_map``, ``members``, ``faces``, ``face_index`` and every count exactly, positions
and attribute means within one fp32 ulp (``np.spacing`` of the larger magnitude) of the restatement's float64 value rounded to fp32.

Why one ulp: both sides sum in float64 and differ only by summation order and solve method, a relative 1e-13 at the condition bound 1e3,
so after rounding to fp32 they agree or straddle one rounding boundary.  That error is relative to the solve's unknown y (|y| <= cell),
not to the coordinate c0 + y, so a coordinate that cancels to (almost) nothing counts with the magnitude 2^-20 max(|c0|, cell), whose ulp
is that 1e-13 (``simplify_restatement.position_floor``).  Attribute rows are drawn from [0.5, 1.5]: their means do not cancel.

Hand meshes, the tessellated box at three (cell, origin) pairs with both placements, a packed launch of four objects against the
per-object calls bit for bit, clusters of 4096 and 4097 vertices (slab seams), an extracted sphere, guard bands around every output of
the C ABI, two runs bit for bit, and the three ways to be rejected."""
import numpy as np
import pytest
import torch

import simplify_restatement as SR
from segment_sum_restatement import banded as _banded, bands_intact as _bands_intact, segments as slab_segments
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

HALF = (0.25, 0.2, 0.15)
TABLE = [(0.07, (0.013, 0.021, -0.017), 190, 376), (0.11, (0.0, 0.0, 0.0), 80, 156), (0.05, (0.01, 0.0, 0.02), 378, 752)]
INT_FIELDS = (("faces", np.int32), ("vert_map", np.int32), ("members", np.int32), ("face_index", np.int64))


def _np(t):
    return t.detach().cpu().numpy()


def _to_gpu(mesh, dev):  # noqa: F811
    return torch.from_numpy(np.ascontiguousarray(mesh[0], np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(mesh[1], np.int32)).to(dev)


def _attributes(n, channels, seed=0):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (n, channels)).astype(np.float32)


def _compare(got, ref, cell, origin, tag):
    for name, dtype in INT_FIELDS:
        g = _np(getattr(got, name))
        assert g.dtype == dtype and g.shape == ref[name].shape, (tag, name, g.dtype, g.shape, ref[name].shape)
        assert np.array_equal(g, ref[name]), (tag, name)
    v = _np(got.verts)
    assert v.dtype == np.float32 and v.shape == ref["verts"].shape and not got.verts.requires_grad, tag
    worst = SR.ulp_distance(v, ref["verts64"], SR.position_floor(ref, cell, origin)).max(initial=0.0)
    worst_a = 0.0
    if ref["attributes"] is None:
        assert got.attributes is None, tag
    else:
        a = _np(got.attributes)
        assert a.dtype == np.float32 and a.shape == ref["attributes"].shape, tag
        worst_a = SR.ulp_distance(a, ref["attributes64"]).max(initial=0.0)
    print(f"{tag}: V {ref['vert_map'].shape[0]} -> {v.shape[0]}, F' {ref['faces'].shape[0]}; positions {worst:.2f} ulp, attributes {worst_a:.2f} ulp")
    assert worst <= 1.0 and worst_a <= 1.0, (tag, worst, worst_a)


def _check(G, mesh, cell, origin, placement, tag, attributes=None):
    """One object through ``geometry.simplify_mesh`` against the restatement, with and without ``drop_unreferenced``; returns the raw one."""
    dev = mesh[0].device  # noqa: F811
    att = None if attributes is None else torch.from_numpy(attributes).to(dev)
    ref = SR.simplify(_np(mesh[0]), _np(mesh[1]), cell, origin, placement, attributes)
    got = G.simplify_mesh(mesh, cell, origin=torch.tensor(origin), placement=placement, attributes=att, drop_unreferenced=False)
    assert isinstance(got, G.Simplified)
    _compare(got, ref, cell, origin, tag)
    dropped, want = G.simplify_mesh([mesh], cell, origin=torch.tensor(origin), placement=placement, attributes=att)[0], SR.drop_unreferenced(ref)
    for name, dtype in INT_FIELDS:
        g = _np(getattr(dropped, name))
        assert g.dtype == dtype and np.array_equal(g, want[name]), (tag, "drop_unreferenced", name)
    used = np.zeros(ref["members"].shape[0], bool)
    used[ref["faces"].reshape(-1)] = True
    assert np.array_equal(_np(dropped.verts), _np(got.verts)[used]), tag
    if attributes is not None:
        assert np.array_equal(_np(dropped.attributes), _np(got.attributes)[used]), tag
    return got, ref


@pytest.fixture(scope="module")
def box(dev):  # noqa: F811
    verts, faces = SR.box_mesh(HALF, 24)
    return _to_gpu((verts, faces), dev)


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_hand_meshes(amd, dev, placement):  # noqa: F811
    from supnerf_amd import geometry as G
    tri = np.array([[0, 1, 2]], np.int32)
    # one triangle, three cells
    got, _ = _check(G, _to_gpu(([[0.1, 0.1, 0.0], [1.1, 0.1, 0.0], [0.1, 1.1, 0.0]], tri), dev), 1.0, (0, 0, 0), placement, "three cells")
    assert got.faces.shape == (1, 3) and got.members.tolist() == [1, 1, 1]
    # two corners in one cell: the face goes, and with drop_unreferenced everything
    mesh = _to_gpu(([[0.1, 0.1, 0.0], [0.2, 0.1, 0.0], [0.1, 1.1, 0.0]], tri), dev)
    got, _ = _check(G, mesh, 1.0, (0, 0, 0), placement, "two corners in a cell")
    assert got.faces.shape == (0, 3) and got.members.tolist() == [2, 1]
    gone = G.simplify_mesh(mesh, 1.0, placement=placement)
    assert gone.verts.shape == (0, 3) and gone.vert_map.tolist() == [-1, -1, -1]
    # a closed tetrahedron with one edge inside a cell: two faces go, two come out as opposite flaps, both kept
    tet = SR.tetrahedron([[0.2, 0.2, 0.2], [0.6, 0.3, 0.2], [0.3, 1.4, 0.3], [0.4, 0.5, 1.5]])
    got, ref = _check(G, _to_gpu(tet, dev), 1.0, (0, 0, 0), placement, "tetrahedron")
    assert got.faces.shape == (2, 3) and got.members.tolist() == [2, 1, 1] and SR.directed_edges_balance(_np(got.faces))
    # vertices exactly on cell faces: the upper cell; -0 is 0; negative cells
    c = 0.125
    verts = np.array([[-0.0, 0.0, 0.125], [-0.125, -0.25, 0.25], [0.375, -0.0, -0.5], [0.125, 0.125, 0.125], [0.0, 0.0, 0.25],
                      [-0.125, -0.125, -0.125], [0.124, 0.124, 0.249], [-0.001, -0.001, -0.001]], np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [0, 3, 5], [6, 7, 2], [1, 4, 6]], np.int32)
    got, ref = _check(G, _to_gpu((verts, faces), dev), c, (0, 0, 0), placement, "ties")
    assert ref["cluster_q"].tolist() == [[-1, -2, 2], [-1, -1, -1], [0, 0, 1], [0, 0, 2], [1, 1, 1], [3, 0, -4]]
    assert got.vert_map.tolist() == [2, 0, 5, 4, 3, 1, 2, 1]
    _check(G, _to_gpu((verts + np.float32(1.0), faces), dev), c, (1, 1, 1), placement, "ties, shifted")
    # a vertex no face names: a cluster of its own, or one more member of a cluster that faces do name
    verts = np.array([[0.1, 0.1, 0.0], [1.1, 0.1, 0.0], [0.1, 1.1, 0.0], [5.5, 5.5, 5.5], [1.3, 0.3, 0.2]], np.float32)
    got, _ = _check(G, _to_gpu((verts, tri), dev), 1.0, (0, 0, 0), placement, "unreferenced vertex")
    assert got.members.tolist() == [1, 1, 2, 1] and got.vert_map.tolist() == [0, 2, 1, 3, 2]
    assert G.simplify_mesh(_to_gpu((verts, tri), dev), 1.0, placement=placement).vert_map.tolist() == [0, 2, 1, -1, 2]


@pytest.mark.parametrize("placement", ["quadric", "mean"])
@pytest.mark.parametrize("cell,origin,want_verts,want_faces", TABLE)
def test_box(amd, dev, box, cell, origin, want_verts, want_faces, placement):  # noqa: F811
    from supnerf_amd import geometry as G
    for channels in (1, 3, 16):
        got, ref = _check(G, box, cell, origin, placement, f"box {cell} {placement} C={channels}", _attributes(box[0].shape[0], channels, channels))
        assert (got.verts.shape[0], got.faces.shape[0]) == (want_verts, want_faces)
    assert SR.directed_edges_balance(_np(got.faces))
    # determinism: the same call twice, the same bits in every output
    att = torch.from_numpy(_attributes(box[0].shape[0], 16, 16)).to(dev)
    again = G.simplify_mesh(box, cell, origin=torch.tensor(origin), placement=placement, attributes=att, drop_unreferenced=False)
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    if placement == "quadric":                                                    # what the placement is for, on the device's numbers
        v = _np(got.verts)
        assert abs(SR.signed_volume(v, _np(got.faces)) - 0.06) <= 1e-3 * 0.06 and SR.corner_error(v, HALF) <= 1e-3


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_packed_launch_equals_per_object_calls(amd, dev, box, placement):  # noqa: F811
    """B = 4 in one call -- the box at two cells, the box swallowed by one cell, an empty mesh -- bit for bit what four calls give."""
    from supnerf_amd import geometry as G
    empty = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))
    meshes = [box, box, box, empty]
    cells = [0.07, 0.11, 0.6, 0.05]
    origins = torch.tensor([[0.013, 0.021, -0.017], [0.0, 0.0, 0.0], [-0.3, -0.3, -0.3], [0.01, 0.0, 0.02]])
    atts = [torch.from_numpy(_attributes(m[0].shape[0], 3, 5 + i)).to(dev) for i, m in enumerate(meshes)]
    for drop in (False, True):
        packed = G.simplify_mesh(meshes, cells, origin=origins, placement=placement, attributes=atts, drop_unreferenced=drop)
        assert len(packed) == 4
        for b in range(4):
            one = G.simplify_mesh(meshes[b], cells[b], origin=origins[b], placement=placement, attributes=atts[b], drop_unreferenced=drop)
            for name, x, y in zip(G.Simplified._fields, packed[b], one):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (b, name, drop)
    raw = G.simplify_mesh(meshes, cells, origin=origins, placement=placement, drop_unreferenced=False)
    assert [(s.verts.shape[0], s.faces.shape[0]) for s in raw] == [(190, 376), (80, 156), (1, 0), (0, 0)]
    assert raw[2].members.tolist() == [3458] and raw[0].attributes is None
    assert [(s.verts.shape[0], s.faces.shape[0]) for s in packed] == [(190, 376), (80, 156), (0, 0), (0, 0)]
    assert bool((packed[2].vert_map == -1).all()) and packed[2].vert_map.shape == (3458,)
    _compare(raw[2], SR.simplify(_np(box[0]), _np(box[1]), 0.6, (-0.3, -0.3, -0.3), placement), 0.6, (-0.3, -0.3, -0.3), "one cell")
    # the packed form straight from ops
    s = amd.ops.mesh_simplify(torch.cat([m[0] for m in meshes]), torch.cat([m[1] for m in meshes]), [3458, 3458, 3458, 0],
                              [6912, 6912, 6912, 0], cells, origins, placement)
    assert s.n_verts == [190, 80, 1, 0] and s.n_faces == [376, 156, 0, 0] and s.attributes is None
    assert torch.equal(s.verts, torch.cat([r.verts for r in raw])) and torch.equal(s.faces, torch.cat([r.faces for r in raw]))
    assert torch.equal(s.face_index, torch.cat([raw[0].face_index, raw[1].face_index + 6912]))
    assert torch.equal(s.vert_map, torch.cat([r.vert_map for r in raw])) and torch.equal(s.members, torch.cat([r.members for r in raw]))


@pytest.mark.parametrize("n_inside", [4096, 4097])
def test_slab_seams(amd, dev, n_inside):  # noqa: F811
    """One cluster of exactly 4096 and of 4097 vertices (one slab; one and a slab of one); its corner list, 12 285 and 12 288 entries,
    crosses 4096 and 8192 and ends on a slab border."""
    from supnerf_amd import geometry as G
    verts, faces = SR.strip(n_inside)
    for placement in ("quadric", "mean"):
        got, ref = _check(G, _to_gpu((verts, faces), dev), 1.0, (0.0, -0.5, -0.5), placement, f"strip {n_inside} {placement}",
                          _attributes(verts.shape[0], 3, n_inside))
        assert got.members.tolist() == [n_inside, 1, 1, 1, 1, 1, 1] and got.faces.shape == (5, 3)
        corners = np.bincount(ref["vert_map"][faces].reshape(-1))
        assert corners[0] == 3 * n_inside - 3 and (corners[0] > 8192)


def test_extracted_sphere(amd, dev):  # noqa: F811
    """``extract_mesh`` on an analytic 33^3 grid, a ball of radius 0.3, simplified at two grid steps: still one closed, positive piece."""
    from supnerf_amd import geometry as G
    ax = torch.linspace(-0.5, 0.5, 33, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    grid = (0.3 - torch.sqrt(x * x + y * y + z * z))[None].contiguous()
    mesh = G.extract_mesh(grid, level=0.0)[0]
    assert SR.directed_edges_balance(_np(mesh[1]))
    cell = 2.0 / 32
    got, ref = _check(G, mesh, cell, (-0.5, -0.5, -0.5), "quadric", "sphere")
    s = G.simplify_mesh([mesh], cell, origin=torch.tensor([-0.5, -0.5, -0.5]))[0]
    assert 0 < s.faces.shape[0] < mesh[1].shape[0] // 3 and s.verts.shape[0] < mesh[0].shape[0] // 3
    comps = G.mesh_components((s.verts, s.faces))
    assert comps.n_verts.tolist() == [s.verts.shape[0]] and float(comps.volume[0]) > 0
    assert SR.directed_edges_balance(_np(s.faces))
    full = float(G.mesh_components(mesh).volume[0])
    print(f"sphere: F {mesh[1].shape[0]} -> {s.faces.shape[0]}, volume {full:.6f} -> {float(comps.volume[0]):.6f}")
    assert abs(float(comps.volume[0]) - full) < 0.05 * full                       # (a ball has no edges to keep: a loose sanity bound)


def test_canaries_through_the_c_abi(amd, dev, box):  # noqa: F811
    """Every output buffer of every entry point between NaN- or -1-filled guard bands, the sorted lists fed from the restatement: the
    outputs are the restatement's and the bands are intact."""
    ops, lib = amd.ops, amd._lib.lib()
    P, st = ops._ptr, ops._stream(dev)
    i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
    cell, origin = 0.07, (0.013, 0.021, -0.017)
    verts, faces = box
    nV, nF, nCh = verts.shape[0], faces.shape[0], 3
    att = _attributes(nV, nCh, 3)
    ref = SR.simplify(_np(verts), _np(faces), cell, origin, "quadric", att)
    nC, nK = ref["members"].shape[0], ref["faces"].shape[0]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)  # noqa: E731
    voff, foff = up(np.array([0, nV]), i64), up(np.array([0, nF]), i64)
    cell_t, origin_t = torch.tensor([cell], device=dev), torch.tensor([origin], device=dev)
    nan = float("nan")
    checks = []

    bad = torch.zeros(2, dtype=i32, device=dev)
    key_full, key = _banded(nV, i64, dev, -1)
    assert lib.snr_simplify_keys(P(verts), P(voff, i64), P(cell_t), P(origin_t), 1, nV, P(key, i64), P(bad[:1], i32), st) == 0
    checks.append((key_full, nV, -1))
    q = ref["cluster_q"].astype(np.int64)[ref["vert_map"]] + (1 << 20)
    assert np.array_equal(_np(key), (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2])

    nf_full, new_faces = _banded(nF * 3, i32, dev, -1)
    keep_full, keep = _banded(nF, u8, dev, 255)
    assert lib.snr_simplify_faces(P(faces, i32), P(up(ref["vert_map"], i32), i32), P(voff, i64), P(foff, i64), 1, nV, nF, P(new_faces, i32),
                                  P(keep, u8), P(bad[1:], i32), st) == 0
    checks += [(nf_full, nF * 3, -1), (keep_full, nF, 255)]
    keep_ref = np.zeros(nF, np.uint8)
    keep_ref[ref["face_index"]] = 1
    assert np.array_equal(_np(keep), keep_ref) and np.array_equal(_np(new_faces).reshape(-1, 3), ref["vert_map"][_np(faces)])
    assert bad.tolist() == [0, 0]

    of_full, out_faces = _banded(nK * 3, i32, dev, -1)
    fi_full, face_index = _banded(nK, i64, dev, -1)
    keep_scan = torch.cumsum(keep, 0, dtype=i64)
    assert lib.snr_simplify_compact(P(new_faces, i32), P(keep, u8), P(keep_scan, i64), nF, nK, P(out_faces, i32), P(face_index, i64), st) == 0
    checks += [(of_full, nK * 3, -1), (fi_full, nK, -1)]
    assert np.array_equal(_np(out_faces).reshape(-1, 3), ref["faces"]) and np.array_equal(_np(face_index), ref["face_index"])

    vorder, vseg, vslab = (up(a, i64) for a in slab_segments(ref["vert_map"].astype(np.int64), nC))
    corder, cseg, cslab = (up(a, i64) for a in slab_segments(ref["vert_map"].astype(np.int64)[_np(faces)].reshape(-1), nC))
    n_vs, n_cs = int(lib.snr_segment_slab_bound(nC, nV)), int(lib.snr_segment_slab_bound(nC, nF * 3))
    assert n_vs == nC + nV // 4096 and n_cs == nC + 3 * nF // 4096
    for quadric in (1, 0):
        vp_full, vpart = _banded(n_vs * 3, f64, dev, nan)
        cp_full, cpart = _banded(n_cs * 9, f64, dev, nan)
        ov_full, out_verts = _banded(nC * 3, torch.float32, dev, nan)
        assert lib.snr_simplify_positions(P(verts), P(faces, i32), P(voff, i64), P(foff, i64), P(cell_t), P(origin_t), 1, nV, nF,
                                          P(vorder, i64), P(vseg, i64), P(vslab, i64), P(corder, i64), P(cseg, i64), P(cslab, i64), nC,
                                          quadric, P(vpart, f64), n_vs, P(cpart, f64), n_cs, P(out_verts), st) == 0
        torch.cuda.synchronize()
        assert _bands_intact(vp_full, n_vs * 3, nan) and _bands_intact(cp_full, n_cs * 9, nan) and _bands_intact(ov_full, nC * 3, nan)
        want = ref if quadric else SR.simplify(_np(verts), _np(faces), cell, origin, "mean")
        assert SR.ulp_distance(_np(out_verts).reshape(-1, 3), want["verts64"], SR.position_floor(ref, cell, origin)).max() <= 1.0
    ap_full, apart = _banded(n_vs * nCh, f64, dev, nan)
    oa_full, out_att = _banded(nC * nCh, torch.float32, dev, nan)
    assert lib.snr_simplify_attributes(P(up(att, torch.float32)), nCh, nV, P(vorder, i64), P(vseg, i64), P(vslab, i64), nC, P(apart, f64), n_vs,
                                       P(out_att), st) == 0
    checks += [(ap_full, n_vs * nCh, nan), (oa_full, nC * nCh, nan)]
    assert SR.ulp_distance(_np(out_att).reshape(-1, nCh), ref["attributes64"]).max() <= 1.0
    torch.cuda.synchronize()
    for full, n, fill in checks:
        assert _bands_intact(full, n, fill), (n, fill)


def test_what_has_no_cell_or_no_vertex_raises(amd, dev, box):  # noqa: F811
    """A NaN coordinate, a coordinate 2^20 cells out and a face index out of range set their device flags -- nothing is dereferenced with
    them -- and the call raises; the next call is sound."""
    from supnerf_amd import geometry as G
    verts, faces = box
    for value in (float("nan"), float("inf"), 0.05 * 2 ** 20 + 1.0, -0.05 * 2 ** 20 - 1.0):
        v2 = verts.clone()
        v2[1234, 1] = value
        with pytest.raises(amd.SnrError, match="not finite or lies"):
            G.simplify_mesh([box, (v2, faces)], 0.05)
    v2 = verts.clone()
    v2[0, 0] = 0.05 * (2 ** 20 - 2)                                               # still inside: a cluster of its own
    assert G.simplify_mesh((v2, faces), 0.05, origin=torch.tensor([0.01, 0.0, 0.02]), drop_unreferenced=False).verts.shape[0] == 379
    for index in (verts.shape[0], verts.shape[0] + 12345, -1, 2 ** 31 - 1):
        f2 = faces.clone()
        f2[faces.shape[0] // 2, 1] = index
        for placement in ("quadric", "mean"):
            with pytest.raises(amd.SnrError, match="face index"):
                G.simplify_mesh([box, (verts, f2)], 0.05, placement=placement)
    with pytest.raises(amd.SnrError, match="cell"):
        G.simplify_mesh(box, torch.tensor([0.0], device=dev))
    with pytest.raises(amd.SnrError, match="cell"):
        G.simplify_mesh([box, box], [0.05, -1.0])
    s = G.simplify_mesh(box, 0.05, origin=torch.tensor([0.01, 0.0, 0.02]))
    assert (s.verts.shape[0], s.faces.shape[0]) == (378, 752)
    # vertices with a grad_fn are read by value; the output carries none
    vg = verts.clone().requires_grad_()
    s2 = G.simplify_mesh((vg * 1.0, faces), 0.05, origin=torch.tensor([0.01, 0.0, 0.02]))
    assert s2.verts.grad_fn is None and not s2.verts.requires_grad and torch.equal(s2.verts, s.verts)
