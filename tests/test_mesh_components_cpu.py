"""Mesh components on the host: the rules of include/supnerf_hip.h ("Mesh components") as tests/mesh_restatement.py restates them, judged
against ``scipy.sparse.csgraph.connected_components`` and against what the planted five-piece grid must give; and the parts of the new API
that need no GPU (symbols, signatures, argument checks of the C ABI, the selection policy)."""
import inspect

import numpy as np
import pytest
import torch

import iso_restatement as IR
import mesh_restatement as MR


def _scipy_labels(n_verts, faces):
    """Component ids by scipy, renumbered by rule 2: in the order of each component's smallest vertex index."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows, cols = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    g = coo_matrix((np.ones(rows.shape[0], np.int8), (rows, cols)), shape=(n_verts, n_verts))
    n, lab = connected_components(g, directed=False)
    first = np.full(n, n_verts, np.int64)
    np.minimum.at(first, lab, np.arange(n_verts))
    rank = np.empty(n, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(n)
    return n, rank[lab].astype(np.int32)


def _check_against_scipy(verts, faces, tag):
    c = MR.components(verts, faces)
    n, want = _scipy_labels(verts.shape[0], faces)
    assert c["n_verts"].shape[0] == n, (tag, c["n_verts"].shape[0], n)
    assert c["vert_label"].dtype == np.int32 and np.array_equal(c["vert_label"], want), tag
    assert np.array_equal(c["face_label"], want[np.asarray(faces)[:, 0]] if len(faces) else np.zeros(0, np.int32)), tag
    assert int(c["n_verts"].sum()) == verts.shape[0] and int(c["n_faces"].sum()) == len(faces), tag
    assert c["vert_label"][0] == 0 and np.array_equal(c["first"], np.sort(c["first"])), tag
    # every face lies within one component
    assert (c["vert_label"][np.asarray(faces, dtype=np.int64)] == c["face_label"][:, None]).all(), tag
    return c


@pytest.fixture(scope="module")
def planted():
    f, lo, h = MR.planted_field(48)
    verts, faces = IR.extract(f, 0.0, lo, h)
    return verts, faces, MR.components(verts, faces)


def test_planted_grid_has_its_five_pieces(planted):
    """n = 48, bound +-0.5, level 0: 14 074 vertices, 28 076 faces, 5 components -- floater, body (volume +0.113), the closed cavity
    inside it (volume -0.0071), floater, and the ball the border cuts open."""
    verts, faces, c = planted
    assert verts.shape == (14074, 3) and faces.shape == (28076, 3)
    assert c["n_verts"].tolist()[:4] == [284, 11138, 1778, 446] and c["n_verts"].shape == (5,)
    assert int(c["n_verts"].sum()) == 14074 and int(c["n_faces"].sum()) == 28076
    assert (np.sign(c["volume"][:4]) == [1, 1, -1, 1]).all(), c["volume"]
    assert abs(c["volume"][1] - 0.1127) < 2e-4 and abs(c["volume"][2] + 0.0071) < 1e-4
    euler = [IR.euler_characteristic(*MR.select(verts, faces, c, [i])[:2]) for i in range(5)]
    assert euler == [2, 2, 2, 2, 1]
    # closed components: n_faces = 2 n_verts - 4, and the volume does not depend on the reference vertex
    assert (c["n_faces"][:4] == 2 * c["n_verts"][:4] - 4).all()
    for i in range(4):
        sv, sf, _, _ = MR.select(verts, faces, c, [i])
        assert abs(IR.signed_volume(sv, sf) - c["volume"][i]) <= 1e-12
        assert abs(IR.area(sv, sf) - c["area"][i]) <= 1e-12
    # the open piece reaches the bound, the others do not
    assert c["bbox_hi"][4, 0] > 0.4999 and (np.abs(np.concatenate([c["bbox_lo"][:4], c["bbox_hi"][:4]])) < 0.47).all()
    for by in ("area", "volume", "faces"):
        assert MR.largest(c, by).tolist() == [False, True, False, False, False], by
        assert MR.largest(c, by, drop_cavities=False).tolist() == [False, True, True, False, False], by


def test_labels_equal_scipy(planted):
    verts, faces, _ = planted
    _check_against_scipy(verts, faces, "planted")
    f, lo, h = IR.noise_field(40)
    c = _check_against_scipy(*IR.extract(f, 0.0, lo, h), "noise")
    assert c["n_verts"].shape == (14,) and c["n_verts"][0] == 54061 and sorted(c["n_verts"][1:].tolist())[::12] == [6, 558]
    f, lo, h = IR.level_equal_field(12)
    c = _check_against_scipy(*IR.extract(f, 0.0, lo, h), "level-equal")
    assert c["n_verts"].shape[0] > 1
    # unreferenced vertices: components of their own with 0 faces; equal positions do not connect
    verts, faces = planted[0][:600], planted[1][(planted[1] < 300).all(1)]
    verts = np.concatenate([verts, verts[:3]])                                   # three exact copies of referenced vertices
    c = _check_against_scipy(verts, faces, "unreferenced")
    lone = c["n_faces"] == 0
    assert lone.sum() >= 303 and (c["n_verts"][lone] == 1).all() and (c["area"][lone] == 0).all() and (c["volume"][lone] == 0).all()
    assert np.array_equal(c["bbox_lo"][lone], c["bbox_hi"][lone])
    copies = c["vert_label"][-3:]
    assert len(set(copies.tolist())) == 3 and lone[copies].all() and not lone[c["vert_label"][faces[0]]].any()
    # an empty mesh
    c = MR.components(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert c["n_verts"].shape == (0,) and c["vert_label"].shape == (0,) and not MR.largest(c).any()


def test_labels_follow_a_renumbering(planted):
    """The rules lean on nothing but the indices: renumber the vertices, shuffle the faces, and the partition is the same while the ids
    follow the new smallest indices."""
    verts, faces, c = planted
    g = np.random.default_rng(7)
    for perm in (g.permutation(verts.shape[0]), np.arange(verts.shape[0])[::-1].copy()):
        pv, pf = MR.permuted(verts, faces, perm, g.permutation(faces.shape[0]))
        pc = _check_against_scipy(pv, pf, "permuted")
        assert sorted(pc["n_verts"].tolist()) == sorted(c["n_verts"].tolist())
        ba, bv = MR.sum_bounds(c)
        for i in range(0, verts.shape[0], 7):
            new, old = int(pc["vert_label"][perm[i]]), int(c["vert_label"][i])
            assert pc["n_verts"][new] == c["n_verts"][old] and pc["n_faces"][new] == c["n_faces"][old]
            assert np.array_equal(pc["bbox_lo"][new], c["bbox_lo"][old]) and np.array_equal(pc["bbox_hi"][new], c["bbox_hi"][old])
            assert abs(pc["area"][new] - c["area"][old]) <= ba
            if old != 4:                                      # (the open piece's volume depends on its reference vertex)
                assert abs(pc["volume"][new] - c["volume"][old]) <= bv


def test_selection_restated(planted):
    verts, faces, c = planted
    sv, sf, vi, fi = MR.select(verts, faces, c, [1, 2])
    assert sv.shape[0] == 11138 + 1778 and sf.shape[0] == int(c["n_faces"][1] + c["n_faces"][2])
    assert np.array_equal(sv, verts[vi]) and np.array_equal(sv[sf], verts[faces[fi]])
    assert (np.diff(vi) > 0).all() and (np.diff(fi) > 0).all() and sf.dtype == np.int32
    mask = np.array([False, True, True, False, False])
    assert all(np.array_equal(a, b) for a, b in zip(MR.select(verts, faces, c, mask), (sv, sf, vi, fi)))
    assert MR.select(verts, faces, c, [])[0].shape == (0, 3)


# ------------------------------------------------------------------ the API without a GPU
MESH_SYMBOLS = ("snr_mesh_hook", "snr_mesh_flatten", "snr_mesh_label", "snr_mesh_boxes", "snr_mesh_face_terms", "snr_segment_slab_bound",
                "snr_mesh_segment_sum")


def test_symbols_and_signatures():
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, geometry as G, ops
    assert all(n in _lib.exported_symbols() for n in MESH_SYMBOLS)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in MESH_SYMBOLS)
    assert _lib.header_abi_version() >= 14
    assert hasattr(ops, "mesh_components") and list(inspect.signature(ops.mesh_components).parameters) == ["verts", "faces", "n_verts", "n_faces"]
    assert ops.MeshComponents._fields[:2] == ("vert_label", "face_label")
    assert G.Components._fields == ("vert_label", "face_label", "n_verts", "n_faces", "area", "volume", "bbox_lo", "bbox_hi")
    assert list(inspect.signature(G.mesh_components).parameters) == ["meshes"]
    assert list(inspect.signature(G.select_components).parameters) == ["mesh", "components", "keep"]
    lc = inspect.signature(G.largest_component)
    assert list(lc.parameters) == ["meshes", "by", "drop_cavities"] and lc.parameters["by"].default == "area"
    assert lc.parameters["drop_cavities"].default is True
    em = inspect.signature(G.extract_mesh)
    assert em.parameters["keep"].default is None and em.parameters["keep"].kind is inspect.Parameter.KEYWORD_ONLY
    # the C ABI validates before it launches: these return without touching a device
    big = 1 << 39
    assert lib.snr_mesh_hook(None, None, None, 1, 4, 4, None, None, None) == -1                  # null flag
    assert lib.snr_mesh_hook(None, None, None, 1, -1, 4, None, None, None) == -1
    assert lib.snr_mesh_hook(None, None, None, -1, 4, 4, None, None, None) == -1
    assert lib.snr_mesh_hook(None, None, None, 1, big, 4, None, None, None) == -5
    assert lib.snr_mesh_hook(None, None, None, 1, 4, big, None, None, None) == -5
    assert lib.snr_mesh_flatten(None, None, 1, 4, None, None, None) == -1
    assert lib.snr_mesh_flatten(None, None, 1, 0, None, None, None) == 0
    assert lib.snr_mesh_flatten(None, None, 1, -2, None, None, None) == -1
    assert lib.snr_mesh_flatten(None, None, 1, big, None, None, None) == -5
    assert lib.snr_mesh_label(None, None, None, None, None, 1, 4, 4, None, None, None) == -1
    assert lib.snr_mesh_label(None, None, None, None, None, 1, 0, 0, None, None, None) == 0
    assert lib.snr_mesh_label(None, None, None, None, None, 1, 4, big, None, None, None) == -5
    assert lib.snr_mesh_boxes(None, None, None, None, 1, 4, 2, None, None, None, None) == -1
    assert lib.snr_mesh_boxes(None, None, None, None, 1, 0, 0, None, None, None, None) == 0
    assert lib.snr_mesh_boxes(None, None, None, None, 1, 4, -1, None, None, None, None) == -1
    assert lib.snr_mesh_boxes(None, None, None, None, 1, 4, big, None, None, None, None) == -5
    assert lib.snr_mesh_face_terms(None, None, None, None, None, None, 1, 4, 4, None, None, None) == -1
    assert lib.snr_mesh_face_terms(None, None, None, None, None, None, 1, 4, 0, None, None, None) == 0
    assert lib.snr_mesh_face_terms(None, None, None, None, None, None, 1, 4, big, None, None, None) == -5
    assert lib.snr_segment_slab_bound(5, 10000) == 5 + 10000 // ops.MESH_SLAB and lib.snr_segment_slab_bound(-1, 4) == 0
    assert lib.snr_mesh_segment_sum(None, None, None, None, 2, 100, None, 2, None, None, None) == -1
    assert lib.snr_mesh_segment_sum(None, None, None, None, 2, 10000, None, 3, None, None, None) == -3     # workspace: 4 slabs needed
    assert lib.snr_mesh_segment_sum(None, None, None, None, 0, 0, None, 0, None, None, None) == 0
    assert lib.snr_mesh_segment_sum(None, None, None, None, 2, 100, None, -1, None, None, None) == -1
    assert lib.snr_mesh_segment_sum(None, None, None, None, big, 100, None, big, None, None, None) == -5


def test_cpu_tensors_and_bad_arguments_raise(planted):
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    verts, faces, _ = planted
    mesh = (torch.from_numpy(verts), torch.from_numpy(faces))
    with pytest.raises(A.SnrError):
        G.mesh_components([mesh])                                                # CPU tensors: no fallback
    with pytest.raises(A.SnrError):
        G.mesh_components(mesh)
    with pytest.raises(A.SnrError):
        G.largest_component([mesh])
    with pytest.raises(A.SnrError):
        G.largest_component([mesh], by="weight")
    with pytest.raises(A.SnrError):
        G.extract_mesh(torch.zeros(4, 4, 4), level=0.0, keep="smallest")
    with pytest.raises(A.SnrError):
        A.ops.mesh_components(mesh[0], mesh[1], [verts.shape[0]], [faces.shape[0]])
    assert G.mesh_components([]) == [] and G.largest_component([]) == []


@pytest.mark.parametrize("by", ["area", "volume", "faces"])
def test_largest_keep_is_the_restated_policy(planted, by):
    """``geometry.largest_keep`` is plain tensor arithmetic on a ``Components``: fed the restatement's numbers it picks the body (id 1) and,
    with ``drop_cavities=False``, the cavity inside it; ties go to the lowest id."""
    from supnerf_amd import geometry as G
    _, _, c = planted
    comp = G.Components(*[torch.from_numpy(np.ascontiguousarray(c[k])) for k in G.Components._fields])
    for drop in (True, False):
        assert G.largest_keep(comp, by, drop).tolist() == MR.largest(c, by, drop).tolist()
    assert G.largest_keep(comp, by).tolist() == [False, True, False, False, False]
    tie = comp._replace(area=torch.ones(5, dtype=torch.float64), volume=-torch.ones(5, dtype=torch.float64), n_faces=torch.full((5,), 7))
    assert G.largest_keep(tie, by).tolist() == [True, False, False, False, False]
    empty = G.Components(*[torch.from_numpy(np.ascontiguousarray(c[k][:0])) for k in G.Components._fields])
    assert G.largest_keep(empty, by).shape == (0,)
