"""Mesh simplification on the host: the rules of include/supnerf_hip.h ("Mesh simplification") as tests/simplify_restatement.py restates
them, held against what the tessellated box +-(0.25, 0.2, 0.15) must give -- exact counts, a closed result, quadric placement that keeps
volume and corners where mean placement demonstrably loses them -- with planted mistakes that the same checks reject; and the parts of
the new API that need no GPU (symbols, signatures, the argument checks of the C ABI and of the Python layer).

The bounds are on the restatement, not on the code under test: 1e-3 lies above its 1.7e-4 .. 3.5e-4 (quadric, volume, relative) and
1.3e-4 .. 3.4e-4 (quadric, corners) and below its 2.1e-2 .. 1.1e-1 (mean, volume, relative) and 2.1e-2 .. 4.2e-2 (mean, corners)."""
import inspect

import numpy as np
import pytest
import torch

import simplify_restatement as SR

HALF = (0.25, 0.2, 0.15)
VOLUME = 0.06
# (cell, origin) -> (vertices, faces) after clustering
TABLE = [(0.07, (0.013, 0.021, -0.017), 190, 376), (0.11, (0.0, 0.0, 0.0), 80, 156), (0.05, (0.01, 0.0, 0.02), 378, 752)]


@pytest.fixture(scope="module")
def box():
    verts, faces = SR.box_mesh(HALF, 24)
    assert verts.shape == (3458, 3) and faces.shape == (6912, 3) and verts.dtype == np.float32 and faces.dtype == np.int32
    assert abs(SR.signed_volume(verts, faces) - VOLUME) < 1e-7 and SR.directed_edges_balance(faces)
    return verts, faces


def _quadric_checks(verts, faces, cell, origin, want_verts, want_faces, planted=None):
    """Every check a quadric-placed box has to pass; a list of the ones it fails."""
    s = SR.simplify(verts, faces, cell, origin, "quadric", planted=planted)
    failed = []
    if (s["verts"].shape[0], s["faces"].shape[0]) != (want_verts, want_faces):
        failed.append("counts")
    if not SR.directed_edges_balance(s["faces"]):
        failed.append("closed")
    if abs(SR.signed_volume(s["verts"], s["faces"]) - VOLUME) > 1e-3 * VOLUME:
        failed.append("volume")
    if SR.corner_error(s["verts"], HALF) > 1e-3:
        failed.append("corners")
    if not SR.inside_cells(s, cell, origin):
        failed.append("inside its cell")
    return failed


@pytest.mark.parametrize("cell,origin,want_verts,want_faces", TABLE)
def test_box_counts_closure_and_placement(box, cell, origin, want_verts, want_faces):
    verts, faces = box
    assert _quadric_checks(verts, faces, cell, origin, want_verts, want_faces) == []
    q = SR.simplify(verts, faces, cell, origin, "quadric")
    m = SR.simplify(verts, faces, cell, origin, "mean")
    for name in ("faces", "vert_map", "members", "face_index"):                 # the placement moves vertices and nothing else
        assert np.array_equal(q[name], m[name]), name
    assert SR.directed_edges_balance(m["faces"])
    vol_m, corner_m = SR.signed_volume(m["verts"], m["faces"]), SR.corner_error(m["verts"], HALF)
    print(f"cell {cell}: quadric volume {SR.signed_volume(q['verts'], q['faces']):.6f} corners {SR.corner_error(q['verts'], HALF):.2e}; "
          f"mean volume {vol_m:.6f} corners {corner_m:.2e}")
    assert vol_m < VOLUME * (1 - 2e-2) and corner_m > 1e-2                      # mean placement shrinks edges and corners
    # rule 2 and rule 6, stated as properties
    assert q["vert_map"].dtype == np.int32 and q["members"].dtype == np.int32 and q["face_index"].dtype == np.int64
    assert int(q["members"].sum()) == verts.shape[0] and np.array_equal(np.bincount(q["vert_map"]), q["members"])
    cq = q["cluster_q"].astype(np.int64)
    packed = (cq[:, 0] * (1 << 42)) + (cq[:, 1] * (1 << 21)) + cq[:, 2]
    assert (np.diff(packed) > 0).all()                                          # ascending lexicographic (qx, qy, qz), each once
    assert (np.diff(q["face_index"]) > 0).all()
    assert np.array_equal(q["faces"], q["vert_map"][faces[q["face_index"]]])
    dropped = np.setdiff1d(np.arange(faces.shape[0]), q["face_index"])
    nf = q["vert_map"][faces[dropped]]
    assert ((nf[:, 0] == nf[:, 1]) | (nf[:, 1] == nf[:, 2]) | (nf[:, 0] == nf[:, 2])).all()
    # every cluster of the box is named by a face: nothing for drop_unreferenced to do
    d = SR.drop_unreferenced(q)
    assert np.array_equal(d["verts"], q["verts"]) and np.array_equal(d["faces"], q["faces"]) and np.array_equal(d["vert_map"], q["vert_map"])


def test_one_cell_swallows_the_box(box):
    verts, faces = box
    for placement in ("quadric", "mean"):
        s = SR.simplify(verts, faces, 0.6, (-0.3, -0.3, -0.3), placement)
        assert s["verts"].shape == (1, 3) and s["faces"].shape == (0, 3) and s["members"].tolist() == [3458]
        assert not s["vert_map"].any() and s["face_index"].shape == (0,)
        assert np.abs(s["verts"]).max() < 1e-6                                   # the centre of the box, either way
        d = SR.drop_unreferenced(s)
        assert d["verts"].shape == (0, 3) and d["faces"].shape == (0, 3) and d["members"].shape == (0,)
        assert d["vert_map"].shape == (3458,) and (d["vert_map"] == -1).all()


@pytest.mark.parametrize("planted", SR.PLANTED)
def test_planted_mistakes_are_rejected(box, planted):
    """The checks of test_box_counts_closure_and_placement, plus the same ones on a thin wedge seen edge-on (two sheets through one cell
    whose planes meet outside it), reject every planted mistake at least once and pass the rules as they stand everywhere."""
    verts, faces = box
    wv, wf = SR.wedge()
    wcell, worigin = 1.0, (0.0, -0.5, -0.5)
    clean, dirty = [], []
    for cell, origin, nv, nf in TABLE:
        clean += _quadric_checks(verts, faces, cell, origin, nv, nf)
        dirty += _quadric_checks(verts, faces, cell, origin, nv, nf, planted)
    for p, sink in ((None, clean), (planted, dirty)):
        s = SR.simplify(wv, wf, wcell, worigin, "quadric", planted=p)
        assert (s["verts"].shape[0], s["faces"].shape[0]) == (12, 24)
        if not SR.inside_cells(s, wcell, worigin):
            sink.append("wedge: inside its cell")
    print(planted, "->", dirty)
    assert clean == [] and dirty != []
    if planted == "no_clamp":                                                     # the wedge's unclamped solve does leave its cell
        assert "wedge: inside its cell" in dirty
        free = SR.simplify(wv, wf, wcell, worigin, "quadric", planted=planted)
        held = SR.simplify(wv, wf, wcell, worigin, "quadric")
        k = int(np.argmax(np.abs(free["verts64"] - held["verts64"]).max(1)))
        assert free["verts64"][k, 0] < free["cluster_q"][k, 0] * wcell < held["verts64"][k, 0] + 1e-12
    else:
        assert "corners" in dirty


def test_rule_one_ties_and_limits():
    """A coordinate exactly on a cell face belongs to the upper cell, -0 counts as 0, and what has no usable cell is rejected."""
    c = 0.125
    x = np.array([[-0.0, 0.0, 0.125], [-0.125, -0.25, 0.25], [0.124999, -1e-9, -0.125001]], np.float32)
    assert SR.cell_index(x, c, (0, 0, 0)).tolist() == [[0, 0, 1], [-1, -2, 2], [0, -1, -2]]
    assert SR.cell_index(x + np.float32(1.0), c, (1, 1, 1)).tolist()[:2] == [[0, 0, 1], [-1, -2, 2]]
    assert SR.cell_index([[c * (2 ** 20 - 1), 0, 0]], c, (0, 0, 0))[0, 0] == 2 ** 20 - 1
    for bad in ([[np.nan, 0, 0]], [[0, np.inf, 0]], [[c * 2 ** 20, 0, 0]], [[0, 0, -c * (2 ** 20 + 1)]]):
        with pytest.raises(SR.Rejected):
            SR.cell_index(bad, c, (0, 0, 0))
    with pytest.raises(SR.Rejected):
        SR.simplify(x, [[0, 1, 3]], c)
    with pytest.raises(SR.Rejected):
        SR.simplify(x, [[0, 1, 2]], 0.0)


# ------------------------------------------------------------------ the API without a GPU
SIMPLIFY_SYMBOLS = ("snr_simplify_keys", "snr_simplify_faces", "snr_simplify_compact", "snr_segment_slab_bound", "snr_simplify_positions",
                    "snr_simplify_attributes")


def test_symbols_and_signatures():
    import os
    import re
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, geometry as G, ops
    assert all(n in _lib.exported_symbols() for n in SIMPLIFY_SYMBOLS)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in SIMPLIFY_SYMBOLS)
    assert _lib.header_abi_version() >= 21 and lib.snr_abi_version() == _lib.header_abi_version()
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    hdr = open(os.path.join(here, "..", "include", "supnerf_hip.h")).read()
    assert all(re.search(r"\b" + n + r"\(", hdr) for n in SIMPLIFY_SYMBOLS) and "Mesh simplification" in hdr
    assert float(re.search(r"#define\s+SNR_SIMPLIFY_EPS\s+(\S+)", hdr).group(1)) == SR.EPS
    exports = open(os.path.join(here, "csrc", "exports.map")).read()
    assert re.search(r"global:[^;]*\bsnr_\*", exports)                           # every snr_* name is exported, the new ones with them
    assert list(inspect.signature(ops.mesh_simplify).parameters) == ["verts", "faces", "n_verts", "n_faces", "cell", "origin", "placement",
                                                                     "attributes"]
    assert inspect.signature(ops.mesh_simplify).parameters["placement"].default == "quadric"
    assert ops.SimplifiedMesh._fields == ("verts", "faces", "n_verts", "n_faces", "vert_map", "members", "face_index", "attributes")
    assert G.Simplified._fields == ("verts", "faces", "vert_map", "face_index", "members", "attributes")
    sig = inspect.signature(G.simplify_mesh)
    assert list(sig.parameters) == ["meshes", "cell", "origin", "placement", "attributes", "drop_unreferenced"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig.parameters)[2:])
    assert sig.parameters["placement"].default == "quadric" and sig.parameters["drop_unreferenced"].default is True
    assert sig.parameters["origin"].default is None and sig.parameters["attributes"].default is None
    # the C ABI validates before it launches: these return without touching a device
    big = 1 << 39
    assert lib.snr_simplify_keys(None, None, None, None, 1, 4, None, None, None) == -1                       # null flag
    assert lib.snr_simplify_keys(None, None, None, None, 1, -1, None, None, None) == -1
    assert lib.snr_simplify_keys(None, None, None, None, -1, 4, None, None, None) == -1
    assert lib.snr_simplify_keys(None, None, None, None, 1, big, None, None, None) == -5
    assert lib.snr_simplify_faces(None, None, None, None, 1, 4, 4, None, None, None, None) == -1
    assert lib.snr_simplify_faces(None, None, None, None, 1, 4, -4, None, None, None, None) == -1
    assert lib.snr_simplify_faces(None, None, None, None, 1, 4, big, None, None, None, None) == -5
    assert lib.snr_simplify_compact(None, None, None, 4, 2, None, None, None) == -1
    assert lib.snr_simplify_compact(None, None, None, 4, 5, None, None, None) == -1                          # more kept than there are
    assert lib.snr_simplify_compact(None, None, None, 4, 0, None, None, None) == 0
    assert lib.snr_simplify_compact(None, None, None, big, 1, None, None, None) == -5
    assert lib.snr_segment_slab_bound(5, 10000) == 5 + 10000 // ops.MESH_SLAB and lib.snr_segment_slab_bound(-1, 4) == 0
    pos = lambda nV, nF, nC, quadric, vs, cs: lib.snr_simplify_positions(None, None, None, None, None, None, 1, nV, nF, None, None, None,  # noqa: E731
                                                                         None, None, None, nC, quadric, None, vs, None, cs, None, None)
    assert pos(100, 50, 10, 1, 10, 10) == -1
    assert pos(100, 50, 0, 1, 0, 0) == 0
    assert pos(100, 50, 10, 2, 10, 10) == -1
    assert pos(100, 50, 101, 1, 200, 200) == -1                                                               # more clusters than vertices
    assert pos(10000, 50, 10, 0, 11, 0) == -3                                                                 # workspace: 12 slabs needed
    assert pos(100, 10000, 10, 1, 10, 16) == -3                                                               # 17 corner slabs needed
    assert pos(100, 10000, 10, 0, 10, 0) == -1                                                                # (mean: no corner scratch)
    assert pos(big, 50, 10, 1, 10, 10) == -5 and pos(100, big, 10, 1, 10, 10) == -5
    att = lambda C_, nV, nC, ns: lib.snr_simplify_attributes(None, C_, nV, None, None, None, nC, None, ns, None, None)  # noqa: E731
    assert att(3, 100, 10, 10) == -1 and att(0, 100, 10, 10) == -1 and att(17, 100, 10, 10) == -1
    assert att(3, 100, 0, 0) == 0 and att(3, 10000, 10, 11) == -3 and att(3, big, 10, 10) == -5


def test_cpu_tensors_and_bad_arguments_raise(box):
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    verts, faces = box
    v, f = torch.from_numpy(verts), torch.from_numpy(faces)
    with pytest.raises(A.SnrError, match="GPU|gpu|CPU|device"):
        G.simplify_mesh([(v, f)], 0.05)                                          # CPU tensors: no fallback
    with pytest.raises(A.SnrError):
        G.simplify_mesh((v, f), 0.05)
    with pytest.raises(A.SnrError):
        A.ops.mesh_simplify(v, f, [v.shape[0]], [f.shape[0]], 0.05, torch.zeros(1, 3))
    with pytest.raises(A.SnrError, match="int32"):
        A.ops.mesh_simplify(v, f.long(), [v.shape[0]], [f.shape[0]], 0.05, torch.zeros(1, 3))
    for cell in (0.0, -0.05, float("nan"), [0.05, 0.0]):
        with pytest.raises(A.SnrError, match="cell"):
            A.ops.mesh_simplify(v, f, [v.shape[0]], [f.shape[0]], cell, torch.zeros(1, 3))
    with pytest.raises(A.SnrError, match="placement"):
        A.ops.mesh_simplify(v, f, [v.shape[0]], [f.shape[0]], 0.05, torch.zeros(1, 3), placement="median")
    with pytest.raises(A.SnrError, match="placement"):
        G.simplify_mesh([(v, f)], 0.05, placement="median")
    assert G.simplify_mesh([], 0.05) == []
