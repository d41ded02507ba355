"""The density backward's host side: the PLY writer's normals and colours, the argument checks of the new ``geometry`` and ``ops`` entry
points (no GPU needed: CPU tensors and malformed shapes raise ``SnrError``), and ``to_object_frame(direction=True)``."""
import numpy as np
import pytest
import torch

import iso_restatement as I


def _write_ply_before(path, verts, faces):
    """The writer as it was before normals and colours: float x, y, z and the face lists, nothing else."""
    v = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
    rec = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    rec["n"], rec["i"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def _read_ply(path):
    """(property names of the vertex element, vertex records, faces) of a binary little-endian PLY written by ``write_ply``."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = n_f = None
    props, elem = [], None
    for ln in lines[2:]:
        w = ln.split()
        if not w:
            continue
        if w[0] == "element":
            elem = w[1]
            if elem == "vertex":
                n_v = int(w[2])
            else:
                n_f = int(w[2])
        elif w[0] == "property" and elem == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        elif w[0] == "property":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    vd = np.dtype(props)
    v = np.frombuffer(raw, dtype=vd, count=n_v, offset=end)
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=n_f, offset=end + n_v * vd.itemsize)
    assert (rec["n"] == 3).all()
    assert end + n_v * vd.itemsize + n_f * rec.dtype.itemsize == len(raw)
    return [p for p, _ in props], v, rec["i"]


def _mesh():
    f, lo, h = I.sphere_field(14)
    return I.extract(f, 0.0, lo, h)


def test_write_ply_without_the_new_fields_is_byte_identical(tmp_path):
    from supnerf_amd import geometry as G
    verts, faces = _mesh()
    for v, fa in ((verts, faces), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        a, b = tmp_path / "new.ply", tmp_path / "old.ply"
        G.write_ply(str(a), torch.from_numpy(v), torch.from_numpy(fa))
        _write_ply_before(str(b), torch.from_numpy(v), torch.from_numpy(fa))
        assert a.read_bytes() == b.read_bytes()


def test_write_ply_normals_and_colors_round_trip(tmp_path):
    from supnerf_amd import geometry as G
    verts, faces = _mesh()
    V = verts.shape[0]
    g = np.random.default_rng(5)
    normals = g.standard_normal((V, 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    colors = g.uniform(-0.5, 1.5, (V, 3)).astype(np.float32)          # a third of them outside [0, 1]: clamped
    colors[:4] = np.array([[0.0, 1.0, 0.5], [0.5 / 255, 1.5 / 255, 254.5 / 255], [np.nan, -0.0, 2.0], [1 / 255, 127 / 255, 0.999]],
                          np.float32)
    want_q = np.rint(np.clip(np.nan_to_num(colors.astype(np.float64), nan=0.0), 0, 1) * 255).astype(np.uint8)
    assert want_q[0].tolist() == [0, 255, 128] and want_q[2].tolist() == [0, 0, 255]
    p = tmp_path / "full.ply"
    G.write_ply(str(p), torch.from_numpy(verts), torch.from_numpy(faces), normals=torch.from_numpy(normals), colors=torch.from_numpy(colors))
    names, v, f = _read_ply(str(p))
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), verts)
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), normals)
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), want_q)
    assert np.array_equal(f, faces)
    assert np.array_equal(G.quantize_colors(torch.from_numpy(colors)), want_q)
    # the header's property order
    head = p.read_bytes().split(b"end_header\n")[0].decode()
    assert head.index("property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n"
                      "property uchar green\nproperty uchar blue\nelement face") > 0
    # either one alone
    G.write_ply(str(p), verts, faces, normals=normals)
    names, v, _ = _read_ply(str(p))
    assert names == ["x", "y", "z", "nx", "ny", "nz"] and np.array_equal(v["nz"], normals[:, 2])
    G.write_ply(str(p), verts, faces, colors=colors)
    names, v, _ = _read_ply(str(p))
    assert names == ["x", "y", "z", "red", "green", "blue"] and np.array_equal(v["green"], want_q[:, 1])
    # an empty mesh with the extra fields
    G.write_ply(str(p), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), normals=np.zeros((0, 3)), colors=np.zeros((0, 3)))
    names, v, f = _read_ply(str(p))
    assert len(names) == 9 and v.shape == (0,) and f.shape == (0, 3)
    import supnerf_amd as A
    with pytest.raises(A.SnrError):
        G.write_ply(str(p), verts, faces, normals=normals[:-1])
    with pytest.raises(A.SnrError):
        G.write_ply(str(p), verts, faces, colors=colors[:, :2])


def test_new_entry_points_refuse_cpu_tensors_and_malformed_shapes():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    from supnerf_amd import ops
    model = A.CodeNeRF(shape_blocks=1, texture_blocks=1)
    xyz, sc = torch.zeros(8, 3), torch.zeros(2, 256)
    mesh = [(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))]
    calls = [
        lambda: G.density(model, xyz, sc),                               # CPU tensors
        lambda: G.density(model, torch.zeros(8, 2), sc),                 # malformed shapes ...
        lambda: G.density(model, xyz, torch.zeros(2, 255)),
        lambda: G.density(torch.nn.Linear(3, 1), xyz, sc),               # not a supnerf_amd decoder
        lambda: G.density_gradient(model, xyz, sc),
        lambda: G.density_gradient(model, torch.zeros(7, 3), sc),
        lambda: G.density_gradient(model, xyz, torch.zeros(3, 2, 256)),
        lambda: G.vertex_normals(model, mesh, sc[:1]),
        lambda: G.vertex_normals(model, mesh[0], sc[:1]),                # one pair instead of the list
        lambda: G.vertex_normals(model, [(torch.zeros(3, 2), torch.zeros(1, 3))], sc[:1]),
        lambda: G.vertex_colors(model, mesh, [torch.zeros(3, 3)], sc[:1], sc[:1]),
        lambda: G.vertex_colors(model, mesh, [], sc[:1], sc[:1]),
        lambda: ops.density_fwd(xyz, torch.zeros(2, 2, 256), None, 1, 1),
        lambda: ops.density_fwd(torch.zeros(8, 4), torch.zeros(2, 2, 256), None, 1, 1),
        lambda: ops.density_fwd(xyz, torch.zeros(3, 2, 256), None, 1, 1),   # 8 points over 3 objects
        lambda: ops.density_fwd(xyz, torch.zeros(2, 3, 256), None, 1, 1),   # NLAT = 2
        lambda: ops.density_bwd(xyz, torch.zeros(2, 2, 256), None, torch.zeros(16, dtype=torch.uint8), torch.zeros(8), torch.zeros(8), 1, 1),
        lambda: ops.density_bwd(xyz, torch.zeros(2, 2, 256), None, None, torch.zeros(8), torch.zeros(8), 1, 1),
        lambda: ops.density_bwd(xyz, torch.zeros(2, 2, 256), None, torch.zeros(16, dtype=torch.uint8), torch.zeros(7), torch.zeros(8), 1, 1),
        lambda: ops.DensityPoints.apply(xyz, torch.zeros(2, 2, 256), torch.zeros(4), 1, 1),
        lambda: ops.DensityPoints.apply(torch.zeros(8, 3, 1), torch.zeros(2, 2, 256), torch.zeros(4), 1, 1),
    ]
    for call in calls:
        with pytest.raises(A.SnrError):
            call()


def test_density_refuses_to_drop_the_weight_gradients():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    model = A.CodeNeRF(shape_blocks=1, texture_blocks=1)
    model.train_decoder_weights = True
    with pytest.raises(A.SnrError, match="train_decoder_weights"):
        G.density(model, torch.zeros(8, 3), torch.zeros(2, 256))


def test_to_object_frame_direction_is_the_frame_without_scale():
    from supnerf_amd import geometry as G
    from supnerf_amd import utils as U
    g = torch.Generator().manual_seed(4)
    n = torch.nn.functional.normalize(torch.randn(40, 3, generator=g, dtype=torch.float64), dim=1)
    for kitti, shapenet in ((False, False), (True, False), (False, True), (True, True)):
        m = torch.tensor(U._frame(False, kitti, shapenet), dtype=torch.float64).view(3, 3)
        assert torch.allclose(m @ m.T, torch.eye(3, dtype=torch.float64), rtol=0, atol=0)      # orthonormal (a signed permutation)
        for fam, diag in (("a", 2.5), ("b", 7.0)):
            got = G.to_object_frame(n, diag, fam, shapenet, kitti, direction=True)
            assert torch.equal(got, n @ m)
            assert torch.allclose(got.norm(dim=1), torch.ones(40, dtype=torch.float64), rtol=0, atol=1e-15)
            # a direction maps like the difference of two mapped points, divided by the scale
            p, q = torch.randn(40, 3, generator=g, dtype=torch.float64), torch.randn(40, 3, generator=g, dtype=torch.float64)
            dp = G.to_object_frame(p, diag, fam, shapenet, kitti) - G.to_object_frame(q, diag, fam, shapenet, kitti)
            scale = diag if fam == "a" else diag / 2
            assert torch.allclose(dp / scale, G.to_object_frame(p - q, diag, fam, shapenet, kitti, direction=True), rtol=1e-13, atol=1e-13)
