"""supnerf_amd.geometry on the host: the iso-surface rules (tests/iso_restatement.py) on analytic fields, the PLY writer, and the
argument checks that need no GPU."""
import math

import numpy as np
import pytest
import torch

import iso_restatement as I


def _closed(faces):
    cnt, oriented = I.edge_use(faces)
    return bool((cnt == 2).all()) and oriented


def test_sphere_is_a_closed_oriented_genus0_surface():
    r = 0.35
    f, lo, h = I.sphere_field(64, r=r)
    verts, faces = I.extract(f, 0.0, lo, h)
    assert verts.dtype == np.float32 and faces.dtype == np.int32
    assert faces.shape[0] > 1000
    assert _closed(faces)
    assert np.unique(faces).size == verts.shape[0]              # every vertex is used
    assert I.euler_characteristic(verts, faces) == 2
    vol = I.signed_volume(verts, faces)
    assert vol > 0                                               # counter-clockwise seen from outside: outward normals
    assert abs(vol - 4 / 3 * math.pi * r ** 3) < 0.01 * 4 / 3 * math.pi * r ** 3
    assert abs(I.area(verts, faces) - 4 * math.pi * r * r) < 0.01 * 4 * math.pi * r * r
    assert np.abs(np.linalg.norm(verts.astype(np.float64), axis=1) - r).max() < h.max()


def test_torus_has_euler_characteristic_zero():
    f, lo, h = I.torus_field(48)
    verts, faces = I.extract(f, 0.0, lo, h)
    assert _closed(faces)
    assert I.euler_characteristic(verts, faces) == 0
    assert I.signed_volume(verts, faces) > 0


def test_inverted_field_flips_the_winding():
    f, lo, h = I.sphere_field(24)
    v1, f1 = I.extract(f, 0.0, lo, h)
    v2, f2 = I.extract(-f, np.float32(-1e-30), lo, h)           # inside <-> outside (no sample sits at the level)
    assert _closed(f2) and I.signed_volume(v2, f2) < 0
    assert abs(I.signed_volume(v1, f1) + I.signed_volume(v2, f2)) < 1e-6


@pytest.mark.parametrize("value", [-1.0, 1.0, 0.0])
def test_empty_and_full_fields_have_no_faces(value):
    f = np.full((9, 7, 5), value, dtype=np.float32)
    verts, faces = I.extract(f, 0.0)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_samples_at_the_level_count_as_outside():
    f, lo, h = I.level_equal_field(20)
    assert (f == 0).mean() > 0.3
    verts, faces = I.extract(f, 0.0, lo, h)
    inside = f > 0
    # a vertex sits on an edge whose ends disagree under value > level; where the lower end is exactly at the level, t = 0: the vertex is
    # that grid point
    assert verts.shape[0] > 0 and faces.shape[0] > 0
    cnt, oriented = I.edge_use(faces)
    assert oriented and cnt.max() <= 2
    # the same field with the tied samples nudged below the level gives the same topology
    g = np.where(f == 0, np.float32(-1e-3), f)
    assert ((g > 0) == inside).all()
    v2, f2 = I.extract(g, 0.0, lo, h)
    assert np.array_equal(f2, faces) and v2.shape == verts.shape


def test_single_tetrahedron_cases():
    """A 2x2x2 grid (one cell) with every inside pattern of its 8 corners: at most 12 triangles, every triangle's vertices distinct,
    orientation consistent, and the complementary pattern gives the same faces reversed."""
    for code in range(256):
        f = np.array([[[(code >> (4 * i + 2 * j + k)) & 1 for k in range(2)] for j in range(2)] for i in range(2)], dtype=np.float32)
        # corner index in the field above is x*4 + y*2 + z; the kernels' corner bits are x=1, y=2, z=4 -- only the pattern matters here
        v, fa = I.extract(f - np.float32(0.5), 0.0)
        w, fb = I.extract(np.float32(0.5) - f, 0.0)
        assert fa.shape[0] <= 12
        assert np.array_equal(v, w)
        if fa.shape[0]:
            assert (fa[:, 0] != fa[:, 1]).all() and (fa[:, 1] != fa[:, 2]).all() and (fa[:, 0] != fa[:, 2]).all()
            assert I.edge_use(fa)[1]
            # the complement: same triangles, opposite orientation (as cyclic sequences)
            sa = {tuple(np.roll(t, -int(np.argmin(t)))) for t in fa.tolist()}
            sb = {tuple(np.roll(t[::-1], -int(np.argmin(t[::-1])))) for t in fb.tolist()}
            assert sa == sb, code


def test_write_ply_round_trip(tmp_path):
    from supnerf_amd import geometry as G
    f, lo, h = I.sphere_field(12)
    verts, faces = I.extract(f, 0.0, lo, h)
    p = tmp_path / "sphere.ply"
    G.write_ply(str(p), torch.from_numpy(verts), torch.from_numpy(faces))
    v2, f2 = I.read_ply(str(p))
    assert np.array_equal(v2, verts) and np.array_equal(f2, faces)
    G.write_ply(str(p), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v3, f3 = I.read_ply(str(p))
    assert v3.shape == (0, 3) and f3.shape == (0, 3)


def test_lattice_matches_the_restatement():
    from supnerf_amd import geometry as G
    lat = G.lattice((17, 5, 9), ((-0.5, -0.25, -1.0), (0.75, 0.3, 0.1)))
    lo, h, axes = I.lattice((17, 5, 9), (-0.5, -0.25, -1.0), (0.75, 0.3, 0.1))
    assert list(lat.n) == [17, 5, 9]
    assert np.array_equal(np.array(list(lat.lo), np.float32), lo) and np.array_equal(np.array(list(lat.h), np.float32), h)
    pts = G.lattice_points(lat).numpy()
    assert pts.shape == (17 * 5 * 9, 3)
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    assert np.array_equal(pts, np.stack([X, Y, Z], -1).reshape(-1, 3))
    one = G.lattice(1, (0.25, 0.75))
    assert list(one.h) == [0.0, 0.0, 0.0] and list(one.lo) == [0.25, 0.25, 0.25]


def test_argument_checks_without_a_gpu():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    with pytest.raises(A.SnrError):
        G.lattice(513)
    with pytest.raises(A.SnrError):
        G.lattice((4, 0, 4))
    with pytest.raises(A.SnrError):
        G.extract_mesh(torch.zeros(4, 4, 4), level=0.0)                 # a CPU grid: no CPU fallback
    with pytest.raises(A.SnrError):
        G.density_grid(torch.nn.Linear(3, 1), torch.zeros(1, 256), 8)    # not a supnerf_amd decoder
    model = A.CodeNeRF(shape_blocks=1, texture_blocks=1)
    with pytest.raises(A.SnrError):
        G.query_density(model, torch.zeros(4, 3), torch.zeros(1, 256))  # CPU tensors
    with pytest.raises(A.SnrError):
        G.to_object_frame(torch.zeros(2, 3), 1.0, family="c")


def test_to_object_frame_inverts_the_frame_on_the_host():
    from supnerf_amd import geometry as G
    from supnerf_amd import utils as U
    g = torch.Generator().manual_seed(3)
    p = torch.randn(50, 3, generator=g, dtype=torch.float64)
    for kitti, shapenet in ((False, False), (True, False), (False, True), (True, True)):
        m = torch.tensor(U._frame(False, kitti, shapenet), dtype=torch.float64).view(3, 3)
        x_a = (p / 2.5) @ m.T
        x_b = (p / 1.25) @ m.T
        assert torch.allclose(G.to_object_frame(x_a, 2.5, "a", shapenet, kitti), p, rtol=0, atol=1e-12)
        assert torch.allclose(G.to_object_frame(x_b, 2.5, "b", shapenet, kitti), p, rtol=0, atol=1e-12)
