"""supnerf_amd.geometry on the MI355X: the density-only decoder kernels against the full fp32 forward (bit for bit) and the float64 oracle,
the lattice kernel against the list kernel, the iso-surface kernels against tests/iso_restatement.py (bit for bit), an end-to-end mesh of
the planted box decoder, and ``to_object_frame`` against the package's own point mappings."""
import numpy as np
import pytest
import torch

import iso_restatement as I
from geometry_cases import BOUND_BOX, LEVEL_BOX, box, codes as _codes, model as _model
from oracle import supnerf_oracle as O
from oracle_bands import amd, dev, in_band  # noqa: F401  (fixtures)
from planted_decoder import HALF, H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("blocks", [(0, 0), (0, 3), (3, 1), (5, 5), (8, 8)])
def test_list_kernel_is_the_fp32_forward_sigma(amd, dev, blocks):  # noqa: F811
    from supnerf_amd import geometry as G
    sb, tb = blocks
    model = _model(amd, dev, sb, tb, seed=sb * 10 + tb)
    params64 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    for B in (1, 3):
        sc = _codes(B, 7 + B, dev)
        for ppo in (1, 33, 1000):
            g = torch.Generator().manual_seed(100 * B + ppo)
            xyz = (torch.rand(B * ppo, 3, generator=g) - 0.5).to(dev)
            sig = G.query_density(model, xyz, sc)
            lat = model.latent_terms(sc, torch.zeros_like(sc)).detach()
            vd = torch.nn.functional.normalize(torch.randn(B * ppo, 3, generator=g), dim=1).to(dev)
            ref, _, _ = amd.ops.decoder_fwd(xyz, vd, lat, model.packed_weights(), sb, tb, precision="fp32")
            assert sig.shape == (B * ppo,)
            assert torch.equal(sig, ref), (blocks, B, ppo, float((sig - ref).abs().max()))
            # ... and within the fp32 band of the float64 oracle (the density does not depend on the view direction)
            x3 = xyz.cpu().view(B * ppo, 1, 3)
            d3 = vd.cpu().view(B * ppo, 1, 3)
            zt = torch.zeros(B, 256)
            o64 = O.decoder_forward(params64, x3.double(), d3.double(), sc.cpu().double(), zt.double())[0].view(-1)
            o32 = O.decoder_forward({k: v.float() for k, v in params64.items()}, x3, d3, sc.cpu(), zt)[0].view(-1)
            ok, _, msg = in_band(sig, o32, o64, "fp32", f"sigma {blocks} B={B} ppo={ppo}")
            assert ok, msg


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (17, 17, 17), (64, 64, 64)])
def test_grid_kernel_is_the_list_kernel_on_the_lattice(amd, dev, shape):  # noqa: F811
    from supnerf_amd import geometry as G
    model = _model(amd, dev, 3, 1, seed=5)
    sc = _codes(2, 11, dev)
    bound = ((-0.6, -0.25, -0.4), (0.5, 0.35, 0.45))
    grid = G.density_grid(model, sc, shape, bound)
    assert grid.shape == (2,) + shape
    pts = G.lattice_points(G.lattice(shape, bound), dev)
    lst = G.query_density(model, pts.repeat(2, 1), sc)
    assert torch.equal(grid.reshape(-1), lst)
    assert bool(torch.isfinite(grid).all())


def _iso_gpu(G, fields, level, bound, dev):  # noqa: F811
    grid = torch.from_numpy(np.stack(fields)).to(dev)
    return G.extract_mesh(grid, level=level, bound=bound)


def _fields():
    n = 40
    return {"sphere": I.sphere_field(n)[0], "torus": I.torus_field(n)[0], "noise": I.noise_field(n, seed=4)[0],
            "constant": np.full((n, n, n), 0.25, np.float32), "level_equal": I.level_equal_field(n)[0]}


def test_iso_kernels_are_the_restatement(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    bound = (-0.5, 0.5)
    fields = _fields()
    lat = G.lattice(40, bound)
    lo, h = np.array(list(lat.lo), np.float32), np.array(list(lat.h), np.float32)
    want = {k: I.extract(f, 0.0, lo, h) for k, f in fields.items()}
    for k, f in fields.items():                                      # one object per launch
        (v, fa), = _iso_gpu(G, [f], 0.0, bound, dev)
        assert v.dtype == torch.float32 and fa.dtype == torch.int32
        assert np.array_equal(v.cpu().numpy(), want[k][0]), k
        assert np.array_equal(fa.cpu().numpy(), want[k][1]), k
    out = _iso_gpu(G, list(fields.values()), 0.0, bound, dev)           # all of them in one launch
    for (v, fa), k in zip(out, fields):
        assert np.array_equal(v.cpu().numpy(), want[k][0]), k
        assert np.array_equal(fa.cpu().numpy(), want[k][1]), k
    # an asymmetric lattice and a non-zero level
    f, _, _ = I.noise_field(24, seed=9)
    f = f[:, :17, 3:]
    b2 = ((-0.3, 0.1, -0.7), (0.6, 0.45, 0.2))
    lat2 = G.lattice(f.shape, b2)
    w = I.extract(f, np.float32(0.1), np.array(list(lat2.lo), np.float32), np.array(list(lat2.h), np.float32))
    (v, fa), = _iso_gpu(G, [f], 0.1, b2, dev)
    assert np.array_equal(v.cpu().numpy(), w[0]) and np.array_equal(fa.cpu().numpy(), w[1])
    # a larger sphere: closed, Euler characteristic 2, outward
    f, _, _ = I.sphere_field(128)
    (v, fa), = _iso_gpu(G, [f], 0.0, bound, dev)
    v, fa = v.cpu().numpy(), fa.cpu().numpy()
    cnt, oriented = I.edge_use(fa)
    assert (cnt == 2).all() and oriented and I.euler_characteristic(v, fa) == 2 and I.signed_volume(v, fa) > 0


def test_iso_rejects_non_finite_grids(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    f = torch.zeros(2, 8, 8, 8, device=dev)
    f[1, 3, 4, 5] = float("nan")
    with pytest.raises(amd.SnrError):
        G.extract_mesh(f, level=0.0)


@pytest.mark.parametrize("sb", [1, 3, 5])
def test_planted_box_mesh(amd, dev, sb):  # noqa: F811
    from supnerf_amd import geometry as G
    model = box(amd, dev, sb, 1, seed=sb)
    sc = _codes(2, 20 + sb, dev)
    res = 96
    meshes = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=res, bound=BOUND_BOX)
    hstep = 1.4 / (res - 1)
    assert len(meshes) == 2
    for v, fa in meshes:
        v64 = v.cpu().double()
        fa = fa.cpu().numpy()
        cnt, oriented = I.edge_use(fa)
        assert (cnt == 2).all() and oriented
        assert I.euler_characteristic(v64.numpy(), fa) == 2
        assert I.signed_volume(v64.numpy(), fa) > 0
        d1 = torch.relu(v64.abs() - torch.tensor(HALF, dtype=torch.float64)).sum(-1)
        assert float((d1 - H).abs().max()) <= 2 * hstep


def test_to_object_frame_inverts_the_encode_paths(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    from supnerf_amd import ops, utils as U
    g = torch.Generator().manual_seed(2)
    N, S = 64, 8
    rays_o = (torch.randn(N, 3, generator=g) * 2).to(dev)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=1).to(dev)
    obj_diag = 3.7
    # family A (utils render paths): x = F ((o + z d) / obj_diag), z shared by the rays
    z = torch.linspace(0.5, 4.0, S).to(dev)
    for kitti, shapenet in ((False, True), (True, False)):
        frame = U._frame(False, kitti, shapenet)
        cfg = ops.RenderCfg(S, ops.Z_SHARED, N, 0, 0, frame=frame)
        xyz, _, _ = ops.encode(rays_o, d, z, torch.full((1,), obj_diag, device=dev), None, cfg)
        want = (rays_o[:, None, :].double() + d[:, None, :].double() * z[None, :, None].double()).reshape(-1, 3)
        got = G.to_object_frame(xyz.reshape(-1, 3).double(), obj_diag, "a", shapenet_obj_cood=shapenet, kitti2nusc=kitti)
        assert float(((got - want).norm(dim=1) / want.norm(dim=1)).max()) < 1e-6
    # family B (NeRFRenderer): x = F (o / (diag / 2) + t d), depths per ray
    t = torch.rand(N, S, generator=g).to(dev) * 2
    frame = U._frame(False, True, False)
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, N, 0, 0, frame=frame, metric_z=True)
    o_n = rays_o / (obj_diag / 2)
    xyz, _, _ = ops.encode(o_n, d, t, torch.ones(1, device=dev), torch.full((1,), obj_diag / 2, device=dev), cfg)
    want = ((o_n[:, None, :].double() + t[:, :, None].double() * d[:, None, :].double()) * (obj_diag / 2)).reshape(-1, 3)
    got = G.to_object_frame(xyz.reshape(-1, 3).double(), obj_diag, "b", kitti2nusc=True)
    assert float(((got - want).norm(dim=1) / want.norm(dim=1)).max()) < 1e-6
