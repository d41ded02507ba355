"""Differentiable mesh extraction on the MI355X: ``extract_mesh(..., differentiable=True)`` returns the meshes it returns without it,
``snr_iso_grad`` equals tests/iso_grad_restatement.py bit for bit, ``snr_iso_surface_points`` lists the lattice points the surface touches
(where the density forward returns the grid's values bit for bit), and the shape-code gradient of a loss on the vertices agrees with float64
autograd of the oracle decoder through the same edge list, with the grid path pushed through ``geometry.density``, and between dense and
narrow-band grids."""
import numpy as np
import pytest
import torch

import iso_grad_restatement as IG
import iso_restatement as IR
from geometry_cases import BOUND_BOX, LEVEL_BOX, box, codes as _codes, model as _model, same_meshes as _same_meshes
from oracle import supnerf_oracle as O
from oracle_bands import amd, dev, in_band  # noqa: F401  (fixtures)
from planted_decoder import WOBBLE
from relu_bits import decode_relu_bits

pytestmark = pytest.mark.gpu

def _box(amd, dev, sb=3, tb=1, seed=1):  # noqa: F811
    return box(amd, dev, sb, tb, seed, wobble=WOBBLE)


def _weights(meshes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(v.shape, generator=g).to(v.device) for v, _ in meshes]


def _loss(meshes, w):
    return sum((v * wb).sum() for (v, _), wb in zip(meshes, w))


def test_differentiable_meshes_are_the_meshes(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    f = np.stack([IR.sphere_field(33)[0], IR.torus_field(33)[0]])
    grid = torch.from_numpy(f).to(dev).requires_grad_()
    plain = G.extract_mesh(grid, level=0.0)
    diff = G.extract_mesh(grid, level=0.0, differentiable=True)
    assert _same_meshes(plain, diff)
    assert all(v.grad_fn is not None and v.requires_grad for v, _ in diff)
    assert all(v.grad_fn is None for v, _ in plain)
    one = G.extract_mesh(grid[1], level=0.0, differentiable=True)               # (nx, ny, nz): a view of the leaf, still differentiable
    assert _same_meshes(one, plain[1:]) and one[0][0].grad_fn is not None
    model = _box(amd, dev)
    sc = _codes(3, 5, dev).requires_grad_()
    for nb in (False, True):
        plain = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=72, bound=BOUND_BOX, narrow_band=nb)
        diff = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=72, bound=BOUND_BOX, narrow_band=nb, differentiable=True)
        assert _same_meshes(plain, diff), nb
        assert all(f.shape[0] > 0 for _, f in diff)
        assert all(v.grad_fn is not None for v, _ in diff) and all(v.grad_fn is None for v, _ in plain)
        with torch.no_grad():
            assert _same_meshes(G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=72, bound=BOUND_BOX, narrow_band=nb,
                                               differentiable=True), plain)


def _grad_of(amd, grid, lat, level, seed):  # noqa: F811
    """iso_extract + a random d_verts + iso_grad (with the surface flags) on the device."""
    ops = amd.ops
    m = ops.iso_extract(grid, lat, level)
    g = torch.randn(m.verts.shape, generator=torch.Generator().manual_seed(seed)).to(grid.device)
    d_grid, on = ops.iso_grad(grid, lat, level, m.edge_mask, m.edge_scan, m.vert_offset, g, want_surface=True)
    return m, g, d_grid, on


def test_iso_grad_is_the_restatement(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    ops = amd.ops
    cases = [(np.stack([IR.sphere_field(40)[0], IR.torus_field(40)[0], IR.noise_field(40, seed=2)[0]]), 0.0, (-0.5, 0.5)),
             (IR.noise_field(37, seed=9)[0][None], 0.1, (-0.5, 0.5)),
             (IR.level_equal_field(20)[0][None], 0.0, (-0.5, 0.5))]
    fog = _model(amd, dev, 3, 1, seed=0)
    dg = G.density_grid(fog, _codes(2, 3, dev), (45, 38, 29), ((-0.6, -0.5, -0.4), (0.5, 0.45, 0.55)))
    # (cut at object 0's median: the fog's density differs a little per code, so object 1 may lie wholly on one side)
    cases.append((dg.cpu().numpy(), float(dg[0].median()), ((-0.6, -0.5, -0.4), (0.5, 0.45, 0.55))))
    for k, (f, level, bound) in enumerate(cases):
        level = float(np.float32(level))
        grid = torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).to(dev)
        lat = G.lattice(tuple(f.shape[1:]), bound)
        h = np.array(list(lat.h), dtype=np.float32)
        m, g, d_grid, on = _grad_of(amd, grid, lat, level, 100 + k)
        assert m.verts.shape[0] > 0
        again, _ = ops.iso_grad(grid, lat, level, m.edge_mask, m.edge_scan, m.vert_offset, g)
        assert torch.equal(again, d_grid)                                           # deterministic: no atomics
        gc, v0 = g.cpu().numpy(), 0
        for b in range(f.shape[0]):
            n = m.n_verts[b]
            want, won = IG.grid_grad(f[b], level, h, gc[v0:v0 + n])
            v0 += n
            got = d_grid[b].cpu().numpy()
            assert np.array_equal(got, want), (k, b, float(np.abs(got - want).max()))
            assert np.array_equal(on[b].cpu().numpy().reshape(f.shape[1:]), won), (k, b)
            assert (got[won == 0] == 0).all() and not np.signbit(got[won == 0]).any()
        # the autograd Function's backward is the same launch
        gr = grid.clone().requires_grad_()
        verts, _, _ = ops.IsoVertices.apply(gr, lat, level)
        assert torch.equal(verts, m.verts)
        (verts * g).sum().backward()
        assert torch.equal(gr.grad, d_grid), k


def test_surface_points_are_the_lattice_points(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    ops = amd.ops
    model = _box(amd, dev, 3, 1, seed=3)
    sc = _codes(3, 8, dev)
    R = 61
    lat = G.lattice(R, BOUND_BOX)
    lo, h = np.array(list(lat.lo), dtype=np.float32), np.array(list(lat.h), dtype=np.float32)
    dense = G.density_grid(model, sc, R, BOUND_BOX)
    nbg = G.narrow_band_grid(model, sc, R, level=LEVEL_BOX, bound=BOUND_BOX)
    for name, grid in (("dense", dense), ("narrow", nbg.grid)):
        m, _, d_grid, on = _grad_of(amd, grid, lat, LEVEL_BOX, 7)
        xyz, d_sig, n, counts = ops.iso_surface_points(on, d_grid, lat)
        wx, wd, wn, wc = IG.surface_points(on.cpu().numpy().reshape(grid.shape), d_grid.cpu().numpy(), lo, h)
        assert n == wn and n % 64 == 0 and np.array_equal(counts.cpu().numpy(), wc), name
        assert np.array_equal(xyz.cpu().numpy(), wx) and np.array_equal(d_sig.cpu().numpy(), wd), name
        pts = G.lattice_points(lat)
        sig = G.query_density(model, xyz, sc).view(3, n)
        for b in range(3):
            c = int(counts[b])
            idx = torch.nonzero(on[b]).flatten()
            assert c == idx.numel() > 0
            assert torch.equal(xyz[b * n:b * n + c].cpu(), pts[idx.cpu()]), (name, b)
            assert torch.equal(sig[b, :c], dense[b].reshape(-1)[idx]), (name, b)            # the decoder's value at the point
            assert torch.equal(sig[b, :c], grid[b].reshape(-1)[idx]), (name, b)             # ... which the grid holds
    assert torch.equal(G.extract_mesh(nbg.grid, level=LEVEL_BOX, bound=BOUND_BOX)[0][0],
                       G.extract_mesh(dense, level=LEVEL_BOX, bound=BOUND_BOX)[0][0])


def _oracle_code_grad(amd, model, sc_b, grid_b, lat, level, w_b, dtype):  # noqa: F811
    """d sum(w . verts) / d shapecode of one object in ``dtype`` on the CPU: the oracle decoder at the ends of the fp32 mesh's crossing
    edges, mask-matched on the kernel's ReLU bits, through the vertex formula.  The formula is evaluated at the grid's sigma (the values
    the mesh was made from) with the oracle's derivative: an edge nearly tangent to the surface has va ~ vb, and 1 / (vb - va)^2 would
    turn any other rounding of sigma into an error of its own -- the derivative is what is checked here, at the forward's values."""
    from supnerf_amd import geometry as G
    ops = amd.ops
    sb, tb = model.shape_blocks, model.texture_blocks
    u, d = IG.vertex_edges(grid_b.cpu().numpy(), level)
    n1, n2 = lat.n[1], lat.n[2]
    ends = np.unique(np.concatenate([u, u + IG._offset(np.array(IR.DIR_BITS)[d], n1, n2)]))
    xyz = G.lattice_points(lat)[torch.as_tensor(ends)]
    P = xyz.shape[0]
    xd = xyz.to(sc_b.device)
    lat_t = model.latent_terms(sc_b.detach(), torch.zeros_like(sc_b)).detach()
    _, masks = ops.density_fwd(xd, lat_t, model.packed_weights(), sb, tb, save_masks=True)
    vd = torch.nn.functional.normalize(torch.ones(P, 3, device=sc_b.device), dim=1)
    _, _, mf = ops.decoder_fwd(xd, vd, lat_t, model.packed_weights(), sb, tb, save_masks=True, precision="fp32")
    bd, bf = decode_relu_bits(masks, P, sb, tb), decode_relu_bits(mf, P, sb, tb)
    layers = [m.to(dtype) for m in bd[:sb + 1] + bf[sb + 1:]]
    params = {k: v.detach().cpu().to(dtype) for k, v in model.state_dict().items()}
    s = sc_b.detach().cpu().to(dtype).requires_grad_()
    x = xyz.to(dtype).view(-1, 1, 3)
    with O.given_relu_masks(layers):
        sig, _ = O.decoder_forward(params, x, torch.zeros_like(x), s, torch.zeros_like(s))
    sig = sig.view(-1)
    sig = grid_b.reshape(-1)[torch.as_tensor(ends).to(grid_b.device)].cpu().to(dtype) + (sig - sig.detach())
    full = torch.zeros(lat.n[0] * n1 * n2, dtype=dtype)
    full = full.index_put((torch.as_tensor(ends),), sig)
    v = IG.vertices64(full.view(lat.n[0], n1, n2), u, d, level, list(lat.lo), list(lat.h))
    (v * w_b.detach().cpu().to(dtype)).sum().backward()
    return s.grad.view(-1)


@pytest.mark.parametrize("blocks", [(3, 1), (1, 1)])
@pytest.mark.parametrize("B", [1, 3])
def test_shape_code_gradient_against_float64(amd, dev, blocks, B):  # noqa: F811
    from supnerf_amd import geometry as G
    sb, tb = blocks
    model = _box(amd, dev, sb, tb, seed=10 + sb)
    sc0 = _codes(B, 20 + B, dev)
    R = 40
    lat = G.lattice(R, BOUND_BOX)
    grads = {}
    for nb in (False, True):
        sc = sc0.clone().requires_grad_()
        meshes = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=R, bound=BOUND_BOX, narrow_band=nb, differentiable=True)
        w = _weights(meshes, 3)
        _loss(meshes, w).backward()
        grads[nb] = sc.grad.clone()
        assert float(sc.grad.abs().max()) > 0
    # the narrow band at its fixpoint: the same mesh, the same surface points, the same values: the same gradient, bit for bit
    assert torch.equal(grads[False], grads[True])
    dense = G.density_grid(model, sc0, R, BOUND_BOX)
    for b in range(B):
        o64 = _oracle_code_grad(amd, model, sc0[b:b + 1], dense[b], lat, LEVEL_BOX, w[b], torch.float64)
        o32 = _oracle_code_grad(amd, model, sc0[b:b + 1], dense[b], lat, LEVEL_BOX, w[b], torch.float32)
        ok, _, msg = in_band(grads[False][b], o32, o64, "fp32", f"d_shapecode {blocks} B={B} obj {b}")
        print(msg)
        assert ok, msg


def test_model_path_is_the_grid_path_through_density(amd, dev):  # noqa: F811
    """The same loss to the shape codes two ways: the model path (decoder at the surface points only) and the grid path (grid gradient
    at every lattice point pushed through geometry.density): equal within fp32 summation."""
    from supnerf_amd import geometry as G
    model = _box(amd, dev, 3, 1, seed=4)
    B, R = 2, 24
    sc0 = _codes(B, 31, dev)
    lat = G.lattice(R, BOUND_BOX)
    sc = sc0.clone().requires_grad_()
    meshes = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=R, bound=BOUND_BOX, differentiable=True)
    w = _weights(meshes, 5)
    _loss(meshes, w).backward()
    sc2 = sc0.clone().requires_grad_()
    pts = G.lattice_points(lat, dev).repeat(B, 1)
    grid = G.density(model, pts, sc2).view(B, R, R, R)
    assert torch.equal(grid.detach(), G.density_grid(model, sc0, R, BOUND_BOX))
    meshes2 = G.extract_mesh(grid, level=LEVEL_BOX, bound=BOUND_BOX, differentiable=True)
    assert _same_meshes(meshes, meshes2)
    _loss(meshes2, w).backward()
    err = float((sc.grad - sc2.grad).abs().max()) / float(sc2.grad.abs().max())
    print(f"model path vs grid path: rel {err:.2e}")
    assert float(sc2.grad.abs().max()) > 0 and err < 1e-4


def test_edge_cases(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    # no surface: empty vertices, a zero gradient
    grid = torch.full((2, 9, 9, 9), -1.0, device=dev, requires_grad=True)
    meshes = G.extract_mesh(grid, level=0.0, differentiable=True)
    assert all(v.shape == (0, 3) and f.shape == (0, 3) for v, f in meshes)
    sum(v.sum() for v, _ in meshes).backward()
    assert grid.grad is not None and bool((grid.grad == 0).all())
    model = _box(amd, dev, 3, 1, seed=6)
    sc = _codes(2, 7, dev).requires_grad_()
    meshes = G.extract_mesh(model, sc, level=1e6, resolution=24, bound=BOUND_BOX, differentiable=True)
    assert all(v.shape == (0, 3) for v, _ in meshes)
    sum(v.sum() for v, _ in meshes).backward()
    assert sc.grad is not None and bool((sc.grad == 0).all())
    # a surface in one object only
    f = torch.full((2, 12, 12, 12), -1.0, device=dev)
    f[1] = torch.from_numpy(IR.sphere_field(12)[0]).to(dev)
    f.requires_grad_()
    meshes = G.extract_mesh(f, level=0.0, differentiable=True)
    assert meshes[0][0].shape[0] == 0 and meshes[1][0].shape[0] > 0
    (meshes[1][0] ** 2).sum().backward()
    assert bool((f.grad[0] == 0).all()) and float(f.grad[1].abs().max()) > 0
    # a non-finite grid raises as before
    bad = torch.from_numpy(IR.sphere_field(10)[0]).to(dev)
    bad[3, 4, 5] = float("nan")
    with pytest.raises(amd.SnrError):
        G.extract_mesh(bad.requires_grad_(), level=0.0, differentiable=True)
    # the weight-training guard
    model.train_decoder_weights = True
    with pytest.raises(amd.SnrError):
        G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=24, bound=BOUND_BOX, differentiable=True)
    with torch.no_grad():
        assert _same_meshes(G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=24, bound=BOUND_BOX, differentiable=True),
                            G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=24, bound=BOUND_BOX))
