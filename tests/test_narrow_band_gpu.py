"""Narrow-band grids on the MI355X: the brick mode of the density decoder against the lattice kernel (bit for bit), the coarse pass against
the fine grid, the band kernels against tests/band_restatement.py, and narrow-band meshes against dense ones (planted box on cubic lattices and
on (61, 40, 23) with and without a band, growth from one brick, the fog decoder cut at its median).  The band kernels alone, on analytic
fields: tests/test_band_kernels_gpu.py."""
import numpy as np
import pytest
import torch

import band_restatement as NB
from geometry_cases import BOUND_BOX, LEVEL_BOX, box, codes as _codes, latent, model as _model, same_meshes as _same_meshes
from oracle_bands import amd, dev  # noqa: F401  (fixtures)
from planted_decoder import FAR_PRE, WOBBLE, planted_params

pytestmark = pytest.mark.gpu

def _on_lattice(amd, model, sc, lat):  # noqa: F811
    """snr_density_grid on an arbitrary Lattice."""
    return amd.ops.density_grid(lat, latent(model, sc), model.packed_weights(), model.shape_blocks, model.texture_blocks)


def _bricks(amd, model, sc, lat, bricks):  # noqa: F811
    """snr_density_bricks of the (n, 4) int32 list into a NaN-filled grid."""
    out = torch.full((sc.shape[0], *lat.n), float("nan"), device=sc.device)
    bl = torch.as_tensor(bricks, dtype=torch.int32).reshape(-1, 4).to(sc.device).contiguous()
    return amd.ops.density_bricks(lat, bl, bl.shape[0], latent(model, sc), model.packed_weights(), model.shape_blocks, model.texture_blocks,
                                  out)


def _listed_points(shape, B, bricks):
    """(B, n0, n1, n2) bool: the grid points of the listed bricks whose object and coordinates are in range."""
    nb = NB.n_bricks(shape)
    m = np.zeros((B,) + nb, dtype=bool)
    for b, i, j, k in bricks:
        if 0 <= b < B and 0 <= i < nb[0] and 0 <= j < nb[1] and 0 <= k < nb[2]:
            m[b, i, j, k] = True
    pb = NB.point_bricks(shape)
    return np.stack([m[b].reshape(-1)[pb] for b in range(B)])


@pytest.mark.parametrize("blocks", [(0, 0), (3, 1), (5, 5), (8, 8)])
def test_brick_mode_is_the_lattice_kernel(amd, dev, blocks):  # noqa: F811
    from supnerf_amd import geometry as G
    sb, tb = blocks
    model = _model(amd, dev, sb, tb, seed=sb * 10 + tb + 1)
    rng = np.random.default_rng(sb * 10 + tb)
    for shape in ((8, 8, 8), (17, 17, 17), (61, 40, 23), (128, 128, 128)):
        lat = G.lattice(shape, ((-0.6, -0.25, -0.4), (0.5, 0.35, 0.45)))
        nb = NB.n_bricks(shape)
        for B in (1, 3):
            sc = _codes(B, 3 + B, dev)
            ref = _on_lattice(amd, model, sc, lat)
            bricks = []
            for b in range(B):
                if B == 3 and b == 1:
                    continue                                                   # an object with no brick
                all_b = [(b, i, j, k) for i in range(nb[0]) for j in range(nb[1]) for k in range(nb[2])]
                take = rng.choice(len(all_b), size=max(1, int(rng.integers(1, len(all_b) + 1)) // (1 + b)), replace=False)
                bricks += [all_b[t] for t in take]                             # ragged: a different number per object
            rng.shuffle(bricks)
            bricks += [(B, 0, 0, 0), (0, nb[0], 0, 0), (0, 0, -1, 0), (-1, 0, 0, 0)]          # out of range: skipped
            got = _bricks(amd, model, sc, lat, bricks)
            listed = torch.from_numpy(_listed_points(shape, B, bricks)).to(dev)
            assert bool(listed.any())
            assert torch.equal(got[listed], ref[listed]), (blocks, shape, B)
            assert bool(torch.isnan(got[~listed]).all()), (blocks, shape, B)


def test_coarse_grid_is_the_fine_grid_at_coarse_points(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    model = _model(amd, dev, 3, 1, seed=4)
    sc = _codes(2, 5, dev)
    for shape, bound in (((64, 64, 64), (-0.5, 0.5)), ((61, 40, 23), ((-0.6, -0.25, -0.4), (0.5, 0.35, 0.45))), ((129, 17, 9), (-0.7, 0.7))):
        lat = G.lattice(shape, bound)
        fine = G.density_grid(model, sc, shape, bound)
        coarse = _on_lattice(amd, model, sc, G.coarse_lattice(lat))
        inner = coarse[:, :(shape[0] - 1) // 8 + 1, :(shape[1] - 1) // 8 + 1, :(shape[2] - 1) // 8 + 1]
        assert torch.equal(inner, fine[:, ::8, ::8, ::8]), shape


def _restated(amd, model, sc, R, bound, level, band=0.0, initial=None):  # noqa: F811
    """The restatement run per object on the dense grid and the coarse grid copied to the host: (grid, active, rounds, points) of the
    batch (rounds: the most any object needs -- the objects grow in the same rounds)."""
    from supnerf_amd import geometry as G
    lat = G.lattice(R, bound)
    dense = G.density_grid(model, sc, R, bound).cpu().numpy()
    coarse = _on_lattice(amd, model, sc, G.coarse_lattice(lat)).cpu().numpy()
    out = [NB.narrow_band(dense[b], coarse[b], level, band, None if initial is None else initial[b]) for b in range(sc.shape[0])]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), max(o[2] for o in out), sum(o[3] for o in out))


@pytest.mark.parametrize("sb", [1, 3, 5])
@pytest.mark.parametrize("far", [False, True])
def test_planted_box_narrow_band_mesh_is_the_dense_mesh(amd, dev, sb, far):  # noqa: F811
    from supnerf_amd import geometry as G
    model = box(amd, dev, sb, 1, seed=sb, far_pre=FAR_PRE if far else None, wobble=WOBBLE)
    sc = _codes(3, 40 + sb, dev)
    for R in (64, 129, 200):
        nbg = G.narrow_band_grid(model, sc, R, level=LEVEL_BOX, bound=BOUND_BOX)
        dense = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=R, bound=BOUND_BOX)
        narrow = G.extract_mesh(nbg.grid, level=LEVEL_BOX, bound=BOUND_BOX)
        assert all(f.shape[0] > 0 for _, f in dense)
        assert _same_meshes(narrow, dense), (sb, far, R)
        assert _same_meshes(G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=R, bound=BOUND_BOX, narrow_band=True), dense)
        g, active, rounds, points = _restated(amd, model, sc, R, BOUND_BOX, LEVEL_BOX)
        assert np.array_equal(nbg.active.cpu().numpy(), active), (sb, far, R)
        assert nbg.rounds == rounds and nbg.points == points, (sb, far, R, nbg.rounds, rounds, nbg.points, points)
        assert np.array_equal(nbg.grid.cpu().numpy(), g, equal_nan=True)
        assert nbg.points < 3 * R ** 3                                      # the work the dense grid does
        if R >= 129:
            assert nbg.points < 3 * R ** 3 // 2


def test_planted_box_off_the_cube_and_with_a_band(amd, dev):  # noqa: F811
    """The decoder path on a lattice whose brick counts differ per axis (8, 5, 3), at band 0 and at a band read from the coarse grid itself:
    the median |corner - level|, so that half the corners lie within it and one lies exactly on it."""
    from supnerf_amd import geometry as G
    sb, R = 3, (61, 40, 23)
    model = box(amd, dev, sb, 1, seed=sb, wobble=WOBBLE)
    sc = _codes(3, 43, dev)
    dense = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=R, bound=BOUND_BOX)
    assert all(f.shape[0] > 0 for _, f in dense)
    coarse = _on_lattice(amd, model, sc, G.coarse_lattice(G.lattice(R, BOUND_BOX)))
    band = float((coarse - np.float32(LEVEL_BOX)).abs().median())
    assert band > 0
    actives = []
    for b in (0.0, band):
        nbg = G.narrow_band_grid(model, sc, R, level=LEVEL_BOX, band=b, bound=BOUND_BOX)
        assert tuple(nbg.grid.shape) == (3,) + R and tuple(nbg.active.shape) == (3,) + NB.n_bricks(R)
        assert _same_meshes(G.extract_mesh(nbg.grid, level=LEVEL_BOX, bound=BOUND_BOX), dense), b
        g, active, rounds, points = _restated(amd, model, sc, R, BOUND_BOX, LEVEL_BOX, band=b)
        assert np.array_equal(nbg.active.cpu().numpy(), active), b
        assert nbg.rounds == rounds and nbg.points == points, (b, nbg.rounds, rounds, nbg.points, points)
        assert np.array_equal(nbg.grid.cpu().numpy().view(np.uint32), g.view(np.uint32)), b
        actives.append(active)
    assert (actives[1] & ~actives[0]).any()                                               # the band adds bricks
    assert _same_meshes(G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=R, bound=BOUND_BOX, narrow_band=True, band=band), dense)


def test_growth_from_one_brick_reaches_the_whole_box(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    sb = 3
    model = box(amd, dev, sb, 1, seed=7, wobble=WOBBLE)
    sc = _codes(2, 9, dev)
    R = 96
    full = G.narrow_band_grid(model, sc, R, level=LEVEL_BOX, bound=BOUND_BOX)
    seed = torch.zeros_like(full.active)
    for b in range(2):
        idx = torch.nonzero(full.active[b])
        seed[(b,) + tuple(int(x) for x in idx[len(idx) // 2])] = True    # one brick the surface crosses, per object
    grown = G.narrow_band_grid(model, sc, R, level=LEVEL_BOX, bound=BOUND_BOX, initial_bricks=seed)
    assert grown.rounds > 1
    dense = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=R, bound=BOUND_BOX)
    assert _same_meshes(G.extract_mesh(grown.grid, level=LEVEL_BOX, bound=BOUND_BOX), dense)
    g, active, rounds, points = _restated(amd, model, sc, R, BOUND_BOX, LEVEL_BOX, initial=seed.cpu().numpy())
    assert np.array_equal(grown.active.cpu().numpy(), active) and grown.rounds == rounds and grown.points == points
    assert np.array_equal(grown.grid.cpu().numpy(), g, equal_nan=True)


def test_fog_decoder_cut_at_its_median(amd, dev):  # noqa: F811
    """The worst case: the surface runs through most bricks."""
    from supnerf_amd import geometry as G
    model = _model(amd, dev, 3, 1, seed=0)
    sc = _codes(2, 1, dev)
    R, bound = 64, (-0.5, 0.5)
    dense_grid = G.density_grid(model, sc, R, bound)
    level = float(dense_grid.median())
    nbg = G.narrow_band_grid(model, sc, R, level=level, bound=bound)
    assert _same_meshes(G.extract_mesh(nbg.grid, level=level, bound=bound), G.extract_mesh(dense_grid, level=level, bound=bound))
    g, active, rounds, points = _restated(amd, model, sc, R, bound, level)
    assert np.array_equal(nbg.active.cpu().numpy(), active) and nbg.rounds == rounds and nbg.points == points
    assert float(nbg.active.float().mean()) > 0.5


def test_non_finite_density_raises(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    params = planted_params(3, 1, seed=2)
    params["encoding_shape.bias"][0] = float("nan")
    model = _model(amd, dev, 3, 1, params=params)
    sc = _codes(2, 3, dev)
    with pytest.raises(amd.SnrError):
        G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=40, bound=BOUND_BOX)
    with pytest.raises(amd.SnrError):
        G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=40, bound=BOUND_BOX, narrow_band=True)
    nbg = G.narrow_band_grid(model, sc, 40, level=LEVEL_BOX, bound=BOUND_BOX)
    assert bool(nbg.active.all())                                           # every corner is NaN: every brick is evaluated
