"""CPU tests of the iso-surface backward's restatement (tests/iso_grad_restatement.py): its fp32 gather against float64 autograd through
the vertex formula, against a central difference at fixed topology, against its own per-point loop bit for bit, and its compaction."""
import numpy as np
import pytest
import torch

import iso_grad_restatement as IG
import iso_restatement as IR

FIELDS = {
    "sphere": lambda: IR.sphere_field(24) + (0.0,),
    "torus": lambda: IR.torus_field(28) + (0.0,),
    "noise": lambda: IR.noise_field(20, seed=3) + (0.1,),
}


def _field(name):
    f, lo, h, level = FIELDS[name]()
    return f, lo, h, np.float32(level)


def _d_verts(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3)).astype(np.float32)


def _autograd64(f, level, lo, h, g):
    """d grid of sum(g . verts) in float64 through the vertex formula on the fp32 forward's edge list."""
    u, d = IG.vertex_edges(f, level)
    f64 = torch.tensor(f, dtype=torch.float64, requires_grad=True)
    v = IG.vertices64(f64, u, d, float(level), lo, h)
    (v * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return f64.grad.numpy()


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_edge_list_is_the_forward_vertex_order(name):
    f, lo, h, level = _field(name)
    verts, _ = IR.extract(f, level, lo, h)
    u, d = IG.vertex_edges(f, level)
    assert u.shape[0] == verts.shape[0] > 0
    v64 = IG.vertices64(f.astype(np.float64), u, d, float(level), lo, h)
    assert np.abs(v64 - verts).max() < 1e-5 * (1 + np.abs(verts).max())


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_restated_gradient_is_float64_autograd(name):
    f, lo, h, level = _field(name)
    n = IG.vertex_edges(f, level)[0].shape[0]
    g = _d_verts(n, 1)
    got, on = IG.grid_grad(f, level, h, g)
    want = _autograd64(f, level, lo, h, g)
    assert got.dtype == np.float32 and got.shape == f.shape
    # fp32 sums of at most 14 terms: relative to the terms' own size
    scale = np.abs(IG.grid_grad(f, level, h, np.abs(g))[0]) + np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 1e-5 * scale + 1e-30).all(), float((err / (scale + 1e-30)).max())
    # zero exactly off the surface, and the surface is exactly the ends of crossing edges
    u, d = IG.vertex_edges(f, level)
    ends = np.zeros(f.size, dtype=bool)
    ends[u] = True
    ends[u + IG._offset(np.array(IR.DIR_BITS)[d], f.shape[1], f.shape[2])] = True
    assert np.array_equal(on.reshape(-1).astype(bool), ends)
    assert (got.reshape(-1)[~ends] == 0).all() and not np.signbit(got.reshape(-1)[~ends]).any()
    assert np.count_nonzero(got) > 0


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_vertex_motion_matches_a_central_difference(name):
    """f + eps q with eps small enough that no sample changes side: d/d eps of sum(w . verts) = sum(d_grid . q)."""
    f, lo, h, level = _field(name)
    rng = np.random.default_rng(7)
    q = rng.normal(size=f.shape)
    u, d = IG.vertex_edges(f, level)
    w = _d_verts(u.shape[0], 2)
    got = float((IG.grid_grad(f, level, h, w)[0].astype(np.float64) * q).sum())
    gap = np.abs(f.astype(np.float64) - float(level)).min()
    eps = 1e-3 * gap / np.abs(q).max()
    f64 = f.astype(np.float64)
    lp, lm = f64 + eps * q, f64 - eps * q
    for x in (lp, lm):                                             # topology held fixed
        assert np.array_equal(x > float(level), f64 > float(level))

    def loss(x):
        return float((IG.vertices64(x, u, d, float(level), lo, h) * w.astype(np.float64)).sum())

    fd = (loss(lp) - loss(lm)) / (2 * eps)
    assert abs(got - fd) <= 1e-4 * abs(fd) + 1e-6 * np.abs(w).sum(), (got, fd)


@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_gather_order_reproduces_its_own_fp32_sums(name):
    """The vectorised gather is the per-point loop of the kernel (outgoing d = 0..6, then incoming d = 0..6), bit for bit."""
    f, lo, h, level = {"sphere": lambda: IR.sphere_field(9, r=0.3) + (np.float32(0),),
                       "noise": lambda: IR.noise_field(9, seed=5) + (np.float32(0.05),)}[name]()
    n = IG.vertex_edges(f, level)[0].shape[0]
    assert n > 0
    for seed in range(3):
        g = _d_verts(n, 10 + seed) * np.float32(10.0 ** (seed - 1))
        vec, _ = IG.grid_grad(f, level, h, g)
        loop = IG.grid_grad_loop(f, level, h, g)
        assert np.array_equal(vec, loop)


def test_surface_points_compaction():
    fields = [IR.sphere_field(12)[0], IR.torus_field(12)[0], np.full((12, 12, 12), -1.0, dtype=np.float32)]
    lo, h, _ = IR.lattice(12, -0.5, 0.5)
    on, dg = [], []
    for k, f in enumerate(fields):
        n = IG.vertex_edges(f, 0.0)[0].shape[0]
        g, o = IG.grid_grad(f, 0.0, h, _d_verts(n, k))
        dg.append(g)
        on.append(o)
    on, dg = np.stack(on), np.stack(dg)
    xyz, ds, n, counts = IG.surface_points(on, dg, lo, h)
    assert n % 64 == 0 and n >= counts.max() > 0 and counts[2] == 0
    assert xyz.shape == (3 * n, 3) and ds.shape == (3 * n,)
    axes = IR.lattice(12, -0.5, 0.5)[2]
    for b in range(3):
        v = np.nonzero(on[b].reshape(-1))[0]
        pts = np.stack([axes[0][v // 144], axes[1][v // 12 % 12], axes[2][v % 12]], axis=1)
        assert np.array_equal(xyz[b * n:b * n + v.size], pts)
        assert np.array_equal(ds[b * n:b * n + v.size], dg[b].reshape(-1)[v])
        assert (xyz[b * n + v.size:(b + 1) * n] == lo).all() and (ds[b * n + v.size:(b + 1) * n] == 0).all()
