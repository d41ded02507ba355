"""Narrow-band grids on the host: the rules of tests/band_restatement.py on analytic fields (the fixpoint mesh is the dense mesh bit for
bit, no crossing edge keeps an unevaluated end, growth from one brick, the documented miss), the coarse-lattice identity, and the argument
checks of the new entry points that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import band_restatement as NB
import iso_restatement as I
from band_cases import FIELDS


def _evaluated(active, shape):
    return active.reshape(-1)[NB.point_bricks(shape)]


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_fixpoint_mesh_is_the_dense_mesh(name):
    fn, shape = FIELDS[name]
    shape = tuple(np.broadcast_to(shape, (3,)))
    dense, coarse, lo, h = NB.on_lattices(fn, shape)
    g, active, rounds, points = NB.narrow_band(dense, coarse, 0.0)
    vd, fd = I.extract(dense, 0.0, lo, h)
    vn, fn_ = I.extract(g, 0.0, lo, h)
    assert fd.shape[0] > 0
    assert np.array_equal(vn, vd) and np.array_equal(fn_, fd), name
    ev = _evaluated(active, shape)
    assert np.array_equal(g[ev], dense[ev])                        # exact wherever evaluated
    assert NB.unevaluated_crossings(g, ev, 0.0)[0] == 0             # no crossing edge with an unevaluated end
    nb = NB.n_bricks(shape)
    assert points == int(np.prod([b + 1 for b in nb])) + 512 * int(active.sum())
    if name == "plane_between_bricks":
        assert rounds >= 1                                          # the bricks past the face are found by growth, not by their corners


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_inactive_bricks_never_share_a_crossing_edge(name):
    """After classification alone: filled bricks holding adjacent points share a coarse corner, so they lie on one side together."""
    fn, shape = FIELDS[name]
    shape = tuple(np.broadcast_to(shape, (3,)))
    dense, coarse, _, _ = NB.on_lattices(fn, shape)
    active, fill = NB.classify(coarse, 0.0)
    pb = NB.point_bricks(shape)
    ev = active.reshape(-1)[pb]
    g = np.where(ev, dense, fill.reshape(-1)[pb]).astype(np.float32)
    assert NB.unevaluated_crossings(g, ev, 0.0)[1] == 0
    assert np.isfinite(fill).all()
    # the fill lies on the side of every corner of its brick, and is one of them
    inside = fill[~active] > 0
    for q in range(8):
        s = NB.corner_values(coarse, q)
        assert np.array_equal(s[~active] > 0, inside)


def test_plane_on_coarse_points_is_active_through_the_tie():
    lo, h, _ = I.lattice(40, -0.5, 0.5)
    x0 = NB.coarse_axes(lo, h, (40, 40, 40))[0][2]                # the plane through the coarse points I = 2: values exactly at the level
    dense, coarse, lo, h = NB.on_lattices(NB.plane(x0), (40, 40, 40))
    active, _ = NB.classify(coarse, 0.0)
    assert active[1].all() and active[2].all() and not active[0].any() and not active[3:].any()
    g, _, _, _ = NB.narrow_band(dense, coarse, 0.0)
    assert all(np.array_equal(a, b) for a, b in zip(I.extract(g, 0.0, lo, h), I.extract(dense, 0.0, lo, h)))


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres_one"])
def test_growth_from_one_brick_recovers_the_connected_surface(name):
    if name == "two_spheres_one":
        fn, shape = NB.sphere((0.2, 0.1, -0.04), 0.2), 61           # one sphere: a connected surface
    else:
        fn, shape = FIELDS[name][0], 64
    shape = tuple(np.broadcast_to(shape, (3,)))
    dense, coarse, lo, h = NB.on_lattices(fn, shape)
    active, _ = NB.classify(coarse, 0.0)
    seed = np.zeros_like(active)
    seed[tuple(np.argwhere(active)[len(np.argwhere(active)) // 2])] = True
    g, grown, rounds, _ = NB.narrow_band(dense, coarse, 0.0, initial=seed)
    assert rounds > 1
    assert all(np.array_equal(a, b) for a, b in zip(I.extract(g, 0.0, lo, h), I.extract(dense, 0.0, lo, h))), name
    assert NB.unevaluated_crossings(g, _evaluated(grown, shape), 0.0)[0] == 0


def test_a_sphere_inside_one_brick_is_missed_unless_the_band_reaches_it():
    """The documented limit: a component wholly inside bricks whose corners are all on one side is not found; ``band`` is the knob."""
    n = 64
    lo, h, axes = I.lattice(n, -0.5, 0.5)
    c = [axes[a][8 * 3 + 4] for a in range(3)]                     # the centre of brick (3, 3, 3)
    r = float(2.5 * h[0])
    dense, coarse, lo, h = NB.on_lattices(NB.sphere(c, r), (n, n, n))
    vd, fd = I.extract(dense, 0.0, lo, h)
    assert fd.shape[0] > 0
    g, active, rounds, _ = NB.narrow_band(dense, coarse, 0.0)
    assert not active.any() and rounds == 0
    assert I.extract(g, 0.0, lo, h)[1].shape[0] == 0                # missed
    band = float(np.abs(coarse).min()) * 1.01                      # a band that reaches the nearest corners
    g, active, _, _ = NB.narrow_band(dense, coarse, 0.0, band=band)
    assert active.any()
    assert all(np.array_equal(a, b) for a, b in zip(I.extract(g, 0.0, lo, h), (vd, fd)))


def test_non_finite_corners_are_active_and_fill_nan():
    coarse = np.full((3, 3, 3), -1.0, np.float32)
    coarse[2, 2, 2] = np.nan
    coarse[0, 0, 0] = np.inf
    active, fill = NB.classify(coarse, 0.0)
    assert active[1, 1, 1] and active[0, 0, 0] and not active[0, 1, 0]
    assert np.isnan(fill[1, 1, 1]) and np.isnan(fill[0, 0, 0]) and fill[0, 1, 0] == -1.0


def test_coarse_lattice_formula_is_exact():
    """(8h) I and h (8I) are the same real product rounded once: lo + (8h) I == lo + h (8I) in fp32 for every I <= 64, whatever h."""
    from supnerf_amd import geometry as G
    rng = np.random.default_rng(0)
    cases = [(n, (-0.5, 0.5)) for n in (2, 9, 17, 61, 64, 100, 129, 200, 256, 511, 512)]
    cases += [(int(rng.integers(2, 513)), (float(rng.uniform(-3, 0)), float(rng.uniform(0.01, 3)))) for _ in range(40)]
    I_ = np.arange(65, dtype=np.float32)
    for n, bound in cases:
        lat = G.lattice(n, bound)
        lo, h = np.float32(lat.lo[0]), np.float32(lat.h[0])
        a = (lo + (np.float32(8) * h) * I_).astype(np.float32)
        b = (lo + h * (np.float32(8) * I_)).astype(np.float32)
        assert np.array_equal(a, b), (n, bound)
        c = G.coarse_lattice(lat)
        assert c.n[0] == (n + 7) // 8 + 1 and np.float32(c.h[0]) == np.float32(8) * h and c.lo[0] == lat.lo[0]
    # ... so the coarse grid of a field is the fine grid at every coarse point inside the grid
    for shape in ((64, 64, 64), (61, 40, 23), (17, 17, 17), (9, 2, 30)):
        dense, coarse, _, _ = NB.on_lattices(NB.torus(), shape)
        inner = coarse[:(shape[0] - 1) // 8 + 1, :(shape[1] - 1) // 8 + 1, :(shape[2] - 1) // 8 + 1]
        assert np.array_equal(inner, dense[::8, ::8, ::8])


def test_band_entry_points_reject_null_pointers_and_bad_lattices():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    lib = A._lib.lib()                       # loads without a GPU; every call below returns before any device work
    E_ARG = -1
    buf = (C.c_float * 64)()
    ib = (C.c_int32 * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(ib, C.c_void_p)
    good = G.lattice(16)
    bad = [G.lattice(16), G.lattice(16), G.lattice(16)]
    bad[0].n[1] = 1
    bad[1].n[2] = 513
    bad[2].n[0] = 0
    null = C.c_void_p(0)

    # (entry point, its arguments with a good lattice and host pointers, the positions of its pointers).  Every call below has exactly one
    # bad argument: with all of them good the call would launch a kernel on these host buffers.
    entries = [
        (lib.snr_band_classify, lambda lat: [p, 2, lat, 0.0, 0.0, q, p, null], (0, 5, 6)),
        (lib.snr_band_compact, lambda lat: [q, q, 2, lat, q, null], (0, 1, 4)),
        (lib.snr_band_fill, lambda lat: [p, 2, lat, q, p, null], (0, 3, 4)),
        (lib.snr_band_seam, lambda lat: [p, 2, lat, 0.0, 2, q, q, q, null], (0, 5, 6, 7)),
    ]
    for fn, args, ptrs in entries:
        for lat in bad:                                                # a bad lattice, good pointers
            assert fn(*args(lat)) == E_ARG
        for i in ptrs:                                                 # a good lattice, one null pointer
            a = args(good)
            a[i] = null
            assert fn(*a) == E_ARG, (fn, i)
    assert lib.snr_band_classify(p, 2, None, 0.0, 0.0, q, p, null) == E_ARG
    assert lib.snr_band_classify(p, 2, good, 0.0, -1.0, q, p, null) == E_ARG        # negative band
    assert lib.snr_band_classify(p, 2, good, 0.0, float("nan"), q, p, null) == E_ARG
    assert lib.snr_band_seam(p, 2, good, 0.0, 1, q, q, q, null) == E_ARG            # stamp < 2
    assert lib.snr_band_fill(p, -1, good, q, p, null) == E_ARG
    # the brick mode of the density decoder
    bl = G.lattice(16)
    for args in [(None, 1, q, 1, p, p, 1, 1, p, null), (bl, 1, null, 1, p, p, 1, 1, p, null), (bl, 1, q, 1, null, p, 1, 1, p, null),
                 (bl, 1, q, 1, p, null, 1, 1, p, null), (bl, 1, q, 1, p, p, 1, 1, null, null), (bl, -1, q, 1, p, p, 1, 1, p, null),
                 (bl, 1, q, -1, p, p, 1, 1, p, null), (bl, 1, q, 1, p, p, 9, 1, p, null), (bad[1], 1, q, 1, p, p, 1, 1, p, null),
                 (bad[2], 1, q, 1, p, p, 1, 1, p, null)]:
        assert lib.snr_density_bricks(*args) == E_ARG, args


def test_narrow_band_argument_checks_without_a_gpu():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    model = A.CodeNeRF(shape_blocks=1, texture_blocks=1)
    calls = [
        lambda: G.narrow_band_grid(model, torch.zeros(1, 256), 16, level=0.0),                   # CPU codes
        lambda: G.narrow_band_grid(torch.nn.Linear(3, 1), torch.zeros(1, 256), 16, level=0.0),  # not a supnerf_amd decoder
        lambda: G.narrow_band_grid(model, torch.zeros(1, 256), 513, level=0.0),
        lambda: G.extract_mesh(torch.zeros(8, 8, 8), level=0.0, narrow_band=True),              # a grid has no decoder to narrow
    ]
    for call in calls:
        with pytest.raises(A.SnrError):
            call()
    lat = G.lattice((61, 40, 23), ((-0.6, -0.25, -0.4), (0.5, 0.35, 0.45)))
    c = G.coarse_lattice(lat)
    lo, h, _ = I.lattice((61, 40, 23), (-0.6, -0.25, -0.4), (0.5, 0.35, 0.45))
    want = NB.coarse_axes(lo, h, (61, 40, 23))
    for a in range(3):
        got = (np.float32(c.lo[a]) + np.float32(c.h[a]) * np.arange(c.n[a], dtype=np.float32)).astype(np.float32)
        assert np.array_equal(got, want[a])
