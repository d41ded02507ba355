"""What the narrow-band tests share: analytic fields on fine and coarse lattices (``band_restatement.on_lattices``), the cases that
tests/test_band_kernels_gpu.py runs through the band kernels and tests/test_band_cases_cpu.py shows to be sharp, their restatement, and
the one comparison both files use.  Everything is fp32 numpy; every comparison is exact (integers, sets, float bits with NaN equal to NaN).

A case is B objects of (dense, coarse) with a level, a band and an optional mask of initial bricks.  No lattice has more than 61 points per
axis, and no case more than 4 objects."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import band_restatement as NB
import iso_restatement as I

# the analytic fields of tests/test_narrow_band_cpu.py: (field, lattice)
FIELDS = {
    "sphere": (NB.sphere(), 64),
    "torus": (NB.torus(), 48),
    "two_spheres": (NB.two_spheres(), (61, 40, 23)),
    "sphere_17": (NB.sphere(r=0.3), 17),
    "torus_45": (NB.torus(0.28, 0.15), (45, 50, 39)),
    "sphere_30": (NB.sphere(r=0.3), (30, 33, 26)),
    "plane_between_bricks": (NB.plane(-0.5 + 15.5 / 47), 48),     # between fine points 15 and 16: growth across a brick face
}


class Case(NamedTuple):
    shape: tuple                      # the fine lattice
    dense: np.ndarray                 # (B, n0, n1, n2) float32: the field at every fine point
    coarse: np.ndarray                # (B, nb0+1, nb1+1, nb2+1) float32: the field on the coarse lattice
    level: float
    band: float
    initial: Optional[np.ndarray]     # (B, nb0, nb1, nb2) bool: replaces the classification
    finite: bool                      # dense and coarse hold finite values only: the grid can be meshed
    found: bool                       # ... and the band finds the whole surface: the narrow-band mesh is the dense mesh


class Run(NamedTuple):
    """One run of the narrow band's loop, by the kernels or by the restatement."""
    state: np.ndarray                 # (B, nb0, nb1, nb2) int32: 0 filled, 1 the first evaluation, s growth round s - 1
    fill: np.ndarray                  # (B, nb0, nb1, nb2) float32
    grid: np.ndarray                  # (B, n0, n1, n2) float32
    rounds: int
    evaluated: int
    lists: tuple                      # per evaluation, in order: the (n, 4) bricks (object, I, J, K) handed to it


def tilted_plane(X, Y, Z):
    return (X + np.float32(0.5) * Y - np.float32(0.25) * Z) - np.float32(0.07)


def constant(c):
    return lambda X, Y, Z: np.float32(c) + np.float32(0.0) * (X + Y + Z)


def diagonal_points(shape):
    """Inside at the fine points (7, 7, 7) and (15, 15, 15) alone, the far corners of the bricks (0, 0, 0) and (1, 1, 1): from brick
    (0, 0, 0) the only edge into brick (1, 1, 1) that crosses the level is the xyz diagonal from (7, 7, 7), and so on to (2, 2, 2)."""
    _, h, axes = I.lattice(shape, -0.5, 0.5)
    r = 0.5 * float(min(h))
    a, b = (NB.sphere([axes[x][p] for x in range(3)], r) for p in (7, 15))
    return lambda X, Y, Z: np.maximum(a(X, Y, Z), b(X, Y, Z))


def _case(fields, shape, level=0.0, band=0.0, initial=None):
    made = [NB.on_lattices(fn, shape) for fn in fields]
    dense, coarse = np.stack([m[0] for m in made]), np.stack([m[1] for m in made])
    return Case(tuple(shape), dense, coarse, float(level), float(band), initial, True, True)


def _name(prefix, shape):
    return prefix + "_" + "x".join(str(n) for n in shape)


TILTED_SHAPES = ((2, 2, 2), (8, 8, 8), (2, 9, 3), (9, 2, 30), (9, 9, 9), (16, 17, 8), (17, 17, 17), (23, 40, 61))
NON_CUBIC = ((61, 40, 23), (45, 50, 39), (30, 33, 26))
SURFACES = {"sphere": NB.sphere(r=0.3), "torus": NB.torus(0.28, 0.15), "two_spheres": NB.two_spheres()}
SMALL_SPHERE_BRICK = (3, 3, 3)        # the brick of a 40^3 lattice that holds the whole small sphere
BOUNDARY_POINT = (23, 0, 8)           # sphere at (30, 33, 26): a point of an active brick whose +x neighbour lies in an inactive one


def small_sphere():
    """The sphere of radius 0.05 centred in brick (3, 3, 3) of the 40^3 lattice: (dense, coarse), and the smallest |corner - level| of that
    brick read from the coarse array."""
    _, _, axes = I.lattice(40, -0.5, 0.5)
    c = [axes[a][8 * SMALL_SPHERE_BRICK[a] + 4] for a in range(3)]
    dense, coarse, _, _ = NB.on_lattices(NB.sphere(c, 0.05), (40, 40, 40))
    corners = np.stack([NB.corner_values(coarse, q)[SMALL_SPHERE_BRICK] for q in range(8)])
    return dense, coarse, float(np.abs(corners).min())


def boundary_points(state):
    """The points (i, j, k) of evaluated bricks (state (nb0, nb1, nb2) != 0) whose +x neighbour lies in a brick that is not."""
    act = np.asarray(state) != 0
    face = act[:-1] & ~act[1:]                                     # brick (I, J, K) evaluated, (I + 1, J, K) not
    out = []
    for I_, J, K in np.argwhere(face):
        out += [(8 * I_ + 7, j, k) for j in range(8 * J, 8 * J + 8) for k in range(8 * K, 8 * K + 8)]
    return out


def _seed(shape, brick):
    m = np.zeros((1,) + NB.n_bricks(shape), dtype=bool)
    m[(0,) + tuple(brick)] = True
    return m


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}, built once; nothing changes them."""
    out = {}
    for shape in TILTED_SHAPES:
        out[_name("tilted", shape)] = _case([tilted_plane], shape)
    for shape in NON_CUBIC:
        for name, fn in SURFACES.items():
            out[_name(name, shape)] = _case([fn], shape)
    out["batch_of_four"] = _case([SURFACES["sphere"], constant(-1.0), SURFACES["two_spheres"], constant(1.0)], (61, 40, 23))
    out["seed_tilted"] = _case([tilted_plane], (23, 40, 61), initial=_seed((23, 40, 61), (0, 3, 0)))
    out["seed_torus"] = _case([NB.torus()], (45, 50, 39), initial=_seed((45, 50, 39), (2, 0, 2)))
    out["seed_diagonal"] = _case([diagonal_points((23, 40, 61))], (23, 40, 61), initial=_seed((23, 40, 61), (0, 0, 0)))

    lo, h, _ = I.lattice((40, 33, 18), -0.5, 0.5)
    x0 = NB.coarse_axes(lo, h, (40, 33, 18))[0][2]                 # the plane through the coarse points I = 2: values exactly at the level
    out["tie_plane"] = _case([NB.plane(x0)], (40, 33, 18))

    dense, coarse, nearest = small_sphere()
    for name, band in (("0", 0.0), ("0.02", 0.02), ("0.05", 0.05), ("boundary", nearest)):
        out["small_sphere_band_" + name] = Case((40, 40, 40), dense[None], coarse[None], 0.0, band, None, True, band >= nearest)

    # non-finite corners: brick (0, 0, 0) has a +inf corner, (0, 1, 0) a -inf one, (1, 1, 1) a NaN one; (1, 0, 0) has none
    shape = (16, 12, 9)
    dense = np.full(shape, -1.0, np.float32)
    coarse = np.full((3, 3, 3), -1.0, np.float32)
    coarse[2, 2, 2] = np.nan
    coarse[0, 0, 0] = dense[0, 0, 0] = np.inf
    coarse[0, 2, 0] = -np.inf
    out["coarse_non_finite"] = Case(shape, dense[None], coarse[None], 0.0, 0.0, None, False, False)

    dense, coarse, _, _ = NB.on_lattices(SURFACES["sphere"], (30, 33, 26))
    for name, v in (("pinf", np.inf), ("nan", np.nan), ("ninf", -np.inf)):
        d = dense.copy()
        d[BOUNDARY_POINT] = v
        out["dense_" + name] = Case((30, 33, 26), d[None], coarse[None], 0.0, 0.0, None, False, False)
    return out


def brick_lists(state):
    """Per evaluation, in order: the sorted (n, 4) bricks (object, I, J, K) of state 1, 2, ... (no first evaluation where no brick has state
    1: the loop skips an empty one)."""
    state = np.asarray(state)
    out = [np.argwhere(state == s) for s in range(1, int(state.max(initial=0)) + 1)]
    return tuple(x for s, x in enumerate(out) if s > 0 or len(x))


def restated(case, wrong=None):
    """The ``Run`` of tests/band_restatement.py on a case, object by object.  The objects grow in the same rounds (a brick's stamp does not
    depend on the other objects), so the batch's rounds are the most any object needs.  ``wrong``: one of ``NB.WRONG``."""
    B = case.dense.shape[0]
    t = [NB.narrow_band(case.dense[b], case.coarse[b], case.level, case.band, None if case.initial is None else case.initial[b], trace=True,
                        wrong=wrong) for b in range(B)]
    state = np.stack([x.state for x in t]).astype(np.int32)
    return Run(state, np.stack([x.fill for x in t]), np.stack([x.grid for x in t]), max(x.rounds for x in t), sum(x.evaluated for x in t),
               brick_lists(state))


@functools.lru_cache(maxsize=None)
def wanted(name):
    """The restated ``Run`` of the case ``name``, computed once; nothing changes it."""
    return restated(cases()[name])


def same_bits(a, b):
    """Per element: the same fp32 bit pattern, or both NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def differences(got, want):
    """What of a ``Run`` differs from another, as a list of words (empty: the runs are the same):
      state   the rounds of activation, exactly;
      fill    at the bricks of state 0, by bits;
      grid    the final grid, by bits;
      rounds, evaluated;
      lists   per evaluation the set of listed bricks (compared sorted: a growth round lists in no fixed order), each brick listed once and
              in range, and as many as ``got.state`` holds of that round."""
    out = []
    if got.state.shape != want.state.shape or not np.array_equal(got.state, want.state):
        out.append("state")
    if got.fill.shape != want.fill.shape or not same_bits(got.fill, want.fill)[want.state == 0].all():
        out.append("fill")
    if got.grid.shape != want.grid.shape or not same_bits(got.grid, want.grid).all():
        out.append("grid")
    if got.rounds != want.rounds:
        out.append("rounds")
    if got.evaluated != want.evaluated:
        out.append("evaluated")
    ok = len(got.lists) == len(want.lists)
    hi = np.array(got.state.shape)
    first = 1 if (got.state == 1).any() else 2
    for s, l in enumerate(got.lists, first):
        l = np.asarray(l, dtype=np.int64).reshape(-1, 4)
        ok = ok and len(l) == int((got.state == s).sum())                       # n_new
        ok = ok and bool(((l >= 0) & (l < hi)).all()) and len(np.unique(l, axis=0)) == len(l)
    if ok:
        for l, w in zip(got.lists, want.lists):
            l = np.asarray(l, dtype=np.int64).reshape(-1, 4)
            ok = ok and np.array_equal(l[np.lexsort(l.T[::-1])], np.asarray(w, dtype=np.int64))
    if not ok:
        out.append("lists")
    return out


def compare(got, want):
    diff = differences(got, want)
    assert not diff, diff
