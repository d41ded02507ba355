"""Test helper: a numpy restatement of the narrow-band rules of include/supnerf_hip.h ("Narrow band"), sup-nerf_amd/csrc/snr_band.hip and
``geometry.narrow_band_grid``, on top of ``iso_restatement`` (the 7 Kuhn edge directions, the mesh).

Rules:
  * brick (I, J, K) owns the fine points [8I, 8I+8) x [8J, 8J+8) x [8K, 8K+8) inside the grid; nb = ceil(n / 8) bricks per axis;
  * the coarse lattice: lo, spacing 8 h (fp32, exact), nb + 1 points per axis -- the fine points at multiples of 8 and one row past the
    far edge; a brick's corners are its coarse points (I..I+1, J..J+1, K..K+1);
  * active: the corners are not all on one side of the level (inside iff value > level), or |corner - level| <= band (fp32), or a corner
    is not finite.  Fill: the largest corner when all 8 are inside, else the smallest; NaN when a corner is not finite;
  * growth: every edge (u, u + d) of the 7 directions whose ends are on different sides of the level and not both in evaluated bricks
    activates the bricks of its unevaluated ends; they are evaluated and the next round starts; a round that activates nothing ends it;
  * state per brick: 0 = not evaluated (its points hold the fill), 1 = the first evaluation, s = activated by growth round s - 1; within a
    round a brick counts as evaluated iff 1 <= state < the round's stamp, and a brick the round activates keeps its fill until the round is over;
  * points evaluated: the coarse lattice's points plus 512 per evaluated brick.

Written for clarity (vectorised over points, looped over directions and rounds), like ``iso_restatement``."""
from typing import NamedTuple

import numpy as np

import iso_restatement as I

BRICK = 8


def n_bricks(shape):
    return tuple((int(n) + BRICK - 1) // BRICK for n in shape)


def coarse_axes(lo, h, shape):
    """Per axis the fp32 coordinates lo + (8 h) I of the coarse lattice, I = 0 .. nb."""
    nb = n_bricks(shape)
    lo = np.asarray(lo, dtype=np.float32)
    h8 = (np.float32(BRICK) * np.asarray(h, dtype=np.float32)).astype(np.float32)
    return [(lo[a] + h8[a] * np.arange(nb[a] + 1, dtype=np.float32)).astype(np.float32) for a in range(3)]


def fine_axes(lo, h, shape):
    lo = np.asarray(lo, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    return [(lo[a] + h[a] * np.arange(shape[a], dtype=np.float32)).astype(np.float32) for a in range(3)]


def on_lattices(fn, shape, lo=-0.5, hi=0.5):
    """(dense (n0, n1, n2), coarse (nb0+1, nb1+1, nb2+1), lo, h) of the fp32 field fn(X, Y, Z) on the fine lattice and on its coarse
    lattice, both made by the kernels' formula."""
    lo, h, _ = I.lattice(shape, lo, hi)
    dense = fn(*np.meshgrid(*fine_axes(lo, h, shape), indexing="ij")).astype(np.float32)
    coarse = fn(*np.meshgrid(*coarse_axes(lo, h, shape), indexing="ij")).astype(np.float32)
    return dense, coarse, lo, h


# One wrong rule each, for tests/test_band_cases_cpu.py: what the cases of tests/band_cases.py must be able to tell from the rules above.
WRONG = (
    "swap_axes",      # nb1 and nb2 exchanged in the linear index of a brick and of a corner (where a kernel would then read out of range,
                      # the index wraps): invisible wherever nb1 = nb2
    "near_strict",    # |corner - level| < band
    "no_near",        # the band ignored
    "fill_smallest",  # an all-inside brick filled with its smallest corner
    "no_diagonal",    # growth without the xyz diagonal, 6 directions
    "order",          # a brick activated earlier in the same round (grid points in index order) is evaluated at once
    "no_stamp_test",  # ... merely counts as evaluated for the rest of the round, its points still filled
)


def _wrong(wrong):
    assert wrong is None or wrong in WRONG, wrong
    return wrong


def corner_values(coarse, q, wrong=None):
    """(nb0, nb1, nb2): corner q (bit a = +1 on axis a) of every brick."""
    dx, dy, dz = q & 1, q >> 1 & 1, q >> 2 & 1
    b0, b1, b2 = (s - 1 for s in coarse.shape)
    if _wrong(wrong) == "swap_axes":
        i, j, k = np.meshgrid(np.arange(b0) + dx, np.arange(b1) + dy, np.arange(b2) + dz, indexing="ij")
        return coarse.reshape(-1)[((i * (b2 + 1) + j) * (b1 + 1) + k) % coarse.size]
    return coarse[dx:dx + b0, dy:dy + b1, dz:dz + b2]


def classify(coarse, level, band=0.0, wrong=None):
    """coarse (nb0+1, nb1+1, nb2+1) -> (active (nb0, nb1, nb2) bool, fill (nb0, nb1, nb2) float32)."""
    c = np.ascontiguousarray(coarse, dtype=np.float32)
    level, band = np.float32(level), np.float32(band)
    corners = np.stack([corner_values(c, q, wrong) for q in range(8)], axis=-1)
    n_in = (corners > level).sum(-1)
    finite = np.isfinite(corners).all(-1)
    with np.errstate(invalid="ignore"):
        dist = np.abs((corners - level).astype(np.float32))
        near = ((dist < band) if wrong == "near_strict" else (dist <= band)).any(-1)
        fill = np.where((n_in == 8) & (wrong != "fill_smallest"), corners.max(-1), corners.min(-1)).astype(np.float32)
    if wrong == "no_near":
        near = np.zeros_like(near)
    fill[~finite] = np.float32(np.nan)
    active = ~finite | near | ((n_in != 0) & (n_in != 8))
    return active, fill


def point_bricks(shape, wrong=None):
    """(n0, n1, n2) int64: the linear index (I nb1 + J) nb2 + K of every fine point's brick."""
    nb = n_bricks(shape)
    i, j, k = np.meshgrid(*[np.arange(n) // BRICK for n in shape], indexing="ij")
    if _wrong(wrong) == "swap_axes":
        return ((i * nb[2] + j) * nb[1] + k) % (nb[0] * nb[1] * nb[2])
    return (i * nb[1] + j) * nb[2] + k


def _edges(shape, wrong=None):
    """Per direction: the slices of the lower and of the upper ends of every edge inside the grid."""
    n0, n1, n2 = shape
    for bits in I.DIR_BITS:
        if bits == 7 and _wrong(wrong) == "no_diagonal":
            continue
        dx, dy, dz = bits & 1, bits >> 1 & 1, bits >> 2 & 1
        yield (slice(0, n0 - dx), slice(0, n1 - dy), slice(0, n2 - dz)), (slice(dx, None), slice(dy, None), slice(dz, None))


def unevaluated_crossings(grid, evaluated, level):
    """Number of crossing edges of ``grid`` with an end outside ``evaluated`` (a per-point bool array), and of those with both ends
    outside it."""
    inside = np.asarray(grid, dtype=np.float32) > np.float32(level)
    some = both = 0
    for a, b in _edges(inside.shape):
        cross = inside[a] != inside[b]
        some += int((cross & ~(evaluated[a] & evaluated[b])).sum())
        both += int((cross & ~evaluated[a] & ~evaluated[b]).sum())
    return some, both


class Trace(NamedTuple):
    grid: np.ndarray       # (n0, n1, n2) float32: the final grid
    state: np.ndarray      # (nb0, nb1, nb2) int32: the header's state -- 0 not evaluated, 1 the first evaluation, s growth round s - 1
    fill: np.ndarray       # (nb0, nb1, nb2) float32: the fill value of every brick
    rounds: int            # growth rounds that added bricks
    evaluated: int         # bricks evaluated


def seam(grid, state, level, stamp, wrong=None):
    """One growth round on a grid as it stands: the (nb0, nb1, nb2) bool mask of the bricks it activates.  A brick counts as evaluated
    iff 1 <= state < stamp."""
    g = np.asarray(grid, dtype=np.float32)
    st = np.asarray(state).reshape(-1)
    pb = point_bricks(g.shape, wrong)
    ev = ((st >= 1) & (st < stamp))[pb]
    inside = g > np.float32(level)
    new = np.zeros(st.shape, dtype=bool)
    for a, b in _edges(g.shape, wrong):
        grow = (inside[a] != inside[b]) & ~(ev[a] & ev[b])
        new[pb[a][grow & ~ev[a]]] = True
        new[pb[b][grow & ~ev[b]]] = True
    return (new & (st == 0)).reshape(np.shape(state))


def _seam_in_order(g, f, st, level, stamp, wrong):
    """The two order-dependent rounds, thread after thread: grid point u in index order, its edges in direction order, every brick
    activated so far counting as evaluated.  "order" also evaluates it at once (``g`` is updated in place); "no_stamp_test" leaves its
    points filled.  Returns the mask of the bricks activated."""
    shape = g.shape
    pb = point_bricks(shape).reshape(-1)
    idx = np.arange(g.size).reshape(shape)
    U, W, D = [], [], []
    for d, (a, b) in enumerate(_edges(shape)):
        U.append(idx[a].reshape(-1)), W.append(idx[b].reshape(-1)), D.append(np.full(idx[a].size, d))
    U, W, D = (np.concatenate(x) for x in (U, W, D))
    o = np.lexsort((D, U))
    U, W = U[o], W[o]
    ev = (st >= 1) & (st < stamp)
    new = np.zeros_like(ev)
    gf, ff = g.reshape(-1), f.reshape(-1)
    pos = 0
    while pos < len(U):
        u, w = U[pos:], W[pos:]
        inside = gf > level
        hit = np.flatnonzero((inside[u] != inside[w]) & ~(ev[pb[u]] & ev[pb[w]]))
        if len(hit) == 0:
            break
        pos += int(hit[0])
        for r in (pb[U[pos]], pb[W[pos]]):
            if not ev[r]:
                ev[r] = new[r] = True
                if wrong == "order":
                    m = pb == r
                    gf[m] = ff[m]
        pos += 1
    return new


def narrow_band(dense, coarse, level, band=0.0, initial=None, trace=False, wrong=None):
    """The narrow-band grid of one object.  ``dense``: the exact values at every fine point (what the decoder would give), ``coarse``: its
    coarse grid.  ``initial``: a (nb0, nb1, nb2) mask replacing the classification.  Returns (grid, active, rounds, points), or with
    ``trace`` a ``Trace``.  ``wrong``: one of ``WRONG``, a mistake planted on purpose."""
    f = np.asarray(dense, dtype=np.float32)
    shape = f.shape
    nb = n_bricks(shape)
    level = np.float32(level)
    active, fill = classify(coarse, level, band, wrong)
    if initial is not None:
        active = np.asarray(initial, dtype=bool).copy()
    st = active.reshape(-1).astype(np.int32)
    pb = point_bricks(shape, wrong)
    g = np.where(st[pb] != 0, f, fill.reshape(-1)[pb]).astype(np.float32)
    rounds, stamp = 0, 2
    while True:
        if wrong in ("order", "no_stamp_test"):
            new = _seam_in_order(g, f, st, level, stamp, wrong)
        else:
            new = seam(g, st, level, stamp, wrong).reshape(-1)
        if not new.any():
            break
        st[new] = stamp
        m = new[pb]
        g[m] = f[m]
        rounds += 1
        stamp += 1
    evaluated = int((st != 0).sum())
    if trace:
        return Trace(g, st.reshape(nb), fill, rounds, evaluated)
    points = int(np.prod([x + 1 for x in nb])) + BRICK ** 3 * evaluated
    return g, (st != 0).reshape(nb), rounds, points


# ---------------------------------------------------------------------------------------------------------------- analytic fields
def sphere(c=(0.0, 0.0, 0.0), r=0.35):
    c = [np.float32(x) for x in c]
    return lambda X, Y, Z: np.float32(r * r) - ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)


def torus(R=0.3, r=0.1):
    def f(X, Y, Z):
        q = np.sqrt(X * X + Y * Y) - np.float32(R)
        return np.float32(r * r) - (q * q + Z * Z)
    return f


def two_spheres():
    a, b = sphere((-0.22, -0.05, 0.03), 0.16), sphere((0.2, 0.1, -0.04), 0.2)
    return lambda X, Y, Z: np.maximum(a(X, Y, Z), b(X, Y, Z))


def plane(x0):
    return lambda X, Y, Z: (X - np.float32(x0)) + np.float32(0.0) * (Y + Z)
