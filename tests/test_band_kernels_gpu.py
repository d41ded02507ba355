"""The four narrow-band kernels of csrc/snr_band.hip on the MI355X, against tests/band_restatement.py on the analytic and edge cases of
tests/band_cases.py (non-cubic lattices, band > 0, ties, non-finite values, B = 4, growth from one brick; tests/test_band_cases_cpu.py shows
what each case tells apart).  First through the product's own loop, ``geometry._band_rounds``, with the case's dense values standing in for
the decoder; then each kernel alone through ``ops``, every buffer between guard bands.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import band_cases as BC
import band_restatement as NB
from geometry_cases import same_meshes
from oracle_bands import amd, dev  # noqa: F401  (fixtures)
from segment_sum_restatement import banded, bands_intact

pytestmark = pytest.mark.gpu

NAMES = sorted(BC.cases())
NAN = float("nan")


def _loop(dev, case):  # noqa: F811
    """``geometry._band_rounds`` on a case: (its ``Run`` on the host, the grid on the device).  ``evaluate`` copies the case's dense values
    into the points of the listed bricks that lie inside the grid, skipping rows out of range as ``density_bricks`` does, and keeps each
    round's list."""
    from supnerf_amd import geometry as G
    B = case.dense.shape[0]
    dense = torch.from_numpy(case.dense).to(dev)
    n = case.shape
    hi = torch.tensor((B,) + NB.n_bricks(n), device=dev)
    off = torch.arange(8, device=dev)
    lists = []

    def evaluate(bricks, k, grid):
        rows = bricks[:k].long()
        lists.append(rows.cpu().numpy())
        rows = rows[((rows >= 0) & (rows < hi)).all(1)]
        i, j, l = (rows[:, a + 1, None] * 8 + off for a in range(3))                       # (m, 8) each
        ok = (i < n[0])[:, :, None, None] & (j < n[1])[:, None, :, None] & (l < n[2])[:, None, None, :]
        i, j, l = i.clamp(max=n[0] - 1), j.clamp(max=n[1] - 1), l.clamp(max=n[2] - 1)
        flat = ((rows[:, 0, None, None, None] * n[0] + i[:, :, None, None]) * n[1] + j[:, None, :, None]) * n[2] + l[:, None, None, :]
        flat = flat[ok]
        grid.view(-1)[flat] = dense.view(-1)[flat]

    initial = None if case.initial is None else torch.from_numpy(case.initial).to(dev)
    grid, state, fill, rounds, evaluated = G._band_rounds(G.lattice(n), B, torch.from_numpy(case.coarse).to(dev), evaluate,
                                                          float(np.float32(case.level)), float(np.float32(case.band)), initial)
    return BC.Run(state.cpu().numpy(), fill.cpu().numpy(), grid.cpu().numpy(), rounds, evaluated, tuple(lists)), grid


@pytest.mark.parametrize("name", NAMES)
def test_product_loop_on_analytic_fields(amd, dev, name):  # noqa: F811
    from supnerf_amd import geometry as G
    case, want = BC.cases()[name], BC.wanted(name)
    got, grid = _loop(dev, case)
    BC.compare(got, want)
    if case.finite:
        narrow = G.extract_mesh(grid, level=case.level)
        dense = G.extract_mesh(torch.from_numpy(case.dense).to(dev), level=case.level)
        assert same_meshes(narrow, dense) == case.found, name
        if not case.found:                                         # the documented miss: nothing of the small sphere is meshed
            assert all(f.shape[0] == 0 for _, f in narrow) and all(f.shape[0] > 0 for _, f in dense)
    # again: the same states, grid and per-round sets.  A growth round appends its bricks in the order the threads arrive, so the order
    # within a list may differ from run to run; ``compare`` sorts the lists.
    again, _ = _loop(dev, case)
    BC.compare(again, want)
    assert np.array_equal(again.state, got.state) and BC.same_bits(again.grid, got.grid).all() and BC.same_bits(again.fill, got.fill).all()
    if (got.state == 1).any():                                     # band_compact's list has an order: (object, I, J, K) ascending
        assert np.array_equal(got.lists[0], want.lists[0]) and np.array_equal(again.lists[0], want.lists[0])


# ------------------------------------------------------------------------------------------------------------- each kernel alone
def _guarded(shape, dtype, dev):  # noqa: F811
    """(the whole buffer, its middle as a ``shape`` tensor, the sentinel): NaN (floats) or -1 (int32) everywhere, 64 elements of it on either
    side of the middle."""
    fill = NAN if dtype == torch.float32 else -1
    full, mid = banded(int(np.prod(shape)), dtype, dev, fill)
    return full, mid.view(*shape), fill


def _intact(*buffers):
    return all(bands_intact(full, mid.numel(), fill) for full, mid, fill in buffers)


def _is_sentinel(t):
    return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == -1).all())


def _classified(case):
    """(state (B, nb) int32 of 0 / 1, fill (B, nb) float32) of the restated classification."""
    out = [NB.classify(c, case.level, case.band) for c in case.coarse]
    return np.stack([o[0] for o in out]).astype(np.int32), np.stack([o[1] for o in out])


@pytest.mark.parametrize("name", NAMES)
def test_classify_alone(amd, dev, name):  # noqa: F811
    from supnerf_amd import geometry as G
    case = BC.cases()[name]
    B, nb = case.dense.shape[0], NB.n_bricks(case.shape)
    state, fill = _guarded((B,) + nb, torch.int32, dev), _guarded((B,) + nb, torch.float32, dev)
    amd.ops.band_classify(torch.from_numpy(case.coarse).to(dev), G.lattice(case.shape), case.level, case.band, state[1], fill[1])
    want_state, want_fill = _classified(case)
    assert np.array_equal(state[1].cpu().numpy(), want_state), name
    assert BC.same_bits(fill[1].cpu().numpy(), want_fill).all(), name              # of every brick, active or not
    assert _intact(state, fill)


def _stamped(state, seed):
    """A state array that also holds stamps >= 2: some bricks of state 0 and some of state 1 moved to 2, 3 or 4."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(state.shape) < 0.4, rng.integers(2, 5, state.shape), state).astype(np.int32)


@pytest.mark.parametrize("name", NAMES)
def test_compact_alone(amd, dev, name):  # noqa: F811
    from supnerf_amd import geometry as G
    case = BC.cases()[name]
    lat = G.lattice(case.shape)
    classified = _classified(case)[0]
    for which, state_h in (("classified", classified), ("stamped", _stamped(classified, 3)), ("all", np.ones_like(classified))):
        state = _guarded(state_h.shape, torch.int32, dev)
        state[1].copy_(torch.from_numpy(state_h))
        scan = _guarded((state_h.size,), torch.int32, dev)
        scan[1].copy_(torch.cumsum((state[1] == 1).view(-1), 0, dtype=torch.int32))
        bricks = _guarded((state_h.size, 4), torch.int32, dev)
        amd.ops.band_compact(state[1], scan[1], lat, bricks[1])
        want = np.argwhere(state_h == 1)                                            # (object, I, J, K) ascending: row scan - 1
        got = bricks[1].cpu().numpy()
        assert np.array_equal(got[:len(want)], want), (name, which)
        assert (got[len(want):] == -1).all(), (name, which)                         # nothing past the count
        assert np.array_equal(state[1].cpu().numpy(), state_h) and _intact(state, scan, bricks), (name, which)


@pytest.mark.parametrize("name", NAMES)
def test_fill_alone(amd, dev, name):  # noqa: F811
    from supnerf_amd import geometry as G
    case = BC.cases()[name]
    B, lat = case.dense.shape[0], G.lattice(case.shape)
    classified, fill_h = _classified(case)
    pb = NB.point_bricks(case.shape)
    for which, state_h in (("classified", classified), ("stamped", _stamped(classified, 5)), ("none", np.zeros_like(classified))):
        state, fill = _guarded(state_h.shape, torch.int32, dev), _guarded(state_h.shape, torch.float32, dev)
        state[1].copy_(torch.from_numpy(state_h))
        fill[1].copy_(torch.from_numpy(fill_h))
        grid = _guarded((B,) + case.shape, torch.float32, dev)
        amd.ops.band_fill(grid[1], lat, state[1], fill[1])
        got = grid[1].cpu().numpy()
        for b in range(B):
            filled = (state_h[b].reshape(-1) == 0)[pb]
            assert BC.same_bits(got[b], fill_h[b].reshape(-1)[pb])[filled].all(), (name, which, b)
            assert np.isnan(got[b][~filled]).all(), (name, which, b)               # every other point still holds the sentinel
        assert _intact(state, fill, grid), (name, which)


def _first_grid(case, state_h, fill_h):
    """The grid after the evaluation of the bricks with state != 0: dense values there, fill values elsewhere."""
    pb = NB.point_bricks(case.shape)
    return np.stack([np.where((state_h[b].reshape(-1) != 0)[pb], case.dense[b], fill_h[b].reshape(-1)[pb]) for b in range(len(state_h))])


def _seam_call(amd, dev, case, grid_h, state_h, stamp):  # noqa: F811
    """One ``ops.band_seam`` on guarded buffers: (state after, the listed rows, n_new, the rows past n_new are untouched and every guard
    band is intact)."""
    from supnerf_amd import geometry as G
    grid, state = _guarded(grid_h.shape, torch.float32, dev), _guarded(state_h.shape, torch.int32, dev)
    grid[1].copy_(torch.from_numpy(grid_h))
    state[1].copy_(torch.from_numpy(state_h))
    bricks, n_new = _guarded((state_h.size, 4), torch.int32, dev), _guarded((1,), torch.int32, dev)
    amd.ops.band_seam(grid[1], G.lattice(case.shape), case.level, stamp, state[1], bricks[1], n_new[1])
    k = int(n_new[1].item())
    assert 0 <= k <= state_h.size
    clean = _is_sentinel(bricks[1][k:]) and _intact(grid, state, bricks, n_new) and BC.same_bits(grid[1].cpu().numpy(), grid_h).all()
    return state[1].cpu().numpy(), bricks[1][:k].cpu().numpy(), k, clean


def _check_seam(amd, dev, case, grid_h, state_h, stamp):  # noqa: F811
    """One round against ``NB.seam``: n_new, the listed set, the new stamps; everything else as it was.  Returns (state after, n_new)."""
    new = np.stack([NB.seam(grid_h[b], state_h[b], case.level, stamp) for b in range(len(state_h))])
    after, rows, k, clean = _seam_call(amd, dev, case, grid_h, state_h, stamp)
    assert clean
    assert k == int(new.sum())
    if k:                                                                          # each brick once; the order is the threads'
        assert len(np.unique(rows, axis=0)) == k and np.array_equal(rows[np.lexsort(rows.T[::-1])], np.argwhere(new))
    assert np.array_equal(after, np.where(new, stamp, state_h))                    # state 0 -> stamp where listed; every other state kept
    assert not new[state_h != 0].any()
    return after, k


SEAM_CASES = ("batch_of_four", "two_spheres_30x33x26", "seed_diagonal", "seed_tilted", "dense_pinf", "dense_nan", "tilted_9x2x30",
              "tilted_16x17x8", "torus_45x50x39", "small_sphere_band_0", "tie_plane")


@pytest.mark.parametrize("name", SEAM_CASES)
def test_seam_alone_first_round(amd, dev, name):  # noqa: F811
    case = BC.cases()[name]
    state_h, fill_h = _classified(case)
    if case.initial is not None:
        state_h = case.initial.astype(np.int32)
    grid_h = _first_grid(case, state_h, fill_h)
    after, k = _check_seam(amd, dev, case, grid_h, state_h, 2)
    assert (k > 0) == (BC.wanted(name).rounds > 0), name
    # Again with stamp 3 and nothing evaluated in between.  By the header's rule a brick of state 2 counts as evaluated at stamp 3, and the
    # first call moved every state-0 end of every crossing edge to 2: on the unchanged grid no crossing edge is left with an unevaluated
    # end, so nothing is listed and no state moves.  (The restatement is asked too.)
    again, k = _check_seam(amd, dev, case, grid_h, after, 3)
    assert k == 0 and np.array_equal(again, after)


@pytest.mark.parametrize("name", ("seed_tilted", "two_spheres_30x33x26", "two_spheres_61x40x23"))
def test_seam_alone_late_round(amd, dev, name):  # noqa: F811
    """stamp = 5 on a hand-made state of 1, 3 and 4 (all evaluated) and 0: the run's bricks of the rounds before its last, relabelled, and
    the last round's back at 0 -- which the seam must find again, and nothing else."""
    case, want = BC.cases()[name], BC.wanted(name)
    last = int(want.state.max())
    assert last == 4
    state_h = np.select([want.state == 1, want.state == 2, want.state == 3], [1, 4, 3], 0).astype(np.int32)
    grid_h = _first_grid(case, state_h, want.fill)
    after, k = _check_seam(amd, dev, case, grid_h, state_h, 5)
    assert k == int((want.state == last).sum()) > 0
    assert np.array_equal(after == 5, want.state == last)
    again, k = _check_seam(amd, dev, case, grid_h, after, 6)
    assert k == 0 and np.array_equal(again, after)


def test_refused_arguments_leave_the_buffers_alone(amd, dev):  # noqa: F811
    """stamp = 1 and band < 0 are refused (SNR_E_ARG) before anything is written; the next valid call is sound."""
    from supnerf_amd import geometry as G
    case = BC.cases()["tilted_9x2x30"]
    lat, nb = G.lattice(case.shape), NB.n_bricks(case.shape)
    coarse = torch.from_numpy(case.coarse).to(dev)
    state, fill = _guarded((1,) + nb, torch.int32, dev), _guarded((1,) + nb, torch.float32, dev)
    for band in (-1.0, -1e-30, NAN):
        with pytest.raises(amd.SnrError):
            amd.ops.band_classify(coarse, lat, case.level, band, state[1], fill[1])
    assert _is_sentinel(state[1]) and _is_sentinel(fill[1]) and _intact(state, fill)
    amd.ops.band_classify(coarse, lat, case.level, 0.0, state[1], fill[1])
    want_state, want_fill = _classified(case)
    assert np.array_equal(state[1].cpu().numpy(), want_state) and BC.same_bits(fill[1].cpu().numpy(), want_fill).all()

    grid_h = _first_grid(case, want_state, want_fill)
    grid = torch.from_numpy(grid_h).to(dev)
    bricks, n_new = _guarded((want_state.size, 4), torch.int32, dev), _guarded((1,), torch.int32, dev)
    for stamp in (1, 0, -3):
        with pytest.raises(amd.SnrError):
            amd.ops.band_seam(grid, lat, case.level, stamp, state[1], bricks[1], n_new[1])
    assert np.array_equal(state[1].cpu().numpy(), want_state) and _is_sentinel(bricks[1]) and _is_sentinel(n_new[1])
    assert _intact(state, bricks, n_new)
    _check_seam(amd, dev, case, grid_h, want_state, 2)
