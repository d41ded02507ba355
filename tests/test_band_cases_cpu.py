"""The narrow-band cases of tests/band_cases.py on the host: every case is what its name says (counts of bricks and rounds, so that none
silently becomes empty), and the cases tell the rules of tests/band_restatement.py from each wrong rule planted there -- the restatement with
the mistake, handed to the comparison the GPU tests use, is rejected by the case made for it.  The wrong rules live in the restatement
alone: no kernel is ever built with one."""
import numpy as np
import pytest

import band_cases as BC
import band_restatement as NB


_want = BC.wanted


# (bricks of the object, bricks evaluated, growth rounds) of the single-object cases
COUNTS = {
    "tilted_2x2x2": (1, 1, 0), "tilted_8x8x8": (1, 1, 0), "tilted_2x9x3": (2, 2, 0), "tilted_9x2x30": (8, 6, 1), "tilted_9x9x9": (8, 6, 1),
    "tilted_16x17x8": (6, 6, 1), "tilted_17x17x17": (27, 16, 1), "tilted_23x40x61": (120, 63, 1),
    "sphere_61x40x23": (120, 47, 1), "torus_61x40x23": (120, 58, 1), "two_spheres_61x40x23": (120, 30, 3),
    "sphere_45x50x39": (210, 51, 1), "torus_45x50x39": (210, 86, 1), "two_spheres_45x50x39": (210, 46, 1),
    "sphere_30x33x26": (80, 28, 1), "torus_30x33x26": (80, 31, 2), "two_spheres_30x33x26": (80, 21, 3),
    "seed_tilted": (120, 86, 3), "seed_torus": (210, 51, 7), "seed_diagonal": (120, 15, 2),
    "tie_plane": (75, 30, 0),
    "small_sphere_band_0": (125, 0, 0), "small_sphere_band_0.02": (125, 0, 0), "small_sphere_band_0.05": (125, 27, 0),
    "small_sphere_band_boundary": (125, 27, 0),
    "coarse_non_finite": (8, 3, 0),
    "dense_pinf": (80, 30, 1), "dense_nan": (80, 28, 1), "dense_ninf": (80, 28, 1),
}


def test_every_case_is_counted_and_small():
    cases = BC.cases()
    assert set(cases) == set(COUNTS) | {"batch_of_four"}
    for c in cases.values():
        assert max(c.shape) <= 61 and min(c.shape) >= 2 and c.dense.shape[0] <= 4
        assert c.dense.dtype == c.coarse.dtype == np.float32
        assert c.dense.shape[1:] == c.shape and c.coarse.shape[1:] == tuple(b + 1 for b in NB.n_bricks(c.shape))


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_case_counts(name):
    w = _want(name)
    assert (w.state[0].size, w.evaluated, w.rounds) == COUNTS[name]
    assert w.evaluated == int((w.state != 0).sum()) and w.rounds == max(int(w.state.max()) - 1, 0)
    assert sum(len(l) for l in w.lists) == w.evaluated
    assert BC.differences(w, w) == []


def test_non_cubic_cases_have_different_brick_counts_on_axes_1_and_2():
    for shape in BC.NON_CUBIC + ((23, 40, 61), (16, 17, 8), (9, 2, 30), (2, 9, 3)):
        nb = NB.n_bricks(shape)
        assert nb[1] != nb[2], shape


def test_batch_of_four_objects_stop_in_different_rounds():
    c, w = BC.cases()["batch_of_four"], _want("batch_of_four")
    assert [int(s.max()) - 1 if s.any() else 0 for s in w.state] == [1, 0, 3, 0] and w.rounds == 3
    assert [int((s != 0).sum()) for s in w.state] == [47, 0, 30, 0]
    assert (w.fill[1] == -1).all() and (w.grid[1] == -1).all()                 # all outside
    assert (w.fill[3] == 1).all() and (w.grid[3] == 1).all()                   # all inside: the fill is the largest corner, here any
    sphere = NB.classify(c.coarse[0], 0.0)[1]
    assert (sphere[w.state[0] == 0] > 0).any()                                 # ... and the sphere has all-inside bricks of unequal corners


def test_seeded_cases_grow_for_at_least_two_rounds():
    for name in ("seed_tilted", "seed_torus", "seed_diagonal"):
        c, w = BC.cases()[name], _want(name)
        assert int(c.initial.sum()) == 1 and int((w.state == 1).sum()) == 1
        assert w.rounds >= 2 and w.evaluated > 2


def test_tie_plane_is_active_through_the_tie_alone():
    c, w = BC.cases()["tie_plane"], _want("tie_plane")
    assert c.band == 0.0 and int((c.coarse == 0).sum()) == 24
    corners = np.stack([NB.corner_values(c.coarse[0], q) for q in range(8)], -1)
    one_sided = (corners > 0).sum(-1) % 8 == 0
    assert int(((w.state[0] == 1) & one_sided).sum()) == 15                    # no corner inside, 4 at the level
    assert w.state[0][1].all() and w.state[0][2].all() and not w.state[0][0].any() and not w.state[0][3:].any()


def test_small_sphere_is_found_from_the_boundary_band_on():
    dense, coarse, nearest = BC.small_sphere()
    assert int((dense > 0).sum()) == 27 and 0.02 < nearest < 0.05
    corners = np.stack([NB.corner_values(coarse, q)[BC.SMALL_SPHERE_BRICK] for q in range(8)])
    assert np.float32(nearest) == np.abs(corners).min() and (corners < 0).all()
    for name, found in (("0", False), ("0.02", False), ("0.05", True), ("boundary", True)):
        c, w = BC.cases()["small_sphere_band_" + name], _want("small_sphere_band_" + name)
        assert np.float32(c.band) == np.float32({"0": 0.0, "0.02": 0.02, "0.05": 0.05, "boundary": nearest}[name])
        assert int((w.grid > 0).sum()) == (27 if found else 0)
        assert bool(w.state[0][BC.SMALL_SPHERE_BRICK]) == found


def test_non_finite_corners_are_active_and_fill_nan():
    c, w = BC.cases()["coarse_non_finite"], _want("coarse_non_finite")
    assert np.isposinf(c.coarse[0, 0, 0, 0]) and np.isneginf(c.coarse[0, 0, 2, 0]) and np.isnan(c.coarse[0, 2, 2, 2])
    active = w.state[0] == 1
    assert active[0, 0, 0] and active[0, 1, 0] and active[1, 1, 1] and int(active.sum()) == 3
    assert np.isnan(w.fill[0][active]).all() and (w.fill[0][~active] == -1).all()


def test_non_finite_dense_point_sits_on_the_boundary_of_the_band():
    clean = _want("sphere_30x33x26")
    points = BC.boundary_points(clean.state[0])
    assert len(points) == 512 and BC.BOUNDARY_POINT in points
    for name, v in (("pinf", np.inf), ("nan", np.nan), ("ninf", -np.inf)):
        c, w = BC.cases()["dense_" + name], _want("dense_" + name)
        changed = ~BC.same_bits(c.dense, BC.cases()["sphere_30x33x26"].dense)
        assert int(changed.sum()) == 1 and changed[(0,) + BC.BOUNDARY_POINT]
        assert BC.same_bits(w.grid[(0,) + BC.BOUNDARY_POINT], np.float32(v)).all()
        assert not c.finite
        if name == "pinf":                                                     # inside: its edges into the filled brick cross the level
            assert w.evaluated == 30 and (clean.state[0] != 0)[w.state[0] != 0].sum() == 28
        else:                                                                  # NaN and -inf count as outside, like the fill next to them
            assert np.array_equal(w.state, clean.state)


def test_found_cases_mesh_like_their_dense_fields():
    """What decides the mesh: which points are inside, and the values at both ends of every crossing edge.  Where a case says ``found``
    the restated grid has the dense field's; the other finite cases are the documented miss (the mesh is empty, the dense one is not)."""
    for name, c in BC.cases().items():
        w = _want(name)
        assert c.finite == bool(np.isfinite(c.dense).all() and np.isfinite(c.coarse).all()) and (c.finite or not c.found), name
        if not c.finite:
            continue
        inside, dense_inside = w.grid > np.float32(c.level), c.dense > np.float32(c.level)
        if not c.found:
            assert dense_inside.any() and not inside.any(), name
            continue
        assert np.array_equal(inside, dense_inside), name
        for a, b in NB._edges(c.shape):
            a, b = (slice(None),) + a, (slice(None),) + b
            cross = inside[a] != inside[b]
            assert BC.same_bits(w.grid[a], c.dense[a])[cross].all() and BC.same_bits(w.grid[b], c.dense[b])[cross].all(), name


# wrong rule -> the cases named for it, which must reject it, and with which words of ``differences``
REJECTED_BY = {
    "swap_axes": {"tilted_9x2x30": "grid", "tilted_16x17x8": "state", "tilted_23x40x61": "state", "sphere_61x40x23": "state",
                  "torus_45x50x39": "state", "two_spheres_30x33x26": "state", "batch_of_four": "state"},
    "near_strict": {"tie_plane": "state", "small_sphere_band_boundary": "state"},
    "no_near": {"small_sphere_band_0.05": "state"},
    "fill_smallest": {"batch_of_four": "fill"},
    "no_diagonal": {"seed_diagonal": "state"},
    "order": {"seed_tilted": "state", "seed_torus": "state"},
}
# ... and cases that cannot see it: where nb1 = nb2, below the band, without an all-inside brick
BLIND = {
    "swap_axes": ("tilted_9x9x9", "tilted_17x17x17", "small_sphere_band_0.05"),
    "near_strict": ("small_sphere_band_0.02", "small_sphere_band_0.05", "sphere_30x33x26"),
    "no_near": ("small_sphere_band_0", "small_sphere_band_0.02"),
    "fill_smallest": ("two_spheres_30x33x26", "small_sphere_band_0.05"),
    "no_diagonal": ("seed_tilted", "tilted_9x9x9"),
    "order": ("tilted_9x9x9", "sphere_30x33x26"),                              # one growth round, then nothing: no order to depend on
}


@pytest.mark.parametrize("wrong", sorted(REJECTED_BY))
def test_planted_mistake_is_rejected_by_its_cases(wrong):
    for name, word in REJECTED_BY[wrong].items():
        case = BC.cases()[name]
        diff = BC.differences(BC.restated(case, wrong), _want(name))
        assert word in diff, (wrong, name, diff)
        with pytest.raises(AssertionError):
            BC.compare(BC.restated(case, wrong), _want(name))
    for name in BLIND[wrong]:
        assert BC.differences(BC.restated(BC.cases()[name], wrong), _want(name)) == [], (wrong, name)


def test_every_planted_mistake_has_a_case():
    assert set(REJECTED_BY) | {"no_stamp_test"} == set(NB.WRONG)


def test_counting_an_activated_brick_as_evaluated_changes_nothing_by_itself():
    """A finding, kept as a test.  Dropping ``state < stamp`` from "evaluated" while the brick's points stay filled (threads in index order)
    activates the same bricks: an edge is skipped only when both ends are evaluated or already activated, and every other crossing edge
    still activates each end of state 0.  The order dependence the stamp rules out is the one of "order": a brick whose values change
    within the round."""
    for name in ("seed_tilted", "seed_diagonal", "two_spheres_30x33x26", "tilted_9x2x30"):
        assert BC.differences(BC.restated(BC.cases()[name], "no_stamp_test"), _want(name)) == [], name


def test_comparison_sees_each_field():
    w = _want("tilted_9x9x9")

    def flip(a, at):
        b = a.copy()
        b[at] += 1
        return b

    assert BC.differences(w._replace(state=flip(w.state, (0, 0, 0, 0))), w) == ["state", "lists"]
    at = tuple(np.argwhere(w.state == 0)[0])
    assert BC.differences(w._replace(fill=flip(w.fill, at)), w) == ["fill"]
    assert BC.differences(w._replace(fill=flip(w.fill, tuple(np.argwhere(w.state != 0)[0]))), w) == []   # an evaluated brick's fill is unused
    assert BC.differences(w._replace(grid=-w.grid), w) == ["grid"]
    assert BC.differences(w._replace(rounds=w.rounds + 1), w) == ["rounds"]
    assert BC.differences(w._replace(evaluated=w.evaluated + 1), w) == ["evaluated"]
    first = np.asarray(w.lists[0])
    for lists in ((first[::-1],) + w.lists[1:], ):                             # another order: the same set
        assert BC.differences(w._replace(lists=lists), w) == []
    twice = np.concatenate([first[:-1], first[:1]])                            # a brick twice, one missing
    past = np.concatenate([first[:-1], [[0, 2, 0, 0]]])                        # a brick out of range
    for lists in ((twice,) + w.lists[1:], (past,) + w.lists[1:], (first[:-1],) + w.lists[1:], w.lists[:1], w.lists + (first[:0],)):
        assert BC.differences(w._replace(lists=lists), w) == ["lists"]
    zero = np.zeros((1, 2, 2, 2), np.float32)
    assert not BC.same_bits(zero, -zero).any() and BC.same_bits(zero * np.nan, -zero * np.nan).all()
