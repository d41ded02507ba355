"""The stand-alone composite's seams without a GPU.

a. ``ops.composite_fwd`` / ``ops.composite_bwd`` refuse operands whose sizes the kernels would read past (``ops._composite_shapes``):
   the check runs before any launch, so CPU tensors show it -- and correct shapes on the CPU still meet "need tensors on the GPU".
b. The judgement of tests/unfused_seam_cases.py, which tests/test_unfused_seams_gpu.py applies to the kernels, sees the mistakes it is
   there for: torch restatements of a kernel that is wrong at one seam each are flagged on the smallest shape that shows the seam, and
   the fp32 oracle passes every one of those judgements."""
import pytest
import torch

import unfused_seam_cases as SC


@pytest.fixture(scope="module")
def ops():
    from supnerf_amd import ops
    return ops


# ------------------------------------------------------------------ a. the shape checks
N, S = 6, 8


def operands(n=N, s=S):
    return torch.rand(n, s), torch.rand(n, s, 3), torch.rand(n, s)


def grads(n=N):
    return torch.rand(n, 3), torch.rand(n), torch.rand(n)


def test_correct_shapes_reach_the_gpu_check(ops):
    sig, rgbs, z = operands()
    calls = [(sig, rgbs, z[0], ops.Z_SHARED, 0), (sig, rgbs, z, ops.Z_PER_RAY, 0), (sig, rgbs, z[:2], ops.Z_PER_OBJECT, 3),
             (sig.reshape(2, 3, S), rgbs.reshape(2, 3, S, 3), z[:2].reshape(2, 1, S), ops.Z_PER_OBJECT, 3),     # (B, n, S), as utils._composite passes
             (sig[..., None], rgbs, z, ops.Z_PER_RAY, 0)]
    for s, r, zz, mode, rpo in calls:
        with pytest.raises(ops.SnrError, match="need tensors on the GPU"):
            ops.composite_fwd(s, r, zz, mode, False, rpo)
        for g in (grads(), (None, None, None), (grads()[0], None, grads()[2].reshape(2, 3))):
            with pytest.raises(ops.SnrError, match="need tensors on the GPU"):
                ops.composite_bwd(s, r, zz, mode, False, rpo, *g, mode == ops.Z_PER_RAY)
    # an empty packet is legal whatever its depth table holds (nothing is launched); on the CPU it reaches the same refusal
    with pytest.raises(ops.SnrError, match="need tensors on the GPU"):
        ops.composite_fwd(torch.empty(0, S), torch.empty(0, S, 3), torch.rand(S), ops.Z_SHARED, False)
    with pytest.raises(ops.SnrError, match="need tensors on the GPU"):
        ops.composite_fwd(torch.empty(0, S), torch.empty(0, S, 3), torch.empty(0, S), ops.Z_PER_OBJECT, False, 0)


def shape_text(t):
    import re
    return re.escape(str(tuple(t.shape)))


MISMATCHES = [
    # (name, sigmas, rgbs, z_vals, mode, rays_per_obj, the operand whose shape the message must name)
    ("rgbs without three colours", lambda sig, rgbs, z: (sig, rgbs[..., :2], z, "per_ray", 0, 1)),
    ("rgbs without a sample axis", lambda sig, rgbs, z: (sig, torch.rand(3), z, "per_ray", 0, 1)),
    ("sigmas one sample short", lambda sig, rgbs, z: (sig[:, :-1], rgbs, z, "per_ray", 0, 0)),
    ("sigmas one ray short", lambda sig, rgbs, z: (sig[:-1], rgbs, z, "per_ray", 0, 0)),
    ("shared depths one short", lambda sig, rgbs, z: (sig, rgbs, z[0, :-1], "shared", 0, 2)),
    ("shared depths given per ray", lambda sig, rgbs, z: (sig, rgbs, z, "shared", 0, 2)),
    ("per-ray depths one ray short", lambda sig, rgbs, z: (sig, rgbs, z[:-1], "per_ray", 0, 2)),
    ("per-ray depths given shared", lambda sig, rgbs, z: (sig, rgbs, z[0], "per_ray", 0, 2)),
    ("per-object depths one object short", lambda sig, rgbs, z: (sig, rgbs, z[:1], "per_object", 3, 2)),
    ("per-object depths one object long", lambda sig, rgbs, z: (sig, rgbs, z[:3], "per_object", 3, 2)),
]


@pytest.mark.parametrize("name,make", MISMATCHES, ids=[m[0] for m in MISMATCHES])
def test_a_short_operand_is_refused_by_name(ops, name, make):
    *ts, mode, rpo, named = make(*operands())
    z_mode = {"shared": ops.Z_SHARED, "per_object": ops.Z_PER_OBJECT, "per_ray": ops.Z_PER_RAY}[mode]
    with pytest.raises(ops.SnrError, match=shape_text(ts[named])) as e:
        ops.composite_fwd(*ts, z_mode, False, rpo)
    assert "composite_fwd" in str(e.value) and "GPU" not in str(e.value)
    with pytest.raises(ops.SnrError, match=shape_text(ts[named])) as e:
        ops.composite_bwd(*ts, z_mode, False, rpo, *grads(), False)
    assert "composite_bwd" in str(e.value) and "GPU" not in str(e.value)


@pytest.mark.parametrize("rpo", [0, -1, 4, 5, 7])
def test_per_object_rays_must_tile_the_packet(ops, rpo):
    """B * rays_per_obj == n_rays with rays_per_obj >= 1: 6 rays in objects of 0, -1, 4, 5 or 7 are none of that."""
    sig, rgbs, z = operands()
    for zz in (z[:1], z[:2], z):
        with pytest.raises(ops.SnrError, match=f"rays_per_obj {rpo} for {N} rays"):
            ops.composite_fwd(sig, rgbs, zz, ops.Z_PER_OBJECT, False, rpo)
        with pytest.raises(ops.SnrError, match=f"rays_per_obj {rpo} for {N} rays"):
            ops.composite_bwd(sig, rgbs, zz, ops.Z_PER_OBJECT, False, rpo, *grads(), False)


@pytest.mark.parametrize("which,bad", [(0, torch.rand(N, 2)), (0, torch.rand(N - 1, 3)), (1, torch.rand(N + 1)), (1, torch.rand(N, 3)), (2, torch.rand(N - 1)),
                                       (2, torch.rand(1))])
def test_upstream_gradients_are_counted(ops, which, bad):
    sig, rgbs, z = operands()
    g = list(grads())
    g[which] = bad
    with pytest.raises(ops.SnrError, match=("d_rgb", "d_depth", "d_acc")[which] + " " + shape_text(bad)):
        ops.composite_bwd(sig, rgbs, z, ops.Z_PER_RAY, True, 0, *g, True)


# ------------------------------------------------------------------ b. the judgement sees a kernel that is wrong at one seam
def flagged(tag, got, r32, r64, sig):
    """The judgement's complaint about ``got``, or None."""
    try:
        SC.judge(tag, got, r32, r64, sig)
    except AssertionError as e:
        return str(e)
    return None


def case(Nr, Sr, mode, rpo, seed, white=True):
    sig, rgbs, z, wts = SC.seam_inputs(Nr, Sr, seed)
    zt = SC.depth_table(z, mode, rpo)
    return (sig, rgbs, zt, wts, mode, rpo, white), SC.references(sig, rgbs, zt, wts, mode, rpo, white)


SEAMS = [
    # (mistake, rays, samples, depth layout, rays per object, restatement arguments)
    ("last_interval_at_lane_15", 1, 12, "per_ray", 0, {}),
    ("last_interval_at_lane_15", 1, 12, "shared", 0, {}),
    ("group_takes_its_first_rays_object", 6, 4, "per_object", 3, {}),          # ray 3 of group 0 belongs to object 1
    ("ray_dropped", 7, 4, "per_ray", 0, dict(dropped=3)),                      # the fourth ray of the full group
    ("ray_dropped", 7, 4, "per_ray", 0, dict(dropped=6)),                      # the third, last ray of the partial group 4 .. 6
    ("ray_dropped", 7, 4, "shared", 0, dict(dropped=6)),
    ("negative_density_gradient", 3, 8, "per_ray", 0, {}),
    ("trip_not_written", 8 + 5, 4, "per_ray", 0, dict(sweep=8)),               # one full group and one ray in the second trip
    ("trip_repeats_the_first", 8 + 5, 4, "per_ray", 0, dict(sweep=8)),
    ("trip_repeats_the_first", 8 + 5, 4, "shared", 0, dict(sweep=8)),
]


@pytest.mark.parametrize("wrong,Nr,Sr,mode,rpo,kw", SEAMS, ids=[f"{s[0]}-N{s[1]}-S{s[2]}-{s[3]}" + "".join(f"-{v}" for v in s[5].values()) for s in SEAMS])
def test_the_judgement_flags_each_mistake(wrong, Nr, Sr, mode, rpo, kw):
    args, (r32, r64) = case(Nr, Sr, mode, rpo, 7)
    sig = args[0]
    # the premises: a negative density to zero the gradient of, a last sample dense enough for its interval to matter
    assert bool((sig < 0).any()) or wrong != "negative_density_gradient"
    assert bool((sig[:, -1] > 0.1).all()) or wrong != "last_interval_at_lane_15"
    right = SC.restated(*args)
    assert flagged("right", right, r32, r64, sig) is None
    for backward in (True, False):                               # the forward alone (what the grid-stride and long-ray tests hold) as well
        if wrong == "negative_density_gradient" and not backward:
            continue
        got = SC.restated(*args, wrong=wrong, backward=backward, **kw)
        said = flagged(wrong, got, r32, r64, sig)
        print(f"[{wrong} N={Nr} S={Sr} {mode} backward={backward}] {said}")
        assert said is not None, (wrong, backward)


def test_the_zero_gradient_rule_stands_on_its_own():
    """A d_sigma that is a rounding away from 0.0 on a negative density is inside every band; the rule is exact."""
    args, (r32, r64) = case(5, 8, "per_ray", 0, 3)
    sig = args[0]
    got = SC.restated(*args)
    neg = torch.nonzero(sig < 0)
    zero = torch.nonzero(sig == 0)
    assert len(neg) and len(zero)
    for where in (neg[0], zero[0]):
        g = {k: (v.clone() if v is not None else None) for k, v in got.items()}
        g["d_sigma"][tuple(where)] = 1e-30
        assert SC.zero_gradient_violations(g["d_sigma"], sig) == [where.tolist()]
        said = flagged("tiny", g, r32, r64, sig)
        assert said is not None and "sigma <= 0" in said
    wrong = SC.restated(*args, wrong="negative_density_gradient")
    bad = SC.zero_gradient_violations(wrong["d_sigma"], sig)
    assert all(w.tolist() in bad for w in neg)


def test_position_independence_sees_a_slot_dependent_ray():
    args, _ = case(11, 12, "per_ray", 0, 5)
    base = SC.restated(*args)
    for shift in (1, 2, 3):
        perm = torch.arange(11).roll(shift)
        moved_args = [a[perm] if torch.is_tensor(a) else a for a in args[:3]] + [[w[perm] for w in args[3]], *args[4:]]
        moved = SC.restated(*moved_args)
        assert SC.position_mismatches(base, moved, perm) == []
        # slot 3 of every group of four sums its colours in another order: one rounding, far inside the band
        for k in ("rgb", "d_rgbs"):
            odd = {n: (v.clone() if v is not None else None) for n, v in moved.items()}
            odd[k][3::4] = torch.nextafter(odd[k][3::4], torch.full_like(odd[k][3::4], 10.0))
            assert SC.position_mismatches(base, odd, perm) == [k]


def test_trip_comparison_sees_a_second_trip_that_differs():
    sweep = 8
    args, _ = case(sweep + 5, 4, "per_ray", 0, 9)
    got = SC.restated(*args)
    tail_args = [a[sweep:] for a in args[:3]] + [[w[sweep:] for w in args[3]], *args[4:]]
    head = SC.restated(*tail_args)
    assert SC.trip_mismatches(got, head, sweep) == []
    rep = SC.restated(*args, wrong="trip_repeats_the_first", sweep=sweep)
    assert set(SC.trip_mismatches(rep, head, sweep)) == {k for k in SC.NAMES if head[k] is not None}
    nan = SC.restated(*args, wrong="trip_not_written", sweep=sweep)
    assert set(SC.trip_mismatches(nan, head, sweep)) == {k for k in SC.NAMES if head[k] is not None}


@pytest.mark.parametrize("Sr", [2, 4, 8, 12, 16, 20, 32, 36, 48, 60, 64, 257, 320])
def test_the_references_are_finite_and_the_fp32_oracle_is_close(Sr):
    """The premise of the inputs: float64 finite throughout, the fp32 oracle within 1.7e-6 of it relative to each tensor's largest entry
    -- so the band, 4 x that + 2e-5, is a few 1e-5 wide, and a ray or an interval that is wrong by its own size cannot hide in it."""
    worst = 0.0
    for Nr in (1, 2, 3, 4, 5, 7, 8, 9):
        sig, rgbs, z, wts = SC.seam_inputs(Nr, Sr, 1000 * Sr + Nr)
        for white in (True, False):
            r32, r64 = SC.references(sig, rgbs, z, wts, "per_ray", 0, white)
            for k in SC.NAMES:
                assert bool(torch.isfinite(r64[k]).all()), (k, Nr)
                worst = max(worst, float((r32[k].double() - r64[k]).abs().max()) / float(r64[k].abs().max()))
    print(f"[S={Sr}] fp32 oracle at most {worst:.2e} from float64")
    assert worst <= 1.7e-6
