"""The box sampler's special rays on the CPU: the table (tests/special_rays.py) is what it claims, the guarded slab test of the oracle is
the plain one with a finite gradient, the bands the GPU tests apply can see the bugs they are for, and the package's torch formulation of
family B (``renderer._box_bounds``) follows the kernels' rule.

The rules (include/supnerf_hip.h at SNR_Z_BOX): (1) a NaN of the slab test, 0 * inf, makes the ray a miss and reaches no output; (2) ties in
maximum / minimum split the gradient evenly like torch's; (3) an axis whose direction component is exactly 0 adds nothing to the gradient
of the bounds, where torch multiplies a zero gradient by the infinite 1/d into a NaN; (4) the comparisons are strict.

Rules 2 and 3 each have a deliberately wrong reference here (``tie_mutant_slab``: tie share 1 / 0; ``whole_ray_drop_slab``: the bounds'
path dropped on the whole ray instead of in the one component) that the per-ray band must catch.  Rule 1 has none, because none is
observable: with NaN-IGNORING fmin / fmax in place of the propagating ones, the on-face axis (o = +-hb, d = +-0: the pair of products is
{NaN, +-inf}) becomes lo = hi = +inf or lo = hi = -inf, so t_near = +inf or t_far = -inf and the ray misses exactly as it does with the NaN
(``test_on_face_nan_is_unobservable`` works the four sign combinations out).  What the tests hold such a ray to is the observable part:
hit == 0, all points at o - d, every value and gradient finite."""
import numpy as np
import pytest
import torch

import special_rays as SR
from oracle import supnerf_oracle as O
from oracle_bands import per_ray_errors

DTYPES = [torch.float32, torch.float64]
PER_RAY_BAND = 1e-3                      # oracle_bands.check_per_ray: a ray passes within 1e-3 of its own largest float64 entry


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("scale", [1.0, 0.5, 0.25])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_table_is_what_it_claims(dt, scale):
    o, d, hb = SR.table_tensors(dt)
    o, hb = o * scale, hb * scale                      # every object's box of ``embed``
    near, far, hit = SR.bounds_of(O.slab_intersect, o, d, hb)
    lo, hi = SR.slab_axes(o, d, hb)
    seen = {c: 0 for c in SR.CLASSES}
    for i, r in enumerate(SR.TABLE):
        seen[r.cls] += 1
        assert bool(hit[i]) == r.hit, r.name
        if r.near is not None:
            assert float(near[i]) == r.near * scale and float(far[i]) == r.far * scale, (r.name, float(near[i]), float(far[i]))
        if not r.hit:
            assert float(near[i]) == -1.0 and float(far[i]) == -1.0, r.name
        if r.cls in ("parallel", "zero_in"):
            assert r.zero_axes == tuple(a for a in range(3) if float(d[i, a]) == 0), r.name
            for a in r.zero_axes:
                assert float(lo[i, a]) == -SR.INF and float(hi[i, a]) == SR.INF and abs(float(o[i, a])) < float(hb[i, a]), (r.name, a)
        if r.cls == "zero_out":
            assert float(lo.amax(1)[i]) == SR.INF or float(hi.amin(1)[i]) == -SR.INF, r.name
        if r.cls == "zero_face":
            assert bool(torch.isnan(lo[i]).any()) and bool(torch.isnan(hi[i]).any()), r.name          # the NaN is there, in the plain test
        if r.cls == "tie":
            which, share = SR.TIES[r.name]
            v, best = (lo[i], lo[i].max()) if which == "lo" else (hi[i], hi[i].min())
            assert [float(v[a]) == float(best) for a in range(3)] == [share[a] > 0 for a in range(3)], (r.name, v.tolist())
        if r.cls == "inside":
            assert float(near[i]) < 0 < float(far[i]), r.name
        if r.cls == "face_in":
            assert float(near[i]) == 0.0 and float(lo[i].max()) == 0.0, r.name
        if r.cls == "behind":
            assert float(hi[i].min()) < 0, r.name
        if r.cls == "graze":
            assert float(lo[i].max()) == float(hi[i].min()) > 0, r.name
    assert all(seen[c] >= 2 for c in SR.CLASSES), seen
    assert len([r for r in SR.TABLE if r.hit]) == 17 and len(SR.TABLE) == 26


def test_on_face_nan_is_unobservable():
    """Rule 1 has no mutant: NaN-ignoring fmin / fmax turn the on-face axis into lo = hi = +-inf and the ray misses as with the NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        for o_x in (0.5, -0.5):
            for d_x in (0.0, -0.0):
                inv = np.float32(1) / np.float32(d_x)
                ta, tb = (np.float32(-0.5) - np.float32(o_x)) * inv, (np.float32(0.5) - np.float32(o_x)) * inv
                assert np.isnan(ta) != np.isnan(tb) and np.isinf(ta if np.isnan(tb) else tb)
                lo, hi = np.fmin(ta, tb), np.fmax(ta, tb)                       # NaN-ignoring
                assert lo == hi and np.isinf(lo)
                t_near, t_far = np.fmax(np.fmax(lo, -2.5), -1.25), np.fmin(np.fmin(hi, 2.5), 3.0)      # any finite other axes
                assert not (t_far > t_near and t_far > 0)                       # a miss: near = far = -1, as with the propagated NaN
                assert not (np.minimum(ta, tb) < np.inf)                        # (the propagating pair: NaN, a miss too)


# ------------------------------------------------------------------ the guarded slab test
def slab_grads(slab, o, d, hb):
    o, d = o.clone().requires_grad_(), d.clone().requires_grad_()
    near, far, hit = SR.bounds_of(slab, o, d, hb)
    (2 * near + 3 * far).sum().backward()
    return near.detach(), far.detach(), hit, o.grad, d.grad


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_guarded_slab_is_the_plain_one_with_a_finite_gradient(dt):
    o, d, hb = SR.table_tensors(dt)
    g = torch.Generator().manual_seed(3)
    ro = torch.randn(10000, 3, generator=g, dtype=dt)
    rd = torch.randn(10000, 3, generator=g, dtype=dt)
    rd[torch.rand(10000, 3, generator=g) < 0.1] = 0.0                           # random rays with zero components too
    o, d = torch.cat([o, ro]), torch.cat([d, rd])
    hb = torch.tensor(SR.HB, dtype=dt).expand_as(o)
    pn, pf, ph, po, pd = slab_grads(O.slab_intersect, o, d, hb)
    gn, gf, gh, go, gd = slab_grads(O.guarded_slab_intersect, o, d, hb)
    assert torch.equal(ph, gh) and torch.equal(pn, gn) and torch.equal(pf, gf)             # bit for bit
    assert bool(torch.isfinite(go).all()) and bool(torch.isfinite(gd).all())
    fin = (torch.isfinite(po) & torch.isfinite(pd)).all(1)
    T = len(SR.TABLE)
    assert int((~fin[:T]).sum()) >= 10 and int(fin[T:].sum()) > 5000
    assert torch.equal(po[fin], go[fin]) and torch.equal(pd[fin], gd[fin])
    assert not bool(go[~gh].any()) and not bool(gd[~gh].any())                             # zeros on the misses
    for i, r in enumerate(SR.TABLE):
        for a in r.zero_axes:
            assert float(go[i, a]) == 0.0 and float(gd[i, a]) == 0.0, r.name               # zeros in the dropped axes
        if r.cls == "tie":                                                                 # d lo_a / d o_a = -1 / d_a, times the axis' share
            which, share = SR.TIES[r.name]
            w = 2.0 if which == "lo" else 3.0
            other = torch.tensor([0.0, 0.0, 0.0], dtype=dt)
            k = int(hi_or_lo_single_axis(o[i], d[i], hb[i], which))
            other[k] = -(5.0 - w) / float(d[i, k])
            want = torch.tensor([-w * share[a] / float(d[i, a]) for a in range(3)], dtype=dt) + other
            assert torch.equal(go[i], want), (r.name, go[i].tolist(), want.tolist())


def hi_or_lo_single_axis(o, d, hb, tied):
    """The axis that alone decides the bound which does NOT tie (the exit of an entry-tie ray, the entry of an exit-tie ray)."""
    lo, hi = SR.slab_axes(o, d, hb)
    v = hi if tied == "lo" else lo
    best = v.min() if tied == "lo" else v.max()
    axes = [a for a in range(3) if float(v[a]) == float(best)]
    assert len(axes) == 1, axes
    return axes[0]


# ------------------------------------------------------------------ the batch
@pytest.mark.parametrize("S,n,B", SR.CASES, ids=lambda v: str(v))
def test_embedding_places_the_table(S, n, B):
    b = SR.embed(n, B, S)
    N = B * n
    assert b.rays_o.shape == (N, 3) and b.jitter.shape == (N, S) and b.half.shape == (B, 3)
    assert len(set(map(tuple, b.half.tolist()))) == B and len(set(b.z_scale.tolist())) == B            # different boxes, different scales
    zs, h = b.z_scale.repeat_interleave(n)[:, None], b.half.repeat_interleave(n, 0)
    for dt in DTYPES:
        o_n = b.rays_o.to(dt) / zs.to(dt)
        assert torch.equal((o_n * zs.to(dt)), b.rays_o.to(dt))                                       # the division is exact
        near, far, hit = SR.bounds_of(O.slab_intersect, o_n, b.rays_d.to(dt), h.to(dt))
        for s in b.special:
            assert bool(hit[s.index]) == s.ray.hit, s
            if s.ray.near is not None:
                assert float(near[s.index]) == s.ray.near * s.scale and float(far[s.index]) == s.ray.far * s.scale, s
            assert float(b.jitter[s.index, 0]) == 0.0
    n_l, r128, r64 = SR.launch_rays(n, S), max(128 // S, 1), max(64 // S, 1)
    pos = {s.obj * n_l + s.local for s in b.special}
    assert any(p % r128 == 0 for p in pos) and any(p % r128 == r128 - 1 for p in pos)
    assert any(p % r64 == 0 for p in pos) and any(p % r64 == r64 - 1 for p in pos)
    assert any(s.local == 0 for s in b.special) and any(s.local == n - 1 for s in b.special)
    counts = SR.count_by_class(b, [s.index for s in b.special])
    assert all(counts[c] >= 2 for c in SR.CLASSES), counts
    generic = sorted(set(range(N)) - {s.index for s in b.special})
    assert bool((b.rays_d[generic] != 0).all())                                                      # generic rays are generic
    assert bool((b.jitter == 0).sum() > len(b.special))


# ------------------------------------------------------------------ the bands can see what the GPU tests are for
@pytest.mark.parametrize("S,n,B", SR.CASES, ids=lambda v: str(v))
def test_mutants_of_the_reference_are_caught(oracle_params, S, n, B):
    """On the inputs of every GPU case, float64: the 1 / 0 tie share moves d_rays_o / d_rays_d of EVERY tie ray, and the whole-ray drop
    those of EVERY hit ray with a zero component, by at least 10x the per-ray band of ``check_per_ray``; no other ray moves at all."""
    case = SR.case_inputs(n, B, S)
    b = case.batch
    true = SR.oracle_render(oracle_params, case, torch.float64)
    for name, slab, pred in (("tie 1/0", SR.tie_mutant_slab, lambda s: s.ray.cls == "tie"),
                             ("whole-ray drop", SR.whole_ray_drop_slab, lambda s: s.ray.hit and len(s.ray.zero_axes) > 0)):
        wrong = SR.oracle_render(oracle_params, case, torch.float64, slab=slab)
        for k in ("rgb", "depth", "acc"):
            assert torch.equal(wrong[k], true[k]), (name, k)                                # the same function, a wrong derivative
        idx, names = SR.rays_of(b, pred)
        assert len(idx) >= (5 if name == "tie 1/0" else 8) * (B if n >= len(SR.TABLE) else 1), (name, names)
        moved = torch.zeros(B * n, dtype=torch.bool)
        for g in ("d_rays_o", "d_rays_d"):
            err, _ = per_ray_errors(wrong[g], true[g], true[g])
            moved |= err > 0
            print(f"[{name}] {g}: " + ", ".join(f"{nm} {float(err[i]):.1%}" for i, nm in zip(idx, names)))
            assert bool((err[idx] >= 10 * PER_RAY_BAND).all()), (name, g, [(nm, float(err[i])) for i, nm in zip(idx, names)])
        assert sorted(torch.nonzero(moved).flatten().tolist()) == sorted(idx), name


def test_on_face_and_miss_rays_render_finite(oracle_params):
    """The observable part of rule 1 on the oracle's side: the on-face rays are misses, their points lie at o - d, and with the guarded
    slab test every output and gradient of the batch is finite (with the plain one the gradient is not)."""
    case = SR.case_inputs(32, 3, 8)
    b = case.batch
    out = SR.oracle_render(oracle_params, case, torch.float64)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    plain = SR.oracle_render(oracle_params, case, torch.float64, slab=O.slab_intersect)
    assert not bool(torch.isfinite(plain["d_rays_o"]).all())
    idx, _ = SR.rays_of(b, lambda s: s.ray.cls == "zero_face")
    assert len(idx) == 9
    zs, h = b.z_scale.repeat_interleave(b.n)[:, None], b.half.repeat_interleave(b.n, 0)
    o_n = b.rays_o / zs
    near, far, hit = SR.bounds_of(O.guarded_slab_intersect, o_n, b.rays_d, h)
    t = O.unit_interval_samples(near[:, None], far[:, None], b.S, b.jitter)
    xyz = o_n[:, None] + b.rays_d[:, None] * t[:, :, None]
    assert not bool(hit[idx].any()) and torch.equal(xyz[idx], (o_n - b.rays_d)[idx][:, None].expand(-1, b.S, -1))


# ------------------------------------------------------------------ the package's torch formulation of family B
WLH = np.asarray([1.9, 4.6, 1.5], dtype=np.float32)        # a car, float32 like the datasets' sizes: half extents (l, w, h) / diag, not dyadic


def table_for_box(half, dtype=torch.float32):
    """The table's rays moved to the box ``half`` (3,), axis by axis: origins on a face stay on it exactly, zeros stay zeros."""
    o, d, hb = SR.table_tensors(dtype)
    k = half.to(dtype)[None, :]
    return (o / hb) * k, (d / hb) * k


def test_box_bounds_keep_their_bits():
    import supnerf_amd as A
    from supnerf_amd import renderer as R
    o, d, hb = SR.table_tensors()
    g = torch.Generator().manual_seed(5)
    ro = torch.randn(10000, 3, generator=g)
    aim = (torch.rand(10000, 3, generator=g) * 2 - 1) * torch.tensor(SR.HB) * 1.5
    rd = torch.nn.functional.normalize(aim - ro, dim=-1)                 # about half of them meet the box
    rd[torch.rand(10000, 3, generator=g) < 0.1] = 0.0
    o, d = torch.cat([o, ro]), torch.cat([d, rd])
    l, w, h = SR.HB                                                      # _box_bounds: half = (l, w, h) / diag
    near, far, hit = R._box_bounds(o, d, (w, l, h), 1.0)
    hb = torch.tensor(SR.HB).expand_as(o)
    tn, tf, want = A.utils._slab(o, d, -hb, hb)
    m1 = torch.full_like(tn, -1.0)
    assert torch.equal(hit, want) and int(hit.sum()) > 1000 and int((~hit).sum()) > 1000
    assert torch.equal(near[:, 0], torch.where(want, tn, m1)) and torch.equal(far[:, 0], torch.where(want, tf, m1))
    # the public slab test stays the reference's line for line: NaN gradient and all
    o1, d1 = o[:1].clone().requires_grad_(), d[:1].clone().requires_grad_()
    zi, zo, _ = A.utils.ray_box_intersection_tensor(o1, d1, -hb[:1], hb[:1])
    (zi + zo).sum().backward()
    assert not bool(torch.isfinite(o1.grad).all())


def sampled_grads(fn, rays_o, viewdir):
    ro, vd = rays_o.clone().requires_grad_(), viewdir.clone().requires_grad_()
    xyz, _, z_vals, hit = fn(ro, vd)
    (xyz.sum() + z_vals.sum()).backward()
    return xyz.detach(), z_vals.detach(), hit, ro.grad, vd.grad


def test_prepare_sampled_rays_gradient_follows_the_kernels_rule():
    import supnerf_amd as A
    S = 8
    diag = np.linalg.norm(WLH).astype(np.float32)
    w, l, h = [float(v) for v in WLH]
    half = torch.tensor([l / diag, w / diag, h / diag], dtype=torch.float32)
    o_n, d = table_for_box(half)
    rays_o = o_n * float(diag / 2)
    jit = torch.rand(len(SR.TABLE), S, generator=torch.Generator().manual_seed(1))
    jit[:, 0] = 0.0
    rend = A.NeRFRenderer(n_samples=S)
    with A.utils.jitter_override(jit):
        got = sampled_grads(lambda ro, vd: rend.prepare_sampled_rays(ro, vd, WLH), rays_o, d)
    want = sampled_grads(lambda ro, vd: O.aabb_sampled_rays(ro, vd, WLH, S, jit, slab=O.guarded_slab_intersect), rays_o, d)
    plain = sampled_grads(lambda ro, vd: O.aabb_sampled_rays(ro, vd, WLH, S, jit), rays_o, d)          # the plain formula, as the reference differentiates it
    assert torch.equal(got[2], want[2]) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    hits = {r.name: bool(hh) for r, hh in zip(SR.TABLE, got[2])}
    assert all(hits[r.name] for r in SR.TABLE if r.cls in ("parallel", "zero_in", "inside")), hits
    assert not any(hits[r.name] for r in SR.TABLE if r.cls in ("zero_out", "behind")), hits
    for k, name in ((3, "d_rays_o"), (4, "d_viewdir")):
        assert bool(torch.isfinite(got[k]).all()), name
        scale = want[k].abs().amax(1, keepdim=True).clamp_min(1e-6)
        assert float(((got[k] - want[k]).abs() / scale).max()) < 1e-5, name                          # float32 rounding of the same formula
        fin = torch.isfinite(plain[k]).all(1)
        assert 4 <= int(fin.sum()) < len(SR.TABLE), int(fin.sum())                                   # the plain formula: NaN on the zero-component rays
        assert float(((got[k] - plain[k]).abs() / scale)[fin].max()) < 1e-5, name


def turntable_case():
    K = torch.tensor([[20.0, 0.0, 16.0], [0.0, 20.0, 12.0], [0.0, 0.0, 1.0]])
    pose = O.turntable_poses(radius=12.0, pan_num=4)[0]                  # pan = 0
    roi = O.virtual_roi(K.numpy(), 12)
    return K, pose, roi


def test_turntable_pose_gradient_is_finite():
    import supnerf_amd as A
    S = 8
    K, pose0, roi = turntable_case()
    jit = torch.rand(144, S, generator=torch.Generator().manual_seed(2))
    ro, vd = O.pixel_rays(K, pose0, roi)
    zero_y = (vd[:, 1] == 0) & (ro[:, 1] == 0)
    assert int(zero_y.sum()) == 12                                       # the column px == cx

    def grad(rays, sampled):
        pose = pose0.clone().requires_grad_()
        o, v = rays(K, pose, roi)
        xyz, _, z_vals, hit = sampled(o, v)
        (xyz.sum() + z_vals.sum()).backward()
        return pose.grad, hit
    rend = A.NeRFRenderer(n_samples=S)
    with A.utils.jitter_override(jit):
        got, hit = grad(A.utils.get_rays, lambda o, v: rend.prepare_sampled_rays(o, v, WLH))
    want, _ = grad(O.pixel_rays, lambda o, v: O.aabb_sampled_rays(o, v, WLH, S, jit, slab=O.guarded_slab_intersect))
    plain, _ = grad(O.pixel_rays, lambda o, v: O.aabb_sampled_rays(o, v, WLH, S, jit))
    assert int(hit[zero_y].sum()) > 0
    assert int((~torch.isfinite(plain)).sum()) == 10, plain                                          # the plain formula: 10 NaNs of 12
    assert bool(torch.isfinite(got).all()), got
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), (got, want)
