"""The box sampler (``SNR_Z_BOX``) on axis-parallel, tied and grazing rays: prologue, forward and backward of every render kernel against
the float32 / float64 oracle, on the table of tests/special_rays.py planted among generic rays.

The rules under test (include/supnerf_hip.h at SNR_Z_BOX; csrc/snr_device.hpp ``box_slab``, ``make_sample``, ``ray_finish``): (1) a NaN of the
slab test (0 * inf) makes the ray a miss and reaches no output; (2) ties in maximum / minimum split the gradient evenly like torch's;
(3) an axis whose direction component is exactly 0 adds NOTHING to the gradient of the bounds (torch's autograd returns NaN there, so the
reference is the oracle's ``guarded_slab_intersect``); (4) strict comparisons.  tests/test_special_rays_cpu.py shows that the bands
applied here catch a 1 / 0 tie share and a bounds' path dropped on the whole ray, on the inputs of every case below.  (Tried on the
kernels themselves: with ``w_gt`` returning 1 / 0 on a tie every backward case fails on its tie rays, 30 % .. 300 % off; without the
``g_tmin != 0`` guards of ``ray_finish`` every case fails the finiteness check on its 8 zero-component hits per object.)

Which kernel and which tail a case (S, rays per object, objects) reaches (``special_rays.CASES``; a change to these predicates moves
the coverage):
* forward: "fp32" runs ``decoder_fwd16_kernel`` (csrc/snr_mlp16.hip), "bf16x3" / "auto" ``bf16_fwd_kernel`` (csrc/snr_bf16.hip) whenever
  points per object % 32 == 0; both call ``make_sample``.  The ragged cases run without padding under no_grad ("auto" resolves to fp32).
* backward "bf16x3" and ("fp32", "bf16x3"): ``bf16_bwd16_kernel`` -> ``ray_grad_tail`` (csrc/snr_device.hpp), always: in-wave finish for
  S in {4, 8, 16, 32}, LDS combine for S in {64, 128}.
* backward "fp32": ``decoder_backward`` (csrc/snr_decoder.hip) takes the two-wave ``decoder_bwd16_kernel`` -> ``ray_grad_tail16``
  (csrc/snr_mlp16_bwd.hip) when points per object % 64 == 0 and S <= 64: (4, 32, 1), (4, 32, 3), (8, 32, 3), (16, 28, 1) finish in the wave
  (S <= 16), (32, 26, 3), (64, 26, 1), (64, 26, 3) combine through LDS; otherwise the round-2 ``decoder_bwd_kernel`` -> ``ray_grad_tail``:
  (4, 40, 3), (8, 28, 1), (16, 26, 3), (32, 27, 3) (points per object % 64 == 32) finish in the wave, (128, 26, 3) and (128, 9, 3) (S = 128)
  combine through LDS.
* ragged: (8, 27, 3) is padded by ``pad_render_inputs`` to 28 rays (224 points: round-2 in fp32), (16, 27, 1) to 28 rays (448 points: two-wave);
  the dummy rays are themselves axis-parallel rays from the box centre, d = (0, 0, 1).
* ``box_detach=True`` (``render_rays_v3``): the same launches with SNR_BOX_DETACH, against the oracle with the bounds detached.

Every check prints, per class of the table, how many special rays it compared, and asserts that none is empty."""
import numpy as np
import pytest
import torch

import special_rays as SR
from oracle import supnerf_oracle as O
from oracle_bands import (amd, band_of, capture_latent, check_all, check_per_object, check_per_ray, dev, make_model,  # noqa: F401
                          md, per_ray_errors)
from relu_bits import relu_bits_of

pytestmark = pytest.mark.gpu

PREC_ID = lambda p: "-".join(p) if isinstance(p, tuple) else p
CASE_ID = lambda c: f"S{c[0]}-n{c[1]}-B{c[2]}"
RAGGED = [c for c in SR.CASES if (c[0] * c[1]) % 32]
WLH = np.asarray([1.9, 4.6, 1.5], dtype=np.float32)        # a car, float32 like the datasets' sizes: half extents (l, w, h) / diag, not dyadic


def compared(batch, idx, what, need=SR.CLASSES):
    """Print and return how many special rays of each class a check compared; the classes in ``need`` must not be empty."""
    counts = SR.count_by_class(batch, [i for i in idx if i in {s.index for s in batch.special}])
    print(f"[{what}] special rays compared: " + ", ".join(f"{c} {k}" for c, k in counts.items()))
    assert all(counts[c] > 0 for c in need), (what, counts)
    return counts


def names_of(batch, rays):
    by = {s.index: f"{s.ray.name} [obj {s.obj} ray {s.local}]" for s in batch.special}
    return [by.get(int(r), f"generic ray {int(r)}") for r in rays]


def oracle_prologue(b):
    """hit, xyz, viewdir, metric z of the batch in float32, the arithmetic of ``aabb_sampled_rays`` per object."""
    zs, h = b.z_scale.repeat_interleave(b.n)[:, None], b.half.repeat_interleave(b.n, 0)
    o_n = b.rays_o / zs
    near, far, hit = SR.bounds_of(O.slab_intersect, o_n, b.rays_d, h)
    t = O.unit_interval_samples(near[:, None], far[:, None], b.S, b.jitter)
    xyz = o_n[:, None, :] + t[:, :, None] * b.rays_d[:, None, :]
    z = torch.norm((xyz - o_n[:, None, :]) * zs[:, :, None], p=2, dim=-1)
    return hit, xyz, b.rays_d[:, None, :].repeat(1, b.S, 1), z, o_n


# ------------------------------------------------------------------ a. the prologue alone
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [4, 8, 16, 32, 64, 128])
def test_prologue_bit_for_bit(amd, dev, S, B):
    ops = amd.ops
    b = SR.embed(32, B, S)
    hit, xyz, vd, z, o_n = oracle_prologue(b)
    cfg = ops.RenderCfg(S, ops.Z_BOX, b.n, 0, 0, metric_z=True, box_half=b.half.to(dev))
    out = ops.encode(b.rays_o.to(dev), b.rays_d.to(dev), b.jitter.to(dev), None, b.z_scale.to(dev), cfg, want_hit=True)
    assert all(bool(torch.isfinite(t).all()) for t in out[:3])
    compared(b, range(B * b.n), f"prologue S={S} B={B}")
    wrong = torch.nonzero(out[3].cpu().bool() != hit).flatten()
    assert wrong.numel() == 0, names_of(b, wrong)
    for name, got, want in (("xyz", out[0], xyz), ("viewdir", out[1], vd), ("z", out[2], z)):
        diff = (got.cpu() != want).reshape(B * b.n, -1).any(1)
        assert md(got, want) == 0.0 and not bool(diff.any()), (name, names_of(b, torch.nonzero(diff).flatten()))
    # what the table promises, on the kernel's own output: misses sit at o - d, a ray from a face starts on it at metric depth 0
    miss, _ = SR.rays_of(b, lambda s: not s.ray.hit)
    assert len(miss) == 9 * B and torch.equal(out[0].cpu()[miss], (o_n - b.rays_d)[miss][:, None, :].expand(-1, S, -1))
    face, _ = SR.rays_of(b, lambda s: s.ray.cls == "face_in")
    assert len(face) == 2 * B and torch.equal(out[0].cpu()[face, 0], o_n[face]) and not bool(out[2].cpu()[face, 0].any())


def test_prepare_sampled_rays_axis_parallel_public_path(amd, dev):
    """``NeRFRenderer.prepare_sampled_rays`` (one encode launch) with a box whose half extents are not dyadic: the table moved to that
    box axis by axis, so its zeros stay zeros and its on-face origins stay on the face."""
    S = 16
    diag = np.linalg.norm(WLH).astype(np.float32)
    w, l, h = [float(v) for v in WLH]
    half = torch.tensor([l / diag, w / diag, h / diag], dtype=torch.float32)
    o, d, hb = SR.table_tensors()
    rays_o, rays_d = (o / hb) * half * float(diag / 2), (d / hb) * half
    jit = torch.rand(len(SR.TABLE), S, generator=torch.Generator().manual_seed(4))
    jit[:, 0] = 0.0
    xyz, vd, z, hit = O.aabb_sampled_rays(rays_o, rays_d, WLH, S, jit)
    par = [i for i, r in enumerate(SR.TABLE) if r.cls == "parallel"]
    assert len(par) == 5 and bool(hit[par].all()) and bool(((rays_d[par] == 0).sum(1) == 2).all())
    rend = amd.NeRFRenderer(n_samples=S)
    with amd.utils.jitter_override(jit):
        out = rend.prepare_sampled_rays(rays_o.to(dev), rays_d.to(dev), WLH)
    assert torch.equal(out[3].cpu(), hit), [r.name for r, a, c in zip(SR.TABLE, out[3].cpu(), hit) if bool(a) != bool(c)]
    assert md(out[0], xyz) == 0.0 and md(out[1], vd) == 0.0 and md(out[2], z) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in out[:3])


# ------------------------------------------------------------------ b. forward of every render kernel
def render_cfg(ops, b, dev, box_detach=False):
    return ops.RenderCfg(b.S, ops.Z_BOX, b.n, 3, 1, white_bkgd=True, metric_z=True, box_half=b.half.to(dev), box_detach=box_detach)


# (a ragged case is not padded under no_grad, and the split kernels take whole 32-point tiles per object: "auto" resolves to fp32 there, and
# an explicit "bf16x3" is refused -- the backward test runs the split kernels on the ragged cases, padded)
FORWARD = [(c, p) for c in SR.CASES for p in ("fp32", "bf16x3", "auto") if not (c in RAGGED and p == "bf16x3")]


@pytest.mark.parametrize("case,precision", FORWARD, ids=lambda v: v if isinstance(v, str) else CASE_ID(v))
def test_forward_in_band_on_every_ray(amd, dev, oracle_params, case, precision):
    S, n, B = case
    c = SR.case_inputs(n, B, S)
    b = c.batch
    m = make_model(amd, dev, oracle_params, precision)
    with torch.no_grad():
        out = m.fused_render(b.rays_o.to(dev), b.rays_d.to(dev), b.jitter.to(dev), torch.ones(B, device=dev), b.z_scale.to(dev),
                             c.codes[0].to(dev), c.codes[1].to(dev), render_cfg(amd.ops, b, dev))
    ran = m.last_precision["forward"]
    assert ran == ("fp32" if precision == "fp32" or case in RAGGED else "bf16x3"), m.last_precision
    r32, r64 = [SR.oracle_render(oracle_params, c, dt) for dt in (torch.float32, torch.float64)]
    for name, got in zip(("rgb", "depth", "acc"), out):
        bad = torch.nonzero(~torch.isfinite(got.cpu()).reshape(B * n, -1).all(1)).flatten()
        assert bad.numel() == 0, (name, names_of(b, bad))
    compared(b, range(B * n), f"forward {CASE_ID(case)} {precision}")
    check_all([(k, g, r32[k], r64[k]) for k, g in zip(("rgb", "depth", "acc"), out)], ran)
    # the miss rays (all samples at t = -1) and the hits separately, each in the same band against its own largest value
    for what, pred in (("miss", lambda s: not s.ray.hit), ("hit", lambda s: s.ray.hit)):
        idx, _ = SR.rays_of(b, pred)
        compared(b, idx, f"forward, {what} rays", need=[cl for cl in SR.CLASSES if any(r.cls == cl and r.hit == (what == "hit") for r in SR.TABLE)])
        check_all([(f"{k} ({what} special rays)", g[idx], r32[k][idx], r64[k][idx]) for k, g in zip(("rgb", "depth", "acc"), out)], ran)


# ------------------------------------------------------------------ c. backward of every render kernel and lane layout
def launch(amd, dev, params, c, precision, box_detach):
    b = c.batch
    m = make_model(amd, dev, params, precision)
    lats = capture_latent(m)
    ro, rd, sc, tc = [x.to(dev).requires_grad_() for x in (b.rays_o, b.rays_d, c.codes[0], c.codes[1])]
    out = m.fused_render(ro, rd, b.jitter.to(dev), torch.ones(b.B, device=dev), b.z_scale.to(dev), sc, tc,
                         render_cfg(amd.ops, b, dev, box_detach))
    masks = relu_bits_of(out[0], 3, 1, n_samples=b.S)
    sum((a * w.to(dev)).sum() for a, w in zip(out, c.wts)).backward()
    got = dict(rgb=out[0].detach(), depth=out[1].detach(), acc=out[2].detach(), d_rays_o=ro.grad, d_rays_d=rd.grad, d_latent=lats[0].grad,
               d_shapecode=sc.grad, d_texturecode=tc.grad)
    return {k: v.cpu() for k, v in got.items()}, masks, (lats[0].detach() > 0).cpu()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", ("fp32", "bf16x3")], ids=PREC_ID)
@pytest.mark.parametrize("case", SR.CASES, ids=CASE_ID)
def test_backward_through_the_bounds(amd, dev, oracle_params, case, precision):
    S, n, B = case
    c = SR.case_inputs(n, B, S)
    b = c.batch
    N = B * n
    band = band_of(precision)
    runs = {}
    for detach in (False, True):
        got, masks, on = launch(amd, dev, oracle_params, c, precision, detach)
        r32, r64 = [SR.oracle_render(oracle_params, c, dt, masks=masks, lat_on=on, box_detach=detach) for dt in (torch.float32, torch.float64)]
        runs[detach] = got
        tag = f"{CASE_ID(case)} {PREC_ID(precision)}" + (" box_detach" if detach else "")
        # every entry of every gradient is finite
        for k in ("d_rays_o", "d_rays_d", "d_latent", "d_shapecode", "d_texturecode"):
            bad = torch.nonzero(~torch.isfinite(got[k]).reshape(got[k].shape[0], -1).all(1)).flatten()
            assert bad.numel() == 0, (tag, k, names_of(b, bad) if k.startswith("d_rays") else bad.tolist())
        compared(b, range(N), f"per-ray gradients {tag}")
        bad = []
        for k in ("d_rays_o", "d_rays_d"):
            for name, rays, err, floor in check_per_ray(f"{k} {tag}", got[k], r32[k], r64[k]):
                bad.append((name, list(zip(names_of(b, rays), err, floor))))
        assert not bad, bad
        # the special rays alone, one line per ray: what a failure on these rays is read from
        for k in ("d_rays_o", "d_rays_d"):
            err, floor = per_ray_errors(got[k], r32[k], r64[k])
            print(f"[{k} {tag}] " + "; ".join(f"{s.ray.name}@{s.obj}: {float(err[s.index]):.1e} ({float(floor[s.index]):.1e})" for s in b.special))
        check_all([(k, got[k], r32[k], r64[k]) for k in ("rgb", "depth", "acc")], "fp32" if precision in ("fp32", ("fp32", "bf16x3")) else "bf16x3")
        check_per_object([(k, got[k], r32[k], r64[k]) for k in ("d_latent", "d_shapecode", "d_texturecode")], band)
    att, det = runs[False], runs[True]
    # the flag changes the backward only
    assert all(torch.equal(att[k], det[k]) for k in ("rgb", "depth", "acc"))
    # rule 1 / rule 4: on a miss the bounds are the constants -1 / -1 -- the bounds' path is exactly nothing
    zs, h = b.z_scale.repeat_interleave(n)[:, None], b.half.repeat_interleave(n, 0)
    hit = O.slab_intersect(b.rays_o / zs, b.rays_d, -h, h)[2]
    miss = torch.nonzero(~hit).flatten().tolist()
    cnt = compared(b, miss, f"miss rays, attached == detached {CASE_ID(case)}", need=("zero_out", "zero_face", "behind", "graze"))
    assert sum(cnt.values()) == 9 * (B if n >= len(SR.TABLE) else 1)
    for k in ("d_rays_o", "d_rays_d"):
        diff = torch.nonzero((att[k][miss] != det[k][miss]).any(1)).flatten()
        assert diff.numel() == 0, (k, names_of(b, [miss[i] for i in diff]))
    # rule 3: a hit ray with d_a == +-0 and the origin strictly inside slab a -- component a gets exactly nothing from the bounds, the
    # other components do get something
    zero, _ = SR.rays_of(b, lambda s: s.ray.hit and len(s.ray.zero_axes) > 0)
    cnt = compared(b, zero, f"zero-component hits {CASE_ID(case)}", need=("parallel", "zero_in"))
    assert sum(cnt.values()) == 8 * (B if n >= len(SR.TABLE) else 1)
    by = {s.index: s for s in b.special}
    for i in zero:
        s = by[i]
        others = [a for a in range(3) if a not in s.ray.zero_axes]
        for k in ("d_rays_o", "d_rays_d"):
            for a in s.ray.zero_axes:
                assert float(att[k][i, a]) == float(det[k][i, a]), (k, names_of(b, [i]), a, att[k][i].tolist(), det[k][i].tolist())
            assert any(float(att[k][i, a]) != float(det[k][i, a]) for a in others), (k, names_of(b, [i]), att[k][i].tolist(), det[k][i].tolist())
    # and on every other hit the bounds' path is alive: the attached gradient is not the detached one
    live = [s.index for s in b.special if s.ray.hit]
    assert all(bool((att["d_rays_d"][i] != det["d_rays_d"][i]).any()) for i in live), names_of(b, live)


# ------------------------------------------------------------------ d. where these rays come from
def turntable_case():
    K = torch.tensor([[20.0, 0.0, 16.0], [0.0, 20.0, 12.0], [0.0, 0.0, 1.0]])           # integral cx, cy: the column px == cx exists
    pose = O.turntable_poses(radius=12.0, pan_num=4)[0]                                  # pan = 0
    return K, pose, O.virtual_roi(K.numpy(), 12)


def codes_1(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 256, generator=g) * 0.3, torch.randn(1, 256, generator=g) * 0.3


@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_render_virtual_imgs_holds_axis_parallel_rays(amd, dev, oracle_params, precision):
    K, _, roi = turntable_case()
    S, pan_num, img_sz = 32, 4, 12
    n_zero = n_zero_hit = 0
    for pose in O.turntable_poses(radius=12.0, pan_num=pan_num):
        ro, vd = O.pixel_rays(K, pose, roi)
        hit = O.aabb_sampled_rays(ro, vd, WLH, S, torch.zeros(ro.shape[0], S))[3]
        n_zero += int((vd == 0).any(1).sum())
        n_zero_hit += int(((vd == 0).any(1) & hit).sum())
    assert n_zero == 12 and n_zero_hit >= 4, (n_zero, n_zero_hit)        # the column px == cx of the pan = 0 view; some of it meets the box
    sc, tc = codes_1(9)
    g = torch.Generator().manual_seed(10)
    jitters = [torch.rand(img_sz * img_sz, S, generator=g) for _ in range(pan_num)]
    want = O.nerf_renderer_render_virtual_imgs(oracle_params, WLH, K, sc, tc, n_samples=S, radius=12., pan_num=pan_num, img_sz=img_sz,
                                               jitters=jitters)
    m = make_model(amd, dev, oracle_params, precision)
    rend = amd.NeRFRenderer(n_samples=S, white_bkgd=True)
    with amd.utils.jitter_override(list(jitters)), torch.no_grad():
        views = rend.render_virtual_imgs(m, dev, WLH, K, sc.to(dev), tc.to(dev), radius=12., pan_num=pan_num, img_sz=img_sz)
    assert bool(torch.isfinite(torch.stack(views)).all())
    assert md(torch.stack(views), torch.stack(want)) < 2e-5                              # test_api_parity.py's TOL_RGB


# ------------------------------------------------------------------ the pose gradient on the fused and on the unfused path
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("S", [64, 48], ids=["S64-one-launch", "S48-torch-bounds"])
def test_turntable_pose_gradient_finite_on_both_paths(amd, dev, oracle_params, S, precision):
    """The pan = 0 turntable pose: 12 of its 144 rays have d_y == -0.0 with o_y == 0, and the reference's autograd gives a NaN pose
    gradient.  n_samples = 64 is one SNR_Z_BOX launch; 48 is no power of two, so the bounds are torch's (``renderer._box_bounds``), then
    decoder and composite launches.  Both must return the guarded oracle's gradient at their own sample count."""
    K, pose0, roi = turntable_case()
    img, mask = O.synthetic_targets(11, 12)
    ro, vd = O.pixel_rays(K, pose0, roi)
    N = ro.shape[0]
    assert int(((vd[:, 1] == 0) & (ro[:, 1] == 0)).sum()) == 12
    sc0, tc0 = codes_1(21)
    g = torch.Generator().manual_seed(S)
    jit = torch.rand(N, S, generator=g)
    w_rgb, w_d, w_a = torch.rand(N, 3, generator=g), torch.rand(N, generator=g) * 0.1, torch.rand(N, generator=g)
    m = make_model(amd, dev, oracle_params, precision)
    pose, sc, tc = [x.to(dev).requires_grad_() for x in (pose0, sc0, tc0)]
    rend = amd.NeRFRenderer(n_samples=S, white_bkgd=True)
    with amd.utils.jitter_override(jit):
        out = rend.render_rays(m, dev, img, mask, pose, WLH, K, roi, sc, tc, im_sz=12)
    masks = relu_bits_of(out[0], 3, 1, n_samples=S if S == 64 else 1)
    ((out[0] * w_rgb.to(dev)).sum() + (out[1] * w_d.to(dev)).sum() + (out[2] * w_a.to(dev)).sum()).backward()
    assert bool(torch.isfinite(pose.grad).all()), pose.grad

    def oracle(dt, slab):
        cv = lambda x: x.to(dt)
        p, s, t = [cv(x).clone().requires_grad_() for x in (pose0, sc0, tc0)]
        o, v = O.pixel_rays(cv(K), p, roi, uv_steps=[12, 12])
        xyz, vv, z, hit = O.aabb_sampled_rays(o, v, WLH, S, cv(jit), slab=slab)
        sig, rgb = O.decoder_forward({k: cv(x) for k, x in oracle_params.items()}, xyz, vv, s, t, relu_masks=masks)
        r = O.composite(sig, rgb, z, white_bkgd=True)
        ((r[0] * cv(w_rgb)).sum() + (r[1] * cv(w_d)).sum() + (r[2] * cv(w_a)).sum()).backward()
        return dict(d_pose=p.grad[None], d_shapecode=s.grad, d_texturecode=t.grad, hit=hit)
    assert not bool(torch.isfinite(oracle(torch.float64, O.slab_intersect)["d_pose"]).all())         # the plain formula: NaN
    r32, r64 = [oracle(dt, O.guarded_slab_intersect) for dt in (torch.float32, torch.float64)]
    assert bool(r64["hit"].any()) and bool((~r64["hit"]).any())
    print(f"[pose gradient S={S} {precision}] {pose.grad.flatten().tolist()}")
    check_per_object([("d_pose", pose.grad[None], r32["d_pose"], r64["d_pose"]), ("d_shapecode", sc.grad, r32["d_shapecode"], r64["d_shapecode"]),
                      ("d_texturecode", tc.grad, r32["d_texturecode"], r64["d_texturecode"])], band_of(precision))
