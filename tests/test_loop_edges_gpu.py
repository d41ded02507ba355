"""The small kernels around the render in the optimise loop (csrc/snr_loop.hip, csrc/snr_loss.hip) at their seams, against the float64
references of tests/loop_reference.py (checked on their own by tests/test_loop_reference_cpu.py): rotation magnitudes across the series
threshold and the band above it, ray counts next to the 1024-ray forward chunks and the 256 -> 1024 thread switch at 2048, the ends of
the sample count, the metric row's lidar loop / counts / degenerate rotations, AdamW's grid-stride loop and its tails, the loss tail with
one gradient wanted, the latent layers at an exactly-zero pre-activation.  Inputs are float32-representable, so the kernel and the
reference start from the same numbers; every object of a batch has its own data.  Tolerances are those of tests/test_loop_kernels.py."""
import math

import pytest
import torch

import loop_reference as LR
from oracle_bands import amd, dev, in_band, md, rel  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

ALL_MAGS = LR.MAGNITUDES + LR.BAND_MAGNITUDES
SEAM_RAYS = [1023, 1024, 1025, 2047, 2048, 2049, 3073]
FILL = -7.5                                        # sentinel around buffers handed to the C ABI


def r32(t):
    """float64 holding float32-representable numbers."""
    return t.float().double()


def rows_rel(got, want):
    """per object (dim 0): max |got - want| over the largest |want| of that object."""
    got, want = got.detach().double().cpu().flatten(1), want.detach().double().flatten(1)
    return (got - want).abs().amax(1) / (want.abs().amax(1) + 1e-30)


def guarded(rows, cols, dev, pad=32):
    """(buffer, interior view (rows, cols)): the interior is what the kernel may write, ``pad`` rows of sentinel on either side."""
    buf = torch.full(((rows + 2 * pad) * cols,), FILL, device=dev)
    return buf, buf[pad * cols:(pad + rows) * cols].view(rows, cols)


def guards_intact(buf, inner):
    lo = inner.storage_offset() - buf.storage_offset()
    return bool((buf[:lo] == FILL).all()) and bool((buf[lo + inner.numel():] == FILL).all())


def pose_inputs(B, n, S, seed, rot=None, centre=(0., 1., 15.), spread=3.0):
    g = torch.Generator().manual_seed(seed)
    if rot is None:
        rot = r32(torch.randn(B, 3, generator=g, dtype=torch.float64) * 1.2)
    tr = r32(torch.randn(B, 3, generator=g, dtype=torch.float64) * spread + torch.tensor(centre, dtype=torch.float64))
    cam = r32(torch.cat([torch.randn(B, n, 2, generator=g, dtype=torch.float64) * 0.2, torch.ones(B, n, 1, dtype=torch.float64)], -1))
    half = r32(torch.rand(B, generator=g, dtype=torch.float64) + 2)
    jit = r32(torch.rand(B, S, generator=g, dtype=torch.float64))
    w_o, w_d, w_c = [r32(torch.randn(*s, generator=g, dtype=torch.float64)) for s in ((B * n, 3), (B * n, 3), (B, 3, 4))]
    return rot, tr, cam, half, jit, w_o, w_d, w_c


# ------------------------------------------------------------------ rotation magnitudes
@pytest.mark.parametrize("opt_cam_pose", [0, 1])
@pytest.mark.parametrize("form", ["pose_only", "all_outputs"])
def test_rotation_sweep(amd, dev, form, opt_cam_pose):
    """One object per rotation magnitude about its own random axis.  ``pose_only``: the gradient arrives through cam2opt alone (the kernel
    gets null for d_rays_o and d_viewdir), which isolates the Rodrigues backward; ``all_outputs``: all three outputs weighted.  Every
    magnitude on its own: cam2opt within 2e-6 max(1, |ref|), the gradients within 5e-5 of that object's largest entry."""
    B, n, S = len(ALL_MAGS), 50, 8
    rot, tr, cam, half, jit, w_o, w_d, w_c = pose_inputs(B, n, S, 30 + opt_cam_pose, rot=LR.sweep_vectors(ALL_MAGS, seed=40 + opt_cam_pose))
    rot_r, tr_r = rot.clone().requires_grad_(), tr.clone().requires_grad_()
    ref = LR.pose_rays(rot_r, tr_r, cam, half, jit, S, opt_cam_pose)
    weigh = lambda o, f=(lambda t: t): (o[0] * f(w_c)).sum() + (0 if form == "pose_only" else (o[1] * f(w_o)).sum() + (o[2] * f(w_d)).sum())
    weigh(ref).backward()
    f = lambda t: t.float().to(dev)
    rot_d, tr_d = f(rot).requires_grad_(), f(tr).requires_grad_()
    out = amd.ops.PoseRays.apply(rot_d, tr_d, f(cam), f(half), f(jit), S, opt_cam_pose)
    weigh(out, f).backward()
    e_c = (out[0].detach().double().cpu() - ref[0].detach()).abs().amax((1, 2)) / ref[0].detach().abs().amax((1, 2)).clamp_min(1.0)
    e_r, e_t = rows_rel(rot_d.grad, rot_r.grad), rows_rel(tr_d.grad, tr_r.grad)
    for m, a, b, c in zip(ALL_MAGS, e_c, e_r, e_t):
        print(f"[rotation sweep {form} opt_cam_pose={opt_cam_pose}] |v| = {m:.6g}: cam2opt {float(a):.1e}  d_rot rel {float(b):.1e}  d_trans rel {float(c):.1e}")
    assert bool(torch.isfinite(rot_d.grad).all()) and bool(torch.isfinite(tr_d.grad).all())
    bad = [(m, float(a), float(b), float(c)) for m, a, b, c in zip(ALL_MAGS, e_c, e_r, e_t) if not (a < 2e-6 and b < 5e-5 and c < 5e-5)]
    assert not bad, bad
    if form == "all_outputs":
        for a, b, name, tol in zip(out[1:], ref[1:], ("rays_o", "viewdir", "z"), (2e-6, 5e-7, 5e-6)):
            assert md(a, b) < tol * max(1.0, float(b.abs().max())), (name, md(a, b))


# ------------------------------------------------------------------ ray counts next to the chunk and thread-count seams
@pytest.mark.parametrize("opt_cam_pose", [0, 1])
@pytest.mark.parametrize("n", SEAM_RAYS)
def test_pose_rays_ray_count_seams(amd, dev, n, opt_cam_pose):
    B, S = 3, 5
    rot, tr, cam, half, jit, w_o, w_d, w_c = pose_inputs(B, n, S, 50 + n)
    rot_r, tr_r = rot.clone().requires_grad_(), tr.clone().requires_grad_()
    ref = LR.pose_rays(rot_r, tr_r, cam, half, jit, S, opt_cam_pose)
    ((ref[1] * w_o).sum() + (ref[2] * w_d).sum() + (ref[0] * w_c).sum()).backward()
    f = lambda t: t.float().to(dev)
    rot_d, tr_d = f(rot).requires_grad_(), f(tr).requires_grad_()
    out = amd.ops.PoseRays.apply(rot_d, tr_d, f(cam), f(half), f(jit), S, opt_cam_pose)
    errs = [md(a, b) for a, b in zip(out, ref)]
    ((out[1] * f(w_o)).sum() + (out[2] * f(w_d)).sum() + (out[0] * f(w_c)).sum()).backward()
    g_r, g_t = rel(rot_d.grad, rot_r.grad), rel(tr_d.grad, tr_r.grad)
    print(f"[pose_rays n={n} opt_cam_pose={opt_cam_pose}] cam2opt/rays_o/viewdir/z {errs}  d_rot rel {g_r:.1e}  d_trans rel {g_t:.1e}")
    for e, b, name, tol in zip(errs, ref, ("cam2opt", "rays_o", "viewdir", "z"), (2e-6, 2e-6, 5e-7, 5e-6)):
        assert e < tol * max(1.0, float(b.abs().max())), (name, e)
    assert g_r < 5e-5 and g_t < 5e-5, (g_r, g_t)
    # the same launch through the C ABI into the interiors of sentinel-filled buffers: the same bits, nothing outside them
    P, lib = amd.ops._p, amd._lib.lib()
    bufs = [guarded(r, c, dev) for r, c in ((B * 3, 4), (B * n, 3), (B * n, 3), (B, S))]
    ins = [t.detach() for t in (rot_d, tr_d)] + [f(cam), f(half), f(jit)]
    amd._lib.check(lib.snr_pose_rays_fwd(*[P(t) for t in ins], B, n, S, opt_cam_pose, *[P(v) for _, v in bufs], amd.ops._stream(dev)), "snr_pose_rays_fwd")
    for (buf, inner), o, name in zip(bufs, out, ("cam2opt", "rays_o", "viewdir", "z")):
        assert torch.equal(inner.view(o.shape), o.detach()) and guards_intact(buf, inner), name


@pytest.mark.parametrize("n", SEAM_RAYS)
def test_cam_rays_ray_count_seams(amd, dev, n):
    """``CamRays``: the pose (B,3,4) itself is the leaf (the direct form of the same kernels)."""
    B, S = 3, 5
    rot, tr, cam, half, jit, w_o, w_d, _ = pose_inputs(B, n, S, 70 + n, centre=(0., 1., 10.), spread=1.0)
    c2w = r32(LR.camera_pose(rot, tr, 1))
    c_r = c2w.clone().requires_grad_()
    ref = LR.rays_of_pose(c_r, cam, half, jit, S)
    ((ref[0] * w_o).sum() + (ref[1] * w_d).sum()).backward()
    f = lambda t: t.float().to(dev)
    c_d = f(c2w).requires_grad_()
    cam_d, half_d, jit_d, wo_d, wd_d = f(cam), f(half), f(jit), f(w_o), f(w_d)       # (kept alive: the C ABI below takes their addresses)
    out = amd.ops.CamRays.apply(c_d, cam_d, half_d, jit_d, S)
    errs = [md(a, b) for a, b in zip(out, ref)]
    ((out[0] * wo_d).sum() + (out[1] * wd_d).sum()).backward()
    g_c = rel(c_d.grad, c_r.grad)
    print(f"[cam_rays n={n}] rays_o/viewdir/z {errs}  d_pose rel {g_c:.1e}")
    assert errs[0] < 1e-6 and errs[1] < 2e-7 and errs[2] < 4e-6 and g_c < 2e-5, (errs, g_c)
    P, lib = amd.ops._p, amd._lib.lib()
    bufs = [guarded(r, c, dev) for r, c in ((B * n, 3), (B * n, 3), (B, S))]
    amd._lib.check(lib.snr_cam_rays_fwd(P(c_d.detach()), P(cam_d), P(half_d), P(jit_d), B, n, S, *[P(v) for _, v in bufs], amd.ops._stream(dev)),
                   "snr_cam_rays_fwd")
    for (buf, inner), o, name in zip(bufs, out, ("rays_o", "viewdir", "z")):
        assert torch.equal(inner.view(o.shape), o.detach()) and guards_intact(buf, inner), name
    g_buf, g_in = guarded(B * 3, 4, dev)
    amd._lib.check(lib.snr_cam_rays_bwd(P(c_d.detach()), P(cam_d), B, n, P(wo_d), P(wd_d), P(g_in), amd.ops._stream(dev)), "snr_cam_rays_bwd")
    assert torch.equal(g_in.view(B, 3, 4), c_d.grad) and guards_intact(g_buf, g_in)


def loss_inputs(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    rgb = r32(torch.rand(B * n, 3, generator=g, dtype=torch.float64) * 1.2 - 0.1)
    acc = r32(torch.rand(B * n, generator=g, dtype=torch.float64))
    tgt = r32(torch.rand(B * n, 3, generator=g, dtype=torch.float64))
    occ = (torch.randint(0, 3, (B * n, 1), generator=g) - 1).double()
    up = r32(torch.rand(B, generator=g, dtype=torch.float64) + 0.5)
    return rgb, acc, tgt, occ, up


@pytest.mark.parametrize("n", SEAM_RAYS)
def test_loss_tail_ray_count_seams(amd, dev, n):
    B = 3
    rgb, acc, tgt, occ, up = loss_inputs(B, n, 90 + n)
    rgb_r, acc_r = rgb.clone().requires_grad_(), acc.clone().requires_grad_()
    want = LR.loss_tail(rgb_r, acc_r, tgt, occ, 0.1, n)
    (want[:, 0] * up).sum().backward()
    f = lambda t: t.float().to(dev)
    rgb_d, acc_d = f(rgb).requires_grad_(), f(acc).requires_grad_()
    loss, metrics = amd.ops.LossTail.apply(rgb_d, acc_d, f(tgt), f(occ), 0.1, n)
    (loss * f(up)).sum().backward()
    e = (rel(loss, want[:, 0]), rel(metrics, want[:, 1:]), rel(rgb_d.grad, rgb_r.grad), rel(acc_d.grad, acc_r.grad))
    print(f"[loss_tail n={n}] rel loss/metrics/d_rgb/d_acc {e}")
    assert max(e) < 2e-6, e
    P, lib = amd.ops._p, amd._lib.lib()
    (b_rgb, i_rgb), (b_acc, i_acc), (b_out, i_out) = guarded(B * n, 3, dev), guarded(B * n, 1, dev), guarded(B, 4, dev)
    held = [rgb_d.detach(), acc_d.detach(), f(tgt), f(occ), f(up)]                   # (kept alive: the C ABI takes their addresses)
    ins = [P(t) for t in held[:4]]
    amd._lib.check(lib.snr_loss_tail_bwd(*ins, B * n, n, 0.1, P(held[4]), P(i_rgb), P(i_acc), amd.ops._stream(dev)), "snr_loss_tail_bwd")
    amd._lib.check(lib.snr_loss_tail_fwd(*ins, B * n, n, 0.1, P(i_out), amd.ops._stream(dev)), "snr_loss_tail_fwd")
    assert torch.equal(i_rgb, rgb_d.grad) and torch.equal(i_acc.view(-1), acc_d.grad) and guards_intact(b_rgb, i_rgb) and guards_intact(b_acc, i_acc)
    assert torch.equal(i_out[:, 0], loss.detach()) and torch.equal(i_out[:, 1:], metrics) and guards_intact(b_out, i_out)


# ------------------------------------------------------------------ the ends of the sample count
@pytest.mark.parametrize("with_jitter", [True, False])
@pytest.mark.parametrize("S", [1, 2, 3, 255, 256])
def test_depth_samples_at_the_ends_of_S(amd, dev, S, with_jitter):
    B, n = 3, 3
    rot, tr, cam, half, jit, *_ = pose_inputs(B, n, S, 110 + S)
    jit = jit if with_jitter else None
    f = lambda t: None if t is None else t.float().to(dev)
    for opt_cam_pose in (0, 1):
        ref = LR.pose_rays(rot, tr, cam, half, jit, S, opt_cam_pose)
        out = amd.ops.PoseRays.apply(f(rot), f(tr), f(cam), f(half), f(jit), S, opt_cam_pose)
        assert out[3].shape == (B, S) and md(out[3], ref[3]) < 5e-6 * max(1.0, float(ref[3].abs().max())), (opt_cam_pose, md(out[3], ref[3]))
        assert md(out[2], ref[2]) < 5e-7
    c2w = r32(LR.camera_pose(rot, tr, 1))
    ref = LR.rays_of_pose(c2w, cam, half, jit, S)
    z = amd.ops.CamRays.apply(f(c2w), f(cam), f(half), f(jit), S)[2]
    assert md(z, ref[2]) < 5e-6 * max(1.0, float(ref[2].abs().max()))


def test_depth_samples_reject_more_than_256(amd, dev):
    B, n, S = 2, 3, 257
    rot, tr, cam, half, jit, *_ = pose_inputs(B, n, S, 120)
    f = lambda t: t.float().to(dev)
    with pytest.raises(amd.SnrError):
        amd.ops.PoseRays.apply(f(rot), f(tr), f(cam), f(half), f(jit), S, 0)
    with pytest.raises(amd.SnrError):
        amd.ops.CamRays.apply(f(r32(LR.camera_pose(rot, tr, 1))), f(cam), f(half), f(jit), S)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ metric row
def metric_inputs(B, nl, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c2o = r32(torch.cat([LR.rotation(rnd(B, 3)), rnd(B, 3, 1) * 5], -1))
    gt_R, gt_T = r32(LR.rotation(rnd(B, 3))), r32(rnd(B, 3) * 5)
    loss_out = r32(torch.rand(B, 4, generator=g, dtype=torch.float64) * 0.2 + 0.01)
    d, d0 = r32(torch.rand(B, nl, generator=g, dtype=torch.float64) * 20), r32(torch.rand(B, nl, generator=g, dtype=torch.float64) * 20)
    return loss_out, d, d0, c2o, gt_R, gt_T


def check_metric_row(row, want):
    """the tolerances of test_loop_kernels.test_metric_row; the angle also by its cosine (acos near 0 / pi amplifies the trace's last bits)"""
    assert bool(torch.isfinite(row[:, 1:]).all()), row
    assert md(row[:, :2], want[:, :2]) < 2e-5 and md(row[:, 2], want[:, 2]) < 1e-3 and md(row[:, 3], want[:, 3]) < 1e-5, (row.cpu(), want)
    assert md(torch.cos(row[:, 2]), torch.cos(want[:, 2])) < 2e-6


@pytest.mark.parametrize("opt_cam_pose", [0, 1])
@pytest.mark.parametrize("nl", [0, 1, 63, 64, 65, 200])
def test_metric_row_lidar_widths(amd, dev, nl, opt_cam_pose):
    B = 4
    loss_out, d, d0, c2o, gt_R, gt_T = metric_inputs(B, nl, 130 + nl)
    want = LR.metric_row(loss_out, d, d0, c2o, gt_R, gt_T, opt_cam_pose)
    f = lambda t: t.float().to(dev).contiguous()
    row, d0_d = torch.full((B, 4), FILL, device=dev), f(d0)
    amd.ops.metric_row(f(loss_out), f(d), d0_d, False, f(c2o), f(gt_R), f(gt_T), opt_cam_pose, row)
    check_metric_row(row, want)
    assert torch.equal(d0_d.cpu().double(), d0)                               # (read only when this is not the first iteration)
    amd.ops.metric_row(f(loss_out), f(d), d0_d, True, f(c2o), f(gt_R), f(gt_T), opt_cam_pose, row)
    assert float(row[:, 1].abs().max()) == 0.0 and torch.equal(d0_d.cpu().double(), d)


@pytest.mark.parametrize("opt_cam_pose", [0, 1])
def test_metric_row_counts_are_clamped(amd, dev, opt_cam_pose):
    """``lidar_count`` entries of zero, above the width and below zero; with ``first`` the depth buffer receives exactly each row's first cnt."""
    nl = 65
    cnt = [0, 70, -3, 64, 65, 1]
    B = len(cnt)
    loss_out, d, d0, c2o, gt_R, gt_T = metric_inputs(B, nl, 140)
    want = LR.metric_row(loss_out, d, d0, c2o, gt_R, gt_T, opt_cam_pose, lidar_count=cnt)
    f = lambda t: t.float().to(dev).contiguous()
    cnt_d = torch.tensor(cnt, dtype=torch.int32, device=dev)
    row = torch.full((B, 4), FILL, device=dev)
    amd.ops.metric_row(f(loss_out), f(d), f(d0), False, f(c2o), f(gt_R), f(gt_T), opt_cam_pose, row, lidar_count=cnt_d)
    check_metric_row(row, want)
    assert float(row[0, 1]) == 0.0 and float(row[2, 1]) == 0.0
    buf, d0_d = guarded(B, nl, dev)
    amd.ops.metric_row(f(loss_out), f(d), d0_d, True, f(c2o), f(gt_R), f(gt_T), opt_cam_pose, row, lidar_count=cnt_d)
    assert float(row[:, 1].abs().max()) == 0.0 and guards_intact(buf, d0_d)
    for b, c in enumerate(LR.clamped_counts(cnt, B, nl)):
        assert torch.equal(d0_d[b, :c].cpu().double(), d[b, :c]) and bool((d0_d[b, c:] == FILL).all()), b
    check_metric_row(row, LR.metric_row(loss_out, d, d0, c2o, gt_R, gt_T, opt_cam_pose, first=True, lidar_count=cnt))


@pytest.mark.parametrize("opt_cam_pose", [0, 1])
def test_metric_row_degenerate_rotations(amd, dev, opt_cam_pose):
    """The target equal to the predicted rotation (the fp32 trace may round above 3: clamped, angle ~0, never NaN), a half turn about a random
    axis (trace ~ -1), and a zero foreground MSE (PSNR = +inf like torch)."""
    B, nl = len(ALL_MAGS), 3
    loss_out, d, d0, c2o, _, gt_T = metric_inputs(B, nl, 150)
    c2o = r32(torch.cat([LR.rotation(LR.sweep_vectors(ALL_MAGS, seed=151)), c2o[:, :, 3:]], -1))
    pred_R = c2o[:, :, :3] if opt_cam_pose else c2o[:, :, :3].transpose(-2, -1)
    g = torch.Generator().manual_seed(152)
    axis = torch.randn(B, 3, generator=g, dtype=torch.float64); axis = axis / axis.norm(dim=-1, keepdim=True)
    loss_out[::2, 3] = 0.0
    f = lambda t: t.float().to(dev).contiguous()
    for name, gt_R in (("same", pred_R.contiguous()), ("half turn", r32(pred_R @ LR.rotation(axis * math.pi)))):
        want = LR.metric_row(loss_out, d, d0, c2o, gt_R, gt_T, opt_cam_pose)
        row = torch.full((B, 4), FILL, device=dev)
        amd.ops.metric_row(f(loss_out), f(d), f(d0), False, f(c2o), f(gt_R), f(gt_T), opt_cam_pose, row)
        print(f"[metric_row {name} opt_cam_pose={opt_cam_pose}] angles {row[:, 2].tolist()}")
        assert bool(torch.isfinite(row[:, 2]).all()) and md(torch.cos(row[:, 2]), torch.cos(want[:, 2])) < 2e-6
        if name == "same":
            assert float(row[:, 2].abs().max()) < 1e-3
        assert bool((row[::2, 0] == math.inf).all()) and md(row[1::2, 0], want[1::2, 0]) < 2e-5
        assert md(row[:, 1], want[:, 1]) < 2e-5 and md(row[:, 3], want[:, 3]) < 1e-5


# ------------------------------------------------------------------ AdamW
def adam_case(sizes, seed, n_steps, first_step, zero_first):
    """Parameters, per-step gradients and starting moments (float32-representable float64), and the float64 / float32 references after
    ``n_steps`` steps numbered from ``first_step``.  ``zero_first``: the first step's gradient is zero on a random half of every tensor."""
    g = torch.Generator().manual_seed(seed)
    p0 = [r32(torch.randn(s, generator=g, dtype=torch.float64)) for s in sizes]
    grads = [[r32(torch.randn(s, generator=g, dtype=torch.float64) * (0.1 + k % 3)) for s in sizes] for k in range(n_steps)]
    if zero_first:
        for gr in grads[0]:
            gr[torch.rand(gr.shape, generator=g) < 0.5] = 0.0
    if first_step > 1:        # a run that is already under way: moments of plausible size, the second one non-negative
        m0 = [r32(torch.randn(s, generator=g, dtype=torch.float64) * 0.3) for s in sizes]
        v0 = [r32(torch.rand(s, generator=g, dtype=torch.float64) * 2) for s in sizes]
    else:
        m0, v0 = [torch.zeros(s, dtype=torch.float64) for s in sizes], [torch.zeros(s, dtype=torch.float64) for s in sizes]
    return p0, grads, m0, v0


def adam_reference(p0, grads, m0, v0, lrs, first_step, dtype):
    out = []
    for i, lr in enumerate(lrs):
        p, m, v = p0[i].to(dtype), m0[i].to(dtype), v0[i].to(dtype)
        for k, gr in enumerate(grads):
            p, m, v = LR.adamw_step(p, gr[i].to(dtype), m, v, first_step + k, lr)
        out.append((p, m, v))
    return out


def check_adam(got, p0, grads, m0, v0, lrs, first_step, label):
    o64, o32 = adam_reference(p0, grads, m0, v0, lrs, first_step, torch.float64), adam_reference(p0, grads, m0, v0, lrs, first_step, torch.float32)
    bad = []
    for i, (g3, a3, b3) in enumerate(zip(got, o32, o64)):
        if b3[0].numel() == 0:
            assert all(t.numel() == 0 for t in g3)
            continue
        for name, gt, a, b in zip(("p", "exp_avg", "exp_avg_sq"), g3, a3, b3):
            ok, _, msg = in_band(gt, a, b, "fp32", f"{label} tensor {i} ({b.numel()} elements) {name}")
            print(msg)
            if not ok:
                bad.append(msg)
    assert not bad, bad


@pytest.mark.parametrize("first_step,zero_first", [(1, True), (1000, False)])
def test_device_adamw_grid_stride_and_tails(amd, dev, first_step, zero_first):
    """Groups of 262144 + 257 (the 1024-block grid makes a second trip with a ragged tail), 257, 1 and 0 elements; three steps from the start
    with a zero gradient on the first (denom = eps), and one step number 1000 from given moments (``steps`` preset to 999)."""
    sizes, lrs = [262144 + 257, 257, 1, 0], [0.02, 0.015, 0.01, 0.005]
    n_steps = 3 if first_step == 1 else 1
    p0, grads, m0, v0 = adam_case(sizes, 160 + first_step, n_steps, first_step, zero_first)
    f = lambda t: t.float().to(dev)
    p_dev = [f(p).requires_grad_() for p in p0]
    opt = amd.ops.DeviceAdamW(list(zip(p_dev, lrs)))
    opt.steps = first_step - 1
    for i in range(len(sizes)):
        opt.exp_avg[i].copy_(f(m0[i])); opt.exp_avg_sq[i].copy_(f(v0[i]))
    for gr in grads:
        for p, g_ in zip(p_dev, gr):
            p.grad = f(g_)
        opt.step()
    assert opt.steps == first_step - 1 + n_steps
    check_adam(list(zip(p_dev, opt.exp_avg, opt.exp_avg_sq)), p0, grads, m0, v0, lrs, first_step, "DeviceAdamW")


@pytest.mark.parametrize("first_step,zero_first", [(1, True), (1000, False)])
def test_table_adamw_grid_stride_and_tails(amd, dev, first_step, zero_first):
    """A tensor of 65536 + 1 elements (the 256-block grid makes a second trip of one element) next to small ones in other groups."""
    sizes, lrs = [65536 + 1, 257, 1], [1e-2, 2e-2, 5e-3]
    n_steps = 3 if first_step == 1 else 1
    p0, grads, m0, v0 = adam_case(sizes, 170 + first_step, n_steps, first_step, zero_first)
    f = lambda t: t.float().to(dev)
    p_dev = [torch.nn.Parameter(f(p)) for p in p0]
    for p in p_dev:
        p.grad = torch.zeros_like(p)
    opt = amd.ops.TableAdamW([([p], lr) for p, lr in zip(p_dev, lrs)])
    opt.steps = first_step - 1
    for i in range(len(sizes)):
        opt.exp_avg[i].copy_(f(m0[i])); opt.exp_avg_sq[i].copy_(f(v0[i]))
    for gr in grads:
        for p, g_ in zip(p_dev, gr):
            p.grad.copy_(f(g_))
        opt.step()
    check_adam(list(zip(p_dev, opt.exp_avg, opt.exp_avg_sq)), p0, grads, m0, v0, lrs, first_step, "TableAdamW")


# ------------------------------------------------------------------ loss tail: one gradient wanted, an all-background object
def test_loss_tail_single_gradients_and_background_object(amd, dev):
    B, n = 3, 300
    rgb, acc, tgt, occ, up = loss_inputs(B, n, 180)
    occ[n:2 * n] = -1.0                                                       # the second object: background only
    rgb_r, acc_r = rgb.clone().requires_grad_(), acc.clone().requires_grad_()
    want = LR.loss_tail(rgb_r, acc_r, tgt, occ, 0.1, n)
    (want[:, 0] * up).sum().backward()
    f = lambda t: t.float().to(dev)
    grads = {}
    for which in ("both", "rgb", "acc"):
        rgb_d, acc_d = f(rgb).requires_grad_(which != "acc"), f(acc).requires_grad_(which != "rgb")
        loss, metrics = amd.ops.LossTail.apply(rgb_d, acc_d, f(tgt), f(occ), 0.1, n)
        (loss * f(up)).sum().backward()
        grads[which] = (rgb_d.grad, acc_d.grad)
    assert float(metrics[1, 2]) == 0.0 and float(want[1, 3]) == 0.0           # mse_fg of the background-only object
    assert rel(loss, want[:, 0]) < 2e-6 and rel(metrics, want[:, 1:]) < 2e-6 and rel(loss[1], want[1, 0]) < 2e-6
    assert grads["rgb"][1] is None and grads["acc"][0] is None
    assert torch.equal(grads["rgb"][0], grads["both"][0]) and torch.equal(grads["acc"][1], grads["both"][1])
    assert rel(grads["rgb"][0], rgb_r.grad) < 2e-6 and rel(grads["acc"][1], acc_r.grad) < 2e-6


# ------------------------------------------------------------------ latent layers at a pre-activation of exactly zero
@pytest.mark.parametrize("bias", [0.0, -1.0])
def test_latent_layers_at_exact_zero(amd, dev, bias):
    """Zero codes and latent biases of 0 (the pre-activation is exactly 0: ReLU's gradient there is 0, the mask is z > 0) or -1: z == 0, the
    folded bias is the next layer's bias itself, and no upstream gradient reaches the codes."""
    sb, tb, B = 3, 1, 3
    torch.manual_seed(190)
    m = amd.CodeNeRF(sb, tb).to(dev)
    with torch.no_grad():
        for j in range(sb):
            getattr(m, f"shape_latent_layer_{j + 1}")[0].bias.fill_(bias)
        for j in range(tb):
            getattr(m, f"texture_latent_layer_{j + 1}")[0].bias.fill_(bias)
    lat, nxt, _ = LR.model_latent_weights(m)
    z64, lb64 = LR.latent_layers(torch.zeros(B, 256, dtype=torch.float64), torch.zeros(B, 256, dtype=torch.float64), lat, nxt, sb)
    assert float(z64.abs().max()) == 0.0 and torch.equal(lb64, torch.stack([b for _, b in nxt])[None].expand(B, -1, -1))
    sc, tc = torch.zeros(B, 256, device=dev, requires_grad=True), torch.zeros(B, 256, device=dev, requires_grad=True)
    z = m.latent_terms(sc, tc)
    lb = m.latent_biases(z)
    assert getattr(z, "_snr_latent_bias", None) is lb                         # (the one-launch path ran)
    assert float(z.abs().max()) == 0.0 and torch.equal(lb.cpu().double(), lb64)
    up = torch.randn(B, sb + tb, 256, generator=torch.Generator().manual_seed(191)) * 100
    (z * up.to(dev)).sum().backward()
    assert float(sc.grad.abs().max()) == 0.0 and float(tc.grad.abs().max()) == 0.0
