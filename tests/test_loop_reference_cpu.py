"""The references of tests/loop_reference.py against independent formulations, on the CPU: a wrong reference must not be able to pass a wrong
kernel.  And ``driver.axis_angle_to_matrix`` in float32 (the API loop's rotation, the formulas the pose kernel restates) against the float64
reference across the rotation magnitudes, the band above the series threshold included."""
import math

import numpy as np
import pytest
import torch

import loop_reference as LR
from oracle import supnerf_oracle as O


@pytest.fixture(scope="module")
def amd():
    import supnerf_amd
    return supnerf_amd


ALL_MAGS = LR.MAGNITUDES + LR.BAND_MAGNITUDES


# ------------------------------------------------------------------ rotation
def test_rotation_matches_matrix_exponential():
    v = LR.sweep_vectors(LR.MAGNITUDES, seed=1)
    R = LR.rotation(v)
    want = torch.linalg.matrix_exp(LR.skew(v))
    err = (R - want).abs().amax((-2, -1))
    print("rotation vs matrix_exp:", [f"{m:.3g}: {float(e):.1e}" for m, e in zip(LR.MAGNITUDES, err)])
    assert float(err.max()) < 1e-13
    assert torch.equal(LR.rotation(torch.zeros(3, dtype=torch.float64)), torch.eye(3, dtype=torch.float64))
    # a rotation: orthogonal, determinant 1
    assert float((R @ R.transpose(-2, -1) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-13
    assert float((torch.linalg.det(R) - 1).abs().max()) < 1e-13


def test_rotation_autograd_matches_central_differences():
    """h = 1e-6 in float64: truncation ~ h^2 |f'''| / 6 ~ 1e-12, rounding ~ 2^-53 |f| / h ~ 1e-9 for the |f| ~ 10 of a dense weighting of nine
    entries: held to 1e-7 of the largest gradient entry.  9.9e-5 and 1.01e-4 keep both probes on their own side of the series threshold or
    cross it, where the two branches agree to 1e-17."""
    v = LR.sweep_vectors(ALL_MAGS, seed=2)
    G = torch.randn(len(ALL_MAGS), 3, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    f = lambda x: (LR.rotation(x) * G).sum((-2, -1))
    vr = v.clone().requires_grad_()
    f(vr).sum().backward()
    h = 1e-6
    num = torch.stack([(f(v + h * e) - f(v - h * e)) / (2 * h) for e in torch.eye(3, dtype=torch.float64)], -1)
    err = (vr.grad - num).abs().amax(-1) / num.abs().amax(-1)
    print("rotation autograd vs central differences:", [f"{m:.3g}: {float(e):.1e}" for m, e in zip(ALL_MAGS, err)])
    assert float(err.max()) < 1e-7


def test_pose_rays_reference_against_a_per_ray_loop():
    """The batched broadcasting of ``pose_rays`` against numpy written ray by ray from the matrix exponential; every object different."""
    g = torch.Generator().manual_seed(4)
    B, n, S = 3, 5, 4
    rot = torch.randn(B, 3, generator=g, dtype=torch.float64)
    tr = torch.randn(B, 3, generator=g, dtype=torch.float64) * 3 + torch.tensor([0., 1., 15.], dtype=torch.float64)
    cam = torch.cat([torch.randn(B, n, 2, generator=g, dtype=torch.float64) * 0.2, torch.ones(B, n, 1, dtype=torch.float64)], -1)
    half = torch.rand(B, generator=g, dtype=torch.float64) + 2
    jit = torch.rand(B, S, generator=g, dtype=torch.float64)
    for opt_cam_pose in (0, 1):
        c2o, ro, vd, z = LR.pose_rays(rot, tr, cam, half, jit, S, opt_cam_pose)
        c2o0, _, _, z0 = LR.pose_rays(rot, tr, cam, half, None, S, opt_cam_pose)
        for b in range(B):
            R = torch.linalg.matrix_exp(LR.skew(rot[b])).numpy()
            t = tr[b].numpy()
            Rc, tc = (R, t) if opt_cam_pose else (R.T, -R.T @ t)
            assert np.abs(c2o[b].numpy() - np.concatenate([Rc, tc[:, None]], 1)).max() < 1e-13
            for i in range(n):
                w = Rc @ cam[b, i].numpy()
                assert np.abs(vd[b * n + i].numpy() - w / np.linalg.norm(w)).max() < 1e-14
                assert np.abs(ro[b * n + i].numpy() - tc).max() < 1e-13
            near, far = np.linalg.norm(tc) - float(half[b]), np.linalg.norm(tc) + float(half[b])
            edges = np.linspace(near, far, S + 1)                     # S equal bins: centres of the bins, + jitter * half a bin
            mid, hw = 0.5 * (edges[1:] + edges[:-1]), 0.5 * (edges[1] - edges[0])
            assert np.abs(z0[b].numpy() - mid).max() < 1e-12 and np.abs(z[b].numpy() - (mid + jit[b].numpy() * hw)).max() < 1e-12
    # the depth vector's corner: one sample sits in the middle of [near, far]
    z1 = LR.pose_rays(rot, tr, cam, half, None, 1, 1)[3]
    assert float((z1[:, 0] - tr.norm(dim=-1)).abs().max()) < 1e-12


# ------------------------------------------------------------------ loss tail
def test_loss_tail_reference_against_a_pixel_loop():
    g = torch.Generator().manual_seed(5)
    B, n, coef = 3, 7, 0.1
    rgb, tgt = torch.rand(B * n, 3, generator=g, dtype=torch.float64), torch.rand(B * n, 3, generator=g, dtype=torch.float64)
    acc = torch.rand(B * n, generator=g, dtype=torch.float64)
    occ = (torch.randint(0, 3, (B * n, 1), generator=g) - 1).double()
    occ[2 * n:] = -1                                                  # the last object: background only
    got = LR.loss_tail(rgb, acc, tgt, occ, coef, n)
    for b in range(B):
        s_rgb = s_occ = s_fg = den = den_fg = 0.0
        for i in range(b * n, (b + 1) * n):
            o = float(occ[i])
            sq = sum((float(rgb[i, c]) - float(tgt[i, c])) ** 2 for c in range(3))
            den += abs(o); den_fg += max(o, 0.0)
            s_rgb += sq * abs(o); s_fg += sq * max(o, 0.0)
            s_occ += math.exp(-o * (0.5 - float(acc[i]))) * abs(o)
        want = [s_rgb / (den + 1e-9) + coef * s_occ / (den + 1e-9), s_rgb / (den + 1e-9), s_occ / (den + 1e-9), s_fg / (den_fg + 1e-9)]
        assert np.abs(got[b].numpy() - np.array(want)).max() < 1e-13, (b, got[b], want)
    assert float(got[2, 3]) == 0.0
    # the oracle's own losses object by object (it reports the PSNR of mse_fg)
    for b in range(B):
        sl = slice(b * n, (b + 1) * n)
        loss, l_rgb, l_occ, psnr = O.optimise_losses(rgb[sl], acc[sl], tgt[sl], occ[sl], coef)
        assert float((got[b, :3] - torch.stack([loss, l_rgb, l_occ])).abs().max()) < 1e-14 and (float(psnr) == math.inf if b == 2 else abs(float(psnr + 10 * torch.log10(got[b, 3]))) < 1e-12)
    # gradients stay finite for the object without foreground
    rgb_r, acc_r = rgb.clone().requires_grad_(), acc.clone().requires_grad_()
    LR.loss_tail(rgb_r, acc_r, tgt, occ, coef, n)[:, 0].sum().backward()
    assert bool(torch.isfinite(rgb_r.grad).all()) and bool(torch.isfinite(acc_r.grad).all()) and float(rgb_r.grad[2 * n:].abs().max()) > 0


# ------------------------------------------------------------------ metric row
@pytest.mark.parametrize("opt_cam_pose", [0, 1])
def test_metric_row_reference(amd, opt_cam_pose):
    """Against the package's own CPU helpers (utils.calc_pose_err, the reference's lines) on poses whose errors are known by construction:
    the object rotation is the target's times a rotation by a chosen angle, the translation the target's plus a chosen offset."""
    U = amd.utils
    g = torch.Generator().manual_seed(6)
    angles = torch.tensor([0.0, 1e-3, 0.7, math.pi - 1e-3, math.pi], dtype=torch.float64)
    B, nl = len(angles), 9
    axis = torch.randn(B, 3, generator=g, dtype=torch.float64); axis = axis / axis.norm(dim=-1, keepdim=True)
    gt_R = torch.linalg.matrix_exp(LR.skew(torch.randn(B, 3, generator=g, dtype=torch.float64)))
    gt_T = torch.randn(B, 3, generator=g, dtype=torch.float64) * 5
    off = torch.randn(B, 3, generator=g, dtype=torch.float64)
    obj_R = torch.linalg.matrix_exp(LR.skew(axis * angles[:, None])) @ gt_R
    obj_t = gt_T + off
    obj = torch.cat([obj_R, obj_t[:, :, None]], -1)
    c2o = obj if opt_cam_pose else torch.cat([obj_R.transpose(-2, -1), -obj_R.transpose(-2, -1) @ obj_t[:, :, None]], -1)
    loss_out = torch.rand(B, 4, generator=g, dtype=torch.float64) * 0.2 + 0.01
    loss_out[1, 3] = 0.0
    d, d0 = torch.rand(B, nl, generator=g, dtype=torch.float64) * 20, torch.rand(B, nl, generator=g, dtype=torch.float64) * 20
    row = LR.metric_row(loss_out, d, d0, c2o, gt_R, gt_T, opt_cam_pose)
    assert float(row[1, 0]) == math.inf and float((row[[0, 2, 3, 4], 0] + 10 * torch.log10(loss_out[[0, 2, 3, 4], 3])).abs().max()) < 1e-13
    assert float((torch.cos(row[:, 2]) - torch.cos(angles)).abs().max()) < 1e-13 and float((row[2, 2] - 0.7).abs()) < 1e-13
    assert float((row[:, 3] - off.norm(dim=-1)).abs().max()) < 1e-12
    err_R, err_T = U.calc_pose_err(obj, torch.cat([gt_R, gt_T[:, :, None]], -1))
    assert float((torch.cos(row[:, 2]) - torch.cos(err_R)).abs().max()) < 1e-13 and float((row[:, 3] - err_T).abs().max()) < 1e-12
    assert float((row[:, 1] - (d - d0).abs().mean(dim=1)).abs().max()) < 1e-8         # (the 1e-8 of the count rule's denominator)
    # counts: zero, inside, above the width (clamped to it), negative (clamped to zero)
    cnt = [0, 4, 12, -3, 9]
    row_c = LR.metric_row(loss_out, d, d0, c2o, gt_R, gt_T, opt_cam_pose, lidar_count=cnt)
    for b, c in enumerate([0, 4, 9, 0, 9]):
        want = sum(abs(float(d[b, i]) - float(d0[b, i])) for i in range(c)) / (c + 1e-8)
        assert abs(float(row_c[b, 1]) - want) < 1e-13
    assert torch.equal(row_c[:, [0, 2, 3]], row[:, [0, 2, 3]])
    first = LR.metric_row(loss_out, d, d0, c2o, gt_R, gt_T, opt_cam_pose, first=True, lidar_count=cnt)
    assert float(first[:, 1].abs().max()) == 0.0
    empty = LR.metric_row(loss_out, d[:, :0], d0[:, :0], c2o, gt_R, gt_T, opt_cam_pose)
    assert float(empty[:, 1].abs().max()) == 0.0 and torch.equal(empty[:, 2:], row[:, 2:])


# ------------------------------------------------------------------ AdamW
def test_adamw_step_matches_torch_optimiser():
    g = torch.Generator().manual_seed(7)
    lr, wd = 0.02, 1e-2
    p0 = torch.randn(300, generator=g, dtype=torch.float64)
    p_t = p0.clone().requires_grad_()
    ref = torch.optim.AdamW([p_t], lr=lr, weight_decay=wd, foreach=False)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 26):
        gr = torch.randn(300, generator=g, dtype=torch.float64) * (0.1 + step % 3)
        if step == 1:
            gr[:20] = 0.0                                             # a zero gradient on the first step: denom = eps, the update 0
        p_t.grad = gr.clone()
        ref.step()
        p, m, v = LR.adamw_step(p, gr, m, v, step, lr, weight_decay=wd)
        assert float((p - p_t.detach()).abs().max()) < 1e-12, step
    st = ref.state[p_t]
    assert float((m - st["exp_avg"]).abs().max()) < 1e-12 and float((v - st["exp_avg_sq"]).abs().max()) < 1e-12


# ------------------------------------------------------------------ latent layers
@pytest.mark.parametrize("sb,tb", [(3, 1), (1, 0), (0, 2)])
def test_latent_reference_matches_the_model_on_the_cpu(amd, sb, tb):
    """Against the model's own per-layer nn.Linear modules in float64 (its CPU path), values and code gradients."""
    torch.manual_seed(sb * 10 + tb)
    m = amd.CodeNeRF(sb, tb).double()
    g = torch.Generator().manual_seed(8)
    B = 3
    sc0, tc0 = torch.randn(B, 256, generator=g, dtype=torch.float64) * 0.3, torch.randn(B, 256, generator=g, dtype=torch.float64) * 0.3
    up = torch.randn(B, sb + tb, 256, generator=g, dtype=torch.float64)
    lat, nxt, _ = LR.model_latent_weights(m)
    grads = []
    for fn in (lambda s, t: LR.latent_layers(s, t, lat, nxt, sb), lambda s, t: (lambda z: (z, m.latent_biases(z)))(m.latent_terms(s, t))):
        s, t = sc0.clone().requires_grad_(), tc0.clone().requires_grad_()
        z, lb = fn(s, t)
        (z * up).sum().backward()
        grads.append((z.detach(), lb.detach(), s.grad, t.grad))
    (z, lb, gs, gt), (z_m, lb_m, gs_m, gt_m) = grads
    assert float((z - z_m).abs().max()) < 1e-13 and float((lb - lb_m).abs().max()) < 1e-13 and bool((z == 0).any()) and bool((z > 0).any())
    for a, b in ((gs, gs_m), (gt, gt_m)):
        assert (a is None) == (b is None) and (a is None or float((a - b).abs().max()) < 1e-12)


# ------------------------------------------------------------------ the API loop's rotation in float32
def test_axis_angle_to_matrix_fp32_across_magnitudes(amd):
    """``driver.axis_angle_to_matrix`` in float32, value and the autograd gradient of (R * G).sum(), against the float64 reference from the
    same float32 inputs.  The gradient is held to rel 5e-5 of its largest entry per rotation vector, the project's tolerance for the pose
    gradient; with b = (1 - cos t)/t^2 it is ~3e-4 off for 1e-4 < |v| < 3e-3 (cos t rounds to 1 or its neighbour)."""
    D = amd.driver
    v = LR.sweep_vectors(ALL_MAGS, seed=9)
    G = torch.randn(len(ALL_MAGS), 3, 3, generator=torch.Generator().manual_seed(10), dtype=torch.float64)
    v64 = v.clone().requires_grad_()
    R64 = LR.rotation(v64)
    (R64 * G).sum().backward()
    v32 = v.float().requires_grad_()
    R32 = D.axis_angle_to_matrix(v32)
    (R32 * G.float()).sum().backward()
    e_val = (R32.detach().double() - R64.detach()).abs().amax((-2, -1))
    e_grad = (v32.grad.double() - v64.grad).abs().amax(-1) / v64.grad.abs().amax(-1)
    for m, a, b in zip(ALL_MAGS, e_val, e_grad):
        print(f"|v| = {m:.6g}: value {float(a):.1e}  gradient rel {float(b):.1e}")
    assert bool(torch.isfinite(v32.grad).all())
    assert float(e_val.max()) < 2e-6
    bad = [(m, float(b)) for m, b in zip(ALL_MAGS, e_grad) if not float(b) < 5e-5]
    assert not bad, bad
