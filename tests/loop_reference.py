"""Test helper: plain-torch references of the small kernels around the render in the optimise loop (csrc/snr_loop.hip, csrc/snr_loss.hip):
pose -> rays, loss tail, metric row, AdamW, latent layers.  Dtype-generic: every function computes in the dtype of its arguments, float64
where the tests want the true value, float32 for one sample of the rounding noise.  tests/test_loop_reference_cpu.py checks each of them
against an independent formulation, so that a wrong reference cannot pass a wrong kernel."""
import math

import torch

# rotation magnitudes the tests sweep: zero, both sides of the series threshold |v|^2 = 1e-8, the band above it where 1 - cos t loses its
# digits in fp32, generic angles, and both sides of a half turn
MAGNITUDES = [0.0, 1e-6, 9.9e-5, 1.01e-4, 3e-4, 1e-3, 1e-2, 1.0, 3.1, math.pi - 1e-6, 6.0]
BAND_MAGNITUDES = [1.5e-4, 5e-4, 2e-3, 2.9e-3]            # a few more inside 1e-4 < |v| < 3e-3


def sweep_vectors(mags, seed=0):
    """(len(mags), 3) float64 rotation vectors of the given lengths about random axes, each exactly representable in float32 (so that
    the float32 code under test and the float64 reference start from the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    axis = torch.randn(len(mags), 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    return (axis * torch.tensor(mags, dtype=torch.float64)[:, None]).float().double()


def skew(v):
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    zero = torch.zeros_like(x)
    return torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(*v.shape[:-1], 3, 3)


def rotation(v):
    """(...,3) rotation vector -> (...,3,3): R = I + a K + b K^2 with a = sin(t)/t and b = 2 sin^2(t/2)/t^2 (no cancellation at small t),
    the series 1 - t^2/6, 1/2 - t^2/24 below t^2 = 1e-8 (their next terms, t^4/120 and t^4/720, are below 1e-18 there)."""
    t2 = (v * v).sum(-1, keepdim=True)
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)       # (the branch not taken stays finite for autograd)
    t = torch.sqrt(t2s)
    s = torch.sin(t / 2)
    a = torch.where(small, 1 - t2 / 6, torch.sin(t) / t)
    b = torch.where(small, 0.5 - t2 / 24, 2 * s * s / t2s)
    K = skew(v)
    eye = torch.eye(3, dtype=v.dtype, device=v.device).expand(K.shape)
    return eye + a[..., None] * K + b[..., None] * (K @ K)


def camera_pose(rot_vec, trans_vec, opt_cam_pose):
    """(B,3,4) camera-in-object pose: the object pose [R | t] inverted, or taken as it is when the camera pose itself is optimised."""
    R = rotation(rot_vec)
    t = trans_vec.unsqueeze(-1)
    if not opt_cam_pose:
        Rc = R.transpose(-2, -1)
        return torch.cat([Rc, -Rc @ t], -1)
    return torch.cat([R, t], -1)


def rays_of_pose(c2o, cam, half, jit, S):
    """rays_o (B*n,3), viewdir (B*n,3), z (B,S) of the pixel table ``cam`` (B,n,3) under the poses ``c2o`` (B,3,4); the depths are detached
    from the pose; ``jit`` (B,S) or None."""
    world = (cam[:, :, None, :] * c2o[:, None, :3, :3]).sum(-1)
    unit = world / torch.norm(world, dim=-1, keepdim=True)
    origin = c2o[:, None, :3, 3].expand(world.shape)
    dist = c2o[:, :, 3].detach().norm(dim=-1)
    near, far = (dist - half)[:, None], (dist + half)[:, None]
    idx = torch.arange(S, dtype=cam.dtype)[None, :]
    hw = (far - near) / (2 * S)
    start, end = near + hw, far - hw
    step = (end - start) / max(S - 1, 1)
    z = torch.where(idx < S // 2, start + step * idx, end - step * (S - 1 - idx))
    if jit is not None:
        z = z + jit * hw
    return origin.reshape(-1, 3), unit.reshape(-1, 3), z


def pose_rays(rot_vec, trans_vec, cam, half, jit, S, opt_cam_pose):
    """cam2opt (B,3,4), rays_o, viewdir, z of ``ops.PoseRays`` (src/optimizer_nuscenes.py:685-699, src/utils.py:107-135,159-164,468-469)."""
    c2o = camera_pose(rot_vec, trans_vec, opt_cam_pose)
    return (c2o,) + rays_of_pose(c2o, cam, half, jit, S)


def loss_tail(rgb, acc, tgt, occ, coef, n):
    """(B,4) = [loss, loss_rgb, loss_occ, mse_fg] per object of ``n`` rays (src/optimizer_nuscenes.py:729-744): squared colour error and
    exp(-occ (1/2 - acc)) averaged over the labelled pixels (|occ| = 1), the colour error over the foreground (occ = 1) alone.  mse_fg itself
    rather than its PSNR, so that an object without foreground (mse_fg = 0) keeps finite gradients."""
    B = acc.numel() // n
    rgb, tgt, acc, occ = rgb.reshape(B, n, 3), tgt.reshape(B, n, 3), acc.reshape(B, n, 1), occ.reshape(B, n, 1)
    a, fg = occ.abs(), occ.clamp_min(0)
    den = a.sum((1, 2)) + 1e-9
    sq = (rgb - tgt) ** 2
    l_rgb = (sq * a).sum((1, 2)) / den
    l_occ = (torch.exp(-occ * (0.5 - acc)) * a).sum((1, 2)) / den
    mse_fg = (sq * fg).sum((1, 2)) / (fg.sum((1, 2)) + 1e-9)
    return torch.stack([l_rgb + coef * l_occ, l_rgb, l_occ, mse_fg], 1)


def clamped_counts(lidar_count, B, n_lidar):
    if lidar_count is None:
        return [n_lidar] * B
    return [min(max(int(c), 0), n_lidar) for c in lidar_count]


def metric_row(loss_out, d_vec, d0, cam2opt, gt_R, gt_T, opt_cam_pose, first=False, lidar_count=None):
    """(B,4) = [PSNR of mse_fg (loss_out[:,3]), sum |d - d0| over the object's first cnt depth pixels / (cnt + 1e-8), geodesic angle between
    the predicted object rotation and gt_R, |predicted - gt translation|] (src/optimizer_nuscenes.py:739-765,1736-1741, src/utils.py:713-722).
    cnt = lidar_count clamped to [0, n_lidar], n_lidar without counts; on the first iteration d0 := d, so the depth column is 0."""
    B, n_lidar = cam2opt.shape[0], d_vec.shape[-1]
    pred_R = cam2opt[:, :, :3] if opt_cam_pose else cam2opt[:, :, :3].transpose(-2, -1)
    pred_t = cam2opt[:, :, 3:] if opt_cam_pose else -pred_R @ cam2opt[:, :, 3:]
    psnr = -10 * torch.log10(loss_out[:, 3])
    depth = []
    for b, c in enumerate(clamped_counts(lidar_count, B, n_lidar)):
        diff = torch.zeros(c, dtype=d_vec.dtype) if first else (d_vec[b, :c] - d0[b, :c]).abs()
        depth.append(diff.sum() / (c + 1e-8))
    tr = (pred_R * gt_R).sum((-2, -1)).clamp(-1, 3)                    # trace(pred_R gt_R^T)
    ang = torch.acos(((tr - 1) / 2).clamp(-1, 1))
    err_t = (pred_t[:, :, 0] - gt_T).norm(dim=1)
    return torch.stack([psnr, torch.stack(depth).to(psnr.dtype), ang, err_t], dim=1)


def adamw_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """One step (number ``step``, from 1) of torch.optim.AdamW's single-tensor update, amsgrad off -> (p, m, v), nothing in place."""
    b1, b2 = betas
    p = p * (1 - lr * weight_decay)
    m = torch.lerp(m, g, 1 - b1)
    v = v * b2 + (1 - b2) * g * g
    bias1, bias2 = 1 - b1 ** step, 1 - b2 ** step
    denom = v.sqrt() / math.sqrt(bias2) + eps
    return p - (lr / bias1) * (m / denom), m, v


def latent_layers(sc, tc, lat, nxt, shape_blocks):
    """z (B, n_lat, 256), folded bias (B, n_lat, 256) in the per-layer form (src/model_supnerf.py:253,261): z_j = ReLU(W_j code + b_j) with the
    shape code for the first ``shape_blocks`` layers and the texture code for the rest, bias_j = W'_j z_j + b'_j.
    ``lat``, ``nxt``: [(weight (256,256), bias (256,)), ...] of the latent layers and of the layers their outputs fold into."""
    z = torch.stack([torch.relu((sc if j < shape_blocks else tc) @ w.t() + b) for j, (w, b) in enumerate(lat)], 1)
    lb = torch.stack([z[:, j] @ w.t() + b for j, (w, b) in enumerate(nxt)], 1)
    return z, lb


def model_latent_weights(m, dtype=torch.float64):
    """(lat, nxt, shape_blocks) of a CodeNeRF for ``latent_layers``, detached, on the CPU."""
    sd = m.state_dict()
    c = lambda name: (sd[name + ".0.weight"].detach().cpu().to(dtype), sd[name + ".0.bias"].detach().cpu().to(dtype))
    sb, tb = m.shape_blocks, m.texture_blocks
    lat = [c(f"shape_latent_layer_{j + 1}") for j in range(sb)] + [c(f"texture_latent_layer_{j + 1}") for j in range(tb)]
    nxt = [c(f"shape_layer_{j + 1}") for j in range(sb)] + [c(f"texture_layer_{j + 1}") for j in range(tb)]
    return lat, nxt, sb
