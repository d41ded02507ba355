"""Test helper: the rules of snr_scene_samples_fwd / snr_scene_gather_fwd (include/supnerf_hip.h) in a few lines of torch, dtype-generic
and differentiable with respect to ``cam2obj``.  Its float64 run is the oracle of record for the scene sample kernels; ``existing_route``
is what the package computed before them (``scene.scene_ray_rows`` + the sample lines of ``scene.render_scene_batch``) in any dtype."""
import torch


def cam2obj_of(obj_poses):
    """[R^T | -R^T t] of object poses (Nb,3,4): the two torch ops of ``scene.scene_ray_rows``."""
    R = obj_poses[:, :3, :3].transpose(1, 2)
    return torch.cat([R, -(R @ obj_poses[:, :3, 3:4])], dim=2)


def scene_samples(cam2obj, wlh, rois, pixels, Kvec, jitter, S, adjust_scale=1.0, rend_aabb=True, shapenet_obj_cood=True):
    """dict: xyz, viewdir (Nb*Nr,S,3); z_vals (Nr,Nb*S); hit (Nr,Nb) bool; valid (Nr,) bool; covered (Nr,Nb) bool; gap (Nr,Nb) = far - near."""
    dt, dev = cam2obj.dtype, cam2obj.device
    Nb, Nr = cam2obj.shape[0], pixels.shape[0]
    fx, fy, cx, cy = [torch.as_tensor(float(v), dtype=dt, device=dev) for v in Kvec]
    wlh, rois, pixels = wlh.to(dev, dt), rois.to(dev).long(), pixels.to(dev).long()
    x, y = pixels[:, 0:1], pixels[:, 1:2]                                                        # (Nr,1) against (Nb,)
    live = (rois[:, 2] > rois[:, 0]) & (rois[:, 3] > rois[:, 1])
    covered = live & (x >= rois[:, 0]) & (x < rois[:, 2]) & (y >= rois[:, 1]) & (y < rois[:, 3])      # (Nr,Nb)
    cam = torch.stack([(x[:, 0].to(dt) - cx) / fx, (y[:, 0].to(dt) - cy) / fy, torch.ones(Nr, dtype=dt, device=dev)], -1)
    w = torch.einsum("bij,rj->rbi", cam2obj[:, :, :3], cam)                                      # (Nr,Nb,3)
    u = w / w.norm(dim=-1, keepdim=True)
    diag = wlh.norm(dim=1)
    o = (cam2obj[:, :, 3] / (diag / 2)[:, None])[None].expand_as(u)
    if rend_aabb:
        half = torch.stack([wlh[:, 1], wlh[:, 0], wlh[:, 2]], 1) / diag[:, None]
        zero = u == 0
        inv = 1 / torch.where(zero, torch.ones_like(u), u)
        ta, tb = (-half - o) * inv, (half - o) * inv
        inside = (o > -half) & (o < half)
        inf = torch.full_like(u, float("inf"))
        lo = torch.where(zero, torch.where(inside, -inf, inf), torch.minimum(ta, tb))           # a parallel axis bounds nothing, or misses
        hi = torch.where(zero, torch.where(inside, inf, -inf), torch.maximum(ta, tb))
        near, far = lo.max(-1)[0], hi.min(-1)[0]
    else:
        dist = cam2obj[:, :, 3].norm(dim=1)
        near = ((dist - diag / 2) / (diag / 2))[None].expand(Nr, Nb)
        far = ((dist + diag / 2) / (diag / 2))[None].expand(Nr, Nb)
    hit = covered & (far > near) & (far > 0)
    gap = (far - near).detach()
    jit = torch.zeros(Nr, Nb, S, dtype=dt, device=dev) if jitter is None else jitter.to(dev, dt).view(Nr, Nb, S)
    tau = (torch.arange(S, dtype=dt, device=dev) + jit) / S
    safe = lambda t, fill: torch.where(hit, t, torch.full_like(t, fill))                         # (no value or gradient from pairs that are not hit)
    near, far = safe(near, 0.0), safe(far, 0.0)
    u = torch.where(hit[..., None], u, torch.tensor([0.0, 0.0, 1.0], dtype=dt, device=dev).expand_as(u))
    z = near[..., None] * (1 - tau) + far[..., None] * tau                                        # (Nr,Nb,S)
    step = z[..., None] * u[:, :, None, :]
    xyz = (o[:, :, None, :] + step) * adjust_scale
    z_vals = step.norm(dim=-1) * (diag / 2)[None, :, None]
    xyz = torch.where(hit[..., None, None], xyz, torch.zeros_like(xyz))
    z_vals = torch.where(hit[..., None], z_vals, torch.full_like(z_vals, -1.0))
    viewdir = u[:, :, None, :].expand(Nr, Nb, S, 3)
    if shapenet_obj_cood:
        xyz = torch.stack([-xyz[..., 1], xyz[..., 0], xyz[..., 2]], -1)
        viewdir = torch.stack([-viewdir[..., 1], viewdir[..., 0], viewdir[..., 2]], -1)
    return dict(xyz=xyz.permute(1, 0, 2, 3).reshape(Nb * Nr, S, 3), viewdir=viewdir.permute(1, 0, 2, 3).reshape(Nb * Nr, S, 3),
                z_vals=z_vals.reshape(Nr, Nb * S), hit=hit, valid=hit.any(1), covered=covered, gap=gap)


def gather(sigmas, rgbs, hit, S):
    """The two permutes and two ``torch.where`` of ``scene.render_scene_batch``: sigma rows (Nr,Nb*S), rgb rows (Nr,Nb*S,3)."""
    Nr, Nb = hit.shape
    rgb = rgbs.reshape(Nb, Nr, S, 3).permute(1, 0, 2, 3).reshape(Nr, Nb * S, 3)
    sig = sigmas.reshape(Nb, Nr, S).permute(1, 0, 2).reshape(Nr, Nb * S)
    empty = ~hit.bool()[:, :, None].expand(Nr, Nb, S).reshape(Nr, Nb * S)
    return torch.where(empty, torch.zeros_like(sig), sig), torch.where(empty[..., None], torch.ones_like(rgb), rgb)


def existing_route(scene, obj_poses, wlh, K, pixels, H, W, jitter, S, adjust_scale=1.0, rend_aabb=True, shapenet_obj_cood=True):
    """``scene.scene_ray_rows`` followed by the sample lines of ``scene.render_scene_batch`` in the dtype of ``obj_poses`` (the package itself
    casts the rows to fp32 there): xyz, viewdir (Nb*Nr,S,3), z_vals (Nr,Nb*S), hit (Nr,Nb) = the row's depth is not -1."""
    dt = obj_poses.dtype
    rows, _ = scene.scene_ray_rows(obj_poses, wlh, K, pixels, H, W, rend_aabb=rend_aabb)
    Nr, Nb = rows.shape[:2]
    rays = rows.reshape(-1, 8)
    step = 1.0 / S
    t = torch.linspace(0, 1 - step, S, dtype=dt, device=rays.device)[None, :].repeat(rays.shape[0], 1)
    if jitter is not None:
        t = t + jitter.to(rays.device, dt) * step
    z_coarse = rays[:, 6:7] * (1 - t) + rays[:, 7:8] * t
    empty = z_coarse == -1
    xyz = rays[:, None, :3] + z_coarse[:, :, None] * rays[:, None, 3:6]
    d = wlh.to(rays.device, dt).norm(dim=1).view(1, Nb, 1, 1).repeat(Nr, 1, 1, 1).flatten(0, 1)
    z_vals = torch.norm((xyz - rays[:, None, :3]) * (d / 2), p=2, dim=-1)
    z_vals = torch.where(empty, torch.full_like(z_vals, -1.0), z_vals)
    xyz = xyz.view(Nr, Nb, S, 3).permute(1, 0, 2, 3).flatten(0, 1) * adjust_scale
    viewdir = rays[:, 3:6].view(Nr, Nb, 1, 3).permute(1, 0, 2, 3).expand(Nb, Nr, S, 3).flatten(0, 1)
    if shapenet_obj_cood:
        xyz = torch.stack([-xyz[..., 1], xyz[..., 0], xyz[..., 2]], -1)
        viewdir = torch.stack([-viewdir[..., 1], viewdir[..., 0], viewdir[..., 2]], -1)
    return dict(xyz=xyz, viewdir=viewdir, z_vals=z_vals.view(Nr, Nb * S), hit=~empty.view(Nr, Nb, S)[:, :, 0])


def pair_mask(mask_pairs, S):
    """(Nr,Nb) pair mask -> masks for the object-major (Nb*Nr,S,3) and the pixel-major (Nr,Nb*S) outputs."""
    Nr, Nb = mask_pairs.shape
    return (mask_pairs.t().reshape(Nb * Nr, 1, 1).expand(Nb * Nr, S, 3), mask_pairs[:, :, None].expand(Nr, Nb, S).reshape(Nr, Nb * S))
