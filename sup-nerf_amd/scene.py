"""Multi-object scene rendering: the counterpart of ``OptimizerDemo.vis_scene`` (scripts/demo.py:425-579).

All reconstructed objects are rendered into one camera view: every pixel gets one ray per object (in that object's
frame, origin divided by diag/2, box entry/exit depths from the slab test, -1 where the object does not cover the
pixel); the samples of all objects are decoded in ONE batched-code decoder launch per ray batch (object-major rays,
``Nb`` codes), merged per pixel by metric depth and composited against white by ``ops.scene_composite`` (HIP).

The method's attributes (``self.obj_poses``, ``self.obj_wlh``, ``self.shapecodes`` ...) are function arguments here;
the ray table is built on the host exactly like the reference does (python loop over a handful of objects).

``vis_scene`` makes pictures.  ``render_scene`` renders listed pixels with autograd to the codes and the object poses: its rows come from
``scene_ray_rows`` (torch ops on the device) and its composite from ``ops.SceneComposite`` (HIP forward and backward); with ``fused=True``
rows, samples and regrouping are HIP launches too (``render_pairs``).

What lies between the object poses and the kernels is stated once, here: the box corners (``corners_of_box_batch``), the roi (``scene_rois``,
which ``scene_rays``, ``scene_ray_rows`` and the fused route all call), the pixels the live rois cover (``roi_pixels``), the intrinsics as host
floats (``K_vector``), the fused chain SceneSamples -> decoder -> SceneGather -> composite (``render_pairs``: ``render_scene(fused=True)`` and
``driver.optimize_scene`` differ only in the decoder call they hand it; with a ``capacity`` its compact form, which decodes only the pairs that hit) and the choice between the composite with and without a backward
(``_composite``).  The rigid inverse [R^T | -(R^T t)] is ``utils.invert_pose``.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from . import utils as U
from ._lib import SnrError


_BOX_SIGNS = {}


def corners_of_box_batch(obj_poses: torch.Tensor, wlh: torch.Tensor) -> torch.Tensor:
    """(Nb,3,8) box corners in the camera frame, nuScenes convention (src/utils.py:1110-1148, is_kitti=False): x forward, y left, z up.
    The (3,8) sign table is kept per device and dtype, so a call inside an optimise loop uploads nothing."""
    key = (wlh.device, wlh.dtype)
    if key not in _BOX_SIGNS:
        _BOX_SIGNS[key] = torch.tensor([[1, 1, 1, 1, -1, -1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1], [1, 1, -1, -1, 1, 1, -1, -1]],
                                       dtype=wlh.dtype, device=wlh.device)
    half = wlh / 2
    local = torch.stack([half[:, 1], half[:, 0], half[:, 2]], dim=1)[:, :, None] * _BOX_SIGNS[key]
    return torch.matmul(obj_poses[:, :, :3], local) + obj_poses[:, :, 3:4]


def view_points_batch(points: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """Perspective projection (src/utils.py:1032-1075 with normalize=True): rows (u, v, 1)."""
    uvw = torch.matmul(K, points)
    return uvw / uvw[:, 2:3, :]


def scene_rays(obj_poses, obj_wlh, K, H, W, manipulation=(0.0, 0.0, 0.0), rend_aabb=True):
    """(H,W,Nb,8) ray table [o/(diag/2), dir, near, far], valid-pixel mask (H*W,), diagonals (Nb,) -- scripts/demo.py:437-523.
    CPU tensors, as in the reference."""
    obj_poses, obj_wlh, K = obj_poses.detach().cpu().float(), obj_wlh.detach().cpu().float(), K.detach().cpu().float()
    Nb = obj_poses.shape[0]
    table = torch.full((H, W, Nb, 8), -1.0)
    poses = obj_poses.clone()
    poses[:, :, 3] += torch.tensor(manipulation, dtype=torch.float32).unsqueeze(0)
    rois = scene_rois(poses, obj_wlh, K, H, W).tolist()
    diags = []
    for i in range(Nb):
        x0, y0, x1, y1 = rois[i]
        cam_pose = U.invert_pose(poses[i])
        wlh = obj_wlh[i].numpy()
        diag = np.linalg.norm(wlh).astype(np.float32)
        diags.append(diag)
        if x1 <= x0 or y1 <= y0:
            continue
        rays_o, viewdir = U.get_rays(K, cam_pose, [x0, y0, x1, y1])
        table[y0:y1, x0:x1, i, :3] = rays_o.view(y1 - y0, x1 - x0, 3) / (diag / 2)
        table[y0:y1, x0:x1, i, 3:6] = viewdir.view(y1 - y0, x1 - x0, 3)
        if rend_aabb:
            ow, ol, oh = wlh
            half = torch.from_numpy(np.asarray([ol / diag, ow / diag, oh / diag]).reshape(1, 3).repeat(rays_o.shape[0], axis=0))   # float64 like np.asarray
            o_n = torch.from_numpy(rays_o.numpy() / (diag / 2))
            t_near, t_far, hit = U._slab(o_n, viewdir, -half, half)
            near = torch.full((rays_o.shape[0],), -1.0)
            far = torch.full((rays_o.shape[0],), -1.0)
            near[hit] = t_near[hit].float(); far[hit] = t_far[hit].float()
            table[y0:y1, x0:x1, i, 6] = near.view(y1 - y0, x1 - x0)
            table[y0:y1, x0:x1, i, 7] = far.view(y1 - y0, x1 - x0)
        else:
            dist = torch.linalg.norm(cam_pose[:, -1])
            table[y0:y1, x0:x1, i, 6] = (dist - diag / 2) / (diag / 2)
            table[y0:y1, x0:x1, i, 7] = (dist + diag / 2) / (diag / 2)
    diags = torch.tensor(diags, dtype=torch.float32)
    valid = (table[:, :, :, 7].view(H * W, Nb) - table[:, :, :, 6].view(H * W, Nb)).max(-1)[0] > 0
    return table, valid, diags


def scene_rois(obj_poses, obj_wlh, K, H, W, manipulation=(0.0, 0.0, 0.0)):
    """(Nb,4) int32 [x0, y0, x1, y1]: every object's roi, THE roi of ``scene_rays``, ``scene_ray_rows`` and the fused route -- the truncated
    projection of the box corners at the (manipulated) pose, clamped to the image like ``roi_process(roi, H, W, 0, False)`` -- in fp32 on the
    device of ``obj_poses``, without gradient.  An object whose roi has x1 <= x0 or y1 <= y0 covers no pixel."""
    with torch.no_grad():
        dev = obj_poses.device
        poses = obj_poses.detach().float()
        if any(float(m) != 0.0 for m in manipulation):
            poses = poses.clone()
            poses[:, :, 3] += torch.tensor(manipulation, dtype=torch.float32, device=dev).unsqueeze(0)
        wlh, K32 = obj_wlh.detach().to(dev, torch.float32), K.detach().to(dev, torch.float32)
        uv = view_points_batch(corners_of_box_batch(poses, wlh), K32.unsqueeze(0).repeat(poses.shape[0], 1, 1))
        rois = torch.stack([uv[:, 0].min(dim=1)[0], uv[:, 1].min(dim=1)[0], uv[:, 0].max(dim=1)[0], uv[:, 1].max(dim=1)[0]], dim=1).type(torch.int32)
        return torch.stack([rois[:, 0].clamp(min=0), rois[:, 1].clamp(min=0), rois[:, 2].clamp(max=W - 1), rois[:, 3].clamp(max=H - 1)], 1)


def _host_rois(poses, obj_wlh, K, H, W):
    """``scene_rois`` of the (already manipulated) poses in fp32 on the host, whatever their dtype and device: the ONE host read of the poses
    that ``scene_ray_rows`` and the fused route make, so both see the same pixels."""
    return scene_rois(poses.detach().cpu().float(), obj_wlh.detach().cpu(), K.detach().cpu(), H, W)


def roi_pixels(rois, H, W):
    """(Nr,2) int64 (x, y): the pixels of an H x W image inside the union of the live rois (x1 > x0 and y1 > y0; upper bounds exclusive), row-major."""
    cover = torch.zeros(H, W, dtype=torch.bool)
    for x0, y0, x1, y1 in torch.as_tensor(rois).tolist():
        if x1 > x0 and y1 > y0:
            cover[y0:y1, x0:x1] = True
    ys, xs = torch.nonzero(cover, as_tuple=True)
    return torch.stack([xs, ys], 1)


def K_vector(K):
    """(fx, fy, cx, cy) of the intrinsics as host floats (fp32 values): one host copy, what ``ops.SceneSamples`` takes."""
    Kc = torch.as_tensor(K).detach().cpu().float()
    return float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2])


def _composite(sig, rgb, z_vals, n_samples):
    """The merge-composite against white of pixel-major rows: ``ops.SceneComposite`` when a gradient is wanted, else the forward launch alone."""
    if torch.is_grad_enabled() and (sig.requires_grad or rgb.requires_grad or z_vals.requires_grad):
        return ops.SceneComposite.apply(sig, rgb, z_vals, True, n_samples)              # gradients to the codes and, through the rows, to poses
    return ops.scene_composite(sig, rgb, z_vals, white_bkgd=True, run_length=n_samples)


def render_scene_batch(model, device, batch_rays, diags, shapecodes, texturecodes, n_samples, jitter=None, adjust_scale=1.0,
                       shapenet_obj_cood=True):
    """One ray batch (Nr, Nb, 8) -> rgb (Nr,3), depth (Nr,), acc_trans (Nr,)  (scripts/demo.py:527-566)."""
    dev = torch.device(device)
    Nr, Nb = batch_rays.shape[:2]
    rays = batch_rays.reshape(-1, 8)
    step = 1.0 / n_samples
    t = torch.linspace(0, 1 - step, n_samples)[None, :].repeat(rays.shape[0], 1)
    if jitter is not None and jitter.device.type == dev.type and dev.index in (None, jitter.device.index):
        t = t.to(dev) + jitter * step                                                  # a draw that lives on the device stays there
    else:
        t = t + (torch.rand_like(t) if jitter is None else jitter.cpu()) * step        # CPU draw, like the reference's CPU ray table
    rays, t = rays.to(dev), t.to(dev)
    z_coarse = rays[:, 6:7] * (1 - t) + rays[:, 7:8] * t
    empty = z_coarse == -1
    xyz = rays[:, None, :3] + z_coarse[:, :, None] * rays[:, None, 3:6]
    d = diags.to(dev).view(1, Nb, 1, 1).repeat(Nr, 1, 1, 1).flatten(0, 1)
    z_vals = torch.norm((xyz - rays[:, None, :3]) * (d / 2), p=2, dim=-1)
    z_vals = torch.where(empty, torch.full_like(z_vals, -1.0), z_vals)
    xyz = xyz.view(Nr, Nb, n_samples, 3).permute(1, 0, 2, 3).flatten(0, 1) * adjust_scale
    viewdir = rays[:, 3:6].view(Nr, Nb, 1, 3).permute(1, 0, 2, 3).expand(Nb, Nr, n_samples, 3).flatten(0, 1)
    if shapenet_obj_cood:
        xyz = torch.stack([-xyz[..., 1], xyz[..., 0], xyz[..., 2]], -1)
        viewdir = torch.stack([-viewdir[..., 1], viewdir[..., 0], viewdir[..., 2]], -1)
    sig, rgb = model(xyz.contiguous(), viewdir.contiguous(), shapecodes.to(dev), texturecodes.to(dev))   # object-major, Nb codes
    rgb = rgb.view(Nb, Nr, n_samples, 3).permute(1, 0, 2, 3).reshape(Nr, Nb * n_samples, 3)
    sig = sig.view(Nb, Nr, n_samples).permute(1, 0, 2).reshape(Nr, Nb * n_samples)
    empty = empty.view(Nr, Nb * n_samples)
    rgb = torch.where(empty[..., None], torch.ones_like(rgb), rgb)                       # empty space: white, zero density
    sig = torch.where(empty, torch.zeros_like(sig), sig)
    z_vals = z_vals.view(Nr, Nb * n_samples)
    return _composite(sig, rgb, z_vals, n_samples)


def scene_ray_rows(obj_poses, obj_wlh, K, pixels, H, W, manipulation=(0.0, 0.0, 0.0), rend_aabb=True):
    """rows (Nr, Nb, 8), valid (Nr,): the rows ``scene_rays`` writes for the integer pixels ``pixels`` (Nr, 2) = (x, y), made with torch
    ops on the device and in the dtype of ``obj_poses`` (Nb,3,4) and differentiable with respect to it.

    Every object's roi is ``scene_rois`` of the manipulated poses, in fp32 on the host like ``scene_rays``' and treated as a constant: that
    is this function's ONE host read of the poses.  A pixel outside an object's roi
    gets the all -1 row; inside it the row holds origin / (diag/2) and direction, and near / far from the slab test
    (``utils._slab_guarded``), -1 / -1 where the ray misses the box, or the sphere bounds when ``rend_aabb`` is False.  Rays are those of
    ``utils.get_rays_specified`` for the object-from-camera pose.  ``valid``: some object's far - near is positive, like ``scene_rays``' mask."""
    dev, dt = obj_poses.device, obj_poses.dtype
    Nb = obj_poses.shape[0]
    pixels = torch.as_tensor(pixels).to(dev)
    poses = torch.cat([obj_poses[:, :, :3], obj_poses[:, :, 3:4] + torch.tensor(manipulation, dtype=dt, device=dev).view(1, 3, 1)], dim=2)
    rois = _host_rois(poses, obj_wlh, K, H, W).to(dev)                                                            # the one host read
    px, py = pixels[:, 0], pixels[:, 1]
    in_roi = (px[None, :] >= rois[:, 0:1]) & (px[None, :] < rois[:, 2:3]) & (py[None, :] >= rois[:, 1:2]) & (py[None, :] < rois[:, 3:4])   # (Nb,Nr); a dead roi holds no pixel

    wlh, Kd = obj_wlh.detach().to(dev, dt), K.detach().to(dev, dt)
    diag = torch.linalg.norm(wlh, dim=1)                                                                           # (Nb,)
    cam2obj = U.invert_pose(poses)
    R_c2o, origin = cam2obj[:, :, :3], cam2obj[:, :, 3]                                                            # origin (Nb,3): the camera in the object frame
    fx, fy = px.to(torch.float32).to(dt), py.to(torch.float32).to(dt)
    cam = torch.stack([(fx - Kd[0, 2]) / Kd[0, 0], (fy - Kd[1, 2]) / Kd[1, 1], torch.ones_like(fx)], -1)          # (Nr,3)
    world = (cam[None, :, None, :] * R_c2o[:, None, :, :]).sum(-1)                                                 # (Nb,Nr,3)
    unit = world / torch.norm(world, dim=-1, keepdim=True)
    o_n = (origin / (diag / 2)[:, None])[:, None, :].expand_as(unit)
    if rend_aabb:
        half = torch.stack([wlh[:, 1] / diag, wlh[:, 0] / diag, wlh[:, 2] / diag], 1)[:, None, :].expand_as(unit)
        t_near, t_far, hit = U._slab_guarded(o_n, unit, -half, half)
        hit = hit & in_roi
        near = torch.where(hit, t_near, torch.full_like(t_near, -1.0))
        far = torch.where(hit, t_far, torch.full_like(t_far, -1.0))
    else:
        dist = torch.linalg.norm(origin, dim=1)
        near = ((dist - diag / 2) / (diag / 2))[:, None].expand(Nb, pixels.shape[0])
        far = ((dist + diag / 2) / (diag / 2))[:, None].expand(Nb, pixels.shape[0])
    rows = torch.cat([o_n, unit, near[..., None], far[..., None]], dim=-1)                                         # (Nb,Nr,8)
    rows = torch.where(in_roi[..., None], rows, torch.full_like(rows, -1.0)).permute(1, 0, 2)
    valid = (rows[:, :, 7] - rows[:, :, 6]).max(-1)[0] > 0
    return rows, valid.detach()


def render_scene(model, device, obj_poses, obj_wlh, shapecodes, texturecodes, K, pixels, H, W, n_samples, jitter=None,
                 manipulation=(0.0, 0.0, 0.0), rend_aabb=True, shapenet_obj_cood=True, adjust_scale=1.0, fused=False, compact=False, capacity=None,
                 info: Optional[dict] = None):
    """rgb (Nr,3), depth (Nr,), acc_trans (Nr,) of the scene at the listed integer pixels (Nr,2) = (x, y), with autograd to
    ``shapecodes``, ``texturecodes`` and ``obj_poses``: ``render_scene_batch`` of ``scene_ray_rows``.  ``jitter``: (Nr*Nb, S) draws in
    [0,1), default ``torch.rand_like``.  Every listed pixel is rendered; one that no object covers comes out white.
    ``fused`` (native decoders): rows and samples in one launch (``ops.SceneSamples``) and the decoder's outputs regrouped in one
    (``ops.SceneGather``), each with a one-launch backward, instead of ~65 torch launches each way; same rois, same jitter draw.
    ``compact`` (with ``fused``): the decoder sees only the pairs that hit, ``capacity`` slots per object (a multiple of 32,
    ``ops.scene_capacity``).  ``capacity=None`` reads the Nb hit counts once -- the route's SECOND host read, after the roi read -- and takes
    ``ops.scene_capacity`` of the largest, so no pair is dropped; an int makes no read, and hit pairs of an object beyond it render as
    misses.  ``info`` receives ``count`` (Nb,) int32, every object's true number of hits, and ``capacity``."""
    if obj_poses.shape[0] != shapecodes.shape[0] or obj_poses.shape[0] != texturecodes.shape[0] or obj_poses.shape[0] != obj_wlh.shape[0]:
        raise SnrError("render_scene: obj_poses, obj_wlh, shapecodes and texturecodes must describe the same number of objects")
    dev = torch.device(device)
    if compact and not fused:
        raise SnrError("render_scene(compact=True) is a variant of the fused route: pass fused=True")
    if capacity is not None and not compact:
        raise SnrError("render_scene: capacity belongs to compact=True")
    if fused:
        return _render_scene_fused(model, dev, obj_poses.to(dev), obj_wlh, shapecodes, texturecodes, K, pixels, H, W, n_samples, jitter, manipulation,
                                   rend_aabb, shapenet_obj_cood, adjust_scale, compact, capacity, info)
    rows, _ = scene_ray_rows(obj_poses.to(dev), obj_wlh, K, pixels, H, W, manipulation, rend_aabb)
    diags = torch.linalg.norm(obj_wlh.detach().float(), dim=1)
    return render_scene_batch(model, device, rows.float(), diags, shapecodes, texturecodes, n_samples, jitter, adjust_scale, shapenet_obj_cood)


def _render_scene_fused(model, dev, obj_poses, obj_wlh, shapecodes, texturecodes, K, pixels, H, W, n_samples, jitter, manipulation, rend_aabb,
                        shapenet_obj_cood, adjust_scale, compact=False, capacity=None, info=None):
    """``render_scene`` with the rows, samples and regrouping on the HIP kernels; the decoder and the composite as on the default route."""
    if not U._is_native(model):
        raise SnrError("render_scene(fused=True) needs the package's own decoder; a foreign decoder renders on the default route")
    Nb = obj_poses.shape[0]
    pixels = torch.as_tensor(pixels).to(dev, torch.int32)
    Nr = pixels.shape[0]
    poses = torch.cat([obj_poses[:, :, :3], obj_poses[:, :, 3:4] + torch.tensor(manipulation, dtype=obj_poses.dtype, device=dev).view(1, 3, 1)], dim=2)
    rois = _host_rois(poses, obj_wlh, K, H, W).to(dev)                                              # as in scene_ray_rows
    if jitter is None:
        jitter = torch.rand(Nr * Nb, n_samples)                                                      # CPU draw, like render_scene_batch
    cam2obj, wlh, Kvec = U.invert_pose(poses).float(), obj_wlh.detach().to(dev), K_vector(K)
    if compact and capacity is None:                                                                 # the second host read: Nb counts
        capacity = ops.scene_capacity(int(ops.scene_pair_hits(cam2obj, wlh, rois, pixels, Kvec, rend_aabb).sum(0, dtype=torch.int32).max()) if Nr else 0)
    out = render_pairs(lambda x, d: model(x, d, shapecodes.to(dev), texturecodes.to(dev)), cam2obj, wlh, rois, pixels, Kvec, jitter.to(dev), n_samples,
                       adjust_scale, rend_aabb, shapenet_obj_cood, capacity)
    if compact and info is not None:
        info["count"], info["capacity"] = out[4], capacity
    return out[:3]


def render_pairs(decode, cam2obj, wlh, rois, pixels, Kvec, jitter, n_samples, adjust_scale, rend_aabb, shapenet_obj_cood, capacity=None):
    """THE fused chain of the scene path, all operands on the GPU: rows and samples of every (pixel, object) pair (``ops.SceneSamples``; cam2obj
    (Nb,3,4) differentiable, rois (Nb,4) and pixels (Nr,2) int32, Kvec from ``K_vector``, jitter (Nr*Nb,S) or None), ``decode(xyz, viewdir)
    -> (sigmas, rgbs)`` on the object-major points, ``ops.SceneGather``, the merge-composite.  -> rgb (Nr,3), depth (Nr,), acc_trans (Nr,), hit
    (Nr,Nb) uint8.

    ``capacity`` (an int, a multiple of 32): the compact chain -- the hit flags (``ops.scene_pair_hits``), their prefix sum along the pixels,
    ``ops.SceneSamplesCompact``, ``decode`` on Nb * capacity * S points, ``ops.SceneGatherCompact``, the same composite; no host read.  -> rgb,
    depth, acc_trans, kept (Nr,Nb) uint8, count (Nb,) int32: an object's hit pairs beyond ``capacity`` (count - capacity of them) render as
    misses."""
    compact = capacity is not None
    lists = (cam2obj, wlh, rois, pixels, Kvec, jitter, n_samples, adjust_scale, rend_aabb, shapenet_obj_cood)
    if compact:
        scan = torch.cumsum(ops.scene_pair_hits(cam2obj, wlh, rois, pixels, Kvec, rend_aabb).to(torch.int32), 0, dtype=torch.int32)
        count = scan[-1] if scan.shape[0] else scan.new_zeros(scan.shape[1])
    # flag: hit | kept; last: valid (unused) | pair_of_slot
    xyz, viewdir, z_vals, flag, last = ops.SceneSamplesCompact.apply(*lists, scan, capacity) if compact else ops.SceneSamples.apply(*lists)
    sig, rgb = decode(xyz, viewdir)                                                                  # object-major, Nb codes, Nr | capacity rows each
    sig, rgb = ops.SceneGatherCompact.apply(sig, rgb, scan, flag, last, n_samples) if compact else ops.SceneGather.apply(sig, rgb, flag, n_samples)
    out = _composite(sig, rgb, z_vals, n_samples)
    return (*out, flag, count) if compact else (*out, flag)


def vis_scene(model, device, obj_poses, obj_wlh, shapecodes, texturecodes, K, H, W, n_samples, manipulation=(0.0, 0.0, 0.0),
              ray_batch_size=4096, rend_aabb=True, shapenet_obj_cood=True, adjust_scale=1.0, jitters: Optional[Sequence] = None,
              return_float=False):
    """uint8 canvas (H,W,3) with all objects rendered at their (manipulated) poses; white where nothing is hit.
    ``jitters``: optional list of (Nr*Nb, S) draws, one per ray batch (tests); default ``torch.rand_like`` per batch."""
    if obj_poses.shape[0] != shapecodes.shape[0] or obj_poses.shape[0] != texturecodes.shape[0] or obj_poses.shape[0] != obj_wlh.shape[0]:
        raise SnrError("vis_scene: obj_poses, obj_wlh, shapecodes and texturecodes must describe the same number of objects")
    table, valid, diags = scene_rays(obj_poses, obj_wlh, K, H, W, manipulation, rend_aabb)
    valid_rays = table.view(H * W, -1, 8)[valid, ...]
    out = []
    with torch.no_grad():
        for bi, batch in enumerate(torch.split(valid_rays, ray_batch_size)):
            out.append(render_scene_batch(model, device, batch, diags, shapecodes, texturecodes, n_samples,
                                          None if jitters is None else jitters[bi], adjust_scale, shapenet_obj_cood)[0])
    canvas = torch.ones(H * W, 3)
    if out:
        canvas[valid, :] = torch.cat(out, 0).cpu()
    img = (canvas.view(H, W, 3).numpy() * 255).astype(np.uint8)
    return (img, canvas) if return_float else img
