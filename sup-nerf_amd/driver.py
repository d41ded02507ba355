"""Test-time optimisation loop on the HIP render path: the package's own counterpart of
``OptimizerNuScenes.optimize_objs_w_pose_unified`` (src/optimizer_nuscenes.py:553-794 of the reference; KITTI /
Waymo twins src/optimizer_kitti.py:606-885), plus object sharding across GPUs.

Per object and iteration, exactly as the reference: pose -> cam2opt (:685-699), ``render_rays_v2`` (:716-726),
``loss = loss_rgb + loss_occ_coef * loss_occ`` (:729-736), backward, foreground PSNR (:739-744), pose errors
(:747-750), depth error at "lidar" pixels via ``render_rays_specified`` under no_grad (:757-765), AdamW step over four
parameter groups (:1762-1769) skipped for the first ``reg_iters + 1`` iterations (:768-769), learning rates halved
every ``lr_half_interval`` by re-creating AdamW (:1771-1775, which resets the Adam moments -- kept).

Objects are independent, so multi-GPU = one process per GPU, each taking a contiguous slice of the object list
(the reference's ``--num_subset/--id_subset`` slicing, src/data_nuscenes.py:318-320, but the ``L mod N`` tail is not
dropped) with no communication inside the loop; one ``all_gather`` of the per-object metric rows at the end (RCCL
when the backend is nccl, gloo on CPU in the tests).

Several views of one instance (``optimize_instances``; ``optimize_objs_multi_anns_w_pose`` :1050-1277 and ``optimize_objs_multi_anns``
:796-1048): the I instances' codes are (I,256), their V >= I views lie instance-major and every view is one "object" of the same fused
launches.  ``ops.InstanceRows`` copies an instance's latent row to its views and, backwards, adds its views' gradients in ascending view
order with plain fp32 adds (no atomics: the same bits every run).  With random sampling every iteration picks ``n_rays`` pixels of each
view's native roi (``ops.view_pixels``); a view with fewer pixels is padded with rays of occupancy 0, which weigh exactly 0 in its loss.

Cross-view evaluation (``eval_cross_view``; ``OptimizerNuScenes.eval_cross_view`` :1279-1410): the codes fitted to every view and saved at
``code_save_iters`` by the loops above are rendered in every other view of their instance; every (snapshot, code view, rendered view) pair
is one "object" of the fused forward launches and ``ops.cross_metrics`` reduces a chunk of pairs to PSNR inputs and depth errors at once.

No dataset is available offline: objects come from ``synthetic.py``.  The rotation parametrisation
(pytorch3d ``axis_angle_to_matrix`` / ``matrix_to_axis_angle`` in the reference, un-pinned and not installed) is
restated here via Rodrigues' formula; parity for it is pinned only by self-consistency tests.
"""
import contextlib
import json
import math
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import scene, synthetic, utils as U

DEFAULT_HPAMS = {     # the keys of jsonfiles/supnerf.nusc.vehicle.car.json that the loop reads
    "n_samples": 64, "render_im_sz": 32, "roi_margin": 5, "shapenet_obj_cood": 1, "sym_aug": 0, "loss_occ_coef": 0.1,
    "dataset": {"name": "nusc", "img_h": 900, "img_w": 1600, "mask_pixels": 2500, "max_dist": 40},
    "net_hyperparams": {"shape_blocks": 3, "texture_blocks": 1, "latent_dim": 256, "num_xyz_freq": 10, "num_dir_freq": 4},
    "optimize": {"num_opts": 100, "opt_cam_pose": 0, "lr_shape": 0.02, "lr_texture": 0.02, "lr_pose": 0.01, "lr_half_interval": 1000},
}


# jsonfiles/supnerf.kitti.car.json differs from the nuScenes file on the loop's path only in these (tests/golden/kitti.json holds
# the reference file's values)
KITTI_OVERRIDES = {"roi_margin": 15, "dataset": {"name": "kitti", "mask_pixels": 1600, "max_dist": 40, "min_depth": 3}}


# jsonfiles/supnerf.waymo.car.json: optimize_waymo.py runs the KITTI-convention loop (labels converted by obj_pose_kitti2nusc,
# src/optimizer_waymo.py:125,140: roi_margin 15, sq_pad) on 1920 x 1280 images (tests/golden/waymo.json holds the reference file's values)
WAYMO_OVERRIDES = {"roi_margin": 15, "dataset": {"name": "waymo", "mask_pixels": 2500, "max_dist": 40, "min_depth": 3, "min_lidar_cnt": 10}}


def load_hpams(path: Optional[str] = None, dataset: str = "nusc") -> dict:
    """Read a reference config file (jsonfiles/*.json) -- same keys, verbatim -- or the shipped defaults of ``dataset``
    ('nusc' | 'kitti' | 'waymo')."""
    if path is None:
        hp = json.loads(json.dumps(DEFAULT_HPAMS))
        if dataset == "kitti":
            hp.update(json.loads(json.dumps(KITTI_OVERRIDES)))
        elif dataset == "waymo":
            hp.update(json.loads(json.dumps(WAYMO_OVERRIDES)))
        elif dataset != "nusc":
            raise ValueError(f"unknown dataset {dataset!r}")
        return hp
    with open(path) as f:
        return json.load(f)


# ------------------------------------------------------------------ rotations (restated, quaternion-free Rodrigues)
def axis_angle_to_matrix(v: torch.Tensor) -> torch.Tensor:
    """(...,3) rotation vector -> (...,3,3).  R = I + sin(t)/t K + (1-cos t)/t^2 K^2, series near t = 0.  1 - cos t is taken as
    2 sin^2(t/2): in float32 cos t rounds to 1 or its neighbour just above the series threshold and the difference keeps no digits."""
    t2 = (v * v).sum(-1, keepdim=True)
    t = torch.sqrt(t2.clamp_min(1e-24))
    small = t2 < 1e-8
    a = torch.where(small, 1 - t2 / 6, torch.sin(t) / t)
    s = torch.sin(0.5 * t)
    b = torch.where(small, 0.5 - t2 / 24, 2 * s * s / t2.clamp_min(1e-24))
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], -1).reshape(*v.shape[:-1], 3, 3)
    eye = torch.eye(3, dtype=v.dtype, device=v.device).expand(K.shape)
    return eye + a[..., None] * K + b[..., None] * (K @ K)


def matrix_to_axis_angle(R: torch.Tensor) -> torch.Tensor:
    """(...,3,3) -> (...,3) rotation vector with angle in [0, pi]."""
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    cos = ((tr - 1) / 2).clamp(-1, 1)
    ang = torch.acos(cos)
    w = torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = torch.sin(ang)
    k = torch.where(s.abs() > 1e-6, ang / (2 * torch.where(s.abs() > 1e-6, s, torch.ones_like(s))), torch.full_like(s, 0.5))
    out = w * k[..., None]
    # near pi the antisymmetric part vanishes: take the axis from the diagonal of (R + I)/2
    near_pi = cos < -0.999
    if near_pi.any():
        d = ((torch.diagonal(R, dim1=-2, dim2=-1) + 1) / 2).clamp_min(0).sqrt()
        sign = torch.sign(w)
        sign = torch.where(sign == 0, torch.ones_like(sign), sign)
        out = torch.where(near_pi[..., None], d * sign * ang[..., None], out)
    return out


def rot_dist(R1: torch.Tensor, R2: torch.Tensor) -> torch.Tensor:
    """Geodesic angle between rotations (src/utils.py:713-722)."""
    d = R1 @ R2.transpose(-1, -2)
    tr = (d[..., 0, 0] + d[..., 1, 1] + d[..., 2, 2]).clamp(-1, 3)
    return torch.acos(((tr - 1) / 2).clamp(-1, 1))


# ------------------------------------------------------------------ sharding (src/data_nuscenes.py:318-320, tail kept)
def shard_slice(n_items: int, world_size: int, rank: int) -> range:
    """Contiguous slice of rank ``rank``; the first ``n_items % world_size`` ranks take one extra item."""
    base, extra = divmod(n_items, world_size)
    start = rank * base + min(rank, extra)
    return range(start, start + base + (1 if rank < extra else 0))


def gather_metric_rows(rows: torch.Tensor, ids: torch.Tensor, n_items: int, group=None) -> torch.Tensor:
    """all_gather of per-object metric rows (n_local, n_cols) -> (n_items, n_cols) ordered by object id, on every
    rank.  The only collective of the optimise path."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        out = rows.new_zeros(n_items, rows.shape[1])
        out[ids.long()] = rows
        return out
    world = dist.get_world_size(group)
    n_max = (n_items + world - 1) // world
    pad = rows.new_full((n_max, rows.shape[1] + 1), -1.0)
    pad[: rows.shape[0], 0] = ids.to(rows.dtype)
    pad[: rows.shape[0], 1:] = rows
    bufs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad, group=group)
    out = rows.new_zeros(n_items, rows.shape[1])
    for b in bufs:
        keep = b[:, 0] >= 0
        out[b[keep, 0].long()] = b[keep, 1:]
    return out


# ------------------------------------------------------------------ the stock pose head in the loop (src/optimizer_nuscenes.py:451-551)
def fw_pose_one_step(model, im_feat, src_pose, wlh, roi, K, K_inv):
    """One step of the feed-forward pose refiner, ``OptimizerNuScenes.fw_pose_one_step`` (src/optimizer_nuscenes.py:509-551): project
    the current box (``scene.corners_of_box_batch`` + ``view_points_batch(normalize=True)``), normalise the 8 corners by the roi
    (``normalize_by_roi(need_square=True)``, src/utils.py:1175-1197), let the STOCK pose head ``model.pose_update`` (plain PyTorch,
    src/model_supnerf.py:226-239) regress a 6-vector, and apply it: rotation vector += 2 pi d[:3]; projected centre += d[3:5] * roi size;
    depth *= (d[5] + 1).  (B,3,4) object poses in, (B,3,4) out.  Rotation conversions: Rodrigues (``axis_angle_to_matrix`` above; the
    reference calls pytorch3d, un-pinned)."""
    uvw = torch.matmul(K, scene.corners_of_box_batch(src_pose, wlh))
    uv = (uvw / uvw[:, 2:3, :])[:, :2, :]
    w_, h_ = roi[:, 2] - roi[:, 0], roi[:, 3] - roi[:, 1]
    cx, cy = (roi[:, 2] + roi[:, 0]) / 2, (roi[:, 3] + roi[:, 1]) / 2
    dim = torch.maximum(w_, h_)
    uv_n = torch.stack([uv[:, 0, :] - cx.unsqueeze(-1), uv[:, 1, :] - cy.unsqueeze(-1)], dim=1) / dim.view(-1, 1, 1)
    B = im_feat.shape[0]
    d = model.pose_update(im_feat, uv_n.reshape(B, -1))
    d_rot, d_uv, d_z = d[:, :3] * (math.pi * 2), d[:, 3:5] * dim.unsqueeze(-1), d[:, 5:] + 1
    pred_R = axis_angle_to_matrix(matrix_to_axis_angle(src_pose[:, :, :3]) + d_rot)
    c = torch.matmul(K, src_pose[:, :, 3:])
    pred_u = c[:, 0] / c[:, 2] + d_uv[:, 0:1]
    pred_v = c[:, 1] / c[:, 2] + d_uv[:, 1:2]
    pred_Z = src_pose[:, 2, 3:] * d_z
    pred_T = torch.matmul(K_inv, torch.cat([pred_u * pred_Z, pred_v * pred_Z, pred_Z], dim=1).unsqueeze(-1))
    return torch.cat([pred_R, pred_T], dim=2)


def fw_pose_update(model, im_feat, src_pose, wlh, roi, K, K_inv, iters=3):
    """``OptimizerNuScenes.fw_pose_update`` (src/optimizer_nuscenes.py:451-507) without its PnP start (``start_wt_est_pose``: cv2): the
    start pose followed by ``iters`` refinement steps -> the pose table (B, iters + 1, 3, 4) that the loop's first ``reg_iters + 1``
    iterations render at (:641-651,684-689); the optimiser's ``rot_vec`` / ``trans_vec`` start from its last entry (:652,664-666).
    All of it stock PyTorch on the inputs' device, under ``no_grad`` like the caller (:641)."""
    with torch.no_grad():
        table = [src_pose]
        for _ in range(iters):
            table.append(fw_pose_one_step(model, im_feat, table[-1], wlh, roi, K, K_inv))
        return torch.stack(table, dim=1)


# ------------------------------------------------------------------ one object
def make_optimizer(shapecode, texturecode, rot_vec, trans_vec, lr):
    """AdamW over four groups (src/optimizer_nuscenes.py:1762-1769)."""
    return torch.optim.AdamW([{"params": shapecode, "lr": lr["lr_shape"]}, {"params": texturecode, "lr": lr["lr_texture"]},
                              {"params": rot_vec, "lr": lr["lr_pose"]}, {"params": trans_vec, "lr": lr["lr_pose"]}])


def losses(rgb_rays, acc_trans_rays, rgb_tgt, occ_pixels, loss_occ_coef):
    """src/optimizer_nuscenes.py:729-744: (loss, foreground mse used for the PSNR log)."""
    a = torch.abs(occ_pixels)
    denom = a.sum() + 1e-9
    loss_rgb = (((rgb_rays - rgb_tgt) ** 2) * a).sum() / denom
    loss_occ = (torch.exp(-occ_pixels * (0.5 - acc_trans_rays.unsqueeze(-1))) * a).sum() / denom
    fg = occ_pixels.clamp_min(0)
    mse_fg = (((rgb_rays - rgb_tgt) ** 2) * fg).sum() / (fg.sum() + 1e-9)
    return loss_rgb + loss_occ_coef * loss_occ, mse_fg


def optimize_object(model, device, obj: Dict, hpams: dict, shapecode0, texturecode0, pose_noise=(0.05, 0.3), reg_iters=3,
                    n_lidar=64, seed=0, log=None, jitter=None, info: Optional[dict] = None, pose_per_iter=None):
    """Optimise codes and object pose of one object against its (synthetic) target.  Returns a metric tensor
    (num_opts, 4) = [psnr, depth_err, rot_err, trans_err] per iteration, and the final codes / pose.

    With a native decoder this is the fused iteration of ``optimize_objects_batched`` at one object (about thirty launches, no host
    round trip), fed with the depth jitter the reference's loop would have drawn: two ``torch.rand(S)`` per iteration from the global
    CPU generator, in order.  ``optimize_object_api`` is the same loop written against the public functions, call for call like the
    reference (needed for ``sym_aug``, which flips a python coin inside every render call, for foreign decoders and for ``log``).

    ``pose_per_iter`` ((reg_iters + 1, 3, 4) OBJECT poses in the camera frame, e.g. from ``fw_pose_update``; None = the noise-perturbed
    ground truth): the loop's first ``reg_iters + 1`` iterations render at these poses and the optimiser's ``rot_vec`` / ``trans_vec`` start
    from the last one (src/optimizer_nuscenes.py:641-668,684-689)."""
    if pose_per_iter is not None:
        pose_per_iter = torch.as_tensor(pose_per_iter, dtype=torch.float32).reshape(-1, 3, 4)
        if pose_per_iter.shape[0] != reg_iters + 1:
            raise U.SnrError(f"pose_per_iter holds {pose_per_iter.shape[0]} poses, the loop renders reg_iters + 1 = {reg_iters + 1} of them")
    if not U._is_native(model) or hpams.get("sym_aug", 0) or log is not None or not U.ops.fused_supported(hpams["n_samples"]):
        return optimize_object_api(model, device, obj, hpams, shapecode0, texturecode0, pose_noise, reg_iters, n_lidar, seed, log, jitter, info,
                                   pose_per_iter=pose_per_iter)
    T, S = hpams["optimize"]["num_opts"], hpams["n_samples"]
    if jitter is None:
        jitter = torch.stack([torch.stack([torch.rand(S), torch.rand(S)]) for _ in range(T)]) if T else torch.zeros(0, 2, S)
    m, sc, tc, pose = optimize_objects_batched(model, device, [obj], hpams, shapecode0, texturecode0, [seed], pose_noise, reg_iters, n_lidar,
                                               jitter=jitter[:, :, None, :], info=info,
                                               pose_per_iter=None if pose_per_iter is None else pose_per_iter[None])
    return m[0].cpu(), sc, tc, pose[0]


def optimize_object_api(model, device, obj: Dict, hpams: dict, shapecode0, texturecode0, pose_noise=(0.05, 0.3), reg_iters=3,
                        n_lidar=64, seed=0, log=None, jitter=None, info: Optional[dict] = None, pose_per_iter=None):
    """``optimize_object`` through the public render API, one call per reference call (src/optimizer_nuscenes.py:674-783): ~350 launches
    per iteration, host-bound at one object."""
    opt = hpams["optimize"]
    S, im_sz = hpams["n_samples"], hpams["render_im_sz"]
    dev = torch.device(device)
    rs = np.random.RandomState(seed)
    K, roi, obj_diag = obj["K"], obj["roi"], obj["obj_diag"]
    img, mask = obj["img"], obj["mask"]
    # ground-truth OBJECT pose in the camera frame and a perturbed start
    gt_pose = U.invert_pose(obj["cam_pose"])
    if pose_per_iter is not None:
        pose_per_iter = torch.as_tensor(pose_per_iter, dtype=torch.float32).reshape(-1, 3, 4).to(dev)
    rot_vec, trans_vec = [t.to(dev).requires_grad_() for t in _start_pose(gt_pose, rs, pose_noise, None if pose_per_iter is None else pose_per_iter[-1])]
    shapecode = shapecode0.detach().clone().to(dev).requires_grad_()
    texturecode = texturecode0.detach().clone().to(dev).requires_grad_()
    lr = {k: opt[k] for k in ("lr_shape", "lr_texture", "lr_pose")}
    optim = make_optimizer(shapecode, texturecode, rot_vec, trans_vec, lr)
    # the depth pixels: the object's lidar returns with their measured depths (the reference's metric, :751-765), or -- synthetic objects
    # without a depth map -- random foreground pixels, the metric then being the change of rendered depth against the first iteration
    x_vec, y_vec, gt_depth = _lidar_pixels(obj, rs, n_lidar)
    if info is not None:
        info["lidar_count"] = torch.tensor([len(x_vec)], dtype=torch.int32)
    metrics = torch.zeros(opt["num_opts"], 4, device=dev)      # stays on the device: the reference's per-iteration .item() logging
    gt_dev = gt_pose.to(dev)                                    # would put three host syncs into every iteration
    depth0 = None if gt_depth is None else torch.from_numpy(gt_depth).to(dev)
    for it in range(opt["num_opts"]):
        optim.zero_grad()
        if jitter is not None:                                   # (num_opts, 2, S): the two draws of this iteration (tests)
            U.JITTER_OVERRIDE = jitter[it, 0]
        if pose_per_iter is not None and it <= reg_iters:        # "the first a few to load pre-computed poses" (:684-689)
            pose = pose_per_iter[it]
        else:
            pose = torch.cat([axis_angle_to_matrix(rot_vec[0]), trans_vec[0].unsqueeze(-1)], -1)
        cam2opt = pose if opt.get("opt_cam_pose", 0) else U.invert_pose(pose)      # object pose is optimised: invert to camera-in-object
        rgb, depth, acc, rgb_tgt, occ = U.render_rays_v2(model, dev, img, mask, cam2opt, obj_diag, K, roi, S, shapecode, texturecode,
                                                         hpams["shapenet_obj_cood"], hpams["sym_aug"], im_sz=im_sz, n_rays=None)
        loss, mse_fg = losses(rgb, acc, rgb_tgt, occ, hpams["loss_occ_coef"])
        loss.backward()
        with torch.no_grad():
            if jitter is not None:
                U.JITTER_OVERRIDE = jitter[it, 1]
            _, d_vec, _, _, _ = U.render_rays_specified(model, dev, img, mask, cam2opt.detach(), obj_diag, K, roi, x_vec, y_vec, S,
                                                        shapecode, texturecode, hpams["shapenet_obj_cood"], hpams["sym_aug"])
            if depth0 is None:
                depth0 = d_vec.clone()
            pred = cam2opt.detach() if opt.get("opt_cam_pose", 0) else U.invert_pose(cam2opt.detach())
            pred_R, pred_t = pred[:, :3], pred[:, 3:]
            row = torch.stack([-10 * torch.log10(mse_fg.detach()), (d_vec - depth0).abs().sum() / (len(x_vec) + 1e-8),     # (log_eval_depth_v2, :1736-1741)
                               rot_dist(pred_R, gt_dev[:, :3]), (pred_t - gt_dev[:, 3:]).norm()])
        metrics[it] = row
        if it > reg_iters:
            optim.step()
        if (it + 1) % opt["lr_half_interval"] == 0:
            halvings = (it + 1) // opt["lr_half_interval"]
            lr = {k: v * 2 ** (-halvings) for k, v in lr.items()}     # cumulative like update_learning_rate (:1771-1775)
            optim = make_optimizer(shapecode, texturecode, rot_vec, trans_vec, lr)
        if log is not None:
            log(it, float(loss), metrics[it].cpu())
    if jitter is not None:
        U.JITTER_OVERRIDE = None
    return metrics.cpu(), shapecode.detach(), texturecode.detach(), cam2opt.detach()


# ------------------------------------------------------------------ many objects per launch (BASELINE config 3)
def optimize_objects_batched(model, device, objs: List[Dict], hpams: dict, shapecodes0, texturecodes0, seeds: Sequence[int],
                             pose_noise=(0.05, 0.3), reg_iters=3, n_lidar=64, jitter=None, info: Optional[dict] = None, pose_per_iter=None,
                             code_save_iters=None):
    """The iteration of ``optimize_object`` for B objects at once: ONE fused forward, one backward and one depth render of the lidar pixels
    per iteration for all of them (per-object codes, poses, depth tables and targets; the loss is the sum of the per-object losses, so
    every object sees exactly its own gradient), AdamW over the stacked leaves in one launch, metrics kept on the device until the end --
    no host round trip inside the loop (``_fit_views``: ~24 launches per iteration for any B).  Jitter: ``jitter``
    (num_opts, 2, B, S) or, by default, drawn up front from one CPU generator per object (seeded like the per-object loop seeds its
    RandomState).  ``info`` (optional dict) receives ``lidar_count`` (B,): the number of depth pixels behind every object's depth metric.
    ``pose_per_iter`` (B, reg_iters + 1, 3, 4): every object's pose table for the render-only iterations, see ``optimize_object``.
    ``code_save_iters``: ``info`` also receives ``shape_snapshots`` / ``texture_snapshots`` (C,B,256), see ``_fit_views``.
    Returns metrics (B, num_opts, 4), shape codes, texture codes, poses (B,3,4).
    (Round 2 also carried a HIP-graph replay of the torch-op iteration; it lost to this eager fused loop, 2.3 vs 1.3 ms per iteration, and
    is gone.)"""
    dev = torch.device(device)
    if hpams.get("sym_aug", 0):
        raise U.SnrError("optimize_objects_batched: sym_aug draws one python coin per object and iteration; use optimize_object")
    _save_iters(code_save_iters)
    if pose_per_iter is not None:
        pose_per_iter = torch.as_tensor(pose_per_iter, dtype=torch.float32)
        if tuple(pose_per_iter.shape) != (len(objs), reg_iters + 1, 3, 4):
            raise U.SnrError(f"pose_per_iter must be (B, reg_iters + 1, 3, 4) = ({len(objs)}, {reg_iters + 1}, 3, 4), got {tuple(pose_per_iter.shape)}")
    c = _loop_inputs(objs, seeds, hpams, pose_noise, n_lidar, dev, pose_per_iter)
    if jitter is None:
        jitter = _default_jitter(seeds, hpams["optimize"]["num_opts"], hpams["n_samples"])
    if info is not None:
        info["lidar_count"] = c["lid_cnt"].clone()
    opt_cam = int(bool(hpams["optimize"].get("opt_cam_pose", 0)))
    given = None
    if pose_per_iter is not None:
        # the render-only iterations' camera poses, made once: the inverses of the table's object poses unless the camera pose itself is
        # what is optimised (src/optimizer_nuscenes.py:684-699); (reg_iters + 1, B, 3, 4) on the device
        P = pose_per_iter.to(dev).permute(1, 0, 2, 3)
        given = (P if opt_cam else U.invert_pose(P)).contiguous()
    return _fit_views(model, dev, hpams, c, shapecodes0, texturecodes0, jitter, opt_cam, reg_iters=reg_iters, given=given,
                      code_save_iters=code_save_iters, info=info)


def _start_pose(gt, rs, pose_noise, last=None):
    """Where the optimiser's pose starts: the rotation and translation vectors (1,3) of the ground-truth object pose ``gt`` (3,4), perturbed by
    two ``rs.randn(1, 3)`` draws.  The draws are the FIRST the object's ``RandomState`` makes -- its lidar pixels are drawn next -- and they
    are made also when ``last``, the last pose of a pose table, then replaces the result (src/optimizer_nuscenes.py:652,664-666; on
    ``last``'s device)."""
    rot = matrix_to_axis_angle(gt[None, :, :3]) + torch.from_numpy(rs.randn(1, 3).astype(np.float32)) * pose_noise[0]
    tr = gt[:, 3:].T + torch.from_numpy(rs.randn(1, 3).astype(np.float32)) * pose_noise[1]
    if last is not None:
        rot, tr = matrix_to_axis_angle(last[:3, :3][None]), last[:3, 3][None].clone()
    return rot, tr


def _default_jitter(seeds, T, S):
    """(T, 2, len(seeds), S) depth jitter, the render's and the depth render's draw of every iteration: one CPU generator per seed."""
    return torch.stack([torch.rand(T, 2, S, generator=torch.Generator().manual_seed(int(s_))) for s_ in seeds], dim=2)


def _lidar_pixels(ob, rs, n_lidar):
    """The pixels of the crop whose depth the loop logs every iteration, and their measured depths when the object carries them.
    With ``ob["lidar_xy"]`` (n,2 integer crop pixels x, y) and ``ob["lidar_depth"]`` (n,): the reference's metric -- every lidar return
    on the foreground mask, depth L1 against the measurement (src/optimizer_nuscenes.py:751-765,1736-1741).  Without (synthetic objects
    with no depth map): ``n_lidar`` random foreground pixels, and the metric is the change of rendered depth against iteration 0."""
    if ob.get("lidar_xy") is not None:
        xy = np.asarray(ob["lidar_xy"]).reshape(-1, 2).astype(np.int64)
        depth = np.asarray(ob["lidar_depth"], dtype=np.float32).reshape(-1)
        if depth.shape[0] != xy.shape[0]:
            raise U.SnrError("object: lidar_xy (n,2) and lidar_depth (n,) disagree")
        return xy[:, 0], xy[:, 1], depth
    ys, xs = np.where(ob["mask"][:, :, 0].numpy() > 0)
    pick = rs.permutation(len(ys))[:n_lidar]
    return xs[pick], ys[pick], None


def _loop_inputs(objs, seeds, hpams, pose_noise, n_lidar, dev, pose_per_iter=None, grid=True, need_depth=True):
    """Per-object constants of the loop, built once on the host and moved to the device: perturbed start pose, ground truth, the pixel
    direction tables [(px-cx)/fx, (py-cy)/fy, 1] of the render grid and of the lidar pixels (every object keeps ITS OWN count: the tables
    are padded to the largest, the metric kernel averages each object's first ``lid_cnt`` entries), measured depths when the objects
    carry them, resized targets (the reference resizes the same crop again in every iteration, src/utils.py:447-456).  ``grid=False``
    (a loop that samples native pixels anew every iteration, ``optimize_instances``): no render grid and no resized targets.
    ``need_depth=False`` (``eval_cross_view``): a batch without a single depth pixel is not an error (tables of width 0)."""
    im_sz = hpams["render_im_sz"]
    rot0, tr0, gtR, gtT, cam, lid, lid_d, tgt, occ = [], [], [], [], [], [], [], [], []
    for ob, seed in zip(objs, seeds):
        rs = np.random.RandomState(seed)
        gt = U.invert_pose(ob["cam_pose"])
        rot, tr = _start_pose(gt, rs, pose_noise, None if pose_per_iter is None else pose_per_iter[len(rot0), -1])
        rot0.append(rot); tr0.append(tr)
        gtR.append(gt[:, :3]); gtT.append(gt[:, 3])
        x_vec, y_vec, depth = _lidar_pixels(ob, rs, n_lidar)
        x0, y0, x1, y1 = [int(v) for v in ob["roi"]]
        K = ob["K"]
        cx, cy, fx, fy = K[0, 2], K[1, 2], K[0, 0], K[1, 1]
        if grid:
            gx, gy = torch.linspace(x0, x1 - 1, im_sz), torch.linspace(y0, y1 - 1, im_sz)
            px, py = gx[None, :].expand(im_sz, im_sz).reshape(-1), gy[:, None].expand(im_sz, im_sz).reshape(-1)
            cam.append(torch.stack([(px - cx) / fx, (py - cy) / fy, torch.ones_like(px)], -1))
        lx, ly = torch.from_numpy(x_vec + x0), torch.from_numpy(y_vec + y0)         # integer pixels, like get_rays_specified
        lid.append(torch.stack([(lx - cx) / fx, (ly - cy) / fy, torch.ones_like(lx, dtype=torch.float32)], -1).float().reshape(-1, 3))
        lid_d.append(None if depth is None else torch.from_numpy(depth))
        if grid:
            im, mk = U._resize(ob["img"], ob["mask"], im_sz)
            tgt.append(im.reshape(-1, 3)); occ.append(mk.reshape(-1))
    has_depth = [d is not None for d in lid_d]
    if any(has_depth) and not all(has_depth):
        raise U.SnrError("optimize_objects_batched: either every object of a batch carries lidar_xy / lidar_depth or none does")
    cnt = [v.shape[0] for v in lid]
    n_l = max(cnt) if cnt else 0
    if n_l == 0 and need_depth:
        raise U.SnrError("optimize_objects_batched: no object has a depth pixel (empty foreground / no lidar return)")
    one_ray = torch.tensor([[0.0, 0.0, 1.0]])

    def pad(v, width):          # (the padding rays are rendered and ignored: a valid direction, depth 0)
        return torch.cat([v, (one_ray if width == 3 else torch.zeros(1)).expand(n_l - v.shape[0], *([3] if width == 3 else []))]) if v.shape[0] < n_l else v
    st = lambda xs_: torch.stack(xs_).to(dev).contiguous()
    return dict(rot0=torch.cat(rot0).to(dev), tr0=torch.cat(tr0).to(dev), gtR=st(gtR), gtT=st(gtT), cam=st(cam) if grid else None,
                lid=st([pad(v, 3) for v in lid]),
                lid_depth=st([pad(d, 1) for d in lid_d]) if all(has_depth) else None, lid_cnt=torch.tensor(cnt, dtype=torch.int32, device=dev),
                tgt=st(tgt) if grid else None, occ=st(occ) if grid else None, diag=torch.tensor([float(ob["obj_diag"]) for ob in objs], device=dev), n_lidar=n_l)


@contextlib.contextmanager
def _decoder_frozen(model):
    """The decoder is a constant of the fused loops (the reference leaves its weights trainable and pays for unused weight gradients): inside
    the block none of its parameters requires a gradient; those that did are handed back trainable, also when the loop raises."""
    frozen = [p for p in model.parameters() if p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    try:
        yield
    finally:
        for p in frozen:
            p.requires_grad_(True)


def _leaves_and_adamw(shapecodes0, texturecodes0, rot0, tr0, opt, dev):
    """The leaves of a fused loop on the device -- clones of the start codes and, unless ``rot0`` is None (poses that are not optimised: no
    pose leaves, two parameter groups), the start rotation and translation vectors -- and ``ops.DeviceAdamW`` over them with the three
    learning rates (src/optimizer_nuscenes.py:1762-1769)."""
    shapecode, texturecode = [t.detach().clone().to(dev).contiguous().requires_grad_() for t in (shapecodes0, texturecodes0)]
    groups = [(shapecode, float(opt["lr_shape"])), (texturecode, float(opt["lr_texture"]))]
    rot_vec = trans_vec = None
    if rot0 is not None:
        rot_vec, trans_vec = [t.to(dev).contiguous().requires_grad_() for t in (rot0, tr0)]
        groups += [(rot_vec, float(opt["lr_pose"])), (trans_vec, float(opt["lr_pose"]))]
    return shapecode, texturecode, rot_vec, trans_vec, U.ops.DeviceAdamW(groups)


def _halve_rates(optim, it, opt):
    """After every ``lr_half_interval`` iterations: AdamW as re-created with its rates scaled down (src/optimizer_nuscenes.py:1771-1775)."""
    if (it + 1) % opt["lr_half_interval"] == 0:
        optim.restart(2.0 ** (-((it + 1) // opt["lr_half_interval"])))


def _decide_precision(model, cfg, cfg_l, packed, rays_o, viewdir, z, diag, lat):
    """Which arithmetic a fused loop runs in, set on its two launches' cfgs: "auto" is decided (and range-checked) once, on the first
    batch (``model._auto_precision``); the probe renders one object of it, the decoder being the same for all.  The lidar launch
    ``cfg_l`` follows ``cfg`` except where the split kernels do not take its shape."""
    ops = U.ops
    n, S = cfg.rays_per_obj, cfg.n_samples

    def probe(p_):
        c1 = cfg.replace(latent_bias=None if cfg.latent_bias is None else cfg.latent_bias[:1])
        return ops.render_probe(rays_o.detach()[:n], viewdir.detach()[:n], z.detach()[:1], diag[:1], None, lat.detach()[:1], packed, c1, p_)
    prec = model._auto_precision(model.precision, n * S, probe)
    cfg.precision = prec
    cfg_l.precision = prec if (prec != "bf16x3" or ops.split_supported(cfg.shape_blocks, cfg.texture_blocks, cfg_l.rays_per_obj * S)) else "fp32"


def _fit_views(model, dev, hpams, c, shapecodes0, texturecodes0, jitter, opt_cam, reg_iters=-1, crops=None, picks=None, given=None,
               view_offset=None, opt_pose=True, loss_log=None, grad_log=None, code_save_iters=None, info=None):
    """THE fused iteration of ``optimize_objects_batched`` and ``optimize_instances``, ~30 launches for any number V of views ("objects" of
    the launches): pose -> rays + depths (one launch), the latent layers (two GEMMs), fused render, loss tail (one launch), backward = their
    four backward launches, the 64-pixel depth render, the metric row (one launch), AdamW over the parameter groups (one launch).  Nothing
    reads back until the loop has finished.  ``c``: ``_loop_inputs`` of the V views; ``jitter`` (T, 2, V, S).  What the callers choose:

    * the pixels: the fixed resized grid of ``c`` (``cam``, ``tgt``, ``occ``), or with ``crops`` (``_view_crops``) and ``picks`` (T, V, n) on
      the device every iteration's own native pixels, one ``ops.view_pixels`` launch more;
    * the camera poses: ``given`` (n_given, V, 3, 4) on the device holds those of iterations ``it < n_given`` (``CamRays``, nothing to
      differentiate), every other iteration renders at the optimised ``rot_vec`` / ``trans_vec`` (``PoseRays``).  Iterations ``it <= reg_iters``
      only render (no graph, no step).  ``opt_pose=False``: there are no pose leaves (``given`` covers all T iterations), AdamW has the two
      code groups and its rates are never halved;
    * the code rows: ``view_offset`` None = one row per view, (V,256); a tuple of I + 1 offsets = (I,256) codes, ``ops.InstanceRows`` hands
      every instance's latent row to its views and sums their gradients in view order.

    ``loss_log`` (T,V) on the device and ``grad_log`` (a list), when given, receive every iteration's per-view losses and clones of the code
    gradients the step reads.  ``code_save_iters`` (ascending iterations; None adds no operation): ``info["shape_snapshots"]`` /
    ``info["texture_snapshots"]`` (C, rows, 256), row c = the codes ENTERING iteration ``code_save_iters[c]`` (the reference saves at the top
    of the iteration, src/optimizer_nuscenes.py:675-678), an iteration at or past ``num_opts`` = the returned codes (its ``[-1]`` row,
    :789-790); device clones inside the loop, stacked once after it.
    Returns metrics (V,T,4), shape codes, texture codes, the last iteration's camera-in-object poses (V,3,4)."""
    ops = U.ops
    opt = hpams["optimize"]
    S, T = int(hpams["n_samples"]), int(opt["num_opts"])
    V, n_l = c["lid"].shape[0], c["n_lidar"]
    n = c["cam"].shape[1] if crops is None else picks.shape[2]
    shapecode, texturecode, rot_vec, trans_vec, optim = _leaves_and_adamw(shapecodes0, texturecodes0, c["rot0"] if opt_pose else None, c["tr0"], opt, dev)
    jitter = jitter.to(dev, torch.float32).contiguous()
    frame = U._frame(False, False, hpams["shapenet_obj_cood"])
    sb, tb = model.shape_blocks, model.texture_blocks
    half = (c["diag"] / 2).contiguous()
    coef = float(hpams["loss_occ_coef"])
    metrics = torch.zeros(T, V, 4, device=dev)
    measured = c["lid_depth"] is not None
    depth0 = c["lid_depth"] if measured else torch.zeros(V, n_l, device=dev)       # measured depths, or the rendered depths of iteration 0
    ones = torch.ones(V, device=dev)
    pose = torch.zeros(V, 3, 4, device=dev)
    cfg = ops.RenderCfg(S, ops.Z_PER_OBJECT, n, sb, tb, frame=frame, precision=model.precision)
    cfg_l = ops.RenderCfg(S, ops.Z_PER_OBJECT, n_l, sb, tb, frame=frame, precision=model.precision)
    packed = model.packed_weights()
    save_at = _save_iters(code_save_iters)
    snaps = []
    with _decoder_frozen(model):
        for it in range(T):
            if save_at is not None and it in save_at:
                snaps.append((shapecode.detach().clone(), texturecode.detach().clone()))
            if crops is None:
                cam, tgt, occ = c["cam"], c["tgt"], c["occ"]
            else:               # this iteration's pixels of every view: directions, targets and labels in one launch
                cam, tgt, occ = ops.view_pixels(*crops, picks[it])
            from_given = given is not None and it < given.shape[0]
            if from_given:      # a given camera pose per view: rays straight from the (3,4) poses (snr_cam_rays_fwd), nothing to differentiate
                c2o = given[it]
                rays_o, viewdir, z = ops.CamRays.apply(c2o, cam, half, jitter[it, 0], S)
            else:
                cam2opt, rays_o, viewdir, z = ops.PoseRays.apply(rot_vec, trans_vec, cam, half, jitter[it, 0], S, opt_cam)
            lat = model.latent_terms(shapecode, texturecode)                        # one launch for all code rows
            bias = model.latent_biases(lat)
            if view_offset is not None:                                             # (I, n_lat, 256) -> (V, n_lat, 256): every view reads its instance's row
                lat = ops.InstanceRows.apply(lat, view_offset)
                bias = None if bias is None else ops.instance_rows_fwd(bias, view_offset)
            cfg.latent_bias = cfg_l.latent_bias = bias
            if it == 0:         # which arithmetic the loop runs in: decided once, on the first iteration's batch
                _decide_precision(model, cfg, cfg_l, packed, rays_o, viewdir, z, c["diag"], lat)
            # a render-only iteration (it <= reg_iters): its gradients are cleared unread (:676,768-769), so no_grad keeps autograd from
            # recording it.  FusedRender still pads and saves ReLU bits whenever an input requires grad (needs_input_grad does not see grad
            # mode; the launch that saves them is 9 % slower and writes 208 B per point): avoiding that is left to a later change
            with contextlib.nullcontext() if it > reg_iters else torch.no_grad():
                rgb, depth, acc = ops.FusedRender.apply(rays_o, viewdir, z, c["diag"], None, lat, packed, cfg)
                loss, lm = ops.LossTail.apply(rgb, acc, tgt, occ, coef, n)
            if it > reg_iters:
                torch.autograd.backward(loss, ones)                                 # the sum of the views' losses (:1192, once per view there)
            with torch.no_grad():
                if from_given:
                    lo, lv, lz = ops.CamRays.apply(c2o, c["lid"], half, jitter[it, 1], S)
                else:
                    c2o, lo, lv, lz = ops.PoseRays.apply(rot_vec.detach(), trans_vec.detach(), c["lid"], half, jitter[it, 1], S, opt_cam)
                d_vec = ops.render_fwd(lo, lv, lz, c["diag"], None, lat.detach(), packed, cfg_l)[1]
                out4 = torch.cat([loss.detach()[:, None], lm], dim=1)
                ops.metric_row(out4, d_vec.view(V, n_l), depth0, it == 0 and not measured, c2o, c["gtR"], c["gtT"], opt_cam, metrics[it],
                               lidar_count=c["lid_cnt"])
                if loss_log is not None:
                    loss_log[it] = loss.detach()
                if grad_log is not None:
                    grad_log.append((shapecode.grad.clone(), texturecode.grad.clone()))
                if it == T - 1:
                    pose.copy_(c2o)
            if it > reg_iters:
                optim.step()
            optim.zero_grad()
            if opt_pose:
                _halve_rates(optim, it, opt)
    if save_at is not None and info is not None:
        snaps += [(shapecode.detach(), texturecode.detach())] * (len(save_at) - len(snaps))        # iterations at or past num_opts
        info["shape_snapshots"] = torch.stack([s_[0] for s_ in snaps]) if snaps else shapecode.detach().new_zeros(0, *shapecode.shape)
        info["texture_snapshots"] = torch.stack([s_[1] for s_ in snaps]) if snaps else texturecode.detach().new_zeros(0, *texturecode.shape)
    return metrics.permute(1, 0, 2).contiguous(), shapecode.detach(), texturecode.detach(), pose


def _save_iters(code_save_iters):
    """``code_save_iters`` as a list of ascending non-negative iterations (the reference's ``CODE_SAVE_ITERS_``), or None."""
    if code_save_iters is None:
        return None
    its = [int(i) for i in code_save_iters]
    if any(i < 0 for i in its) or any(b <= a for a, b in zip(its, its[1:])):
        raise U.SnrError(f"code_save_iters must be ascending non-negative iterations, got {its}")
    return its


# ------------------------------------------------------------------ all objects of a frame, jointly against the frame
def optimize_scene(model, device, frame: Dict, hpams: dict, shapecodes0, texturecodes0, pose_noise=(0.05, 0.3), seed=0, jitter=None,
                   pixels=None, info: Optional[dict] = None, compact=False, capacity=None, capacity_margin=1.5):
    """Fit the codes and poses of all Nb objects of one frame JOINTLY against the frame: every listed pixel is rendered through all objects
    (``scene.render_scene``'s fused route) and compared with the image, so objects that occlude each other share their pixels' loss.

    ``frame``: K (3,3), H, W, img (H,W,3), occ (H,W) in {-1,0,1} (1 on any object, -1 known background, 0 unknown), obj_poses (Nb,3,4)
    (the ground truth: the metrics and the noise-perturbed start), obj_wlh (Nb,3).  ``pixels`` (Nr,2) int (x, y), fixed over the loop;
    default: the pixels inside the union of the start poses' rois.  ``jitter`` (T, Nr*Nb, S); default: one seeded CPU generator.

    One iteration, without a host round trip: pose parameters -> camera-in-object poses (``ops.PoseRays``), ``scene.scene_rois`` on the device
    from the detached poses, ``scene.render_pairs`` (``ops.SceneSamples``, the decoder on the object-major points, ``ops.SceneGather``,
    ``ops.SceneComposite``), ``ops.LossTail`` with the scene as one "object", backward, ``ops.DeviceAdamW`` over the four groups (every
    iteration; rates halved every ``lr_half_interval``).  The decoder's weights are constants of the loop.  ``info`` receives ``pixels`` and
    ``hit_share`` (T,), the share of (pixel, object) pairs that hit per iteration.

    ``compact``: ``render_pairs``' compact chain, the decoder on ``capacity`` slots per object instead of all Nr pixels.  The default
    capacity is measured ONCE before the loop (one host read of Nb counts): the fullest object's hit count at the start poses times
    ``capacity_margin``, through ``ops.scene_capacity``, at most ``ops.scene_capacity(Nr)``.  Inside the loop nothing is read: an object whose
    hits outgrow the capacity has the surplus pairs rendered as misses, their number summed on the device into ``info["dropped_pairs"]``
    (0-dim int64), and a ``RuntimeWarning`` is raised after the loop when it is not zero.  ``info["capacity"]`` holds the capacity;
    ``hit_share`` stays the geometric share, dropped pairs included.

    Returns metrics (T,Nb,2) = rotation / translation error of every object at the poses iteration t rendered, losses (T,4) = [loss,
    loss_rgb, loss_occ, mse_fg], shape codes, texture codes and the object poses (Nb,3,4) after the last update."""
    ops = U.ops
    dev = torch.device(device)
    opt = hpams["optimize"]
    S, T = int(hpams["n_samples"]), int(opt["num_opts"])
    gt = torch.as_tensor(frame["obj_poses"], dtype=torch.float32)
    wlh = torch.as_tensor(frame["obj_wlh"], dtype=torch.float32)
    Nb = gt.shape[0]
    if tuple(gt.shape) != (Nb, 3, 4) or tuple(wlh.shape) != (Nb, 3) or shapecodes0.shape[0] != Nb or texturecodes0.shape[0] != Nb:
        raise U.SnrError("optimize_scene: obj_poses (Nb,3,4), obj_wlh (Nb,3), shapecodes0 and texturecodes0 must describe the same number of objects")
    if Nb * S > ops.SCENE_BWD_MAX_N:
        raise U.SnrError(f"optimize_scene: {Nb} objects x {S} samples per pixel, the composite backward takes at most {ops.SCENE_BWD_MAX_N}")
    if not U._is_native(model):
        raise U.SnrError("optimize_scene needs the package's own decoder")
    if hpams.get("sym_aug", 0):
        raise U.SnrError("optimize_scene: sym_aug is a per-object, per-call coin; it has no meaning for a jointly rendered frame")
    if opt.get("opt_cam_pose", 0):
        raise U.SnrError("optimize_scene optimises object poses in one camera (opt_cam_pose = 0)")
    H, W = int(frame["H"]), int(frame["W"])
    K = torch.as_tensor(frame["K"], dtype=torch.float32).cpu()
    Kvec = scene.K_vector(K)
    rs = np.random.RandomState(seed)
    rot0 = matrix_to_axis_angle(gt[:, :, :3]) + torch.from_numpy(rs.randn(Nb, 3).astype(np.float32)) * pose_noise[0]
    tr0 = gt[:, :, 3] + torch.from_numpy(rs.randn(Nb, 3).astype(np.float32)) * pose_noise[1]
    if pixels is None:
        pixels = scene.roi_pixels(scene.scene_rois(torch.cat([axis_angle_to_matrix(rot0), tr0[:, :, None]], dim=2), wlh, K, H, W), H, W)
    pixels = torch.as_tensor(pixels).reshape(-1, 2).to(torch.int32)
    Nr = pixels.shape[0]
    if Nr == 0:
        raise U.SnrError("optimize_scene: no pixel to render (the start poses project outside the image)")
    if bool((pixels[:, 0] < 0).any() | (pixels[:, 0] >= W).any() | (pixels[:, 1] < 0).any() | (pixels[:, 1] >= H).any()):
        raise U.SnrError("optimize_scene: the pixel list leaves the image")
    if jitter is None:
        jitter = torch.rand(T, Nr * Nb, S, generator=torch.Generator().manual_seed(int(seed)))
    if tuple(jitter.shape) != (T, Nr * Nb, S):
        raise U.SnrError(f"optimize_scene: jitter must be (T, Nr*Nb, S) = ({T}, {Nr * Nb}, {S}), got {tuple(jitter.shape)}")
    jitter = jitter.to(dev, torch.float32).contiguous()
    px = pixels.long()
    tgt = torch.as_tensor(frame["img"], dtype=torch.float32)[px[:, 1], px[:, 0]].reshape(Nr, 3).to(dev).contiguous()
    occ = torch.as_tensor(frame["occ"], dtype=torch.float32)[px[:, 1], px[:, 0]].reshape(Nr).to(dev).contiguous()
    pixels, wlh_d, K_d, gt_d = pixels.to(dev), wlh.to(dev), K.to(dev), gt.to(dev)
    shapecode, texturecode, rot_vec, trans_vec, optim = _leaves_and_adamw(shapecodes0, texturecodes0, rot0, tr0, opt, dev)
    sb, tb = model.shape_blocks, model.texture_blocks
    coef = float(hpams["loss_occ_coef"])
    shapenet = bool(hpams["shapenet_obj_cood"])
    one_dir = torch.tensor([0.0, 0.0, 1.0], device=dev).expand(Nb, 1, 3).contiguous()      # PoseRays' ray outputs go unused: one ray is enough
    half = (wlh_d.norm(dim=1) / 2).contiguous()
    pose_log = torch.zeros(T, Nb, 3, 4, device=dev)
    loss_log = torch.zeros(T, 4, device=dev)
    hit_log = torch.zeros(T, device=dev)
    ones = torch.ones(1, device=dev)
    packed = model.packed_weights()
    prec = None
    if compact:
        if capacity is None:    # the fullest object at the start poses, with room to grow: the one host read of the compact route
            with torch.no_grad():
                start = torch.cat([axis_angle_to_matrix(rot0), tr0[:, :, None]], dim=2).to(dev)
                hit0 = ops.scene_pair_hits(U.invert_pose(start), wlh_d, scene.scene_rois(start, wlh_d, K_d, H, W), pixels, Kvec, True)
                capacity = ops.scene_capacity(math.ceil(int(hit0.sum(0, dtype=torch.int32).max()) * float(capacity_margin)))
        capacity = min(int(capacity), ops.scene_capacity(Nr))
        dropped = torch.zeros((), dtype=torch.int64, device=dev)
    elif capacity is not None:
        raise U.SnrError("optimize_scene: capacity belongs to compact=True")

    def decode(xyz, viewdir):
        nonlocal prec
        lat = model.latent_terms(shapecode, texturecode)
        x3, d3 = xyz.view(-1, 3), viewdir.view(-1, 3)
        if prec is None:    # iteration 0 -- which arithmetic the loop runs in: "auto" is decided (and range-checked) once, like CodeNeRF.forward does
            ppo, probe_pts = model._points_shape(x3.detach(), d3.detach(), lat, pad=sb + tb > 0)
            prec = model._auto_precision(model.precision, ppo, lambda p_: ops.decoder_fwd(*probe_pts(), lat.detach(), packed, sb, tb, precision=p_)[:2])
        return ops.DecoderPoints.apply(x3, d3, lat, packed, sb, tb, prec)
    with _decoder_frozen(model):
        for it in range(T):
            cam2obj = ops.PoseRays.apply(rot_vec, trans_vec, one_dir, half, None, 1, 0)[0]
            with torch.no_grad():
                pose_log[it] = U.invert_pose(cam2obj)
                rois = scene.scene_rois(pose_log[it], wlh_d, K_d, H, W)
            if compact:
                rgb, _, acc, _, count = scene.render_pairs(decode, cam2obj, wlh_d, rois, pixels, Kvec, jitter[it], S, 1.0, True, shapenet, capacity)
            else:
                rgb, _, acc, hit = scene.render_pairs(decode, cam2obj, wlh_d, rois, pixels, Kvec, jitter[it], S, 1.0, True, shapenet)
            loss, lm = ops.LossTail.apply(rgb, acc, tgt, occ, coef, Nr)
            torch.autograd.backward(loss, ones)
            with torch.no_grad():
                loss_log[it, 0:1] = loss.detach()
                loss_log[it, 1:] = lm[0]
                if compact:
                    hit_log[it] = count.sum() / float(Nr * Nb)
                    dropped += (count - capacity).clamp_min(0).sum()
                else:
                    hit_log[it] = hit.float().mean()
            optim.step()
            optim.zero_grad()
            _halve_rates(optim, it, opt)
    with torch.no_grad():
        metrics = torch.stack([rot_dist(pose_log[:, :, :, :3], gt_d[None, :, :, :3]), (pose_log[:, :, :, 3] - gt_d[None, :, :, 3]).norm(dim=-1)], dim=-1)
        poses = torch.cat([axis_angle_to_matrix(rot_vec.detach()), trans_vec.detach()[:, :, None]], dim=2)
    if info is not None:
        info["pixels"], info["hit_share"] = pixels, hit_log
        if compact:
            info["capacity"], info["dropped_pairs"] = capacity, dropped
    if compact and int(dropped) > 0:
        warnings.warn(f"optimize_scene: {int(dropped)} hit (pixel, object) pairs beyond the capacity of {capacity} per object were rendered as "
                      "misses; pass a larger capacity or capacity_margin", RuntimeWarning, stacklevel=2)
    return metrics, loss_log, shapecode.detach(), texturecode.detach(), poses


# ------------------------------------------------------------------ several views of one instance: shared codes
def _flatten_instances(instances):
    """Instance-major list of all views and the (I+1,) offsets of every instance's contiguous views."""
    if not instances:
        raise U.SnrError("optimize_instances: no instance")
    counts = []
    for i, inst in enumerate(instances):
        views = inst.get("views") if isinstance(inst, dict) else None
        if not views:
            raise U.SnrError(f"optimize_instances: instance {i} has no view ('views' must be a non-empty list)")
        counts.append(len(views))
    return [v for inst in instances for v in inst["views"]], U.ops.view_offset_of(counts)


def draw_view_picks(views, seeds, num_opts, n_rays):
    """(num_opts, V, n_rays) int32 pixel picks of ``render_rays`` (src/utils.py:380-432), drawn up front: per view one
    ``np.random.RandomState(seed)``, per iteration ``permutation(h w)[:n_rays]`` into the view's native roi, -1 where the roi has fewer
    than ``n_rays`` pixels (the reference's ``n_rays = min(n_all, n_rays)``; a -1 is a padding ray of weight 0)."""
    picks = np.full((num_opts, len(views), n_rays), -1, dtype=np.int32)
    for v, (view, seed) in enumerate(zip(views, seeds)):
        x0, y0, x1, y1 = [int(t) for t in view["roi"]]
        n_all = (x1 - x0) * (y1 - y0)
        rs = np.random.RandomState(seed)
        for it in range(num_opts):
            ids = rs.permutation(n_all)[:n_rays]
            picks[it, v, :len(ids)] = ids
    return torch.from_numpy(picks)


def _view_crops(views, dev):
    """The views' native crops as ``ops.view_pixels`` takes them: concatenated pixels, offsets, rois, intrinsics."""
    img, occ, off, roi, Kv = [], [], [0], [], []
    for v, view in enumerate(views):
        x0, y0, x1, y1 = [int(t) for t in view["roi"]]
        h, w = y1 - y0, x1 - x0
        if h < 1 or w < 1 or tuple(view["img"].shape) != (h, w, 3) or view["mask"].numel() != h * w:
            raise U.SnrError(f"optimize_instances: view {v}: img {tuple(view['img'].shape)} / mask {tuple(view['mask'].shape)} are not the "
                             f"native {h} x {w} crop of its roi (random sampling reads the unresized crop)")
        img.append(view["img"].reshape(-1, 3).float()); occ.append(view["mask"].reshape(-1).float())
        off.append(off[-1] + h * w); roi.append([x0, y0, x1, y1])
        K = view["K"]
        Kv.append([float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])])
    # (K's entries go through python floats and back: float32 -> double -> float32 is exact)
    return (torch.cat(img).to(dev).contiguous(), torch.cat(occ).to(dev).contiguous(), torch.tensor(off, dtype=torch.int64, device=dev),
            torch.tensor(roi, dtype=torch.int32, device=dev), torch.tensor(Kv, dtype=torch.float32, device=dev))


def optimize_instances(model, device, instances: List[Dict], hpams: dict, shapecodes0, texturecodes0, seeds: Sequence[int], opt_pose=True,
                       sampling=None, n_rays=None, pose_noise=(0.05, 0.3), n_lidar=64, picks=None, jitter=None, info: Optional[dict] = None,
                       code_save_iters=None):
    """Fit I instances, each seen in one or more views, with ONE shape code and ONE texture code per instance -- the reference's
    ``optimize_objs_multi_anns_w_pose`` (``opt_pose=True``, src/optimizer_nuscenes.py:1050-1277: also one object pose per VIEW) and
    ``optimize_objs_multi_anns`` (``opt_pose=False``, :796-1048: poses fixed at every view's ``cam_pose``) -- as the fused iteration of
    ``optimize_objects_batched``: all V views of all instances ride in the same ~30 launches.

    ``instances[i]["views"]``: a non-empty list of the dicts ``optimize_object`` consumes (img, mask, cam_pose, obj_diag, K, roi, optional
    lidar_xy / lidar_depth).  Views are laid out instance-major; ``seeds`` holds one seed per view (start-pose noise and lidar pixels like
    ``optimize_objects_batched``; picks and jitter by default).  Layout: codes (I,256) -> latent rows (I, n_lat, 256) by one
    ``LatentLayers`` launch -> ``ops.InstanceRows`` copies every instance's row to its views (V, n_lat, 256); everything after that is per
    view.  Backward: the gradient of an instance's row is the sum of its views' rows in ascending view order, plain fp32 adds (no atomics:
    the same bits every run) -- the reference's successive ``loss.backward()`` calls accumulating into ``.grad``.  Every view has its own
    loss ``loss_rgb + loss_occ_coef loss_occ`` over its own sum of |occ|; one backward of their sum; one AdamW step EVERY iteration (no
    render-only iterations, no pose table): codes at lr_shape / lr_texture, and with ``opt_pose`` rot_vec / trans_vec (V,3) at lr_pose.

    ``sampling``: "random" (default with ``opt_pose``) = ``render_rays``: every iteration ``n_rays`` (argument, else ``hpams["n_rays"]``)
    random pixels of each view's NATIVE roi, targets from the unresized crop, by one ``ops.view_pixels`` launch on ``picks[it]``
    (``picks`` (num_opts, V, n_rays) int32, default ``draw_view_picks``, uploaded once).  A view with fewer pixels than ``n_rays`` is padded
    with -1 picks: rays with occupancy 0, which weigh exactly 0 in every sum of the loss, so its loss is the loss of its own pixels.
    "grid" (default without ``opt_pose``) = ``render_rays_v2``: the ``render_im_sz``^2 resized grid, built once.
    Learning rates are halved every ``lr_half_interval`` with ``opt_pose`` (:1266-1270) and never without (:1039-1040 is commented out).
    ``jitter`` (num_opts, 2, V, S), default one seeded generator per view.  ``info`` receives ``view_offset`` (I+1,), ``lidar_count`` (V,),
    ``rays_per_view`` (V,), ``loss`` (num_opts, V); with ``info["record_grads"]`` set also ``code_grads``: per iteration the
    (shape, texture) code gradients as the optimiser step reads them.  ``code_save_iters`` (ascending iterations): ``info`` also receives
    ``shape_snapshots`` / ``texture_snapshots`` (C,I,256), the codes entering those iterations (``_fit_views``) -- what ``eval_cross_view``
    scores, after ``ops.instance_rows_fwd`` has handed every instance's row to its views.

    Returns metrics (V, num_opts, 4) = [psnr, depth_err, rot_err, trans_err] per view, shape codes (I,256), texture codes (I,256), and the
    camera-in-object poses (V,3,4) of the last iteration.  Not provided: ``sym_aug``, per-view texture residuals (``slack_tex``),
    fine-tuning the decoder (``opt_model``)."""
    ops = U.ops
    dev = torch.device(device)
    opt = hpams["optimize"]
    if hpams.get("sym_aug", 0):
        raise U.SnrError("optimize_instances: sym_aug draws one python coin per view and iteration; it is not provided here")
    for key in ("slack_tex", "opt_model"):
        if hpams.get(key, 0) or opt.get(key, 0):
            raise U.SnrError(f"optimize_instances: the reference's {key} is not provided (codes and poses only, one texture code per instance)")
    if not U._is_native(model):
        raise U.SnrError("optimize_instances needs the package's own decoder")
    _save_iters(code_save_iters)
    views, offsets = _flatten_instances(instances)
    I, V = len(instances), len(views)
    S, T = int(hpams["n_samples"]), int(opt["num_opts"])
    if not ops.fused_supported(S):
        raise U.SnrError(f"optimize_instances: n_samples = {S} is not a divisor of 128 (the fused render)")
    if len(seeds) != V:
        raise U.SnrError(f"optimize_instances: one seed per view expected ({V}), got {len(seeds)}")
    if shapecodes0.shape != (I, 256) or texturecodes0.shape != (I, 256):
        raise U.SnrError(f"optimize_instances: shapecodes0 / texturecodes0 must be (I,256) = ({I},256), one row per instance")
    if sampling is None:
        sampling = "random" if opt_pose else "grid"
    if sampling not in ("random", "grid"):
        raise U.SnrError(f"optimize_instances: sampling is 'random' or 'grid', got {sampling!r}")
    random_px = sampling == "random"
    c = _loop_inputs(views, seeds, hpams, pose_noise, n_lidar, dev, grid=not random_px)
    crops = None
    if random_px:
        n = int(n_rays if n_rays is not None else hpams.get("n_rays", 0))
        if n < 1:
            raise U.SnrError("optimize_instances: random sampling needs n_rays (the argument, or the reference's hpams['n_rays'])")
        if picks is None:
            picks = draw_view_picks(views, seeds, T, n)
        picks = torch.as_tensor(picks)
        if tuple(picks.shape) != (T, V, n):
            raise U.SnrError(f"optimize_instances: picks must be (num_opts, V, n_rays) = ({T}, {V}, {n}), got {tuple(picks.shape)}")
        crops = _view_crops(views, dev)
        picks = picks.to(dev, torch.int32).contiguous()
        rays_per_view = torch.tensor([min(n, int((v["roi"][2] - v["roi"][0]) * (v["roi"][3] - v["roi"][1]))) for v in views], dtype=torch.int32)
    else:
        if picks is not None:
            raise U.SnrError("optimize_instances: picks belong to sampling='random'")
        n = int(hpams["render_im_sz"]) ** 2
        rays_per_view = torch.full((V,), n, dtype=torch.int32)
    if jitter is None:
        jitter = _default_jitter(seeds, T, S)
    if tuple(jitter.shape) != (T, 2, V, S):
        raise U.SnrError(f"optimize_instances: jitter must be (num_opts, 2, V, S) = ({T}, 2, {V}, {S}), got {tuple(jitter.shape)}")
    opt_cam, given = int(bool(opt.get("opt_cam_pose", 0))), None
    if not opt_pose:            # every view's own cam_pose in all T iterations: ONE (V,3,4) tensor, read T times through a stride-0 view
        opt_cam = 0
        given = torch.stack([torch.as_tensor(v["cam_pose"], dtype=torch.float32)[:3, :4] for v in views]).to(dev).contiguous().expand(T, V, 3, 4)
    loss_log = grad_log = None
    if info is not None:
        info["view_offset"] = torch.tensor(offsets, dtype=torch.int64)
        info["lidar_count"], info["rays_per_view"] = c["lid_cnt"].clone(), rays_per_view
        info["loss"] = loss_log = torch.zeros(T, V, device=dev)
        if info.get("record_grads"):
            info["code_grads"] = grad_log = []
    return _fit_views(model, dev, hpams, c, shapecodes0, texturecodes0, jitter, opt_cam, crops=crops, picks=picks, given=given, view_offset=offsets,
                      opt_pose=opt_pose, loss_log=loss_log, grad_log=grad_log, code_save_iters=code_save_iters, info=info)


# ------------------------------------------------------------------ cross-view evaluation: every code of an instance in every one of its views
CROSS_POINTS_PER_LAUNCH = 1 << 24      # eval_cross_view's default chunk: pairs whose grid + lidar points stay below this


def eval_cross_view(model, device, instances: List[Dict], hpams: dict, shapecodes, texturecodes, *, jitter=None, seeds=None, pair_chunk=None,
                    info: Optional[dict] = None):
    """``OptimizerNuScenes.eval_cross_view`` (src/optimizer_nuscenes.py:1279-1410) for all instances, snapshots and view pairs in a handful of
    launches: the codes fitted to view ``ii`` of an instance are rendered from the ground-truth camera of every view ``num`` of that instance
    (``render_rays_v2`` on the ``render_im_sz``^2 grid, :1351-1356), PSNR against that view's whitened crop (:1359-1362), depth L1 against
    its lidar returns (``render_rays_specified``, :1366-1380).

    ``instances`` as for ``optimize_instances`` (views instance-major); every view carries img (already whitened), mask, cam_pose, K, roi,
    obj_diag, lidar_xy (n,2) crop pixels and lidar_depth (n,) -- both may be empty: that view's depth column is 0, the reference's
    0 / (0 + 1e-8).  ``shapecodes`` / ``texturecodes``: (V,256) or (C,V,256), one code per view and snapshot (per-instance codes: expand
    them with ``ops.instance_rows_fwd``).  Instances with fewer than 2 views are skipped (:1318-1319) and listed in ``info["skipped"]``.

    Layout: every (snapshot, ii, num) triple is one PAIR = one "object" of the launches (``ops.cross_pairs``: instance-major, then
    snapshot, ii, num).  One ``latent_terms`` launch covers all C V code rows; per chunk of pairs the rows, camera poses, direction
    tables and half diagonals are gathered with plain indexing, then ``CamRays`` + ``ops.render_fwd`` on the grid, the same on the padded
    lidar tables, and ONE ``ops.cross_metrics`` launch that reads targets, labels and measured depths through the pair's target view.
    ``jitter`` (P,2,S): every pair's grid and depth draw (the reference draws ``torch.rand`` twice per pair); default one CPU generator
    per pair, seeded with ``seeds[p]`` (``seeds``: P integers, or one integer base -> base + p; default base 0).  ``pair_chunk``: pairs
    per launch, default ``CROSS_POINTS_PER_LAUNCH`` points.  Precision as ``_fit_views`` decides it.  One host read at the end; PSNR on
    the host in float64, ``-10 log(mse) / log(10)`` from the fp32 loss (:1362): a view whose mask is all zero gives mse 0, PSNR +inf.

    Returns {instance index: (psnr (C,V_i,V_i), depth (C,V_i,V_i))} float64 numpy, row = the view the codes come from, column = the view
    rendered.  ``info`` also receives ``pairs`` (P,2), ``pair_offset``, ``kept_views``, ``pair_chunk`` and ``metrics`` (P,3) = [mse_fg,
    depth_err, sum |occ|] as the kernel wrote them."""
    ops = U.ops
    dev = torch.device(device)
    if hpams.get("sym_aug", 0):
        raise U.SnrError("eval_cross_view: sym_aug draws one python coin per render call; it is not provided here")
    if not U._is_native(model):
        raise U.SnrError("eval_cross_view needs the package's own decoder")
    views_all, offsets_all = _flatten_instances(instances)
    V_all = len(views_all)
    shapecodes, texturecodes = torch.as_tensor(shapecodes), torch.as_tensor(texturecodes)
    if shapecodes.dim() == 2:
        shapecodes = shapecodes[None]
    if texturecodes.dim() == 2:
        texturecodes = texturecodes[None]
    if shapecodes.dim() != 3 or tuple(shapecodes.shape[1:]) != (V_all, 256) or shapecodes.shape[0] < 1 or texturecodes.shape != shapecodes.shape:
        raise U.SnrError(f"eval_cross_view: shapecodes / texturecodes must both be (V,256) or (C,V,256) with V = {V_all} views, got "
                         f"{tuple(shapecodes.shape)} and {tuple(texturecodes.shape)}")
    C_ = shapecodes.shape[0]
    S = int(hpams["n_samples"])
    if not ops.fused_supported(S):
        raise U.SnrError(f"eval_cross_view: n_samples = {S} is not a divisor of 128 (the fused render)")
    if dev.type != "cuda":
        raise U.SnrError("eval_cross_view runs on the GPU (no CPU fallback)")
    kept = [i for i in range(len(instances)) if offsets_all[i + 1] - offsets_all[i] >= 2]
    if info is not None:
        info["skipped"] = [i for i in range(len(instances)) if i not in kept]
    if not kept:
        return {}
    kept_views = [v for i in kept for v in range(offsets_all[i], offsets_all[i + 1])]
    views = [views_all[v] for v in kept_views]
    for v, view in zip(kept_views, views):
        if view.get("lidar_xy") is None or view.get("lidar_depth") is None:
            raise U.SnrError(f"eval_cross_view: view {v} carries no lidar_xy / lidar_depth (empty arrays are fine: depth error 0)")
    V = len(views)
    offsets = ops.view_offset_of([offsets_all[i + 1] - offsets_all[i] for i in kept])
    pairs, pair_off = ops.cross_pairs(offsets, C_)
    P = pairs.shape[0]
    if jitter is None:
        base = 0 if seeds is None else seeds
        seeds = [int(base) + p for p in range(P)] if isinstance(base, int) else [int(s_) for s_ in base]
        if len(seeds) != P:
            raise U.SnrError(f"eval_cross_view: one seed per pair expected ({P}), got {len(seeds)}")
        jitter = torch.stack([torch.rand(2, S, generator=torch.Generator().manual_seed(s_)) for s_ in seeds])
    jitter = torch.as_tensor(jitter)
    if tuple(jitter.shape) != (P, 2, S):
        raise U.SnrError(f"eval_cross_view: jitter must be (P, 2, S) = ({P}, 2, {S}), got {tuple(jitter.shape)}")
    c = _loop_inputs(views, [0] * V, hpams, (0.0, 0.0), 0, dev, grid=True, need_depth=False)
    n, n_l = c["cam"].shape[1], c["n_lidar"]
    if pair_chunk is None:
        pair_chunk = max(1, CROSS_POINTS_PER_LAUNCH // ((n + n_l) * S))
    pair_chunk = int(pair_chunk)
    if pair_chunk < 1:
        raise U.SnrError(f"eval_cross_view: pair_chunk must be at least 1, got {pair_chunk}")
    jitter = jitter.to(dev, torch.float32).contiguous()
    pairs_d = pairs.to(dev)
    code_row, tgt_view = pairs_d[:, 0].long(), pairs_d[:, 1].long()
    cam_pose = torch.stack([torch.as_tensor(v["cam_pose"], dtype=torch.float32)[:3, :4] for v in views]).to(dev).contiguous()
    half = (c["diag"] / 2).contiguous()
    lid_depth = c["lid_depth"] if c["lid_depth"] is not None else torch.zeros(V, n_l, device=dev)
    frame = U._frame(False, False, hpams["shapenet_obj_cood"])
    sb, tb = model.shape_blocks, model.texture_blocks
    cfg = ops.RenderCfg(S, ops.Z_PER_OBJECT, n, sb, tb, frame=frame, precision=model.precision)
    cfg_l = ops.RenderCfg(S, ops.Z_PER_OBJECT, n_l, sb, tb, frame=frame, precision=model.precision)
    packed = model.packed_weights()
    keep_idx = torch.tensor(kept_views, device=dev)
    out = torch.empty(P, 3, device=dev)
    with torch.no_grad():
        sc = shapecodes.to(dev, torch.float32).index_select(1, keep_idx).reshape(C_ * V, 256).contiguous()
        tc = texturecodes.to(dev, torch.float32).index_select(1, keep_idx).reshape(C_ * V, 256).contiguous()
        lat = model.latent_terms(sc, tc)                                            # one launch for all C V code rows
        bias = model.latent_biases(lat)
        for p0 in range(0, P, pair_chunk):
            p1 = min(P, p0 + pair_chunk)
            rows, tv = code_row[p0:p1], tgt_view[p0:p1]
            lat_p = lat.index_select(0, rows)
            cfg.latent_bias = cfg_l.latent_bias = None if bias is None else bias.index_select(0, rows)
            c2w, half_p, diag_p = cam_pose.index_select(0, tv), half.index_select(0, tv), c["diag"].index_select(0, tv)
            rays_o, viewdir, z = ops.CamRays.apply(c2w, c["cam"].index_select(0, tv), half_p, jitter[p0:p1, 0].contiguous(), S)
            if p0 == 0:         # which arithmetic the evaluation runs in: decided once, on the first chunk, as _fit_views does
                _decide_precision(model, cfg, cfg_l, packed, rays_o, viewdir, z, diag_p, lat_p)
            rgb = ops.render_fwd(rays_o, viewdir, z, diag_p, None, lat_p, packed, cfg)[0]
            if n_l:
                lo, lv, lz = ops.CamRays.apply(c2w, c["lid"].index_select(0, tv), half_p, jitter[p0:p1, 1].contiguous(), S)
                d_vec = ops.render_fwd(lo, lv, lz, diag_p, None, lat_p, packed, cfg_l)[1].view(p1 - p0, n_l)
            else:
                d_vec = torch.zeros(p1 - p0, 0, device=dev)
            out[p0:p1] = ops.cross_metrics(rgb.view(p1 - p0, n, 3), d_vec, c["tgt"], c["occ"], lid_depth, c["lid_cnt"], pairs[p0:p1], n_codes=C_ * V)
    rows_h = out.cpu()                                                              # the one host read
    mse = rows_h[:, 0].numpy().astype(np.float64)
    with np.errstate(divide="ignore"):
        psnr = -10 * np.log(mse) / np.log(10)                                       # (:1362, from the fp32 loss)
    depth = rows_h[:, 1].numpy().astype(np.float64)
    result = {}
    for k, i in enumerate(kept):
        Vi = offsets[k + 1] - offsets[k]
        a, b = int(pair_off[k]), int(pair_off[k + 1])
        result[i] = (psnr[a:b].reshape(C_, Vi, Vi).copy(), depth[a:b].reshape(C_, Vi, Vi).copy())
    if info is not None:
        info.update(pairs=pairs, pair_offset=pair_off, kept_views=kept_views, pair_chunk=pair_chunk, metrics=rows_h)
    return result


def make_instances(ids: Sequence[int], n_views: int, lidar: bool = False) -> List[Dict]:
    """Synthetic instances seen in ``n_views`` cameras each (``synthetic.synthetic_instance``): every view carries its native-size crop
    (``synthetic_crop_targets``, background whitened like src/optimizer_nuscenes.py:1167-1171), so rois differ in size between views.
    ``lidar``: every view also carries synthetic lidar returns with measured depths."""
    out = []
    for i in ids:
        inst = synthetic.synthetic_instance(i, n_views)
        for j, view in enumerate(inst["views"]):
            x0, y0, x1, y1 = [int(t) for t in view["roi"]]
            img, mask = synthetic.synthetic_crop_targets(1000 * i + j, y1 - y0, x1 - x0)
            img = img * (mask > 0) + (mask <= 0)
            view.update(img=img, mask=mask, index=i, view=j)
            if lidar:
                xy, depth = synthetic.synthetic_lidar(1000 * i + j, mask, view)
                view.update(lidar_xy=xy, lidar_depth=depth)
        out.append(inst)
    return out


def make_objects(ids: Sequence[int], im_sz: int, lidar: bool = False) -> List[Dict]:
    """Synthetic nuScenes-like objects.  ``lidar``: also a synthetic set of lidar returns on the foreground (``lidar_xy`` (n,2) crop pixels,
    ``lidar_depth`` (n,) metres; n differs from object to object like real sweeps), which switches the loop's depth metric to the reference's."""
    out = []
    for i in ids:
        ob = synthetic.synthetic_object(i)
        img, mask = synthetic.synthetic_targets(i, im_sz)
        # the reference whitens the background of the crop (src/optimizer_nuscenes.py:711-713)
        img = img * (mask > 0) + (mask <= 0)
        ob.update(img=img, mask=mask, index=i)
        if lidar:
            xy, depth = synthetic.synthetic_lidar(i, mask, ob)
            ob.update(lidar_xy=xy, lidar_depth=depth)
        out.append(ob)
    return out


def make_kitti_objects(ids: Sequence[int], hpams: dict) -> List[Dict]:
    """BASELINE config 4 (src/optimizer_kitti.py:606-672): synthetic KITTI labels -> the dicts ``optimize_object`` consumes.  Per object,
    in the reference's order: ``obj_pose_kitti2nusc`` on the KITTI-convention pose (:638), ``roi_process(roi, H, W, roi_margin, sq_pad=True)``
    on the 2D box (:651; margin 15, clipped to the 1242 x 375 image, so truncated cars give non-square crops), the crop and its mask with the
    background whitened (:654-658).  The camera-in-object pose the renderer wants is the inverse of the converted object pose (:751-754);
    after that the render path is the nuScenes one (the ``kitti2nusc=`` flag of the render functions stays False)."""
    out = []
    margin = hpams.get("roi_margin", 15)
    waymo = hpams.get("dataset", {}).get("name") == "waymo"      # the same loop on 1920 x 1280 images (src/optimizer_waymo.py:125-140)
    for i in ids:
        ob = synthetic.synthetic_kitti_object(i, K=synthetic.WAYMO_K, im_w=synthetic.WAYMO_IM_W, im_h=synthetic.WAYMO_IM_H) if waymo \
            else synthetic.synthetic_kitti_object(i)
        pose_nusc = U.obj_pose_kitti2nusc(ob["obj_pose"][None].clone(), torch.tensor([float(ob["wlh"][2])]))[0]
        cam_pose = U.invert_pose(pose_nusc)
        roi = U.roi_process(ob["box2d"], ob["im_h"], ob["im_w"], margin, sq_pad=True)
        h, w = int(roi[3] - roi[1]), int(roi[2] - roi[0])
        img, mask = synthetic.synthetic_crop_targets(i, h, w)
        img = img * (mask > 0) + (mask <= 0)
        out.append(dict(wlh=ob["wlh"], obj_diag=np.linalg.norm(ob["wlh"]).astype(np.float32), cam_pose=cam_pose, obj_pose=pose_nusc,
                        K=ob["K"], roi=roi, img=img, mask=mask, index=i))
    return out


def optimize_objects(model, device, n_objects: int, hpams: Optional[dict] = None, rank: int = 0, world_size: int = 1, seed: int = 0,
                     group=None, batch: int = 64, dataset: str = "nusc", return_counts: bool = False, lidar: bool = False):
    """Shard ``n_objects`` synthetic objects over the ranks, optimise the local slice ``batch`` objects per launch
    (``batch=1``: the reference's one-object-at-a-time loop with its global random streams), all-gather the metric rows.
    Returns (n_objects, num_opts*4) on every rank; with ``return_counts`` a last column holds every object's depth-pixel count (the
    ``lidar_pts_cnt`` of the saved results).  ``lidar``: the synthetic objects carry lidar returns with measured depths, so the depth
    column is the reference's depth L1 (src/optimizer_nuscenes.py:751-765)."""
    hpams = hpams or load_hpams(dataset=dataset)
    mine = list(shard_slice(n_objects, world_size, rank))
    objs = make_kitti_objects(mine, hpams) if dataset in ("kitti", "waymo") else make_objects(mine, hpams["render_im_sz"], lidar=lidar)
    rows, counts = [], []

    def start_codes(index):
        g = torch.Generator().manual_seed(seed * 7919 + index)
        return torch.randn(1, 256, generator=g) * 0.3, torch.randn(1, 256, generator=g) * 0.3
    if batch <= 1 or hpams.get("sym_aug", 0) or not U._is_native(model):
        for ob in objs:
            sc, tc = start_codes(ob["index"])
            info = {}
            m, *_ = optimize_object(model, device, ob, hpams, sc, tc, seed=seed * 7919 + ob["index"], info=info)
            rows.append(m.reshape(-1)); counts += info["lidar_count"].tolist()
    else:
        for i in range(0, len(objs), batch):
            part = objs[i:i + batch]
            codes = [start_codes(ob["index"]) for ob in part]
            info = {}
            m, *_ = optimize_objects_batched(model, device, part, hpams, torch.cat([c[0] for c in codes]), torch.cat([c[1] for c in codes]),
                                             [seed * 7919 + ob["index"] for ob in part], info=info)
            rows += list(m.reshape(len(part), -1).cpu()); counts += info["lidar_count"].tolist()
    n_cols = hpams["optimize"]["num_opts"] * 4 + (1 if return_counts else 0)
    dev = torch.device(device)
    if return_counts:
        rows = [torch.cat([r, torch.tensor([float(c)])]) for r, c in zip(rows, counts)]
    local = torch.stack(rows).to(dev) if rows else torch.zeros(0, n_cols, device=dev)
    return gather_metric_rows(local, torch.tensor(mine, device=dev, dtype=torch.float32), n_objects, group)
