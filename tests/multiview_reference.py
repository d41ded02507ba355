"""The multi-view fit restated on the CPU oracle: one instance seen in V views is fitted with ONE shape code and ONE texture code
(``optimize_objs_multi_anns_w_pose``, src/optimizer_nuscenes.py:1136-1270: one pose per view, random native-resolution pixels, rates halved;
``optimize_objs_multi_anns``, :883-1040: fixed poses, the resized grid, rates never halved).  Per iteration and view: pose -> camera-in-object
pose, rays of the picked pixels, shared stratified depths, decoder, composite, ``loss_rgb + coef loss_occ`` over the view's own sum of |occ|,
``loss.backward()`` -- the views' gradients accumulate in the shared codes' ``.grad`` -- then one ``torch.optim.AdamW`` step.

Everything random is an argument (``picks``, ``jitter``, the seeds of the start-pose noise) and the dtype is selectable: float32 is the
reference's arithmetic, float64 the truth the GPU gradients are measured against."""
import numpy as np
import torch

from oracle import supnerf_oracle as O


def invert_pose(P):
    Rt = P[:, :3].transpose(-1, -2)
    return torch.cat([Rt, -(Rt @ P[:, 3:])], dim=-1)


def rot_dist(R1, R2):
    d = R1 @ R2.transpose(-1, -2)
    return torch.acos((((d[0, 0] + d[1, 1] + d[2, 2]).clamp(-1, 3) - 1) / 2).clamp(-1, 1))


def render_view(params, view, cam2opt, sc, tc, n_samples, jitter, ids=None, im_sz=None, shapenet_obj_cood=True):
    """One view's render call: ``render_rays`` (``ids``: picks into the native roi, y-major; src/utils.py:380-432) or ``render_rays_v2``
    (``im_sz``: the resized grid; :435-502).  -> rgb (n,3), acc (n,), rgb_tgt (n,3), occ (n,1) in the dtype of ``cam2opt``."""
    dt = cam2opt.dtype
    img, mask = view["img"].to(dt), view["mask"].to(dt)
    if ids is not None:
        ids = np.asarray(ids)
        ids = ids[ids >= 0]                                   # (the reference draws min(h w, n_rays) pixels: the -1 fill is not there)
        rays_o, viewdir = O.pixel_rays(view["K"], cam2opt, view["roi"])
        rays_o, viewdir = rays_o[ids], viewdir[ids]
        rgb_tgt, occ = img.reshape(-1, 3)[ids], mask.reshape(-1, 1)[ids]
    else:
        rays_o, viewdir = O.pixel_rays(view["K"], cam2opt, view["roi"], uv_steps=[im_sz, im_sz])
        im, mk = O.resize_targets(view["img"], view["mask"], im_sz)
        rgb_tgt, occ = im.reshape(-1, 3).to(dt), mk.reshape(-1, 1).to(dt)
    near, far = O.sphere_bounds(cam2opt.detach(), float(view["obj_diag"]))
    z = O.shared_depth_samples(near, far, n_samples, jitter).type_as(rays_o)
    xyz, vd = O.points_on_rays(rays_o, viewdir, z)
    xyz = xyz / float(view["obj_diag"])
    xyz, vd = O.object_frame_transforms(xyz, vd, False, False, shapenet_obj_cood)
    sig, rgb = O.decoder_forward(params, xyz, vd, sc, tc)
    rgb_r, _, acc_r = O.composite(sig, rgb, z)
    return rgb_r, acc_r, rgb_tgt, occ


def start_poses(views, seeds, pose_noise, to_vec):
    """True object pose of every view plus the seeded noise, drawn like the package's loops draw it (rotation first)."""
    rot0, tr0, gt = [], [], []
    for view, seed in zip(views, seeds):
        rs = np.random.RandomState(seed)
        g = invert_pose(view["cam_pose"])
        rot0.append(to_vec(g[None, :, :3]) + torch.from_numpy(rs.randn(1, 3).astype(np.float32)) * pose_noise[0])
        tr0.append(g[:, 3:].T + torch.from_numpy(rs.randn(1, 3).astype(np.float32)) * pose_noise[1])
        gt.append(g)
    return torch.cat(rot0), torch.cat(tr0), gt


def fit(params, views, hpams, sc0, tc0, seeds, jitter, picks=None, opt_pose=True, pose_noise=(0.05, 0.3), dtype=torch.float32,
        to_matrix=O.rotvec_to_matrix, to_vec=O.matrix_to_rotvec, steps=True, start=None):
    """ONE instance: ``views`` share ``sc0`` / ``tc0`` (1,256).  ``picks`` (T,V,n) -> random native pixels, None -> the resized grid.
    ``start``: the start pose parameters themselves.  ``jitter`` (T,2,V,S): draw 0 feeds the render, draw 1 the loop's lidar render (not restated: it moves nothing).
    -> dict: psnr, loss, rot_err, trans_err (T,V); grads [T] of (d shape, d texture, d rot (V,3), d trans (V,3)) as the step reads them;
    codes [T] of (shape, texture) after the step; renders [T][V] of (rgb, acc, rgb_tgt, occ)."""
    opt = hpams["optimize"]
    T, S, V = int(opt["num_opts"]), int(hpams["n_samples"]), len(views)
    p = {k: v.to(dtype) for k, v in params.items()}
    sc, tc = sc0.detach().clone().to(dtype).requires_grad_(), tc0.detach().clone().to(dtype).requires_grad_()
    rot0, tr0, gt = start_poses(views, seeds, pose_noise, to_vec)
    if start is not None:                                     # (rot0 (V,3), tr0 (V,3) as recorded, instead of the seeded draw)
        rot0, tr0 = start
    leaves = [sc, tc]
    if opt_pose:
        rot_vec, trans_vec = rot0.to(dtype).requires_grad_(), tr0.to(dtype).requires_grad_()
        leaves += [rot_vec, trans_vec]
    rates = [opt["lr_shape"], opt["lr_texture"], opt["lr_pose"], opt["lr_pose"]][:len(leaves)]
    make = lambda scale: torch.optim.AdamW([{"params": [q], "lr": lr * scale} for q, lr in zip(leaves, rates)])
    optim = make(1.0)
    out = dict(psnr=torch.zeros(T, V, dtype=dtype), loss=torch.zeros(T, V, dtype=dtype), rot_err=torch.zeros(T, V, dtype=dtype),
               trans_err=torch.zeros(T, V, dtype=dtype), grads=[], codes=[], renders=[])
    for it in range(T):
        optim.zero_grad()
        rendered = []
        for v, view in enumerate(views):
            if opt_pose:
                R = to_matrix(rot_vec[v])
                t = trans_vec[v].unsqueeze(-1)
                if not opt.get("opt_cam_pose", 0):
                    R = R.transpose(-2, -1)
                    t = -R @ t
                cam2opt = torch.cat([R, t], dim=-1)
            else:
                cam2opt = view["cam_pose"].to(dtype)
            rgb, acc, tgt, occ = render_view(p, view, cam2opt, sc, tc, S, jitter[it, 0, v], ids=None if picks is None else picks[it, v],
                                             im_sz=hpams["render_im_sz"], shapenet_obj_cood=bool(hpams["shapenet_obj_cood"]))
            loss, _, _, psnr = O.optimise_losses(rgb, acc, tgt, occ, hpams["loss_occ_coef"])
            loss.backward()                                   # accumulates into the shared codes' .grad (:1192)
            pred = invert_pose(cam2opt.detach())
            out["psnr"][it, v], out["loss"][it, v] = psnr.detach(), loss.detach()
            out["rot_err"][it, v] = rot_dist(pred[:, :3], gt[v][:, :3].to(dtype))
            out["trans_err"][it, v] = (pred[:, 3] - gt[v][:, 3].to(dtype)).norm()
            rendered.append(tuple(x.detach().clone() for x in (rgb, acc, tgt, occ)))
        out["renders"].append(rendered)
        out["grads"].append(tuple(q.grad.detach().clone() for q in leaves))
        if steps:
            optim.step()
        out["codes"].append((sc.detach().clone(), tc.detach().clone()))
        if opt_pose and (it + 1) % opt["lr_half_interval"] == 0:      # (:1266-1270; the fixed-pose variant has it commented out, :1039-1040)
            optim = make(2.0 ** (-((it + 1) // opt["lr_half_interval"])))
    out["poses"] = torch.stack([torch.cat([to_matrix(rot_vec[v]), trans_vec[v].unsqueeze(-1)], -1).detach() for v in range(V)]) if opt_pose else None
    return out
