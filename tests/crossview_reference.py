"""The cross-view evaluation restated on the CPU oracle (``OptimizerNuScenes.eval_cross_view``, src/optimizer_nuscenes.py:1322-1380): the
codes fitted to view ``ii`` rendered from the camera of view ``num`` -- ``render_rays_v2`` on the resized grid against that view's crop
(:1351-1360), ``render_rays_specified`` at its lidar pixels against their measured depths (:1370-1379) -- one (code row, target view) pair
at a time.  Everything random is an argument (``jitter`` (P,2,S): the grid draw and the depth draw of every pair) and the dtype is
selectable: float32 is the reference's arithmetic, float64 the truth the GPU is measured against."""
import numpy as np
import torch

from oracle import supnerf_oracle as O


def fixture_views(g, n_views=3):
    """The views of ``tests/golden/crossview.npz`` (``conftest.load_golden``) as the dicts the driver and ``evaluate`` take."""
    return [dict(img=g[f"img{v}"], mask=g[f"mask{v}"], cam_pose=g[f"cam_pose{v}"], K=g[f"K{v}"], roi=g[f"roi{v}"], obj_diag=np.float32(g[f"obj_diag{v}"]),
                 lidar_xy=np.asarray(g[f"lidar_xy{v}"]), lidar_depth=np.asarray(g[f"lidar_depth{v}"])) for v in range(n_views)]


def psnr_of(mse):
    """src/optimizer_nuscenes.py:1362, from the loss as a python float."""
    with np.errstate(divide="ignore"):
        return -10 * np.log(float(mse)) / np.log(10)


def evaluate(params, views, shapecodes, texturecodes, pairs, jitter, n_samples, im_sz, dtype=torch.float32, shapenet_obj_cood=True):
    """``views``: dicts with img (h,w,3), mask (h,w,1), cam_pose, K, roi, obj_diag, lidar_xy (n,2) crop pixels, lidar_depth (n,);
    ``shapecodes`` / ``texturecodes`` (R,256): the code rows; ``pairs`` (P,2) = [code row, target view]; ``jitter`` (P,2,S).
    -> dict of per-pair lists: rgb (n,3), rgb_tgt (n,3), occ (n,1), depth (n_lidar,), and tensors mse_fg (P,), depth_err (P,) in ``dtype``,
    psnr (P,) float64 (from the loss in ``dtype``)."""
    p = {k: v.to(dtype) for k, v in params.items()}
    out = dict(rgb=[], rgb_tgt=[], occ=[], depth=[], mse_fg=[], depth_err=[], psnr=[])
    with torch.no_grad():
        for k, (row, v) in enumerate(np.asarray(pairs).tolist()):
            view = views[v]
            cam, diag = view["cam_pose"].to(dtype), float(view["obj_diag"])
            sc, tc = shapecodes[row:row + 1].to(dtype), texturecodes[row:row + 1].to(dtype)
            rgb, _, _, tgt, occ = O.render_rays_v2(p, view["img"], view["mask"], cam, diag, view["K"], view["roi"], n_samples, sc, tc,
                                                   shapenet_obj_cood, im_sz=im_sz, jitter=jitter[k, 0])
            tgt_d, a = tgt.to(dtype), occ.to(dtype).abs()
            mse = torch.sum((rgb - tgt_d) ** 2 * a) / (torch.sum(a) + 1e-9)
            xy = np.asarray(view["lidar_xy"]).reshape(-1, 2).astype(np.int64)
            gt = torch.as_tensor(np.asarray(view["lidar_depth"], dtype=np.float32).reshape(-1)).to(dtype)
            if xy.shape[0]:
                _, depth, _, _, _ = O.render_rays_specified(p, view["img"], view["mask"], cam, diag, view["K"], view["roi"], xy[:, 0], xy[:, 1],
                                                            n_samples, sc, tc, shapenet_obj_cood, jitter=jitter[k, 1])
            else:
                depth = torch.zeros(0, dtype=dtype)
            err = (depth - gt).abs().sum() / (xy.shape[0] + 1e-8)
            for key, x in (("rgb", rgb), ("rgb_tgt", tgt), ("occ", occ), ("depth", depth), ("mse_fg", mse), ("depth_err", err)):
                out[key].append(x)
            out["psnr"].append(psnr_of(mse))
    out["mse_fg"], out["depth_err"] = torch.stack(out["mse_fg"]), torch.stack(out["depth_err"])
    out["psnr"] = np.array(out["psnr"], dtype=np.float64)
    return out


def metrics_definition(rgb, depth_pred, tgt, occ, lid_depth, lid_cnt, pairs, dtype):
    """``snr_cross_metrics``' formulas as torch expressions in ``dtype`` on CPU tensors: (P,3) = [mse_fg, depth_err, sum |occ|]."""
    rows = []
    n_l = depth_pred.shape[1]
    for p_, (_, v) in enumerate(pairs.tolist()):
        a = occ[v].to(dtype).abs()
        sq = ((rgb[p_].to(dtype) - tgt[v].to(dtype)) ** 2).sum(-1)
        cnt = min(max(int(lid_cnt[v]), 0), n_l)
        d = (depth_pred[p_, :cnt].to(dtype) - lid_depth[v, :cnt].to(dtype)).abs().sum()
        rows.append(torch.stack([(sq * a).sum() / (a.sum() + torch.tensor(1e-9, dtype=dtype)),
                                 d / (torch.tensor(float(cnt), dtype=dtype) + torch.tensor(1e-8, dtype=dtype)), a.sum()]))
    return torch.stack(rows)
