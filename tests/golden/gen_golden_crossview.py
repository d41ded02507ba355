#!/usr/bin/env python3
"""Fixture of the cross-view evaluation taken from the reference (needs the reference checkout ``gen_golden.py`` imports): ``crossview.npz``.

``OptimizerNuScenes.eval_cross_view`` (src/optimizer_nuscenes.py:1279-1410) lives in a module that cannot be imported here (pytorch3d,
nuscenes-devkit, skimage are absent), so -- as ``gen_golden_multiview.py`` does for the multi-view fit -- this script makes the SAME sequence of
calls into the reference's own building blocks for one instance with V = 3 views and C = 2 code snapshots: per snapshot, per view ``ii`` whose
codes are rendered and per view ``num`` that is rendered, ``utils.render_rays_v2`` (``n_rays=None``, the ``render_im_sz``^2 grid) on the
reference's ``CodeNeRF`` on the CPU, the loss and PSNR of :1359-1362, ``utils.render_rays_specified`` at view ``num``'s lidar pixels and the
depth error of :1378-1379.  ``RandTap`` around each of the two renders records the two ``torch.rand`` draws of every pair.

Rois of 6 x 5, 7 x 9 and 12 x 12 pixels (w x h: one wide, one tall, one square) at non-zero origins with ``render_im_sz`` = 8: the resize sees
crops smaller and larger than the grid.  Masks in {-1,0,1}; S = 16; lidar pixel sets of 3, 4 and 5 returns with made-up measured depths.

Recorded: the inputs, the 2 P draws, per pair rgb / rgb_tgt / occ_pixels / depth_pred_vec, the fp32 loss and the float64 PSNR and depth
error as the reference's lines compute them; and ``cross_psnr_mean`` / ``cross_depth_mean``: the matrices are written with
``supnerf_amd.io.save_cross_eval`` and read back by the reference's own ``collect_eval_results`` (src/utils.py:926-986), whose cross-view
curves are taken from the axes it plots them on.  Numbers only; the decoder weights are ``init_decoder_params(seed=0)`` and are not stored.
The script asserts that ``tests/crossview_reference.py`` in float32 reproduces ``rgb_tgt`` and ``occ_pixels`` exactly and prints the
restatement's distance from the reference's rgb, depth, loss and depth error (the bands of tests/test_crossview_cpu.py).

Usage:  python tests/golden/gen_golden_crossview.py
"""
import io as _io
import os
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from oracle import supnerf_oracle as O  # noqa: E402
import crossview_reference as CR  # noqa: E402
from gen_golden import RandTap, import_reference, make_model, save  # noqa: E402

S, IM_SZ, C_SNAP = 16, 8, 2
SIZES = [(6, 5), (7, 9), (12, 12)]        # (w, h) of the three rois
CODE_SAVE_ITERS = [0, 5]
LIDAR = [(np.array([1, 3, 2]), np.array([0, 2, 4])), (np.array([0, 5, 6, 3]), np.array([1, 6, 8, 3])),
         (np.array([2, 11, 7, 0, 5]), np.array([3, 0, 11, 6, 5]))]      # (x_vec, y_vec) crop pixels per view


def make_views():
    views = []
    g = torch.Generator().manual_seed(707)
    diag = np.float32(O.synthetic_object(60)["obj_diag"])               # one instance: one size
    for j, (w, h) in enumerate(SIZES):
        ob = O.synthetic_object(60 + j)
        x0, y0, x1, y1 = [int(v) for v in ob["roi"]]
        cx, cy = (x0 + x1) // 2, (y0 + y1) // 2
        roi = torch.tensor([cx - w // 2, cy - h // 2, cx - w // 2 + w, cy - h // 2 + h], dtype=torch.int32)
        assert int(roi[0]) > 0 and int(roi[1]) > 0
        img = torch.rand(h, w, 3, generator=g)
        mask = (torch.randint(0, 3, (h, w, 1), generator=g) - 1).float()
        img = img * (mask > 0) + (mask <= 0)
        x_vec, y_vec = LIDAR[j]
        assert x_vec.max() < w and y_vec.max() < h
        dist = float(np.linalg.norm(ob["cam_pose"][:, -1].tolist()))
        depth = (dist + (torch.rand(len(x_vec), generator=g) - 0.5) * float(diag)).numpy().astype(np.float32)      # made-up returns near the object
        views.append(dict(img=img, mask=mask, cam_pose=ob["cam_pose"], K=ob["K"], roi=roi, obj_diag=diag,
                          lidar_xy=np.stack([x_vec, y_vec], -1).astype(np.int64), lidar_depth=depth))
    return views


def main():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import supnerf_amd as A
    codenerf, RU, _ = import_reference()
    model, params = make_model(codenerf)
    views = make_views()
    V = len(views)
    g = torch.Generator().manual_seed(23)
    sc, tc = torch.randn(C_SNAP, V, 256, generator=g) * 0.3, torch.randn(C_SNAP, V, 256, generator=g) * 0.3
    pairs, _ = A.ops.cross_pairs((0, V), C_SNAP)
    P = pairs.shape[0]
    torch.manual_seed(2025)
    jitter = np.zeros((P, 2, S), dtype=np.float32)
    rec = {k: [] for k in ("rgb", "rgb_tgt", "occ_pixels", "depth_pred_vec", "loss")}
    psnr_ref, depth_ref = np.zeros(P), np.zeros(P)
    psnr_mat, depth_mat = np.zeros((C_SNAP, V, V)), np.zeros((C_SNAP, V, V))
    k = 0
    for cid in range(C_SNAP):
        for ii in range(V):
            assert pairs[k].tolist() == [cid * V + ii, 0]
            shapecode, texturecode = sc[cid, ii:ii + 1], tc[cid, ii:ii + 1]
            for num in range(V):
                view = views[num]
                x_vec, y_vec = view["lidar_xy"][:, 0], view["lidar_xy"][:, 1]
                with torch.no_grad(), RandTap() as tap:
                    rgb_rays, _, _, rgb_tgt, occ_pixels = RU.render_rays_v2(model, "cpu", view["img"], view["mask"], view["cam_pose"], view["obj_diag"],
                                                                           view["K"], view["roi"], S, shapecode, texturecode, 1, 0, im_sz=IM_SZ, n_rays=None)
                assert len(tap.draws) == 1
                jitter[k, 0] = tap.draws[0].numpy()
                loss_rgb2 = torch.sum((rgb_rays - rgb_tgt) ** 2 * torch.abs(occ_pixels)) / (torch.sum(torch.abs(occ_pixels)) + 1e-9)       # :1359-1360
                psnr = -10 * np.log(loss_rgb2.item()) / np.log(10)                                                                     # :1362
                gt_depth_vec = view["lidar_depth"]
                with torch.no_grad(), RandTap() as tap:
                    _, depth_pred_vec, _, _, _ = RU.render_rays_specified(model, "cpu", view["img"], view["mask"], view["cam_pose"], view["obj_diag"],
                                                                          view["K"], view["roi"], x_vec, y_vec, S, shapecode, texturecode, 1, 0)
                assert len(tap.draws) == 1
                jitter[k, 1] = tap.draws[0].numpy()
                depth_errs = abs(depth_pred_vec.cpu().numpy() - gt_depth_vec)                                                          # :1378
                depth_err_mean = np.sum(depth_errs) / (len(gt_depth_vec) + 1e-8)                                                       # :1379
                psnr_ref[k], depth_ref[k] = psnr, depth_err_mean
                psnr_mat[cid, ii, num], depth_mat[cid, ii, num] = psnr, depth_err_mean
                for key, x in (("rgb", rgb_rays), ("rgb_tgt", rgb_tgt), ("occ_pixels", occ_pixels), ("loss", loss_rgb2)):
                    rec[key].append(x.detach().clone())
                rec["depth_pred_vec"].append(depth_pred_vec.detach().clone())
                k += 1

    # the restatement on the recorded draws
    jit = torch.from_numpy(jitter)
    flat = lambda t: t.reshape(C_SNAP * V, 256)
    got = CR.evaluate(params, views, flat(sc), flat(tc), pairs, jit, S, IM_SZ, torch.float32)
    got64 = CR.evaluate(params, views, flat(sc), flat(tc), pairs, jit.double(), S, IM_SZ, torch.float64)
    d = dict(rgb=0.0, depth=0.0, loss=0.0, depth_err=0.0)
    d64 = dict(d)
    for k in range(P):
        assert torch.equal(got["rgb_tgt"][k], rec["rgb_tgt"][k]) and torch.equal(got["occ"][k], rec["occ_pixels"][k])
        for out, res in ((d, got), (d64, got64)):
            out["rgb"] = max(out["rgb"], float((res["rgb"][k].double() - rec["rgb"][k].double()).abs().max()))
            out["depth"] = max(out["depth"], float((res["depth"][k].double() - rec["depth_pred_vec"][k].double()).abs().max()))
            out["loss"] = max(out["loss"], abs(float(res["mse_fg"][k]) - float(rec["loss"][k])))
            out["depth_err"] = max(out["depth_err"], abs(float(res["depth_err"][k]) - depth_ref[k]))
    print("restatement fp32    - reference:", " ".join(f"{n} {v:.3e}" for n, v in d.items()))
    print("restatement float64 - reference:", " ".join(f"{n} {v:.3e}" for n, v in d64.items()))
    print(f"scales: rgb {float(torch.stack(rec['rgb']).abs().max()):.3e} depth {max(float(x.abs().max()) for x in rec['depth_pred_vec']):.3e} "
          f"loss {float(torch.stack(rec['loss']).max()):.3e} depth_err {depth_ref.max():.3e}")

    # our writer -> the reference's reader
    tmp = tempfile.mkdtemp(prefix="snr_cross_")
    path = A.io.save_cross_eval(tmp, {0: (psnr_mat, depth_mat)}, CODE_SAVE_ITERS, ids={0: "ins0"})
    res_path = A.io.save_driver_results(os.path.join(tmp, "res"), torch.rand(2, 6 * 4), [0, 1], n_lidar=64)
    fig, axes = plt.subplots(2, 2)
    # (the reference's matrices are numpy arrays and its reader predates torch.load's weights_only default: read the way it was written for)
    load = torch.load
    torch.load = lambda *a, **k: load(*a, **{**k, "weights_only": False})
    try:
        with redirect_stdout(_io.StringIO()):
            RU.collect_eval_results(res_path, 6, axes, "m", True, path, print_iters=[0, 3, 5], rot_outlier_ignore=False)
    finally:
        torch.load = load
    cross_psnr = np.asarray(axes[0, 0].lines[-1].get_ydata(), dtype=np.float64)
    cross_depth = np.asarray(axes[0, 1].lines[-1].get_ydata(), dtype=np.float64)
    assert list(axes[0, 0].lines[-1].get_xdata()) == CODE_SAVE_ITERS and cross_psnr.shape == (C_SNAP,)
    mine = A.io.cross_view_means({0: (psnr_mat, depth_mat)})
    assert np.array_equal(mine[0], cross_psnr) and np.array_equal(mine[1], cross_depth), (mine, cross_psnr, cross_depth)
    plt.close(fig)

    arrays = dict(jitter=jitter, sc=sc, tc=tc, pairs=pairs, n_samples=np.int64(S), render_im_sz=np.int64(IM_SZ), code_save_iters=np.array(CODE_SAVE_ITERS),
                  rgb=torch.stack(rec["rgb"]), rgb_tgt=torch.stack(rec["rgb_tgt"]), occ_pixels=torch.stack(rec["occ_pixels"]), loss=torch.stack(rec["loss"]),
                  psnr=psnr_ref, depth_err=depth_ref, psnr_mat=psnr_mat, depth_mat=depth_mat, cross_psnr_mean=cross_psnr, cross_depth_mean=cross_depth,
                  dist_fp32=np.array([d[n] for n in ("rgb", "depth", "loss", "depth_err")]))
    for k in range(P):
        arrays[f"depth_pred_vec{k}"] = rec["depth_pred_vec"][k]
    for v, view in enumerate(views):
        arrays.update({f"img{v}": view["img"], f"mask{v}": view["mask"], f"cam_pose{v}": view["cam_pose"], f"K{v}": view["K"], f"roi{v}": view["roi"],
                       f"obj_diag{v}": np.float32(view["obj_diag"]), f"lidar_xy{v}": view["lidar_xy"], f"lidar_depth{v}": view["lidar_depth"]})
    save("crossview", **arrays)


if __name__ == "__main__":
    main()
