#!/usr/bin/env python3
"""Fixture of the multi-view fit taken from the reference (needs the reference checkout ``gen_golden.py`` imports): ``multiview.npz``.

``OptimizerNuScenes.optimize_objs_multi_anns_w_pose`` (src/optimizer_nuscenes.py:1050-1277) lives in a module that cannot be imported
here (pytorch3d, nuscenes-devkit, skimage are absent), so -- as ``gen_golden.py`` does for ``vis_scene`` and ``gen_golden_r4.py`` for the
pose table -- this script makes the SAME sequence of calls into the reference's own building blocks for 2 views x 2 iterations of one
instance: per view and iteration ``utils.render_rays`` (a fresh ``np.random.permutation`` of the native roi, ``torch.rand`` depths) on the
reference's ``CodeNeRF``, the loop's loss, ``loss.backward()`` accumulating in the shared codes, ``utils.render_rays_specified`` for the
depth log (it consumes the second ``torch.rand`` draw), then ONE ``torch.optim.AdamW`` step over codes and per-view poses.  The rotation
conversions (pytorch3d in the reference, parity unpinned) are the oracle's.  S = 16, n_rays = 24, rois of 6 x 5 and 9 x 7 pixels: both views
have more pixels than picks, so both go through the permutation.

Recorded: the inputs, the picks and depth draws the reference made, per view the rendered rgb / acc and the gathered targets, the accumulated
code and pose gradients the step read, and the codes after each step.  Numbers only; the decoder weights are ``init_decoder_params(seed=0)``
and are not stored.  The script asserts that ``tests/multiview_reference.py`` in float32 reproduces the picks and targets exactly.

Usage:  python tests/golden/gen_golden_multiview.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from oracle import supnerf_oracle as O  # noqa: E402
import multiview_reference as MR  # noqa: E402
from gen_golden import RandTap, import_reference, make_model, save  # noqa: E402

S, N_RAYS, T = 16, 24, 2
SIZES = [(6, 5), (9, 7)]                  # (w, h) of the two rois
SEEDS = [41, 42]
POSE_NOISE = (0.05, 0.3)
LR = dict(lr_shape=0.02, lr_texture=0.02, lr_pose=0.01)
COEF = 0.1


def make_views():
    views = []
    g = torch.Generator().manual_seed(606)
    diag = np.float32(O.synthetic_object(50)["obj_diag"])               # one instance: one size
    for j, (w, h) in enumerate(SIZES):
        ob = O.synthetic_object(50 + j)
        x0, y0, x1, y1 = [int(v) for v in ob["roi"]]
        cx, cy = (x0 + x1) // 2, (y0 + y1) // 2
        roi = torch.tensor([cx - w // 2, cy - h // 2, cx - w // 2 + w, cy - h // 2 + h], dtype=torch.int32)
        img = torch.rand(h, w, 3, generator=g)
        mask = (torch.randint(0, 3, (h, w, 1), generator=g) - 1).float()
        img = img * (mask > 0) + (mask <= 0)
        views.append(dict(img=img, mask=mask, cam_pose=ob["cam_pose"], K=ob["K"], roi=roi, obj_diag=diag))
    return views


class PermutationTap:
    def __enter__(self):
        self.draws, self._perm = [], np.random.permutation

        def permutation(n):
            out = self._perm(n)
            self.draws.append(np.array(out))
            return out
        np.random.permutation = permutation
        return self

    def __exit__(self, *exc):
        np.random.permutation = self._perm


def main():
    codenerf, RU, _ = import_reference()
    model, params = make_model(codenerf)
    views = make_views()
    V = len(views)
    g = torch.Generator().manual_seed(17)
    sc0, tc0 = torch.randn(1, 256, generator=g) * 0.3, torch.randn(1, 256, generator=g) * 0.3
    rot0, tr0, _ = MR.start_poses(views, SEEDS, POSE_NOISE, O.matrix_to_rotvec)
    sc, tc = sc0.clone().requires_grad_(), tc0.clone().requires_grad_()
    rot_vec, trans_vec = rot0.clone().requires_grad_(), tr0.clone().requires_grad_()
    optim = torch.optim.AdamW([{"params": [sc], "lr": LR["lr_shape"]}, {"params": [tc], "lr": LR["lr_texture"]},
                               {"params": [rot_vec], "lr": LR["lr_pose"]}, {"params": [trans_vec], "lr": LR["lr_pose"]}])
    lidar = [(np.array([1, 3, 2]), np.array([0, 2, 4])), (np.array([0, 5, 8, 3]), np.array([1, 6, 2, 3]))]      # (x_vec, y_vec) per view
    np.random.seed(2024); torch.manual_seed(2024)
    picks = np.full((T, V, N_RAYS), -1, dtype=np.int32)
    jitter = np.zeros((T, 2, V, S), dtype=np.float32)
    rec = {k: [] for k in ("rgb", "acc", "tgt", "occ", "g_sc", "g_tc", "g_rot", "g_tr", "sc", "tc", "rot", "tr", "loss")}
    for it in range(T):
        optim.zero_grad()
        for v, view in enumerate(views):
            R = O.rotvec_to_matrix(rot_vec[v]).transpose(-2, -1)
            cam2opt = torch.cat([R, -R @ trans_vec[v].unsqueeze(-1)], dim=-1)
            with PermutationTap() as ptap, RandTap() as rtap:
                rgb, _, acc, tgt, occ = RU.render_rays(model, "cpu", view["img"], view["mask"], cam2opt, view["obj_diag"], view["K"], view["roi"], S,
                                                       sc, tc, 1, 0, n_rays=N_RAYS)
            assert len(ptap.draws) == 1 and len(rtap.draws) == 1
            ids = ptap.draws[0][:N_RAYS]
            picks[it, v, :len(ids)] = ids
            jitter[it, 0, v] = rtap.draws[0].numpy()
            a = occ.abs()
            loss_rgb = ((rgb - tgt).pow(2) * a).sum() / (a.sum() + 1e-9)
            loss_occ = ((-occ * (0.5 - acc[:, None])).exp() * a).sum() / (a.sum() + 1e-9)
            loss = loss_rgb + COEF * loss_occ
            loss.backward()
            with torch.no_grad(), RandTap() as rtap:
                RU.render_rays_specified(model, "cpu", view["img"], view["mask"], cam2opt, view["obj_diag"], view["K"], view["roi"], lidar[v][0],
                                         lidar[v][1], S, sc, tc, 1, 0)
            jitter[it, 1, v] = rtap.draws[0].numpy()
            for k, x in (("rgb", rgb), ("acc", acc), ("tgt", tgt), ("occ", occ), ("loss", loss)):
                rec[k].append(x.detach().clone())
        for k, q in (("g_sc", sc), ("g_tc", tc), ("g_rot", rot_vec), ("g_tr", trans_vec)):
            rec[k].append(q.grad.detach().clone())
        optim.step()
        for k, q in (("sc", sc), ("tc", tc), ("rot", rot_vec), ("tr", trans_vec)):
            rec[k].append(q.detach().clone())

    # the restatement in float32, on the recorded picks and draws
    hp = dict(n_samples=S, render_im_sz=8, shapenet_obj_cood=1, loss_occ_coef=COEF, optimize=dict(num_opts=T, lr_half_interval=1000, opt_cam_pose=0, **LR))
    got = MR.fit(params, views, hp, sc0, tc0, SEEDS, torch.from_numpy(jitter), picks=picks, pose_noise=POSE_NOISE)
    k = 0
    for it in range(T):
        for v in range(V):
            assert torch.equal(got["renders"][it][v][2], rec["tgt"][k]) and torch.equal(got["renders"][it][v][3], rec["occ"][k])
            print(f"it {it} view {v}: rgb {float((got['renders'][it][v][0] - rec['rgb'][k]).abs().max()):.2e} "
                  f"acc {float((got['renders'][it][v][1] - rec['acc'][k]).abs().max()):.2e}")
            k += 1
        print(f"it {it}: d shape {float((got['grads'][it][0] - rec['g_sc'][it]).abs().max()):.2e} of {float(rec['g_sc'][it].abs().max()):.2e}, "
              f"codes {float((got['codes'][it][0] - rec['sc'][it]).abs().max()):.2e}")
    st = lambda xs: torch.stack(xs).numpy()
    arrays = dict(picks=picks, jitter=jitter, sc0=sc0, tc0=tc0, rot0=rot0, tr0=tr0, seeds=np.array(SEEDS), pose_noise=np.array(POSE_NOISE),
                  n_samples=np.int64(S), n_rays=np.int64(N_RAYS), loss_occ_coef=np.float64(COEF),
                  lr=np.array([LR["lr_shape"], LR["lr_texture"], LR["lr_pose"]]),
                  rgb=st(rec["rgb"]).reshape(T, V, N_RAYS, 3), acc=st(rec["acc"]).reshape(T, V, N_RAYS), tgt=st(rec["tgt"]).reshape(T, V, N_RAYS, 3),
                  occ=st(rec["occ"]).reshape(T, V, N_RAYS), loss=st(rec["loss"]).reshape(T, V),
                  g_sc=st(rec["g_sc"]), g_tc=st(rec["g_tc"]), g_rot=st(rec["g_rot"]), g_tr=st(rec["g_tr"]),
                  sc=st(rec["sc"]), tc=st(rec["tc"]), rot=st(rec["rot"]), tr=st(rec["tr"]))
    for v, view in enumerate(views):
        arrays.update({f"img{v}": view["img"], f"mask{v}": view["mask"], f"cam_pose{v}": view["cam_pose"], f"K{v}": view["K"], f"roi{v}": view["roi"],
                       f"obj_diag{v}": np.float32(view["obj_diag"])})
    save("multiview", **arrays)


if __name__ == "__main__":
    main()
