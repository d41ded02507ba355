"""GPU test of ``driver.optimize_scene`` (the joint fit of a frame's objects on the fused scene kernels) against the same loop written here
from public pieces: ``scene.render_scene`` on its default route, ``driver.losses``, ``driver.make_optimizer`` (torch.optim.AdamW) and
``driver.axis_angle_to_matrix``.

Band, not fixed in advance: per compared quantity 4 x the distance between that twin run with fp32 pose leaves and with float64 pose leaves
(``scene_ray_rows`` works in the poses' dtype), floor one fp32 ulp of the quantity's largest magnitude.  The twin also checks every
iteration that ``scene.scene_rois`` on the device gives the host's rois; if they ever differ the two loops do not render the same pixels
through the same objects and the test says so instead of comparing."""
import copy

import numpy as np
import pytest
import torch

from oracle_bands import amd, dev, make_model  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

T, S = 6, 16
NOISE, SEED = (0.02, 0.1), 3
ULP = float(torch.finfo(torch.float32).eps)


@pytest.fixture(scope="module")
def setup(amd, dev, golden, oracle_params):
    g = golden("scene")
    H, W = int(g["H"]), int(g["W"])
    table, valid, _ = amd.scene.scene_rays(g["obj_poses"], g["obj_wlh"], g["K"], H, W)
    hit = ((table[..., 7] - table[..., 6]) > 0).view(H * W, -1)
    all3 = torch.nonzero(hit.all(1)).flatten()
    others = torch.nonzero(valid & ~hit.all(1)).flatten()
    idx = torch.cat([all3, others[torch.linspace(0, others.numel() - 1, 150).long()]])
    pixels = torch.stack([idx % W, idx // W], 1)
    gen = torch.Generator().manual_seed(11)
    frame = dict(K=g["K"], H=H, W=W, img=torch.rand(H, W, 3, generator=gen), obj_poses=g["obj_poses"], obj_wlh=g["obj_wlh"],
                 occ=torch.where(hit.any(1), 1.0, -1.0).view(H, W))
    frame["occ"][::7, ::5] = 0.0                                              # some pixels of unknown occupancy
    hp = amd.driver.load_hpams()
    hp["n_samples"] = S
    hp["optimize"].update(num_opts=T, lr_half_interval=4)
    jitter = torch.rand(T, pixels.shape[0] * g["obj_poses"].shape[0], S, generator=gen)
    return dict(g=g, frame=frame, pixels=pixels, hp=hp, jitter=jitter, model=make_model(amd, dev, oracle_params, "fp32"))


def twin(amd, dev, s, dtype):
    """The loop from public pieces with pose leaves of ``dtype``: (losses (T,), poses, shape codes, texture codes, rois agreed)."""
    D, g, frame, hp, pixels = amd.driver, s["g"], s["frame"], s["hp"], s["pixels"]
    opt = hp["optimize"]
    gt = frame["obj_poses"].float()
    Nb = gt.shape[0]
    rs = np.random.RandomState(SEED)                                         # the start optimize_scene documents
    rot_vec = (D.matrix_to_axis_angle(gt[:, :, :3]) + torch.from_numpy(rs.randn(Nb, 3).astype(np.float32)) * NOISE[0]).to(dev, dtype).requires_grad_()
    trans_vec = (gt[:, :, 3] + torch.from_numpy(rs.randn(Nb, 3).astype(np.float32)) * NOISE[1]).to(dev, dtype).requires_grad_()
    sc, tc = g["shapecodes"].clone().to(dev).requires_grad_(), g["texturecodes"].clone().to(dev).requires_grad_()
    tgt = frame["img"][pixels[:, 1], pixels[:, 0]].to(dev)
    occ = frame["occ"][pixels[:, 1], pixels[:, 0]].to(dev)[:, None]
    lr = {k: opt[k] for k in ("lr_shape", "lr_texture", "lr_pose")}
    optim = D.make_optimizer(sc, tc, rot_vec, trans_vec, lr)
    losses, agreed = [], True
    for it in range(T):
        optim.zero_grad()
        poses = torch.cat([D.axis_angle_to_matrix(rot_vec), trans_vec[:, :, None]], dim=2)
        on_device = amd.scene.scene_rois(poses.detach().float(), frame["obj_wlh"], frame["K"], frame["H"], frame["W"]).cpu()
        on_host = amd.scene.scene_rois(poses.detach().float().cpu(), frame["obj_wlh"], frame["K"], frame["H"], frame["W"])
        agreed = agreed and torch.equal(on_device, on_host)
        rgb, _, acc = amd.scene.render_scene(s["model"], dev, poses, frame["obj_wlh"], sc, tc, frame["K"], pixels, frame["H"], frame["W"], S,
                                             jitter=s["jitter"][it].to(dev), shapenet_obj_cood=bool(hp["shapenet_obj_cood"]))
        loss, _ = D.losses(rgb, acc, tgt, occ, hp["loss_occ_coef"])
        loss.backward()
        losses.append(loss.detach())
        optim.step()
        if (it + 1) % opt["lr_half_interval"] == 0:
            lr = {k: v * 2 ** (-((it + 1) // opt["lr_half_interval"])) for k, v in lr.items()}
            optim = D.make_optimizer(sc, tc, rot_vec, trans_vec, lr)
    poses = torch.cat([D.axis_angle_to_matrix(rot_vec.detach()), trans_vec.detach()[:, :, None]], dim=2)
    return [t.double().cpu() for t in (torch.stack(losses), poses, sc.detach(), tc.detach())], agreed


def test_optimize_scene_against_its_twin(amd, dev, setup):
    s = setup
    info = {}
    metrics, losses, sc, tc, poses = amd.driver.optimize_scene(s["model"], dev, s["frame"], s["hp"], s["g"]["shapecodes"], s["g"]["texturecodes"],
                                                               pose_noise=NOISE, seed=SEED, jitter=s["jitter"], pixels=s["pixels"], info=info)
    Nb = s["g"]["obj_poses"].shape[0]
    assert metrics.shape == (T, Nb, 2) and losses.shape == (T, 4) and poses.shape == (Nb, 3, 4) and info["hit_share"].shape == (T,)
    assert bool(torch.isfinite(metrics).all()) and bool(torch.isfinite(losses).all()) and 0 < float(info["hit_share"].min()) < 1
    assert all(p.requires_grad for p in s["model"].parameters())              # the decoder's weights are handed back trainable
    t32, ok32 = twin(amd, dev, s, torch.float32)
    t64, ok64 = twin(amd, dev, s, torch.float64)
    assert ok32 and ok64, "scene_rois on the device left the host's rois: the loops render different pixel sets, nothing to compare"
    # the metrics are the errors of the poses each iteration rendered: iteration 0 renders the noisy start
    D = amd.driver
    rs = np.random.RandomState(SEED)
    gt = s["frame"]["obj_poses"].float()
    rot0 = D.matrix_to_axis_angle(gt[:, :, :3]) + torch.from_numpy(rs.randn(Nb, 3).astype(np.float32)) * NOISE[0]
    tr0 = gt[:, :, 3] + torch.from_numpy(rs.randn(Nb, 3).astype(np.float32)) * NOISE[1]
    assert float((metrics[0, :, 0].cpu() - D.rot_dist(D.axis_angle_to_matrix(rot0), gt[:, :, :3])).abs().max()) < 1e-4
    assert float((metrics[0, :, 1].cpu() - (tr0 - gt[:, :, 3]).norm(dim=-1)).abs().max()) < 1e-5
    got = [t.double().cpu() for t in (losses[:, 0], poses, sc, tc)]
    bad = []
    for name, k, a, b in zip(("loss per iteration", "poses", "shape codes", "texture codes"), got, t32, t64):
        top = float(a.abs().max())
        band = max(4 * float((a - b).abs().max()), ULP * 2.0 ** np.floor(np.log2(top)))
        err = float((k - a).abs().max())
        print(f"optimize_scene {name}: loop - twin {err:.3e}, band {band:.3e} (twin fp32 - float64 leaves {band / 4:.3e}), largest {top:.3e}")
        if not err <= band:
            bad.append((name, err, band))
    print("losses", losses[:, 0].tolist(), "twin", t32[0].tolist())
    assert not bad, bad


def test_argument_errors(amd, dev, setup):
    s = setup
    g, D = s["g"], amd.driver
    hp = copy.deepcopy(s["hp"])
    hp["n_samples"] = 256                                                     # 3 objects x 256 samples > 512
    with pytest.raises(amd.SnrError, match="512"):
        D.optimize_scene(s["model"], dev, s["frame"], hp, g["shapecodes"], g["texturecodes"])
    with pytest.raises(amd.SnrError, match="same number"):
        D.optimize_scene(s["model"], dev, s["frame"], s["hp"], g["shapecodes"][:2], g["texturecodes"])
    with pytest.raises(amd.SnrError, match="same number"):
        D.optimize_scene(s["model"], dev, dict(s["frame"], obj_wlh=g["obj_wlh"][:2]), s["hp"], g["shapecodes"], g["texturecodes"])
    with pytest.raises(amd.SnrError, match="jitter"):
        D.optimize_scene(s["model"], dev, s["frame"], s["hp"], g["shapecodes"], g["texturecodes"], jitter=s["jitter"][:, :5], pixels=s["pixels"])
    hp = copy.deepcopy(s["hp"])
    hp["sym_aug"] = 1
    with pytest.raises(amd.SnrError, match="sym_aug"):
        D.optimize_scene(s["model"], dev, s["frame"], hp, g["shapecodes"], g["texturecodes"])
    with pytest.raises(amd.SnrError, match="decoder"):
        D.optimize_scene(torch.nn.Linear(1, 1), dev, s["frame"], s["hp"], g["shapecodes"], g["texturecodes"])
