"""Timing of the cross-view evaluation on one GPU: device-synchronised wall clocks, medians of ``--reps`` calls, the two routes taken in turn.

Workload: ``--instances`` synthetic instances x ``--views`` views x ``--snapshots`` code snapshots (``driver.make_instances(..., lidar=True)``,
random codes), ``render_im_sz``^2 grid pixels and ``--samples`` samples: instances x snapshots x views^2 (code, view) pairs.

  * ``batched``: ``driver.eval_cross_view`` -- all pairs as objects of a handful of launches, one host read;
  * ``loop``: the same pairs rendered one by one through the public ``utils.render_rays_v2`` / ``utils.render_rays_specified`` with the
    reference's host work per pair (``.item()`` of the loss, numpy depth error; src/optimizer_nuscenes.py:1350-1380) -- code this tool
    leaves unchanged: the yardstick.  Both routes are fed the same draws.
  * ``--target batched|loop``: run that route twice (the first run warms up) and nothing else -- the profiling target for the launch counts:

        rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/cross_view_time.py --target batched

    the rows of NAME_kernel_trace.csv over 2.

Prints one JSON line (with the largest difference between the two routes' matrices).

usage: python tools/cross_view_time.py [--reps N] [--instances I] [--views V] [--snapshots C] [--im-sz n] [--samples S] [--target ROUTE]"""
import time

import numpy as np
import torch

import geometry_common as C
from supnerf_amd import driver, ops, utils as U


def wall_ms(fn):
    """Milliseconds of one call on the wall clock, the device idle before and after."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def loop_route(model, dev, inst, hp, sc, tc, jitter):
    """The reference's shape of the loop (src/optimizer_nuscenes.py:1305-1400) on the public render functions."""
    S, im_sz = hp["n_samples"], hp["render_im_sz"]
    out, k, v0 = {}, 0, 0
    for i, one in enumerate(inst):
        views = one["views"]
        n = len(views)
        psnr_mat, depth_mat = np.zeros((sc.shape[0], n, n)), np.zeros((sc.shape[0], n, n))
        for cid in range(sc.shape[0]):
            for ii in range(n):
                shapecode, texturecode = sc[cid, v0 + ii:v0 + ii + 1], tc[cid, v0 + ii:v0 + ii + 1]
                for num, view in enumerate(views):
                    with torch.no_grad(), U.jitter_override(jitter[k, 0]):
                        rgb, _, _, tgt, occ = U.render_rays_v2(model, dev, view["img"], view["mask"], view["cam_pose_dev"], view["obj_diag"], view["K"],
                                                               view["roi"], S, shapecode, texturecode, hp["shapenet_obj_cood"], 0, im_sz=im_sz, n_rays=None)
                    loss = torch.sum((rgb - tgt) ** 2 * torch.abs(occ)) / (torch.sum(torch.abs(occ)) + 1e-9)
                    psnr_mat[cid, ii, num] = -10 * np.log(loss.item()) / np.log(10)
                    xy = np.asarray(view["lidar_xy"])
                    with torch.no_grad(), U.jitter_override(jitter[k, 1]):
                        _, d_vec, _, _, _ = U.render_rays_specified(model, dev, view["img"], view["mask"], view["cam_pose_dev"], view["obj_diag"], view["K"],
                                                                    view["roi"], xy[:, 0], xy[:, 1], S, shapecode, texturecode, hp["shapenet_obj_cood"], 0)
                    errs = abs(d_vec.cpu().numpy() - np.asarray(view["lidar_depth"]))
                    depth_mat[cid, ii, num] = np.sum(errs) / (len(errs) + 1e-8)
                    k += 1
        out[i] = (psnr_mat, depth_mat)
        v0 += n
    return out


def main():
    a = C.arguments(C.BLOCKS, ("--instances", dict(type=int, default=8)), ("--views", dict(type=int, default=6)),
                    ("--snapshots", dict(type=int, default=6)), ("--im-sz", dict(type=int, default=32)), ("--samples", dict(type=int, default=64)),
                    ("--target", dict(choices=("batched", "loop"), default=None)))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    model = C.fog_decoder(sb, tb, dev)
    inst = driver.make_instances(list(range(a.instances)), a.views, lidar=True)
    for one in inst:            # (the loop route's poses live on the GPU: the public functions then make rays and depths in one launch)
        for view in one["views"]:
            view["cam_pose_dev"] = view["cam_pose"].to(dev)
    hp = driver.load_hpams()
    hp["n_samples"], hp["render_im_sz"] = a.samples, a.im_sz
    V = a.instances * a.views
    g = torch.Generator().manual_seed(1)
    sc, tc = (torch.randn(a.snapshots, V, 256, generator=g) * 0.3).to(dev), (torch.randn(a.snapshots, V, 256, generator=g) * 0.3).to(dev)
    P = ops.cross_pairs(ops.view_offset_of([a.views] * a.instances), a.snapshots)[0].shape[0]
    jitter = torch.rand(P, 2, a.samples, generator=g)
    jitter_d = jitter.to(dev)
    info = {}
    batched = lambda: driver.eval_cross_view(model, dev, inst, hp, sc, tc, jitter=jitter_d, info=info)
    loop = lambda: loop_route(model, dev, inst, hp, sc, tc, jitter_d)
    if a.target is not None:
        fn = batched if a.target == "batched" else loop
        for _ in range(2):
            fn()
            torch.cuda.synchronize()
        C.report("cross_view_time", a, (sb, tb), target=a.target, runs=2, pairs=P, precision=str(model.last_precision))
        return
    res_b, res_l = batched(), loop()                                                  # warm-up, and the two routes' answers
    diff_psnr = max(float(np.abs(res_b[i][0] - res_l[i][0]).max()) for i in res_b)
    diff_depth = max(float(np.abs(res_b[i][1] - res_l[i][1]).max()) for i in res_b)
    t_b, t_l = [], []
    for _ in range(a.reps):
        t_b.append(wall_ms(batched)[0])
        t_l.append(wall_ms(loop)[0])
    tb_ms, tl_ms = float(np.median(t_b)), float(np.median(t_l))
    C.report("cross_view_time", a, (sb, tb), reps=a.reps, precision=str(model.last_precision), instances=a.instances, views=V, snapshots=a.snapshots,
             pairs=P, grid_rays=a.im_sz ** 2, S=a.samples, lidar_max=int(max(len(v["lidar_depth"]) for i in inst for v in i["views"])),
             pair_chunk=info["pair_chunk"], batched_ms=round(tb_ms, 3), loop_ms=round(tl_ms, 3), loop_over_batched=round(tl_ms / tb_ms, 2),
             batched_ms_all=[round(t, 3) for t in t_b], loop_ms_all=[round(t, 3) for t in t_l],
             max_abs_diff={"psnr_dB": diff_psnr, "depth_err": diff_depth})


if __name__ == "__main__":
    main()
