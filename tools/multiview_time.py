"""Timing of the multi-view fit on one GPU: device events, medians of ``--reps`` calls, calls that are compared taken in turn.

  * one iteration of ``driver.optimize_instances`` at ``--instances`` instances x ``--views`` views each, ``--rays`` random native pixels per
    view and iteration, ``--samples`` samples: the difference of a 6- and a 2-iteration run over 4 (picks and jitter made beforehand);
  * beside it the same views run one at a time: as many separate ``driver.optimize_object`` loops (the same loop body,
    ``driver._fit_views``, at one object on the fixed grid and without the ``view_pixels`` / ``InstanceRows`` launches; ``render_im_sz``^2 =
    ``--rays`` grid pixels each), the same difference summed over the views;
  * ``--target V T``: only run ``optimize_instances`` on V views (instances of ``--views`` views; one instance of one view at V = 1) for T
    iterations, twice (the first run warms up) -- the profiling target for the launch count per iteration, counted like tools/prof_loop.py:

        rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/multiview_time.py --target V T

    the rows of NAME_kernel_trace.csv at T = 12 minus those at T = 4, over 16 (two runs of 8 more iterations).

Prints one JSON line.

usage: python tools/multiview_time.py [--reps N] [--instances I] [--views V] [--rays n] [--samples S] [--commit SHA] [--target V T]"""
import torch

import geometry_common as C
from ray_surface_time import in_turn
from supnerf_amd import driver


def setup(n_instances, n_views, n_rays, S, T, dev):
    inst = driver.make_instances(list(range(n_instances)), n_views)
    views = [v for i in inst for v in i["views"]]
    V = len(views)
    seeds = list(range(100, 100 + V))
    hp = driver.load_hpams()
    hp["n_samples"] = S
    hp["render_im_sz"] = int(round(n_rays ** 0.5))
    g = torch.Generator().manual_seed(1)
    sc0, tc0 = torch.randn(n_instances, 256, generator=g) * 0.3, torch.randn(n_instances, 256, generator=g) * 0.3
    picks = driver.draw_view_picks(views, seeds, T, n_rays)
    jitter = torch.rand(T, 2, V, S, generator=g).to(dev)        # (the default draw is a CPU generator's: host time that grows with the iterations)
    return inst, views, seeds, hp, sc0, tc0, picks, jitter


def target(model, a, dev):
    V, T = a.target
    n_inst, per = (1, 1) if V < a.views else (V // a.views, a.views)
    inst, views, seeds, hp, sc0, tc0, picks, jitter = setup(n_inst, per, a.rays, a.samples, T, dev)
    hp["optimize"]["num_opts"] = T
    for _ in range(2):
        driver.optimize_instances(model, dev, inst, hp, sc0, tc0, seeds, n_rays=a.rays, picks=picks, jitter=jitter)
        torch.cuda.synchronize()
    return {"views": len(views), "instances": n_inst, "iterations": T, "runs": 2}


def main():
    a = C.arguments(C.BLOCKS, ("--instances", dict(type=int, default=8)), ("--views", dict(type=int, default=4)),
                    ("--rays", dict(type=int, default=1024)), ("--samples", dict(type=int, default=64)),
                    ("--target", dict(type=int, nargs=2, default=None)))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    model = C.fog_decoder(sb, tb, dev)
    if a.target is not None:
        C.report("multiview_time", a, (sb, tb), target=target(model, a, dev), precision=str(model.precision))
        return
    inst, views, seeds, hp, sc0, tc0, picks, jitter = setup(a.instances, a.views, a.rays, a.samples, 6, dev)
    V = len(views)

    def together(T):
        def fn():
            hp["optimize"]["num_opts"] = T
            driver.optimize_instances(model, dev, inst, hp, sc0, tc0, seeds, n_rays=a.rays, picks=picks[:T], jitter=jitter[:T])
        return fn

    def apart(T):
        def fn():
            hp["optimize"]["num_opts"] = T
            for v, view in enumerate(views):
                i = v // a.views
                driver.optimize_object(model, dev, view, hp, sc0[i:i + 1], tc0[i:i + 1], reg_iters=-1, seed=seeds[v], jitter=jitter[:T, :, v])
        return fn
    t2, t6, s2, s6 = in_turn([together(2), together(6), apart(2), apart(6)], a.reps)
    one, sep = (t6 - t2) / 4, (s6 - s2) / 4
    C.report("multiview_time", a, (sb, tb), reps=a.reps, precision=str(model.last_precision), instances=a.instances, views=V, rays_per_view=a.rays,
             S=a.samples, roi_pixels=[int(v["img"].shape[0] * v["img"].shape[1]) for v in views],
             optimize_instances={"iteration_ms": round(one, 4), "run_2_ms": t2, "run_6_ms": t6},
             separate_optimize_object={"iteration_ms_all_views": round(sep, 4), "run_2_ms": s2, "run_6_ms": s6, "loops": V},
             separate_over_together=round(sep / one, 3))


if __name__ == "__main__":
    main()
