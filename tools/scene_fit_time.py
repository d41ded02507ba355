"""Timing of the joint scene fit on one GPU: device events, medians of ``--reps`` calls, calls that are compared taken in turn.

  * one forward + backward of ``scene.render_scene`` on its default route (torch rows and samples) beside ``fused=True`` (the
    snr_scene_samples / snr_scene_gather kernels), on the three objects of the ``scene`` fixture (every covered pixel, the fixture's sample
    count) and on a synthetic frame of ``--objects`` objects with about 4 k covered pixels each at ``--samples`` samples;
  * the two new launches on their own at the frame's size against their least traffic: 28 bytes per sample out of the forward (points,
    directions, depth), 32 bytes per sample into the backward (their three gradients and the jitter);
  * one iteration of ``driver.optimize_scene`` on the frame: the difference of a 6- and a 2-iteration run over 4;
  * the share of (pixel, object) pairs that hit, which sizes what decoding only the hit pairs saves;
  * the compact route (``compact=True``: the decoder on the pairs that hit) in turn with the rows above, in the same calls: forward + backward
    on the fixture and on the frame (its default capacity, with the read of the counts that sets it) and one ``optimize_scene`` iteration;
    the frame's per-object hit counts and the capacity they give.

Prints one JSON line.

usage: python tools/scene_fit_time.py [--reps N] [--objects Nb] [--samples S] [--size H W] [--commit SHA]"""
import torch

import geometry_common as C
from conftest import load_golden
from ray_surface_time import in_turn
from supnerf_amd import driver, ops, scene, synthetic, utils


def render_pair(model, dev, poses, wlh, sc0, tc0, K, pixels, H, W, S, reps):
    """forward + backward of render_scene, default route, fused and compact, in turn; the largest distance between their outputs."""
    Nb = poses.shape[0]
    jitter = torch.rand(pixels.shape[0] * Nb, S, generator=torch.Generator().manual_seed(2)).to(dev)
    sc, tc = sc0.to(dev).requires_grad_(), tc0.to(dev).requires_grad_()
    p = poses.to(dev).requires_grad_()

    def run(fused, compact=False):
        def fn():
            rgb = scene.render_scene(model, dev, p, wlh, sc, tc, K, pixels, H, W, S, jitter=jitter, fused=fused, compact=compact)[0]
            torch.autograd.grad(((rgb - 0.5) ** 2).mean(), (p, sc, tc))
        return fn
    t_default, t_fused, t_compact = in_turn([run(False), run(True), run(True, True)], reps)
    info = {}
    with torch.no_grad():
        a = scene.render_scene(model, dev, p, wlh, sc, tc, K, pixels, H, W, S, jitter=jitter)
        b = scene.render_scene(model, dev, p, wlh, sc, tc, K, pixels, H, W, S, jitter=jitter, fused=True)
        c = scene.render_scene(model, dev, p, wlh, sc, tc, K, pixels, H, W, S, jitter=jitter, fused=True, compact=True, info=info)
    return {"pixels": int(pixels.shape[0]), "objects": int(Nb), "S": S, "default_ms": t_default, "fused_ms": t_fused, "compact_ms": t_compact,
            "default_over_fused": round(t_default / t_fused, 3), "fused_over_compact": round(t_fused / t_compact, 3),
            "max_output_distance": max(float((x - y).abs().max()) for x, y in zip(a, b)),
            "max_compact_distance": max(float((x - y).abs().max()) for x, y in zip(c, b)),
            "hits_per_object": info["count"].tolist(), "capacity": info["capacity"],
            "decoder_points": {"fused": int(pixels.shape[0]) * int(Nb) * S, "compact": info["capacity"] * int(Nb) * S}}


def fixture_row(model, reps, dev):
    g = load_golden("scene")
    H, W, S = int(g["H"]), int(g["W"]), int(g["n_samples"])
    idx = torch.nonzero(scene.scene_rays(g["obj_poses"], g["obj_wlh"], g["K"], H, W)[1]).flatten()
    pixels = torch.stack([idx % W, idx // W], 1)
    return render_pair(model, dev, g["obj_poses"], g["obj_wlh"], g["shapecodes"], g["texturecodes"], g["K"], pixels, H, W, S, reps)


def frame_rows(model, a, dev):
    H, W = a.size
    Nb, S = a.objects, a.samples
    sc0, tc0 = C.codes(Nb, 1, dev), C.codes(Nb, 2, dev)
    frame = synthetic.synthetic_frame(list(range(Nb)), H, W, focal=0.35 * W, model=model, device=dev, shapecodes=sc0, texturecodes=tc0, n_samples=S)
    K, poses, wlh = frame["K"], frame["obj_poses"], frame["obj_wlh"]
    rois = scene.scene_rois(poses, wlh, K, H, W)
    pixels = scene.roi_pixels(rois, H, W)
    Nr = pixels.shape[0]
    render = render_pair(model, dev, poses, wlh, sc0, tc0, K, pixels, H, W, S, a.reps)
    render["roi_pixels_per_object"] = [int((r[2] - r[0]) * (r[3] - r[1])) for r in rois.tolist()]

    # the two launches alone
    cam2obj = utils.invert_pose(poses).to(dev).requires_grad_()
    args = (wlh.to(dev), rois.to(dev), pixels.to(dev, torch.int32), scene.K_vector(K), torch.rand(Nr * Nb, S, device=dev), S, 1.0, True, True)
    xyz, viewdir, z, hit, _ = ops.SceneSamples.apply(cam2obj, *args)
    g = [torch.randn_like(t) for t in (xyz, viewdir, z)]

    def fwd():
        with torch.no_grad():
            ops.SceneSamples.apply(cam2obj, *args)
    t_f, t_b = in_turn([fwd, lambda: torch.autograd.grad((xyz, viewdir, z), cam2obj, g, retain_graph=True)], a.reps)
    n = Nr * Nb * S
    launches = {"samples": n, "fwd_ms": t_f, "bwd_ms": t_b, "fwd_GBps": round(n * 28 / t_f / 1e6, 1), "bwd_GBps": round(n * 32 / t_b / 1e6, 1)}
    hit_share = {"of_all_pairs": round(float(hit.float().mean()), 4), "pixels_hit_by_some_object": round(float(hit.any(1).float().mean()), 4)}

    # one iteration of the joint fit
    hp = driver.load_hpams()
    hp["n_samples"] = S

    jit = torch.rand(6, Nr * Nb, S, device=dev)       # (the default draw is a CPU generator's: host time that grows with the iterations)

    fit_info = {}

    def fit(T, compact=False):
        def fn():
            hp["optimize"]["num_opts"] = T
            driver.optimize_scene(model, dev, frame, hp, sc0, tc0, jitter=jit[:T], pixels=pixels, compact=compact, info=fit_info if compact else None)
        return fn
    t2, t6, c2, c6 = in_turn([fit(2), fit(6), fit(2, True), fit(6, True)], max(1, a.reps // 2))
    return render, launches, hit_share, {"pixels": Nr, "objects": Nb, "S": S, "iteration_ms": round((t6 - t2) / 4, 4), "run_2_ms": t2, "run_6_ms": t6,
                                         "compact_iteration_ms": round((c6 - c2) / 4, 4), "compact_run_2_ms": c2, "compact_run_6_ms": c6,
                                         "compact_capacity": fit_info["capacity"], "compact_dropped_pairs": int(fit_info["dropped_pairs"])}


def main():
    a = C.arguments(C.BLOCKS, ("--objects", dict(type=int, default=8)), ("--samples", dict(type=int, default=64)),
                    ("--size", dict(type=int, nargs=2, default=(160, 640))))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    model = C.fog_decoder(sb, tb, dev)
    fixture = fixture_row(model, a.reps, dev)
    render, launches, hit_share, fit = frame_rows(model, a, dev)
    C.report("scene_fit_time", a, (sb, tb), reps=a.reps, precision=str(model.precision), render_scene_fixture=fixture, render_scene_frame=render,
             sample_launches=launches, hit_share=hit_share, optimize_scene=fit)


if __name__ == "__main__":
    main()
