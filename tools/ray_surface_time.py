"""Timing of ray-cast surfaces on one GPU (device events): ``geometry.ray_surface`` on the planted box (with ``wobble``), B = 1, 8 objects
x N = 4096 rays, 64 samples in the first march:

  * the first march (point list, density forward, crossing search) against ``geometry.query_density`` on the same point list, and the
    three ray passes on their own (``snr_ray_march_points``, ``snr_ray_first_crossing``, ``snr_ray_hit_points``);
  * the four refinement settings that shrink the bracket 256 times -- (8, 3), (4, 5), (2, 17), (1, 257) -- and no refinement: the whole
    ``ray_surface`` call each, called in turn;
  * forward + backward to the shape codes against the forward alone (the default refinement);
  * for context (B = 1): ``surface_depth`` on a 64 x 64 grid against the fused render of the same rays (``utils.render_rays_v2``, whose depth
    is the volumetric expectation: time only, the two depths mean different things) and against ``extract_mesh(narrow_band=True,
    resolution=256)`` of the same code.

The median of ``--reps`` alternated timings is reported.  Prints one JSON line.

usage: python tools/ray_surface_time.py [--reps N] [--batch B ...] [--rays N] [--commit SHA]"""
import json
import sys

import numpy as np
import torch

import geometry_common as C
from geometry_common import BOUND_BOX, LEVEL_BOX as LEVEL, timed
from planted_decoder import box_rays
from supnerf_amd import driver, geometry as G, ops, utils as U

NEAR, FAR, S = 0.75, 2.25, 64
SETTINGS = [(0, 2), (8, 3), (4, 5), (2, 17), (1, 257)]


def in_turn(fns, reps):
    """Median milliseconds of each callable, called in turn ``reps`` times (after one warm-up round)."""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(timed(f))
    return [round(float(np.median(t)), 4) for t in ts]


def row(model, B, N, reps, dev):
    sc0 = C.codes(B, B, dev)
    o, d, _ = box_rays(B * N, S, seed=3)
    o, d = o.to(dev), d.to(dev)
    near, far = torch.full((B * N,), NEAR, device=dev), torch.full((B * N,), FAR, device=dev)
    latent, packed = C.latent(model, sc0), model.packed_weights()
    sb, tb = model.shape_blocks, model.texture_blocks
    pts = ops.ray_march_points(o, d, near, far, S)
    sig = G.query_density(model, pts, sc0).view(-1, S)
    br = ops.ray_brackets(o, d, near, far, latent, packed, LEVEL, S, 0, 2, sb, tb)
    t_query, t_first = in_turn([lambda: G.query_density(model, pts, sc0),
                                lambda: ops.ray_brackets(o, d, near, far, latent, packed, LEVEL, S, 0, 2, sb, tb)], reps)
    t_points, t_cross, t_hit = in_turn([lambda: ops.ray_march_points(o, d, near, far, S),
                                        lambda: ops.ray_first_crossing(sig, near.clone(), far.clone(), LEVEL),
                                        lambda: ops.ray_hit_points(o, d, *br, LEVEL)], reps)
    t_clone, = in_turn([lambda: (near.clone(), far.clone())], reps)
    ob, db = o.view(B, N, 3), d.view(B, N, 3)
    with torch.no_grad():
        t_set = in_turn([lambda r=r: G.ray_surface(model, ob, db, NEAR, FAR, sc0, level=LEVEL, n_samples=S, refine=r) for r in SETTINGS], reps)
        hits = G.ray_surface(model, ob, db, NEAR, FAR, sc0, level=LEVEL, n_samples=S)
    w = torch.randn(B, N, generator=torch.Generator().manual_seed(1)).to(dev)

    def fwd_bwd():
        sc = sc0.clone().requires_grad_()
        (G.ray_surface(model, ob, db, NEAR, FAR, sc, level=LEVEL, n_samples=S).depth * w).sum().backward()

    def fwd():
        with torch.no_grad():
            G.ray_surface(model, ob, db, NEAR, FAR, sc0, level=LEVEL, n_samples=S)
    t_fb, t_f = in_turn([fwd_bwd, fwd], reps)
    return {"B": B, "N": N, "n_samples": S, "points_first_march": B * N * S, "hit_rays": int((hits.state == 1).sum()),
            "query_density_ms": t_query, "first_march_ms": t_first, "march_points_ms": t_points, "first_crossing_ms": t_cross,
            "first_crossing_clones_ms": t_clone, "hit_points_ms": t_hit,
            "ray_surface_ms": {f"{lv}x{sr}": t for (lv, sr), t in zip(SETTINGS, t_set)},
            "forward_ms": t_f, "forward_backward_ms": t_fb}


def context(model, reps, dev):
    ob = driver.make_objects([11], 64)[0]
    sc, tc = C.codes(1, 1, dev), C.codes(1, 2, dev)
    pose, diag = ob["cam_pose"].float().to(dev), float(ob["obj_diag"])
    with torch.no_grad():
        t_sd, t_render, t_mesh = in_turn([
            lambda: G.surface_depth(model, pose, diag, ob["K"], ob["roi"], sc, level=LEVEL, im_sz=64),
            lambda: U.render_rays_v2(model, dev, ob["img"], ob["mask"], pose, diag, ob["K"], ob["roi"], S, sc, tc, False, False, im_sz=64),
            lambda: G.extract_mesh(model, sc, level=LEVEL, resolution=256, bound=BOUND_BOX, narrow_band=True)], reps)
        hits = G.surface_depth(model, pose, diag, ob["K"], ob["roi"], sc, level=LEVEL, im_sz=64)
    return {"grid": 64, "hit_pixels": int((hits.state == 1).sum()), "surface_depth_ms": t_sd, "render_rays_v2_ms": t_render,
            "extract_mesh_narrow_256_ms": t_mesh}


def main():
    a = C.arguments(C.BATCH, ("--rays", dict(type=int, default=4096)))
    dev = torch.device("cuda:0")
    sb, tb = 3, 1
    model = C.box_decoder(sb, tb, dev)
    rows = []
    for B in a.batch:
        r = row(model, B, a.rays, a.reps, dev)
        rows.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    ctx = context(model, a.reps, dev)
    C.report("ray_surface_time", a, (sb, tb), level=LEVEL, near=NEAR, far=FAR, default_refine=list(G.DEFAULT_REFINE), rows=rows, context=ctx)


if __name__ == "__main__":
    main()
