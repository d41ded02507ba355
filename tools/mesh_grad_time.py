"""Timing of differentiable mesh extraction on one GPU (device events): ``extract_mesh(model, codes, differentiable=True)`` on the planted
box (with ``wobble``), at R = 128, 256, 512 and B = 1, 8, on the dense and the narrow-band grid:

  * forward: the grid, the iso-surface passes and the latent terms with their autograd graph (as extract_mesh runs them);
  * backward: ``sum(w . verts).backward()`` to the shape codes, and its parts -- snr_iso_grad, the compaction (flag scan, host read of the
    list size, snr_iso_surface_points) and the density pair (snr_density_fwd_masks + snr_density_bwd) on the surface points.

Reported with the grid size, the vertices and the surface points the backward's decoder ran on.  The median of ``--reps`` is reported.
The dense route at R = 512 takes at most 7 objects per grid launch (fewer than 2^30 points), so its B = 8 row is skipped.
Prints one JSON line.

usage: python tools/mesh_grad_time.py [--reps N] [--res R ...] [--batch B ...] [--commit SHA]"""
import json
import sys

import numpy as np
import torch

import geometry_common as C
from geometry_common import BOUND_BOX as BOUND, LEVEL_BOX as LEVEL, timed
from supnerf_amd import geometry as G, ops


def row(model, sc0, R, narrow, reps):
    B = sc0.shape[0]
    lat = G.lattice(R, BOUND)
    state = {}

    def forward():
        sc = sc0.clone().requires_grad_()
        meshes = G.extract_mesh(model, sc, level=LEVEL, resolution=R, bound=BOUND, narrow_band=narrow, differentiable=True)
        state["sc"], state["meshes"] = sc, meshes

    def backward():
        sum((v * w).sum() for (v, _), w in zip(state["meshes"], state["w"])).backward()

    forward()
    g = torch.Generator().manual_seed(1)
    state["w"] = [torch.randn(v.shape, generator=g).to(v.device) for v, _ in state["meshes"]]
    backward()
    t_f, t_b = [], []
    for _ in range(reps):
        t_f.append(timed(forward))
        t_b.append(timed(backward))
    n_verts = sum(int(v.shape[0]) for v, _ in state["meshes"])
    del state["meshes"]

    # the backward's parts, on the grid the forward meshed
    grid = G.narrow_band_grid(model, sc0, R, level=LEVEL, bound=BOUND).grid if narrow else G.density_grid(model, sc0, R, BOUND)
    m = ops.iso_extract(grid, lat, LEVEL)
    d_verts = torch.cat(state["w"])
    latent, packed = C.latent(model, sc0), model.packed_weights()
    sb, tb = model.shape_blocks, model.texture_blocks
    part = {}

    def grad_pass():
        part["d_grid"], part["on"] = ops.iso_grad(grid, lat, LEVEL, m.edge_mask, m.edge_scan, m.vert_offset, d_verts, want_surface=True)

    def compact():
        part["pts"] = ops.iso_surface_points(part["on"], part["d_grid"], lat)

    def density_pair():
        xyz, d_sig = part["pts"][0], part["pts"][1]
        sig, masks = ops.density_fwd(xyz, latent, packed, sb, tb, save_masks=True)
        ops.density_bwd(xyz, latent, packed, masks, sig, d_sig, sb, tb, need_latent=True, need_xyz=False)

    grad_pass(), compact(), density_pair()
    t_g, t_c, t_d = [], [], []
    for _ in range(reps):
        t_g.append(timed(grad_pass))
        t_c.append(timed(compact))
        t_d.append(timed(density_pair))
    counts = part["pts"][3]
    n_pts, n_pad = int(counts.sum()), B * part["pts"][2]
    med = lambda t: round(float(np.median(t)), 3)                                    # noqa: E731
    out = {"R": R, "B": B, "grid": "narrow" if narrow else "dense", "grid_points": B * R ** 3, "verts": n_verts,
           "surface_points": n_pts, "padded_points": n_pad, "forward_ms": med(t_f), "backward_ms": med(t_b), "iso_grad_ms": med(t_g),
           "compact_ms": med(t_c), "density_pair_ms": med(t_d), "density_Gpts_s": round(n_pad / float(np.median(t_d)) / 1e6, 4)}
    del grid, m, part
    torch.cuda.empty_cache()
    return out


def main():
    a = C.arguments(C.RES, C.BATCH)
    dev = torch.device("cuda:0")
    sb, tb = 3, 1
    model = C.box_decoder(sb, tb, dev)
    rows = []
    for R in a.res:
        for B in a.batch:
            sc = C.codes(B, B, dev)
            for narrow in (False, True):
                if not narrow and B * R ** 3 >= 2 ** 30:
                    continue
                r = row(model, sc, R, narrow, a.reps)
                rows.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    C.report("mesh_grad_time", a, (sb, tb), level=LEVEL, bound=list(BOUND), rows=rows)


if __name__ == "__main__":
    main()
