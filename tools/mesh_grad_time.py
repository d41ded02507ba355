"""Timing of differentiable mesh extraction on one GPU (device events): ``extract_mesh(model, codes, differentiable=True)`` on the planted
box (with ``wobble``), at R = 128, 256, 512 and B = 1, 8, on the dense and the narrow-band grid:

  * forward: the grid, the iso-surface passes and the latent terms with their autograd graph (as extract_mesh runs them);
  * backward: ``sum(w . verts).backward()`` to the shape codes, and its parts -- snr_iso_grad, the compaction (flag scan, host read of the
    list size, snr_iso_surface_points) and the density pair (snr_density_fwd_masks + snr_density_bwd) on the surface points.

Reported with the grid size, the vertices and the surface points the backward's decoder ran on.  The median of ``--reps`` is reported.
The dense route at R = 512 takes at most 7 objects per grid launch (fewer than 2^30 points), so its B = 8 row is skipped.
Prints one JSON line.

usage: python tools/mesh_grad_time.py [--reps N] [--res R ...] [--batch B ...] [--commit SHA]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import supnerf_amd as A  # noqa: E402
from supnerf_amd import geometry as G, ops  # noqa: E402
from planted_decoder import WOBBLE, planted_params  # noqa: E402

LEVEL = float(np.log1p(np.exp(np.float32(0.0))))
BOUND = (-0.7, 0.7)


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, timeout=10).stdout.strip() or None
    except Exception:
        return None


def timed(fn):
    """Milliseconds of one call between two device events (host reads inside the call included)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


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
    latent, packed = G._latent(model, sc0), model.packed_weights()
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--commit", default=None, help="commit to report when the tree has no .git")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sb, tb = 3, 1
    model = A.CodeNeRF(shape_blocks=sb, texture_blocks=tb)
    model.load_state_dict(planted_params(sb, tb, seed=1, wobble=WOBBLE))
    model = model.to(dev)
    rows = []
    for R in a.res:
        for B in a.batch:
            sc = (torch.randn(B, 256, generator=torch.Generator().manual_seed(B)) * 0.5).to(dev)
            for narrow in (False, True):
                if not narrow and B * R ** 3 >= 2 ** 30:
                    continue
                r = row(model, sc, R, narrow, a.reps)
                rows.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "mesh_grad_time", "commit": a.commit or commit(), "device": torch.cuda.get_device_name(0), "blocks": [sb, tb],
                      "level": LEVEL, "bound": list(BOUND), "rows": rows}))


if __name__ == "__main__":
    main()
