"""Timing of the mesh-containment kernels on one GPU (device events, medians of ``--reps`` calls after a warm-up, variants called in turn)
on the planted-box decoder's mesh extracted at ``--mesh-res``:

  * the index build (``geometry.mesh_index``, its host read included) -- the one index both searches walk;
  * ``snr_inside_query`` on ``--queries`` uniform random points of the bound beside ``snr_nearest_query`` on the same points and index;
  * ``snr_inside_lattice`` at every ``--res`` beside ``snr_inside_query`` on the same lattice's points (the points already on the
    device), both beside ``density_grid`` at the same resolution; the two windings must be the same integers, or the tool stops;
  * ``voxelize`` and ``mesh_iou`` through the public API, and the IoU of the voxelised mesh against ``density_grid > level``.

Prints one JSON line.

usage: python tools/mesh_inside_time.py [--reps N] [--res R ...] [--mesh-res R] [--queries Q] [--blocks SB TB] [--commit SHA]"""
import torch

import geometry_common as C
from supnerf_amd import geometry as G, ops


def main():
    a = C.arguments(C.BLOCKS, ("--res", dict(type=int, nargs="+", default=[64, 128, 256])), ("--mesh-res", dict(type=int, default=128)),
                    ("--queries", dict(type=int, default=1000000)))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    box = C.box_decoder(sb, tb, dev)
    sc = C.codes(1, 1, dev)
    lo, hi = C.BOUND_BOX
    mesh = G.extract_mesh(G.density_grid(box, sc, a.mesh_res, C.BOUND_BOX), level=C.LEVEL_BOX, bound=C.BOUND_BOX)[0]
    build = lambda: G.mesh_index(mesh)                                                                 # noqa: E731
    index = build()
    out = {"mesh_res": a.mesh_res, "verts": int(mesh[0].shape[0]), "faces": int(mesh[1].shape[0]), "closed": bool(G.mesh_adjacency(mesh).closed),
           "cell": round(float(index.grid.cell[0]), 6), "cells": index.grid.n_cells, "pairs": index.grid.n_pairs,
           "cells_per_axis": [int(x) for x in torch.ceil((index.grid.grid_hi[0] - index.grid.grid_lo[0]) / index.grid.cell[0]).clamp(1, 256).tolist()],
           "index_ms": round(C.median_ms(build, a.reps), 3)}
    pts = torch.rand(a.queries, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * (hi - lo) + lo
    inside = lambda p=pts: ops.mesh_inside_query(index.mesh, index.grid, p, [p.shape[0]])              # noqa: E731
    nearest = lambda: ops.mesh_nearest_query(index.mesh, index.grid, pts, [a.queries])                 # noqa: E731
    inside(), nearest()                                                                                # warm-up
    t_in, t_near = C.alternate(inside, nearest, a.reps)
    out.update(queries=a.queries, inside_query_ms=round(t_in, 3), nearest_query_ms=round(t_near, 3),
               inside_share=round(float((inside() != 0).double().mean()), 4))
    rows = []
    for R in a.res:
        lat = G.lattice(R, C.BOUND_BOX)
        lat_lo = torch.tensor([[lat.lo[k] for k in range(3)]], device=dev)
        lat_h = torch.tensor([[lat.h[k] for k in range(3)]], device=dev)
        lp = G.lattice_points(lat, dev)
        lattice = lambda: ops.mesh_inside_lattice(index.mesh, index.grid, lat_lo, lat_h, (R, R, R))   # noqa: E731
        by_point = lambda: inside(lp)                                                                  # noqa: E731
        density = lambda: G.density_grid(box, sc, R, C.BOUND_BOX)                                      # noqa: E731
        w = lattice()
        if not torch.equal(w.view(-1), by_point()):
            raise SystemExit(f"R = {R}: the lattice kernel and the point kernel disagree")
        grid = density()
        t_lat, t_pt = C.alternate(lattice, by_point, a.reps)
        vox = lambda: G.voxelize(mesh, R, C.BOUND_BOX, index=index)                                    # noqa: E731
        vox()
        iou = G.occupancy_iou(w[0] != 0, grid[0] > C.LEVEL_BOX)
        rows.append({"R": R, "inside_lattice_ms": round(t_lat, 3), "inside_query_on_lattice_ms": round(t_pt, 3),
                     "density_grid_ms": round(C.median_ms(density, a.reps), 3), "voxelize_ms": round(C.median_ms(vox, a.reps), 3),
                     "voxels_inside": int(iou.count_a), "iou_against_density_grid": round(float(iou.iou), 6),
                     "voxels_that_differ": int(iou.union - iou.intersection)})
        del lp, w, grid
        torch.cuda.empty_cache()
    self_iou = lambda: G.mesh_iou(mesh, mesh, resolution=64, index_a=index, index_b=index)             # noqa: E731
    self_iou()
    out["mesh_iou_64_ms"] = round(C.median_ms(self_iou, a.reps), 3)
    C.report("mesh_inside_time", a, (sb, tb), **out, lattices=rows)


if __name__ == "__main__":
    main()
