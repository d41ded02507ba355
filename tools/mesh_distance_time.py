"""Timing of ``geometry.mesh_index`` / ``closest_point`` / ``sample_surface`` / ``mesh_distance`` on one GPU (device events, medians of
``--reps`` calls after a warm-up, the host read of the index build included) on the planted-box decoder's mesh at R = 128 and R = 256:

  * the index build at every candidate cell factor (cell = factor x the square root of the mean face area, no less than 1/256 of the
    extent) and the sort inside it on its own;
  * ``closest_point`` for ``--queries`` surface samples of the simplified mesh (cells of 2 grid steps, quadric) against the original, at
    every candidate factor and at one cell per object -- the brute force of the same kernel -- the variants called in turn; every grid
    must give the bits of the one-cell run, or the tool stops;
  * ``sample_surface`` and ``mesh_distance`` (both directions, ``--queries`` samples a side, indices built once);
  * the distance ``simplify_mesh`` introduces at cells of 2 and 4 grid steps for both placements: mean, RMS and maximum from the original
    to the simplified mesh and back.

Each row stands beside the ``extract_mesh`` and the ``simplify_mesh`` that made the meshes, from the same run.  Prints one JSON line.

usage: python tools/mesh_distance_time.py [--reps N] [--res R ...] [--factors F ...] [--queries Q] [--brute-queries Q] [--blocks SB TB]
       [--commit SHA]"""
import torch

import geometry_common as C
from supnerf_amd import geometry as G, ops


def cell_for(mesh, factor):
    """The default rule of ``mesh_index`` with another factor: factor x sqrt(mean face area), no less than extent / 256."""
    return float(ops.mesh_default_cell(ops.pack_mesh(mesh[0], mesh[1], [mesh[0].shape[0]], [mesh[1].shape[0]]), factor)[0])


def main():
    a = C.arguments(C.BLOCKS, ("--res", dict(type=int, nargs="+", default=[128, 256])),
                    ("--factors", dict(type=float, nargs="+", default=[1.0, 2.0, 4.0, 8.0])), ("--queries", dict(type=int, default=100000)),
                    ("--brute-queries", dict(type=int, default=2000)))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    box = C.box_decoder(sb, tb, dev)
    sc = C.codes(1, 1, dev)
    lo, hi = C.BOUND_BOX
    origin = torch.full((1, 3), lo)
    gen = lambda seed: torch.Generator(device=dev).manual_seed(seed)                                   # noqa: E731
    rows = []
    for R in a.res:
        grid = G.density_grid(box, sc, R, C.BOUND_BOX)
        extract = lambda: G.extract_mesh(grid, level=C.LEVEL_BOX, bound=C.BOUND_BOX)                   # noqa: E731
        mesh = extract()[0]
        step = (hi - lo) / (R - 1)
        simplify = lambda steps=2, placement="quadric": G.simplify_mesh(mesh, steps * step, origin=origin, placement=placement)  # noqa: E731
        s = simplify()
        small = (s.verts, s.faces)
        row = {"R": R, "verts": int(mesh[0].shape[0]), "faces": int(mesh[1].shape[0]), "faces_simplified": int(s.faces.shape[0]),
               "extract_mesh_ms": round(C.median_ms(extract, a.reps), 3), "simplify_mesh_ms": round(C.median_ms(simplify, a.reps), 3)}
        G.sample_surface(small, a.queries, generator=gen(1))                                           # warm-up
        row["sample_surface_ms"] = round(C.median_ms(lambda: G.sample_surface(small, a.queries, generator=gen(1)), a.reps), 3)
        queries = G.sample_surface(small, a.queries, generator=gen(1)).points
        # the brute force of the same kernel: one cell per object (a cell larger than the object), on a slice of the queries
        one = G.mesh_index(mesh, 4.0 * (hi - lo))
        assert one.grid.n_cells == 1
        sub = queries[:a.brute_queries]
        f1, w1, d1 = ops.mesh_nearest_query(one.mesh, one.grid, sub, [sub.shape[0]])
        row["brute_force_ms_per_1000_queries"] = round(C.median_ms(lambda: ops.mesh_nearest_query(one.mesh, one.grid, sub, [sub.shape[0]]),
                                                                   max(1, a.reps // 2)) * 1000.0 / sub.shape[0], 3)
        sweep = []
        for factor in a.factors:
            cell = cell_for(mesh, factor)
            build = lambda: G.mesh_index(mesh, cell)                                                   # noqa: E731
            index = build()
            key = torch.randint(0, index.grid.n_cells, (index.grid.n_pairs,), device=dev)
            query = lambda index=index: G.closest_point(mesh, queries, index=index)                    # noqa: E731
            query()                                                                                    # warm-up
            f, w, d = ops.mesh_nearest_query(index.mesh, index.grid, sub, [sub.shape[0]])
            if not (torch.equal(f, f1) and torch.equal(w, w1) and torch.equal(d.view(torch.int64), d1.view(torch.int64))):
                raise SystemExit(f"R = {R}, factor {factor}: the grid changed the answer")
            sweep.append({"factor": factor, "cell": round(cell, 6), "cells": index.grid.n_cells, "pairs": index.grid.n_pairs,
                          "index_ms": round(C.median_ms(build, a.reps), 3), "index_sort_ms": round(C.median_ms(lambda: torch.sort(key, stable=True), a.reps), 3),
                          "closest_point_ms": None, "same_bits_as_one_cell": True, "_query": query})
        for _ in range(a.reps):                                                                        # the variants in turn
            for v in sweep:
                v.setdefault("_t", []).append(C.timed(v["_query"]))
        for v in sweep:
            v["closest_point_ms"] = round(float(torch.tensor(v.pop("_t")).median()), 3)
            del v["_query"]
        row["sweep"] = sweep
        row["default_factor"] = ops.NEAREST_CELL_FACTOR
        ia, ib = G.mesh_index(mesh), G.mesh_index(small)
        dist = lambda: G.mesh_distance(mesh, small, n=a.queries, generator=gen(2), index_a=ia, index_b=ib)   # noqa: E731
        dist()
        row["mesh_distance_ms"] = round(C.median_ms(dist, a.reps), 3)
        errors = []
        for steps in (2, 4):
            for placement in ("quadric", "mean"):
                t = simplify(steps, placement)
                m = G.mesh_distance(mesh, (t.verts, t.faces), n=a.queries, generator=gen(3), index_a=ia)
                errors.append({"grid_steps": steps, "placement": placement, "faces": int(t.faces.shape[0]), "cell": round(steps * step, 6),
                               **{k: float(f"{float(getattr(m, k)):.4g}") for k in ("forward_mean", "forward_rms", "forward_max", "backward_mean",
                                                                                     "backward_rms", "backward_max", "chamfer", "hausdorff")}})
        row["simplify_error"] = errors
        rows.append(row)
        del mesh, grid, queries, one, ia, ib
        torch.cuda.empty_cache()
    C.report("mesh_distance_time", a, (sb, tb), queries=a.queries, brute_queries=a.brute_queries, meshes=rows)


if __name__ == "__main__":
    main()
