"""Timing of mesh smoothing on one GPU (device events, medians of ``--reps`` >= 7 calls, the compared calls taken in turn, host reads
inside a call included) on the planted-box decoder's mesh at R = 128 and R = 256 and on what ``simplify_mesh`` makes of each with cells of
2 grid steps: the adjacency build and its sort alone, one half-step (``snr_smooth_step`` between two buffers, positions) with its least
traffic -- 4 B per directed edge, 8 B per vertex of ``nbr_start``, 24 B per vertex read and written at C = 3 -- and the rate that makes,
``smooth_mesh(iterations=10)`` with and without a ready adjacency, and ``laplacian_energy`` forward + backward; beside the
``extract_mesh`` and ``simplify_mesh`` calls of the same run.  Prints one JSON line.

usage: python tools/mesh_smooth_time.py [--reps N] [--res R ...] [--blocks SB TB] [--commit SHA]"""
import numpy as np
import torch

import geometry_common as C
from supnerf_amd import _lib, geometry as G, ops


def in_turn(calls, reps):
    """Median milliseconds of each of ``calls`` (name -> function), all called in turn ``reps`` times."""
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            times[name].append(C.timed(fn))
    return {name: round(float(np.median(t)), 4) for name, t in times.items()}


def measure(mesh, reps):
    v, f = mesh
    dev = v.device
    nV, nF = v.shape[0], f.shape[0]
    adjacency = G.mesh_adjacency(mesh)
    packed = G._pack_adjacency([adjacency], [nV], dev)
    nE = packed.nbr.shape[0]
    voff, foff = ops._offsets([nV], dev)[1], ops._offsets([nF], dev)[1]
    lib, st = _lib.lib(), ops._stream(dev)
    i32, i64 = torch.int32, torch.int64
    key, bad = torch.empty(6 * nF, dtype=i64, device=dev), torch.zeros(1, dtype=i32, device=dev)
    _lib.check(lib.snr_smooth_edge_keys(ops._ptr(f, i32), ops._ptr(voff, i64), ops._ptr(foff, i64), 1, nV, nF, ops._ptr(key, i64),
                                        ops._ptr(bad, i32), st), "snr_smooth_edge_keys")
    a, b = v.detach().clone(), torch.empty_like(v)
    csr = ops._smooth_csr(packed)

    def half_step():
        _lib.check(lib.snr_smooth_step(ops._ptr(a), 3, *csr, None, 0.5, ops._ptr(b), st), "snr_smooth_step")

    def energy():
        x = v.detach().clone().requires_grad_()
        G.laplacian_energy((x, f), adjacency).sum().backward()

    calls = {"adjacency_ms": lambda: G.mesh_adjacency(mesh), "adjacency_sort_ms": lambda: torch.sort(key), "half_step_ms": half_step,
             "smooth_10_ms": lambda: G.smooth_mesh(mesh, 10, adjacency=adjacency), "smooth_10_with_adjacency_build_ms": lambda: G.smooth_mesh(mesh, 10),
             "energy_fwd_bwd_ms": energy}
    in_turn(calls, 2)                                                                                  # warm-up
    row = {"verts": nV, "faces": nF, "directed_edges": nE, "boundary_edges": adjacency.boundary_edges, "closed": adjacency.closed}
    row.update(in_turn(calls, reps))
    traffic = 4 * nE + 8 * nV + 24 * nV
    row.update(half_step_least_bytes=traffic, half_step_gb_per_s=round(traffic / (row["half_step_ms"] * 1e-3) / 1e9, 1))
    return row


def main():
    a = C.arguments(C.BLOCKS, ("--res", dict(type=int, nargs="+", default=[128, 256])))
    reps = max(7, a.reps)
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    box = C.box_decoder(sb, tb, dev)
    sc = C.codes(1, 1, dev)
    lo, hi = C.BOUND_BOX
    origin = torch.full((1, 3), lo)
    rows = []
    for R in a.res:
        grid = G.density_grid(box, sc, R, C.BOUND_BOX)
        cell = 2 * (hi - lo) / (R - 1)
        extract = lambda: G.extract_mesh(grid, level=C.LEVEL_BOX, bound=C.BOUND_BOX)                   # noqa: E731
        mesh = extract()[0]
        simplify = lambda: G.simplify_mesh(mesh, cell, origin=origin)                                  # noqa: E731
        s = simplify()
        same_run = in_turn({"extract_mesh_ms": extract, "simplify_mesh_ms": simplify}, reps)
        rows.append(dict({"R": R, "mesh": "extracted"}, **same_run, **measure(mesh, reps)))
        rows.append(dict({"R": R, "mesh": "simplified, cells of 2 grid steps"}, **same_run, **measure((s.verts, s.faces), reps)))
        del mesh, s, grid
        torch.cuda.empty_cache()
    C.report("mesh_smooth_time", a, (sb, tb), reps=reps, meshes=rows)


if __name__ == "__main__":
    main()
