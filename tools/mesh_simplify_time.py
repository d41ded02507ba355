"""Timing of ``geometry.simplify_mesh`` on one GPU (device events, medians of ``--reps`` calls, the host read inside the call included) on
the planted-box decoder's mesh at R = 128 and R = 256, with cells of 2, 4 and 8 grid steps and both placements: the face counts before and
after, the time of the whole call, the three sorts it makes (vertices by key, corners by cluster, and -- in a packed launch only -- by
object) timed on their own, and ``rasterize`` on the mesh before and after.  Each row stands beside the ``extract_mesh`` that made the mesh
and the ``density_grid`` launch that made its grid, from the same run.  Prints one JSON line.

usage: python tools/mesh_simplify_time.py [--reps N] [--res R ...] [--steps S ...] [--blocks SB TB] [--size PIXELS] [--commit SHA]"""
import torch

import geometry_common as C
from supnerf_amd import geometry as G, ops


def sorts(v, f, cell, origin, reps):
    """Median milliseconds of the two sorts of a one-object call, on the keys and corner clusters that call sorts."""
    s = ops.mesh_simplify(v, f, [v.shape[0]], [f.shape[0]], cell, origin)
    key = torch.floor((v - origin.to(v.device)) / cell).long()
    key = ((key[:, 0] + (1 << 20)) << 42) | ((key[:, 1] + (1 << 20)) << 21) | (key[:, 2] + (1 << 20))
    corner_cluster = s.vert_map.long()[f.long().view(-1)]
    return {"vertex_sort_ms": round(C.median_ms(lambda: torch.sort(key, stable=True), reps), 3),
            "corner_sort_ms": round(C.median_ms(lambda: torch.sort(corner_cluster, stable=True), reps), 3)}


def main():
    a = C.arguments(C.BLOCKS, ("--res", dict(type=int, nargs="+", default=[128, 256])), ("--steps", dict(type=int, nargs="+", default=[2, 4, 8])),
                    ("--size", dict(type=int, default=512)))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    box = C.box_decoder(sb, tb, dev)
    sc = C.codes(1, 1, dev)
    lo, hi = C.BOUND_BOX
    cam = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.8]], device=dev)
    K = (0.8 * a.size, 0.8 * a.size, a.size / 2.0, a.size / 2.0)
    draw = lambda mesh: G.rasterize(mesh, cam, K, (a.size, a.size), cull="back")                       # noqa: E731
    origin = torch.full((1, 3), lo)
    rows = []
    for R in a.res:
        grid = G.density_grid(box, sc, R, C.BOUND_BOX)
        extract = lambda: G.extract_mesh(grid, level=C.LEVEL_BOX, bound=C.BOUND_BOX)                   # noqa: E731
        mesh = extract()[0]
        v, f = mesh
        draw(mesh)                                                                                     # warm-up
        head = {"R": R, "verts": int(v.shape[0]), "faces": int(f.shape[0]),
                "density_grid_ms": round(C.median_ms(lambda: G.density_grid(box, sc, R, C.BOUND_BOX), max(1, a.reps // 2)), 3),
                "extract_mesh_ms": round(C.median_ms(extract, a.reps), 3), "rasterize_before_ms": round(C.median_ms(lambda: draw(mesh), a.reps), 3)}
        for steps in a.steps:
            cell = steps * (hi - lo) / (R - 1)
            row = dict(head, grid_steps=steps, cell=round(cell, 6))
            for placement in ("quadric", "mean"):
                call = lambda: G.simplify_mesh(mesh, cell, origin=origin, placement=placement)         # noqa: E731
                s = call()                                                                             # warm-up
                row[f"simplify_{placement}_ms"] = round(C.median_ms(call, a.reps), 3)
            row.update(verts_after=int(s.verts.shape[0]), faces_after=int(s.faces.shape[0]), **sorts(v, f, cell, origin, a.reps))
            small = (s.verts, s.faces)
            draw(small)
            row["rasterize_after_ms"] = round(C.median_ms(lambda: draw(small), a.reps), 3)
            rows.append(row)
        del mesh, v, f, grid
        torch.cuda.empty_cache()
    C.report("mesh_simplify_time", a, (sb, tb), size=a.size, meshes=rows)


if __name__ == "__main__":
    main()
