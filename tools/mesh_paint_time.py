"""Timing of mesh painting on one GPU (device events, medians of ``--reps`` >= 7 calls, the compared calls taken in turn, host work
inside a call included) on the planted-box decoder's mesh at R = 128 and R = 256, painted from 1, 3 and 6 views of ``--crop`` pixels
that ``mesh_view`` rendered of the mesh's own ``vertex_colors``: ``paint_mesh`` without fill, its rasterise share (``ops.rasterize`` per
view), the paint launches alone (``snr_paint_view`` per view on ready screen positions and depth buffers, and ``snr_paint_finish``) with
the least traffic they must move -- per vertex and view 36 B of screen position, vertex and normal; per vertex the view sees 24 B of
state read and 24 B written (40 B where the view becomes the best) and four taps of 20 B (depth, mask, colour) -- and the rate that
makes, and ten fill rounds over a ready adjacency; beside the ``extract_mesh`` and ``vertex_colors`` calls of the same run.  Prints one
JSON line.

usage: python tools/mesh_paint_time.py [--reps N] [--res R ...] [--views N ...] [--crop H W] [--blocks SB TB] [--commit SHA]"""
import numpy as np
import torch

import geometry_common as C
from mesh_smooth_time import in_turn
from supnerf_amd import geometry as G, ops

K = np.array([[1266.0, 0, 800.0], [0, 1266.0, 450.0], [0, 0, 1]])
DIAG = 4.7
EYES = [(16.0, -9.0, 5.4), (-14.5, -11.0, 7.0), (2.7, 18.0, 4.5), (-17.0, 7.0, 2.7), (11.0, 13.5, 9.0), (1.0, -19.0, 1.8)]      # about 20 m away


def look_at(eye, up=(0.0, 0.0, 1.0)):
    """(3, 4) camera pose in the object's frame: at ``eye``, looking at the origin; columns x right, y down, z forward."""
    eye = np.asarray(eye, np.float64)
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return torch.from_numpy(np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(np.float32))


def make_views(mesh, colors, n, crop):
    """``n`` views of ``crop`` = (h, w) pixels around the principal point, rendered from the mesh's own colours."""
    h, w = crop
    roi = [800 - w // 2, 450 - h // 2, 800 - w // 2 + w, 450 - h // 2 + h]
    views = []
    for eye in EYES[:n]:
        pose = look_at(eye)
        shot = G.mesh_view(mesh, pose, DIAG, K, roi, colors=colors)
        views.append(dict(img=shot.color, mask=shot.mask.float(), cam_pose=pose, obj_diag=DIAG, K=K, roi=roi))
    return views


def measure(mesh, normals, colors, n_views, crop, reps):
    v, f = mesh
    dev, nV = v.device, v.shape[0]
    views = make_views(mesh, colors, n_views, crop)
    packed = ops.pack_mesh(v, f, [nV], [f.shape[0]])
    image_of, sign = torch.zeros(1, dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    ready = []
    for view in views:
        m, cam, (h, w) = G._view_camera(view["cam_pose"], DIAG, K, view["roi"], None, "a", False, False)
        mat = m.unsqueeze(0).float().to(dev)
        _, depth, _, screen = ops.rasterize(packed, mat, cam, image_of, 1, h, w, 1e-3, sign)
        centre = G.to_decoder_frame(view["cam_pose"].double()[:3, 3], DIAG).tolist()
        ready.append((mat, cam, (h, w), screen, depth[0].contiguous(), view["img"].contiguous(), view["mask"].contiguous(), centre))

    def rasterise():
        for mat, cam, (h, w), *_ in ready:
            ops.rasterize(packed, mat, cam, image_of, 1, h, w, 1e-3, sign)

    def paint():
        state = ops.paint_state(nV, dev)
        for k, (_, _, _, screen, depth, img, mask, centre) in enumerate(ready):
            ops.paint_view(packed, screen, normals, img, mask, depth, centre, 0.01 * DIAG, 1e-3, k, state)
        return ops.paint_finish(state, "weighted", 0.0) + (state,)

    colors0, filled0, state = paint()
    seen_pairs, seen = int(state.seen.sum()), int((state.seen > 0).sum())
    adjacency = G._pack_adjacency([G.mesh_adjacency(mesh)], [nV], dev)
    calls = {"paint_mesh_ms": lambda: G.paint_mesh(mesh, views, normals=normals), "rasterise_ms": rasterise, "paint_launches_ms": paint,
             "fill_10_rounds_ms": lambda: ops.paint_fill(colors0, filled0, adjacency, 10)}
    in_turn(calls, 2)                                                                                  # warm-up
    row = {"views": n_views, "crop": list(crop), "verts_seen": seen, "vertex_view_pairs_seen": seen_pairs}
    row.update(in_turn(calls, reps))
    least = 36 * nV * n_views + (24 + 24 + 80) * seen_pairs + 16 * nV
    row.update(paint_least_bytes=least, paint_gb_per_s=round(least / (row["paint_launches_ms"] * 1e-3) / 1e9, 1))
    return row


def main():
    a = C.arguments(C.BLOCKS, ("--res", dict(type=int, nargs="+", default=[128, 256])), ("--views", dict(type=int, nargs="+", default=[1, 3, 6])),
                    ("--crop", dict(type=int, nargs=2, default=(160, 240))))
    reps = max(7, a.reps)
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    box = C.box_decoder(sb, tb, dev)
    sc, tc = C.codes(1, 1, dev), C.codes(1, 2, dev)
    rows = []
    for R in a.res:
        grid = G.density_grid(box, sc, R, C.BOUND_BOX)
        extract = lambda: G.extract_mesh(grid, level=C.LEVEL_BOX, bound=C.BOUND_BOX)                   # noqa: E731
        mesh = extract()[0]
        normals = G.vertex_normals(box, [mesh], sc)[0].contiguous()
        shade = lambda: G.vertex_colors(box, [mesh], [normals], sc, tc)                                # noqa: E731
        colors = shade()[0].contiguous()
        same_run = in_turn({"extract_mesh_ms": extract, "vertex_colors_ms": shade}, reps)
        for n_views in a.views:
            rows.append(dict({"R": R, "verts": mesh[0].shape[0], "faces": mesh[1].shape[0]}, **same_run,
                             **measure(mesh, normals, colors, n_views, tuple(a.crop), reps)))
        del mesh, grid, normals, colors
        torch.cuda.empty_cache()
    C.report("mesh_paint_time", a, (sb, tb), reps=reps, meshes=rows)


if __name__ == "__main__":
    main()
