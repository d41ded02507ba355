"""Timing of the mesh rasteriser on one GPU: device events, medians of ``--reps`` calls, calls that are compared taken in turn.

  * ``geometry.rasterize`` of the narrow-band meshes of the planted box at R = ``--res`` for B = ``--batch`` objects into 256 x 256,
    1024 x 1024 and 1600 x 900 (all objects in one scene image), with the launches behind it one by one (projection, key preset + faces,
    resolve, interpolation of 3 channels) and the ``extract_mesh`` that made the mesh;
  * ``geometry.mesh_view`` against ``geometry.surface_depth`` on the same 256 x 256 pixel grid of one object (65 536 rays: a size at which
    the ray search is feasible), the mesh's extraction beside it;
  * ``--variants NAME=PATH ...``: ``snr_raster_faces`` of libraries built with another whole-wave threshold
    (``tools/build_variant.sh NAME -DSNR_RASTER_BIG_BOX=N``), the key preset included, on three loads: the R = 256 mesh into 1024 x 1024
    (faces of a pixel or less), the R = 128 mesh seen close up into 1600 x 900 (faces of tens of candidate pixels) and a hand-made load of
    two screen-filling triangles over 4096 triangles of about 400 pixels.  Every variant's keys are compared with the product library's.

Prints one JSON line.

usage: python tools/raster_time.py [--reps N] [--res R ...] [--batch B ...] [--variants NAME=PATH ...] [--commit SHA]"""
import ctypes

import numpy as np
import torch

import geometry_common as C
from geometry_common import BOUND_BOX, LEVEL_BOX as LEVEL
from ray_surface_time import in_turn
from supnerf_amd import _lib, driver, geometry as G, ops

SIZES = ((256, 256), (1024, 1024), (900, 1600))


def scene_matrices(B, dev):
    """Object -> camera matrices that set B boxes (decoder bound +-0.7) side by side in front of the camera, each turned a little."""
    cols = int(np.ceil(np.sqrt(B)))
    rows = int(np.ceil(B / cols))
    mats = []
    for b in range(B):
        a = 0.5 + 0.3 * b
        rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])
        t = np.array([1.5 * (b % cols - (cols - 1) / 2), 1.5 * (b // cols - (rows - 1) / 2), 2.2 * max(cols, 1)])
        mats.append(np.concatenate([rot, t[:, None]], 1))
    return torch.from_numpy(np.stack(mats).astype(np.float32)).to(dev)


def camera(H, W):
    f = 1.1 * min(H, W)
    return (f, f, (W - 1) / 2, (H - 1) / 2)


def stage_times(mesh, mats, cam, H, W, reps):
    """Median milliseconds of the launches behind ``ops.rasterize``, each between device events of its own."""
    dev = mesh.verts.device
    image_of = torch.zeros(len(mesh.n_verts), dtype=torch.int32, device=dev)
    screen = ops.raster_project(mesh, mats, cam)
    keys = ops.raster_faces(mesh, screen, image_of, 1, H, W, 1e-3)
    face, depth, weights = ops.raster_resolve(mesh, screen, keys)
    att = torch.rand(mesh.verts.shape[0], 3, device=dev)
    t = in_turn([lambda: ops.raster_project(mesh, mats, cam), lambda: torch.full((1, H, W), -1, dtype=torch.int64, device=dev),
                 lambda: ops.raster_faces(mesh, screen, image_of, 1, H, W, 1e-3), lambda: ops.raster_resolve(mesh, screen, keys),
                 lambda: ops.raster_interpolate(mesh, face, weights, att)], reps)
    names = ("project_ms", "key_preset_ms", "preset_and_faces_ms", "resolve_ms", "interpolate3_ms")
    out = dict(zip(names, t))
    # the least traffic of the pass: faces once (12 B), three screen vertices each (36 B), keys preset and read (16 B a pixel), outputs
    out["covered_pixels"] = int((face >= 0).sum())
    out["candidate_boxes"] = box_sizes(screen, mesh, H, W)
    out["min_bytes"] = int(mesh.faces.shape[0] * 48 + H * W * (16 + 4 + 4 + 12))
    return out


def raster_rows(model, res, batch, reps, dev):
    rows = []
    for R in res:
        for B in batch:
            sc = C.codes(B, B, dev)
            extract = lambda: G.extract_mesh(model, sc, level=LEVEL, resolution=R, bound=BOUND_BOX, narrow_band=True)      # noqa: E731
            meshes = extract()
            mats = scene_matrices(B, dev)
            row = {"R": R, "B": B, "faces": int(sum(m[1].shape[0] for m in meshes)), "verts": int(sum(m[0].shape[0] for m in meshes)),
                   "extract_mesh_ms": in_turn([extract], max(2, reps // 4))[0], "images": []}
            mesh = G._pack(meshes)
            for H, W in SIZES:
                cam = camera(H, W)
                t, = in_turn([lambda: G.rasterize(meshes, mats, cam, (H, W), cull="back")], reps)
                row["images"].append({"H": H, "W": W, "rasterize_ms": t, **stage_times(mesh, mats, cam, H, W, reps)})
            rows.append(row)
            del meshes, mesh
            torch.cuda.empty_cache()
    return rows


def view_row(model, reps, dev, im_sz=256):
    """``mesh_view`` and ``surface_depth`` of one object on the same ``im_sz`` x ``im_sz`` grid, in turn."""
    ob = driver.make_objects([11], 64)[0]
    sc = C.codes(1, 1, dev)
    pose, diag = ob["cam_pose"].float().to(dev), float(ob["obj_diag"])
    extract = lambda: G.extract_mesh(model, sc, level=LEVEL, resolution=256, bound=BOUND_BOX, narrow_band=True)      # noqa: E731
    mesh = extract()[0]
    with torch.no_grad():
        t_view, t_depth, t_extract = in_turn([lambda: G.mesh_view(mesh, pose, diag, ob["K"], ob["roi"], im_sz=im_sz),
                                              lambda: G.surface_depth(model, pose, diag, ob["K"], ob["roi"], sc, level=LEVEL, im_sz=im_sz),
                                              extract], max(2, reps // 2))
        view = G.mesh_view(mesh, pose, diag, ob["K"], ob["roi"], im_sz=im_sz)
        hits = G.surface_depth(model, pose, diag, ob["K"], ob["roi"], sc, level=LEVEL, im_sz=im_sz)
    both = view.mask & (hits.state == 1)
    diff = (view.depth - hits.depth)[both].abs()
    return {"grid": im_sz, "rays": im_sz * im_sz, "mesh_view_ms": t_view, "surface_depth_ms": t_depth, "extract_mesh_narrow_256_ms": t_extract,
            "mesh_pixels": int(view.mask.sum()), "ray_hits": int((hits.state == 1).sum()), "both": int(both.sum()),
            "median_abs_depth_difference_m": float(diff.median()) if both.any() else None, "obj_diag_m": diag}


def hand_made(dev, n=4096, H=900, W=1600, side=28.0, seed=0):
    """Two screen-filling triangles over ``n`` triangles of about side^2 / 2 pixels, as a one-object mesh on the unit camera."""
    g = np.random.default_rng(seed)
    c = g.uniform((0, 0), (W, H), (n, 2))
    tri = c[:, None, :] + g.uniform(-side / 2, side / 2, (n, 3, 2))
    pts = np.concatenate([tri.reshape(-1, 2), [[-1.0, -1.0], [W + 1.0, -1.0], [-1.0, H + 1.0], [W + 1.0, H + 1.0]]])
    z = np.concatenate([g.uniform(1.0, 2.0, 3 * n), [4.0] * 4])
    v = np.stack([pts[:, 0] * z, pts[:, 1] * z, z], 1).astype(np.float32)
    f = np.concatenate([np.arange(3 * n).reshape(n, 3), [[3 * n, 3 * n + 1, 3 * n + 2], [3 * n + 1, 3 * n + 3, 3 * n + 2]]]).astype(np.int32)
    eye = torch.eye(3, 4, device=dev)[None]
    return [(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))], eye, (1.0, 1.0, 0.0, 0.0), (H, W)


def variant_rows(model, variants, reps, dev):
    """``snr_raster_faces`` (behind the preset of its keys) of every library of ``variants`` on three loads, in turn."""
    libs = {"product": _lib.lib()}
    for name, path in variants:
        l = ctypes.CDLL(path)
        l.snr_raster_faces.restype, l.snr_raster_faces.argtypes = _lib._SIGS["snr_raster_faces"]
        libs[name] = l
    loads = []
    close = scene_matrices(1, dev)
    close[0, 2, 3] = 1.3                                                             # the box fills the height of the image
    for tag, R, mats, (H, W) in (("R=256 into 1024 x 1024", 256, scene_matrices(1, dev), (1024, 1024)),
                                 ("R=128 close up into 1600 x 900", 128, close, (900, 1600))):
        meshes = G.extract_mesh(model, C.codes(1, 1, dev), level=LEVEL, resolution=R, bound=BOUND_BOX, narrow_band=True)
        loads.append((tag, meshes, mats, camera(H, W), (H, W)))
    loads.append(("hand-made: 2 screen-filling + 4096 of ~400 pixels, 1600 x 900",) + hand_made(dev))
    rows = []
    i32, i64 = torch.int32, torch.int64
    for tag, meshes, mats, cam, (H, W) in loads:
        mesh = G._pack(meshes)
        screen = ops.raster_project(mesh, mats, cam)
        image_of = torch.zeros(1, dtype=i32, device=dev)
        voff, foff, B, nV, nF = ops._mesh_args(mesh)

        def run(l):
            keys = torch.full((1, H, W), -1, dtype=i64, device=dev)
            _lib.check(l.snr_raster_faces(ops._ptr(screen), ops._ptr(mesh.faces, i32), voff, foff, ops._ptr(image_of, i32), None, B, nV, nF, 1,
                                          H, W, 1e-3, ops._ptr(keys, i64), ops._stream(dev)), "snr_raster_faces")
            return keys
        want = run(libs["product"])
        same = {name: bool(torch.equal(run(l), want)) for name, l in libs.items()}
        times = in_turn([lambda l=l: run(l) for l in libs.values()], reps)
        boxes = box_sizes(screen, mesh, H, W)
        rows.append({"load": tag, "faces": int(nF), "covered_pixels": int((want != -1).sum()), "candidate_boxes": boxes,
                     "preset_and_faces_ms": dict(zip(libs, times)), "same_keys": same})
    return rows


def box_sizes(screen, mesh, H, W):
    """How the candidate boxes of a load are spread: the share of faces with no candidate, 1 - 15, 16 - 63, 64 - 255, 256 and more."""
    obj = torch.bucketize(torch.arange(mesh.faces.shape[0], device=screen.device), mesh.face_offset[1:], right=True)
    tri = screen[mesh.faces.long() + mesh.vert_offset[obj][:, None]]
    ok = torch.isfinite(tri).all(-1).all(-1) & (tri[..., 2] >= 1e-3).all(-1)
    lo, hi = (tri[..., :2].min(1).values * 256).round().long(), (tri[..., :2].max(1).values * 256).round().long()
    lim = torch.tensor([W - 1, H - 1], device=screen.device)
    n = (torch.minimum(hi >> 8, lim) - torch.clamp((lo + 255) >> 8, min=0) + 1).clamp(min=0).prod(1) * ok
    edges = [1, 16, 64, 256]
    share = [float((n < edges[0]).float().mean())] + [float(((n >= a) & (n < b)).float().mean()) for a, b in zip(edges, edges[1:])]
    return {"none": share[0], "1-15": share[1], "16-63": share[2], "64-255": share[3], "256+": float((n >= 256).float().mean())}


def main():
    a = C.arguments(C.BLOCKS, ("--res", dict(type=int, nargs="+", default=[128, 256])), C.BATCH,
                    ("--variants", dict(nargs="*", default=[], help="NAME=PATH of libraries built with another SNR_RASTER_BIG_BOX")))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    model = C.box_decoder(sb, tb, dev)
    fields = {"rasterize": raster_rows(model, a.res, a.batch, a.reps, dev), "view": view_row(model, a.reps, dev)}
    if a.variants:
        fields["variants"] = variant_rows(model, [v.split("=", 1) for v in a.variants], a.reps, dev)
    C.report("raster_time", a, (sb, tb), reps=a.reps, **fields)


if __name__ == "__main__":
    main()
