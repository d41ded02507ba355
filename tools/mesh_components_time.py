"""Timing of ``geometry.mesh_components`` and ``geometry.largest_component`` on one GPU (device events, medians of ``--reps`` calls, host
reads inside the call included) on three meshes: the fog decoder's 256^3 grid cut at its median density (the worst case for the number of
triangles and of components), the planted box at R = 256, and the planted five-piece grid of tests/mesh_restatement.py at R = 256.  Each
time is set beside three figures of the same mesh from the same run: the ``extract_mesh`` that made it, the ``density_grid`` launch that made
its grid (decoder cases), and the host route -- both arrays to the host, ``scipy.sparse.csgraph.connected_components``, the labels back
(labels only: no measures).  ``--stages`` adds the time of each stage of ``ops.mesh_components``, synchronised one by one.  Prints one JSON
line.

usage: python tools/mesh_components_time.py [--reps N] [--res R] [--blocks SB TB] [--no-host] [--stages] [--commit SHA]"""
import time

import numpy as np
import torch

import geometry_common as C
import mesh_restatement as MR
from supnerf_amd import geometry as G


def host_route(v, f):
    """Seconds -> milliseconds of the route a caller had before: arrays to the host, scipy, labels back to the device."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vh, fh = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    rows, cols = np.concatenate([fh[:, 0], fh[:, 0]]), np.concatenate([fh[:, 1], fh[:, 2]])
    g = coo_matrix((np.ones(rows.shape[0], np.int8), (rows, cols)), shape=(vh.shape[0], vh.shape[0]))
    _, lab = connected_components(g, directed=False)
    torch.from_numpy(lab).to(v.device)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stages(v, f, reps):
    """Median milliseconds of the pieces of ``ops.mesh_components`` on one object, each between device events of its own."""
    from supnerf_amd import _lib, ops
    lib, dev = _lib.lib(), v.device
    st = ops._stream(dev)
    i32, i64 = torch.int32, torch.int64
    nV, nF = v.shape[0], f.shape[0]
    voff, foff = torch.tensor([0, nV]).to(dev), torch.tensor([0, nF]).to(dev)
    parent, root = torch.empty(nV, dtype=i32, device=dev), torch.empty(nV, dtype=i32, device=dev)
    is_root, bad = torch.empty(nV, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=i32, device=dev)
    p = ops._ptr
    out = {}
    out["hook_ms"] = C.median_ms(lambda: lib.snr_mesh_hook(p(f, i32), p(voff, i64), p(foff, i64), 1, nV, nF, p(parent, i32), p(bad, i32), st), reps)
    out["flatten_ms"] = C.median_ms(lambda: lib.snr_mesh_flatten(p(parent, i32), p(voff, i64), 1, nV, p(root, i32), p(is_root, torch.uint8), st),
                                    reps)
    out["root_scan_ms"] = C.median_ms(lambda: torch.cumsum(is_root, 0, dtype=i32), reps)
    m = ops.mesh_components(v, f, [nV], [nF])
    out["face_sort_ms"] = C.median_ms(lambda: torch.sort(m.face_label, stable=True), reps)
    out["whole_call_ms"] = C.median_ms(lambda: ops.mesh_components(v, f, [nV], [nF]), reps)
    return out


def main():
    a = C.arguments(C.BLOCKS, ("--res", dict(type=int, default=256)), ("--no-host", dict(action="store_true")),
                    ("--stages", dict(action="store_true")))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    R = a.res
    cases = []
    fog, box = C.fog_decoder(sb, tb, dev), C.box_decoder(sb, tb, dev)
    sc = C.codes(1, 1, dev)
    grid = G.density_grid(fog, sc, R)
    cases.append(("fog at its median", fog, sc, grid, float(grid.float().median()), (-0.5, 0.5)))
    cases.append(("planted box", box, sc, G.density_grid(box, sc, R, C.BOUND_BOX), C.LEVEL_BOX, C.BOUND_BOX))
    cases.append(("five-piece grid", None, None, torch.from_numpy(MR.planted_field(R)[0]).to(dev)[None], 0.0, (-0.5, 0.5)))
    rows = []
    for name, model, code, grid, level, bound in cases:
        extract = lambda: G.extract_mesh(grid, level=level, bound=bound)                      # noqa: E731
        meshes = extract()
        v, f = meshes[0]
        comps = G.mesh_components(meshes)[0]                                                    # warm-up
        sub = G.largest_component(meshes)[0]
        row = {"mesh": name, "R": R, "verts": int(v.shape[0]), "faces": int(f.shape[0]), "components": int(comps.n_verts.shape[0]),
               "largest_verts": int(sub[0].shape[0]), "largest_volume": float(comps.volume[comps.area.argmax()]),
               "components_ms": round(C.median_ms(lambda: G.mesh_components(meshes), a.reps), 3),
               "largest_component_ms": round(C.median_ms(lambda: G.largest_component(meshes), a.reps), 3),
               "extract_mesh_ms": round(C.median_ms(extract, a.reps), 3)}
        if model is not None:
            row["density_grid_ms"] = round(C.median_ms(lambda: G.density_grid(model, code, R, bound), max(1, a.reps // 2)), 3)
        if not a.no_host:
            row["host_route_ms"] = round(float(np.median([host_route(v, f) for _ in range(max(1, a.reps // 2))])), 1)
        if a.stages:
            row["stages"] = {k: round(x, 3) for k, x in stages(v, f, a.reps).items()}
        rows.append(row)
        del meshes, v, f, comps, sub
        torch.cuda.empty_cache()
    C.report("mesh_components_time", a, (sb, tb), meshes=rows)


if __name__ == "__main__":
    main()
