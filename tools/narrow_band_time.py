"""Timing of the narrow-band route of supnerf_amd.geometry on one GPU (device events): the dense grid (``density_grid``) against the
narrow-band grid (``narrow_band_grid``: coarse pass, band kernels, brick-mode decoder, growth rounds with their host reads) for the same
lattice, at R = 128, 256, 512 and B = 1, 8, on two decoders:

  * ``box``: the planted box with ``wobble`` (a closed surface through a few per cent of the bricks), level softplus(0);
  * ``fog``: the fresh decoder (sigma_bias -2), one code, cut at the median of its density: the worst case, the surface runs through most
    bricks.

The two routes are timed alternately, the median of ``--reps`` is reported, together with the iso-surface extraction of the grid (the same
passes for both routes), the points the decoder evaluated, the active fraction, the growth rounds, whether the two meshes are equal and,
where not, the dense grid's crossing edges the narrow band left unevaluated (the surface pieces its coarse pass missed).
Last, the brick-mode kernel's points/s against the lattice kernel's (mode 3) on every brick of an R = 256 grid.  Prints one JSON line.

usage: python tools/narrow_band_time.py [--reps N] [--res R ...] [--batch B ...] [--commit SHA]"""
import json
import sys

import torch

import geometry_common as C
from supnerf_amd import geometry as G, ops


def same_meshes(a, b):
    return all(torch.equal(va, vb) and torch.equal(fa, fb) for (va, fa), (vb, fb) in zip(a, b))


def missed_edges(grids, active, level):
    """Crossing edges of the dense grids (a list of batch pieces) with an end in a brick the narrow band did not evaluate: the surface
    pieces its coarse pass missed.  Zero whenever the two meshes differ would be a defect; the meshes are equal exactly when it is zero."""
    total, b0 = 0, 0
    for g in grids:
        for b in range(g.shape[0]):
            ins = g[b] > level
            n0, n1, n2 = ins.shape
            ev = active[b0 + b].repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:n0, :n1, :n2]
            for bits in (1, 2, 4, 3, 5, 6, 7):
                dx, dy, dz = bits & 1, bits >> 1 & 1, bits >> 2 & 1
                lo_, hi_ = (slice(0, n0 - dx), slice(0, n1 - dy), slice(0, n2 - dz)), (slice(dx, None), slice(dy, None), slice(dz, None))
                total += int(((ins[lo_] != ins[hi_]) & ~(ev[lo_] & ev[hi_])).sum())
        b0 += g.shape[0]
    return total


def row(model, sc, R, bound, level, reps):
    # the lattice kernel takes fewer than 2^30 points per launch (4 threads per point, below 2^32 threads): R = 512 runs 7 objects at a time
    per = max(1, (2 ** 30 - 1) // R ** 3)
    dense = lambda: [G.density_grid(model, sc[c:c + per], R, bound) for c in range(0, sc.shape[0], per)]     # noqa: E731
    narrow = lambda: G.narrow_band_grid(model, sc, R, level=level, bound=bound)                # noqa: E731
    gd, nb = dense(), narrow()                                                                 # warm-up, and the outputs
    md = [m for g in gd for m in G.extract_mesh(g, level=level, bound=bound)]
    mn = G.extract_mesh(nb.grid, level=level, bound=bound)
    equal = same_meshes(md, mn)
    missed = 0 if equal else missed_edges(gd, nb.active, level)
    n_verts, n_faces = sum(int(v.shape[0]) for v, _ in md), sum(int(f.shape[0]) for _, f in md)
    del md, mn
    iso = C.median_ms(lambda: G.extract_mesh(nb.grid, level=level, bound=bound), reps)
    del gd
    torch.cuda.empty_cache()
    d, n = C.alternate(dense, narrow, reps)
    B = sc.shape[0]
    dense_points = B * R ** 3
    out = {"R": R, "B": B, "dense_grid_ms": round(d, 3), "narrow_grid_ms": round(n, 3), "grid_speedup": round(d / n, 3),
           "iso_ms": round(iso, 3), "total_speedup": round((d + iso) / (n + iso), 3),
           "dense_points": dense_points, "narrow_points": nb.points, "work_ratio": round(dense_points / nb.points, 3),
           "active_fraction": round(float(nb.active.float().mean()), 4), "rounds": nb.rounds, "meshes_equal": equal, "missed_edges": missed,
           "verts": n_verts, "faces": n_faces}
    del nb
    torch.cuda.empty_cache()
    return out


def brick_rate(model, R, reps, dev):
    """points/s of snr_density_bricks on every brick of an R^3 grid against snr_density_grid on the same grid (R a multiple of 8: the same
    points, the same values)."""
    sc = C.codes(1, 3, dev)
    lat = G.lattice(R)
    nb = (R + 7) // 8
    idx = torch.arange(nb ** 3, device=dev, dtype=torch.int32)
    bricks = torch.stack([torch.zeros_like(idx), idx // (nb * nb), (idx // nb) % nb, idx % nb], 1).contiguous()
    latent, packed = C.latent(model, sc), model.packed_weights()
    out = torch.empty(1, R, R, R, device=dev)
    run = lambda: ops.density_bricks(lat, bricks, bricks.shape[0], latent, packed, model.shape_blocks, model.texture_blocks, out)  # noqa: E731
    grid = lambda: G.density_grid(model, sc, R)                                                # noqa: E731
    run()
    same = bool(torch.equal(out, grid()))
    b, g = C.alternate(run, grid, reps)
    P = 512 * bricks.shape[0]
    return {"R": R, "points": P, "bricks_ms": round(b, 3), "lattice_ms": round(g, 3), "bricks_Gpts_s": round(P / b / 1e6, 4),
            "lattice_Gpts_s": round(R ** 3 / g / 1e6, 4), "ratio": round((P / b) / (R ** 3 / g), 4), "sigma_bit_identical": same}


def main():
    a = C.arguments(C.RES, C.BATCH)
    dev = torch.device("cuda:0")
    sb, tb = 3, 1
    cases = {"box": (C.box_decoder(sb, tb, dev), C.BOUND_BOX), "fog": (C.fog_decoder(sb, tb, dev), (-0.5, 0.5))}
    rows = []
    for name, (model, bound) in cases.items():
        for R in a.res:
            for B in a.batch:
                sc = C.codes(B, B, dev)
                if name == "box":
                    level = C.LEVEL_BOX
                else:
                    # one code B times: a level cuts one fog code through its median only (the fog's sigma differs a little per code)
                    sc = sc[:1].repeat(B, 1)
                    level = float(G.density_grid(model, sc[:1], min(R, 128), bound).median())
                    torch.cuda.empty_cache()
                r = row(model, sc, R, bound, level, a.reps)
                r = {"case": name, "level": level, **r}
                rows.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    rate = brick_rate(cases["fog"][0], 256, a.reps, dev)
    C.report("narrow_band_time", a, (sb, tb), rows=rows, brick_mode=rate)


if __name__ == "__main__":
    main()
