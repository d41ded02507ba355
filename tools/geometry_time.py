"""Timing of supnerf_amd.geometry on one GPU (device events): the density-only lattice kernel (snr_density_grid) against the full fp32
forward (ops.decoder_fwd, precision "fp32") on the same points, at R = 128 and R = 256 for B = 1 and B = 8, and one whole iso-surface
extraction (count pass, the two scans, the host read of the sizes, emit pass) of an R = 256 grid.  The two decoder launches are timed alternately, each over several repeats; the median is
reported.  Prints one JSON line.

usage: python tools/geometry_time.py [--reps N] [--blocks SB TB] [--commit SHA]   (the commit defaults to `git rev-parse HEAD`)"""
import torch

import geometry_common as C
from supnerf_amd import geometry as G


def main():
    a = C.arguments(C.BLOCKS)
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    model = C.fog_decoder(sb, tb, dev)
    packed = model.packed_weights()
    rows = []
    for R in (128, 256):
        for B in (1, 8):
            sc = C.codes(B, B, dev)
            lat = C.latent(model, sc)
            pts = G.lattice_points(G.lattice(R), dev).repeat(B, 1).contiguous()
            vd = torch.nn.functional.normalize(torch.ones_like(pts), dim=1)
            P = pts.shape[0]
            dens = lambda: G.density_grid(model, sc, R)                                        # noqa: E731
            full = lambda: C.A.ops.decoder_fwd(pts, vd, lat, packed, sb, tb, precision="fp32")   # noqa: E731
            g, (s_full, _, _) = dens(), full()                                                 # warm-up, and the outputs agree bit for bit
            same = bool(torch.equal(g.reshape(-1), s_full))
            md, mf = C.alternate(dens, full, a.reps)
            rows.append({"R": R, "B": B, "points": P, "density_ms": round(md, 3), "full_fwd_ms": round(mf, 3),
                         "density_Gpts_s": round(P / md / 1e6, 3), "full_Gpts_s": round(P / mf / 1e6, 3), "speedup": round(mf / md, 3),
                         "sigma_bit_identical": same})
            del pts, vd
            torch.cuda.empty_cache()
    # iso passes on one R = 256 grid: the fog decoder's density cut at its median, a worst case for the number of triangles
    R = 256
    grid = G.density_grid(model, C.codes(1, 1, dev), R)
    level = float(grid.float().median())
    G.extract_mesh(grid, level=level)
    iso_ms = C.median_ms(lambda: G.extract_mesh(grid, level=level), a.reps)
    v, f = G.extract_mesh(grid, level=level)[0]
    C.report("geometry_time", a, (sb, tb), decoder=rows,
             iso={"R": R, "level": level, "ms_total_incl_host_read": round(iso_ms, 3), "verts": int(v.shape[0]), "faces": int(f.shape[0])})


if __name__ == "__main__":
    main()
