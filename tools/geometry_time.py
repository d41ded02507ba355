"""Timing of supnerf_amd.geometry on one GPU (device events): the density-only lattice kernel (snr_density_grid) against the full fp32
forward (ops.decoder_fwd, precision "fp32") on the same points, at R = 128 and R = 256 for B = 1 and B = 8, and one whole iso-surface
extraction (count pass, the two scans, the host read of the sizes, emit pass) of an R = 256 grid.  The two decoder launches are timed alternately, each over several repeats; the median is
reported.  Prints one JSON line.

usage: python tools/geometry_time.py [--reps N] [--blocks SB TB] [--commit SHA]   (the commit defaults to `git rev-parse HEAD`)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import supnerf_amd as A  # noqa: E402
from supnerf_amd import geometry as G  # noqa: E402
from oracle import supnerf_oracle as O  # noqa: E402


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True, timeout=10).stdout.strip() or None
    except Exception:
        return None


def timed(fn, reps):
    """Median milliseconds of ``reps`` single calls, each between two device events."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, nargs=2, default=(3, 1))
    ap.add_argument("--commit", default=None, help="commit to report when the tree has no .git")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    model = A.CodeNeRF(shape_blocks=sb, texture_blocks=tb)
    model.load_state_dict(O.init_decoder_params(sb, tb, seed=0, sigma_bias=-2.0))
    model = model.to(dev)
    packed = model.packed_weights()
    rows = []
    for R in (128, 256):
        for B in (1, 8):
            sc = (torch.randn(B, 256, generator=torch.Generator().manual_seed(B)) * 0.5).to(dev)
            lat = model.latent_terms(sc, torch.zeros_like(sc)).detach().contiguous()
            pts = G.lattice_points(G.lattice(R), dev).repeat(B, 1).contiguous()
            vd = torch.nn.functional.normalize(torch.ones_like(pts), dim=1)
            P = pts.shape[0]
            dens = lambda: G.density_grid(model, sc, R)                                        # noqa: E731
            full = lambda: A.ops.decoder_fwd(pts, vd, lat, packed, sb, tb, precision="fp32")   # noqa: E731
            g, (s_full, _, _) = dens(), full()                                                 # warm-up, and the outputs agree bit for bit
            same = bool(torch.equal(g.reshape(-1), s_full))
            t_d, t_f = [], []
            for _ in range(a.reps):                                                            # alternate the two
                t_d.append(timed(dens, 1))
                t_f.append(timed(full, 1))
            md, mf = float(np.median(t_d)), float(np.median(t_f))
            rows.append({"R": R, "B": B, "points": P, "density_ms": round(md, 3), "full_fwd_ms": round(mf, 3),
                         "density_Gpts_s": round(P / md / 1e6, 3), "full_Gpts_s": round(P / mf / 1e6, 3), "speedup": round(mf / md, 3),
                         "sigma_bit_identical": same})
            del pts, vd
            torch.cuda.empty_cache()
    # iso passes on one R = 256 grid: the fog decoder's density cut at its median, a worst case for the number of triangles
    R = 256
    sc = (torch.randn(1, 256, generator=torch.Generator().manual_seed(1)) * 0.5).to(dev)
    grid = G.density_grid(model, sc, R)
    level = float(grid.float().median())
    G.extract_mesh(grid, level=level)
    iso_ms = timed(lambda: G.extract_mesh(grid, level=level), a.reps)
    v, f = G.extract_mesh(grid, level=level)[0]
    print(json.dumps({"tool": "geometry_time", "commit": a.commit or commit(), "device": torch.cuda.get_device_name(0), "blocks": [sb, tb],
                      "decoder": rows, "iso": {"R": R, "level": level, "ms_total_incl_host_read": round(iso_ms, 3),
                                                  "verts": int(v.shape[0]), "faces": int(f.shape[0])}}))


if __name__ == "__main__":
    main()
