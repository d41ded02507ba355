"""Timing of the density-only backward on one GPU (device events), printed as one JSON line:

  * ``geometry.density_gradient`` (sigma and d sigma / d xyz: ``snr_density_fwd_masks`` + ``snr_density_bwd``) against the same gradient
    through the full fp32 pair (``ops.decoder_fwd(save_masks=True)`` + ``ops.decoder_bwd(d_rgb = 0)``) on the points of an R^3 lattice,
    R = 128 and 256, B = 1 and 8 objects; d xyz is checked bit for bit between the two in every row;
  * ``geometry.density`` forward + backward to the shape codes at B x N points against the same sigma loss through ``ops.DecoderPoints``
    (the full decoder, colour branch included).

Each pair of timings alternates the two sides; the median of ``--reps`` is reported.

usage: python tools/density_grad_time.py [--reps N] [--blocks SB TB] [--commit SHA] [--sizes R ...]"""
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


def timed(fn):
    """Milliseconds of one call between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(f_a, f_b, reps):
    t_a, t_b = [], []
    for _ in range(reps):
        t_a.append(timed(f_a))
        t_b.append(timed(f_b))
    return float(np.median(t_a)), float(np.median(t_b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, nargs=2, default=(3, 1))
    ap.add_argument("--sizes", type=int, nargs="+", default=(128, 256))
    ap.add_argument("--code-points", type=int, nargs=2, default=(8, 65536), help="B and points per object of the shape-code row")
    ap.add_argument("--commit", default=None, help="commit to report when the tree has no .git")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    ops = A.ops
    model = A.CodeNeRF(shape_blocks=sb, texture_blocks=tb)
    model.load_state_dict(O.init_decoder_params(sb, tb, seed=0, sigma_bias=-2.0))
    model = model.to(dev)
    packed = model.packed_weights()
    rows = []
    for R in a.sizes:
        for B in (1, 8):
            sc = (torch.randn(B, 256, generator=torch.Generator().manual_seed(B)) * 0.5).to(dev)
            lat = model.latent_terms(sc, torch.zeros_like(sc)).detach().contiguous()
            pts = G.lattice_points(G.lattice(R), dev).repeat(B, 1).contiguous()
            vd = torch.nn.functional.normalize(torch.ones_like(pts), dim=1)
            P = pts.shape[0]
            zero_rgb = torch.zeros(P, 3, device=dev)
            ones = torch.ones(P, device=dev)

            def dens():
                return G.density_gradient(model, pts, sc)[1]

            def full():
                s, _, m = ops.decoder_fwd(pts, vd, lat, packed, sb, tb, save_masks=True, precision="fp32")
                return ops.decoder_bwd(pts, vd, lat, packed, m, s, ones, zero_rgb, sb, tb, need_latent=False, need_dir=False, precision="fp32")[1]

            same = bool(torch.equal(dens(), full()))                       # (also the warm-up)
            torch.cuda.synchronize()
            md, mf = alternate(dens, full, a.reps)
            rows.append({"R": R, "B": B, "points": P, "grad_pair_ms": round(md, 3), "full_pair_ms": round(mf, 3),
                         "grad_pair_Gpts_s": round(P / md / 1e6, 4), "full_pair_Gpts_s": round(P / mf / 1e6, 4), "ratio": round(mf / md, 3),
                         "d_xyz_bit_identical": same})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            del pts, vd, zero_rgb, ones
            torch.cuda.empty_cache()

    # the shape-code gradient of a density-only loss: geometry.density against the full decoder's sigma (ops.DecoderPoints)
    B, N = a.code_points
    g = torch.Generator().manual_seed(3)
    sc0 = (torch.randn(B, 256, generator=g) * 0.5).to(dev)
    xyz = (torch.rand(B * N, 3, generator=g) - 0.5).to(dev)
    vd = torch.nn.functional.normalize(torch.randn(B * N, 3, generator=g), dim=1).to(dev)
    w = torch.randn(B * N, generator=g).to(dev)

    def dens_code():
        sc = sc0.clone().requires_grad_()
        (G.density(model, xyz, sc) * w).sum().backward()
        return sc.grad

    def full_code():
        sc = sc0.clone().requires_grad_()
        lat = model.latent_terms(sc, torch.zeros_like(sc))
        sig, _ = ops.DecoderPoints.apply(xyz, vd, lat, packed, sb, tb, "fp32")
        (sig * w).sum().backward()
        return sc.grad

    ga, gb = dens_code(), full_code()
    code_same = bool(torch.equal(ga, gb))
    code_rel = float((ga - gb).abs().max() / gb.abs().max())
    md, mf = alternate(dens_code, full_code, a.reps)
    code = {"B": B, "points_per_obj": N, "density_fwd_bwd_ms": round(md, 3), "decoder_points_fwd_bwd_ms": round(mf, 3), "ratio": round(mf / md, 3),
            "d_shapecode_bit_identical": code_same, "d_shapecode_max_rel_diff": code_rel}
    print(json.dumps({"tool": "density_grad_time", "commit": a.commit or commit(), "device": torch.cuda.get_device_name(0), "blocks": [sb, tb],
                      "gradient": rows, "shape_code": code}))


if __name__ == "__main__":
    main()
