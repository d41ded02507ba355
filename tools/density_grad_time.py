"""Timing of the density-only backward on one GPU (device events), printed as one JSON line:

  * ``geometry.density_gradient`` (sigma and d sigma / d xyz: ``snr_density_fwd_masks`` + ``snr_density_bwd``) against the same gradient
    through the full fp32 pair (``ops.decoder_fwd(save_masks=True)`` + ``ops.decoder_bwd(d_rgb = 0)``) on the points of an R^3 lattice,
    R = 128 and 256, B = 1 and 8 objects; d xyz is checked bit for bit between the two in every row;
  * ``geometry.density`` forward + backward to the shape codes at B x N points against the same sigma loss through ``ops.DecoderPoints``
    (the full decoder, colour branch included).

Each pair of timings alternates the two sides; the median of ``--reps`` is reported.

usage: python tools/density_grad_time.py [--reps N] [--blocks SB TB] [--commit SHA] [--sizes R ...]"""
import json
import sys

import torch

import geometry_common as C
from supnerf_amd import geometry as G


def main():
    a = C.arguments(C.BLOCKS, ("--sizes", dict(type=int, nargs="+", default=(128, 256))),
                    ("--code-points", dict(type=int, nargs=2, default=(8, 65536), help="B and points per object of the shape-code row")))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    ops = C.A.ops
    model = C.fog_decoder(sb, tb, dev)
    packed = model.packed_weights()
    rows = []
    for R in a.sizes:
        for B in (1, 8):
            sc = C.codes(B, B, dev)
            lat = C.latent(model, sc)
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
            md, mf = C.alternate(dens, full, a.reps)
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
    md, mf = C.alternate(dens_code, full_code, a.reps)
    code = {"B": B, "points_per_obj": N, "density_fwd_bwd_ms": round(md, 3), "decoder_points_fwd_bwd_ms": round(mf, 3), "ratio": round(mf / md, 3),
            "d_shapecode_bit_identical": code_same, "d_shapecode_max_rel_diff": code_rel}
    C.report("density_grad_time", a, (sb, tb), gradient=rows, shape_code=code)


if __name__ == "__main__":
    main()
