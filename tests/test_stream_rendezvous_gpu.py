"""The exact-fp32 two-waves kernels' weight ring (csrc/snr_mlp16_core.hpp: RingTurn) at the smallest shapes that walk every chunk of it.

The ring's rendezvous sits inside every chunk's last MFMA group and the next chunk's first fragment pair is requested from the OTHER buffer
behind it, carried into the next chunk and the next layer.  A fragment taken from the wrong buffer is deterministic and shows at any size, so
the shapes are small: every block count below gives the stream a different number of chunks in front of and behind enc_viewdir's nine (both
parities of the ring), the point counts cover one wave tile, one workgroup and a ragged last workgroup, the renders both launch shapes (S = 64:
four waves, one ray per workgroup; S = 128: eight waves).  Everything is held to the float64 oracle through the suite's band
(tests/oracle_bands.py), gradients mask-matched (tests/relu_bits.py).  The other failure of a ring, a buffer overwritten under a slower wave,
is a race no test can force: it is argued where RingTurn is defined.

Also pinned, because the suite relies on them elsewhere: the density-only sigma is the full forward's bit for bit, and a forward that saves
ReLU bits computes what one that does not computes."""
import pytest
import torch

from oracle import supnerf_oracle as O
from oracle_bands import amd, check_all, dev  # noqa: F401  (amd, dev: fixtures)
from relu_bits import decode_relu_bits

pytestmark = pytest.mark.gpu

BLOCKS = [(0, 0), (1, 0), (3, 1), (2, 2)]
POINTS = [1, 16, 63, 64, 65, 129]


def _decoder(amd, dev, sb, tb):
    params = O.init_decoder_params(sb, tb, seed=10 * sb + tb)
    return params, amd.ops.pack_weights({k: v.to(dev) for k, v in params.items()}, sb, tb)


def _latent(params, sb, tb, B, g):
    sc, tc = torch.randn(B, 256, generator=g) * 0.3, torch.randn(B, 256, generator=g) * 0.3
    return O.latent_terms(params, sc, tc) if sb + tb else torch.zeros(B, 1, 256)


@pytest.mark.parametrize("blocks", BLOCKS)
def test_points_forward(amd, dev, blocks):
    """decoder_fwd with and without ReLU bits and density_fwd (mode 2, with and without bits) on 1 .. 129 points of one object."""
    ops = amd.ops
    sb, tb = blocks
    params, packed = _decoder(amd, dev, sb, tb)
    pairs = []
    for P in POINTS:
        g = torch.Generator().manual_seed(100 * sb + 10 * tb + P)
        xyz = torch.rand(P, 3, generator=g) - 0.5
        vd = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1)
        lat = _latent(params, sb, tb, 1, g)
        x_d, v_d, l_d = xyz.to(dev), vd.to(dev), lat.to(dev)
        sig, rgb, masks = ops.decoder_fwd(x_d, v_d, l_d, packed, sb, tb, save_masks=True, precision="fp32")
        sig0, rgb0, _ = ops.decoder_fwd(x_d, v_d, l_d, packed, sb, tb, precision="fp32")
        assert torch.equal(sig0, sig) and torch.equal(rgb0, rgb), (blocks, P, "the forward with ReLU bits is not the forward without")
        sig_d, masks_d = ops.density_fwd(x_d, l_d, packed, sb, tb, save_masks=True)
        assert torch.equal(sig_d, sig) and torch.equal(ops.density_fwd(x_d, l_d, packed, sb, tb)[0], sig), (blocks, P, "density-only sigma")
        full, dens = decode_relu_bits(masks, P, sb, tb), decode_relu_bits(masks_d, P, sb, tb)
        assert all(torch.equal(a, b) for a, b in zip(full[:sb + 1], dens[:sb + 1])), (blocks, P, "density-only ReLU bits")
        (s32, r32), (s64, r64) = [O.decoder_forward({k: v.to(dt) for k, v in params.items()}, xyz.to(dt)[:, None], vd.to(dt)[:, None], None, None,
                                                    latent=lat.to(dt)) for dt in (torch.float32, torch.float64)]
        pairs += [(f"sigma P={P}", sig, s32.reshape(-1), s64.reshape(-1)), (f"rgb P={P}", rgb, r32.reshape(-1, 3), r64.reshape(-1, 3))]
    check_all(pairs, "fp32")


@pytest.mark.parametrize("blocks", [(3, 1), (0, 0)])
def test_lattice_density_on_65_points(amd, dev, blocks):
    """Mode 3 (the lattice's points made in the kernel) on 5 x 13 x 1 = 65 points: the list kernel's sigma, which is the full forward's."""
    from supnerf_amd import geometry as G
    ops = amd.ops
    sb, tb = blocks
    params, packed = _decoder(amd, dev, sb, tb)
    g = torch.Generator().manual_seed(65 + sb)
    lat = _latent(params, sb, tb, 1, g).to(dev)
    lattice = G.lattice((5, 13, 1), ((-0.4, -0.5, 0.1), (0.45, 0.5, 0.1)))
    pts = G.lattice_points(lattice, dev)
    assert pts.shape == (65, 3)
    grid = ops.density_grid(lattice, lat, packed, sb, tb)
    vd = torch.nn.functional.normalize(torch.randn(65, 3, generator=g), dim=1).to(dev)
    assert torch.equal(grid.reshape(-1), ops.density_fwd(pts, lat, packed, sb, tb)[0])
    assert torch.equal(grid.reshape(-1), ops.decoder_fwd(pts, vd, lat, packed, sb, tb, precision="fp32")[0])


@pytest.mark.parametrize("blocks", [(3, 1), (1, 0)])
@pytest.mark.parametrize("S,N", [(64, 2), (64, 3), (128, 2), (128, 3)])
def test_fused_render_and_backward(amd, dev, blocks, S, N):
    """render_fwd (with and without what the backward needs) and render_bwd on 2 and 3 rays of one object, per-ray depths."""
    ops = amd.ops
    sb, tb = blocks
    params, packed = _decoder(amd, dev, sb, tb)
    g = torch.Generator().manual_seed(S + N + sb)
    o = (torch.rand(N, 3, generator=g) - 0.5) * 0.2 - torch.tensor([0.0, 0.0, 1.2])
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 1.0]), dim=1)
    t = torch.linspace(0.5, 2.0, S + 1)[:-1][None] + torch.rand(N, S, generator=g) * (1.5 / S)
    lat = _latent(params, sb, tb, 1, g)
    wts = [torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)]
    one = torch.ones(1)
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, N, sb, tb, white_bkgd=True, metric_z=True, precision="fp32")
    ins = [x.to(dev) for x in (o, d, t, one, one, lat)]
    out = ops.render_fwd(*ins, packed, cfg, save_for_bwd=True)
    plain = ops.render_fwd(*ins, packed, cfg)
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], out[:3])), (blocks, S, N, "the forward with ReLU bits is not the forward without")
    sig, rgbs, masks = out[3:]
    need_lat = sb + tb > 0
    d_o, d_d, d_t, d_lat = ops.render_bwd(*ins, packed, cfg, sig, rgbs, masks, *[w.to(dev) for w in wts], need_t=True, need_latent=need_lat)
    bits = decode_relu_bits(masks, N * S, sb, tb)
    refs = []
    for dt in (torch.float32, torch.float64):
        c = lambda x: x.to(dt)
        leaves = [c(x).clone().requires_grad_() for x in (o, d, t, lat)]
        r = O.fused_render({k: c(v) for k, v in params.items()}, leaves[0], leaves[1], leaves[2], "per_ray", S, N, c(one), latent=leaves[3],
                           relu_masks=bits, white_bkgd=True, metric_z=True)
        sum((a * c(w)).sum() for a, w in zip(r, wts)).backward()
        refs.append([x.detach() for x in r] + [x.grad for x in leaves])
    got = list(out[:3]) + [d_o, d_d, d_t, d_lat]
    names = ["rgb", "depth", "acc", "d_rays_o", "d_rays_d", "d_t", "d_latent"]
    check_all([(nm, a, b, c) for nm, a, b, c in zip(names, got, refs[0], refs[1]) if a is not None], "fp32")
