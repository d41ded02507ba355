"""The five Functions that pad ragged objects -- ``DecoderPoints``, ``DecoderPointsTrain``, ``FusedRender``, ``DensityPoints``,
``RaySurface`` -- against their raw operators on operands padded BY HAND, bit for bit: outputs and every gradient, the latent rows
included.  The hand-padded call is what the Function does internally (``ops._pad_rows`` / ``ops.pad_render_inputs``, zero upstream
gradient on the dummy rows, ``ops._unpad_rows``), so any difference is a moved operand, not rounding.

B = 2 objects, blocks (3, 1), fp32; per-object counts at the seam of each tile: 31 / 32 / 33 points for the 32-point wave tile of the
decoder, 7 / 8 / 9 rays of S = 4 samples for the fused render, 63 / 64 / 65 for the 64-point rows of the density backward.  The padded
count is restated here with literal tiles; at the exact tile it is the caller's own count, and the tensors the Function saved show it.
``DecoderPointsTrain``'s weight gradients are a chain of launches rather than one raw operator: its hand-padded call is the Function
itself on whole tiles, where it pads nothing (asserted)."""
import pytest
import torch

from oracle_bands import amd, dev, make_model  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

B, SB, TB, S = 2, 3, 1, 4


@pytest.fixture(scope="module")
def decoder(amd, dev, oracle_params):  # noqa: F811
    """(model, packed weights, latent terms (B, 4, 256)) shared by every case."""
    m = make_model(amd, dev, oracle_params, "fp32", blocks=(SB, TB))
    g = torch.Generator().manual_seed(5)
    sc, tc = [(torch.randn(B, 256, generator=g) * 0.3).to(dev) for _ in range(2)]
    with torch.no_grad():
        lat = m.latent_terms(sc, tc).clone()
    return m, m.packed_weights(), lat


def leaf(t):
    return t.detach().clone().requires_grad_()


def same(tag, got, want):
    assert len(got) == len(want), tag
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), (tag, k)


def by_hand(ops, n, tile):
    """(n_pad, pad, strip) of n rows per object launched as whole ``tile``-row blocks."""
    n_pad = -(-n // tile) * tile
    assert (n_pad == n) == (n % tile == 0)
    return n_pad, lambda t: ops._pad_rows(t, B, n, n_pad), lambda t: ops._unpad_rows(t, B, n, n_pad)


def saved_rows(out, k=0):
    return out.grad_fn.saved_tensors[k].shape[0]


def point_batch(n, dev):  # noqa: F811
    g = torch.Generator().manual_seed(100 + n)
    xyz = (torch.rand(B * n, 3, generator=g) - 0.5).to(dev)
    vd = torch.nn.functional.normalize(torch.randn(B * n, 3, generator=g), dim=1).to(dev)
    return xyz, vd, torch.randn(B * n, generator=g).to(dev), torch.randn(B * n, 3, generator=g).to(dev)


@pytest.mark.parametrize("n", [31, 32, 33])
def test_decoder_points(amd, dev, decoder, n):  # noqa: F811
    ops = amd.ops
    _, packed, lat0 = decoder
    xyz0, vd0, u_sig, u_rgb = point_batch(n, dev)
    xyz, vd, lat = leaf(xyz0), leaf(vd0), leaf(lat0)
    sig, rgb = ops.DecoderPoints.apply(xyz, vd, lat, packed, SB, TB, "fp32")
    n_pad, pad, strip = by_hand(ops, n, 32)
    assert saved_rows(sig) == B * n_pad
    d_xyz, d_dir, d_lat = torch.autograd.grad((sig, rgb), (xyz, vd, lat), (u_sig, u_rgb))
    xp, vp = pad(xyz0), pad(vd0)
    s, r, masks = ops.decoder_fwd(xp, vp, lat0, packed, SB, TB, save_masks=True, precision="fp32")
    h_lat, h_xyz, h_dir = ops.decoder_bwd(xp, vp, lat0, packed, masks, s, pad(u_sig), pad(u_rgb), SB, TB, precision="fp32")
    same(n, (sig, rgb, d_xyz, d_dir, d_lat), (strip(s), strip(r), strip(h_xyz), strip(h_dir), h_lat))


@pytest.mark.parametrize("n", [31, 32, 33])
def test_decoder_points_train(amd, dev, decoder, n):  # noqa: F811
    ops = amd.ops
    m, _, lat0 = decoder
    w = list(m._per_point_params().values())
    xyz0, vd0, u_sig, u_rgb = point_batch(n, dev)
    n_pad, pad, strip = by_hand(ops, n, 32)

    def run(x, v, us, ur):
        x, v, lat = leaf(x), leaf(v), leaf(lat0)
        sig, rgb = ops.DecoderPointsTrain.apply(x, v, lat, SB, TB, "fp32", *w)
        assert saved_rows(sig) == B * n_pad
        return (sig, rgb, *torch.autograd.grad((sig, rgb), (x, v, lat, *w), (us, ur)))
    got, want = run(xyz0, vd0, u_sig, u_rgb), run(pad(xyz0), pad(vd0), pad(u_sig), pad(u_rgb))
    same(n, got, [strip(t) for t in want[:4]] + list(want[4:]))


def render_batch(ops, n, box, dev):  # noqa: F811
    """(rays_o, rays_d, depths or jitter, xyz_div, z_scale, cfg, the three upstream gradients): rays aimed at the objects from 1.2 away."""
    g = torch.Generator().manual_seed(200 + n + box)
    N = B * n
    aim = torch.randn(N, 3, generator=g) * 0.15
    ro = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=1) * 1.2
    rd = torch.nn.functional.normalize(aim - ro, dim=1)
    div = torch.tensor([1.3, 0.9])
    if box:
        t, zs = torch.rand(N, S, generator=g), torch.tensor([1.1, 0.8])
        cfg = ops.RenderCfg(S, ops.Z_BOX, n, SB, TB, precision="fp32", box_half=torch.tensor([[0.5, 0.4, 0.3], [0.3, 0.5, 0.45]]).to(dev))
    else:
        t, zs = torch.linspace(0.6, 1.8, S).repeat(B, 1) + 0.1 * torch.rand(B, S, generator=g), None
        cfg = ops.RenderCfg(S, ops.Z_PER_OBJECT, n, SB, TB, precision="fp32")
    ups = [torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)]
    return [None if x is None else x.to(dev) for x in (ro, rd, t, div, zs)] + [cfg] + [u.to(dev) for u in ups]


@pytest.mark.parametrize("n,box", [(7, False), (8, False), (9, False), (7, True)], ids=["7", "8", "9", "7-box-jitter"])
def test_fused_render(amd, dev, decoder, n, box):  # noqa: F811
    ops = amd.ops
    _, packed, lat0 = decoder
    ro0, rd0, t, div, zs, cfg, u_rgb, u_depth, u_acc = render_batch(ops, n, box, dev)
    ro, rd, lat = leaf(ro0), leaf(rd0), leaf(lat0)
    out = ops.FusedRender.apply(ro, rd, t, div, zs, lat, packed, cfg)
    n_pad, pad, strip = by_hand(ops, n, 32 // S)
    assert saved_rows(out[0]) == B * n_pad
    d_o, d_d, d_lat = torch.autograd.grad(out, (ro, rd, lat), (u_rgb, u_depth, u_acc))
    assert cfg.rays_per_obj == n and cfg.rng is None                        # (the caller's cfg is left alone)
    rp, dp, tp, zp, cp = ops.pad_render_inputs(ro0, rd0, t, zs, cfg, B, n, n_pad)
    assert cp.rays_per_obj == n_pad and tp.shape[0] == (B * n_pad if box else B)
    if box:                                                                 # the dummy rays' direction: any unit vector, never 0 / 0 in the slab test
        assert torch.equal(dp.view(B, n_pad, 3)[:, n:], torch.tensor([0.0, 0.0, 1.0], device=dev).expand(B, n_pad - n, 3))
    fw = ops.render_fwd(rp, dp, tp, div, zp, lat0, packed, cp, save_for_bwd=True)
    h_o, h_d, h_t, h_lat = ops.render_bwd(rp, dp, tp, div, zp, lat0, packed, cp, fw[3], fw[4], fw[5], pad(u_rgb), pad(u_depth), pad(u_acc))
    assert h_t is None
    same((n, box), (*out, d_o, d_d, d_lat), (strip(fw[0]), strip(fw[1]), strip(fw[2]), strip(h_o), strip(h_d), h_lat))
    assert bool(torch.isfinite(d_lat).all()) and bool(d_lat.any())


@pytest.mark.parametrize("n", [63, 64, 65])
def test_density_points(amd, dev, decoder, n):  # noqa: F811
    ops = amd.ops
    _, packed, lat0 = decoder
    xyz0, _, u, _ = point_batch(n, dev)
    xyz, lat = leaf(xyz0), leaf(lat0)
    sig = ops.DensityPoints.apply(xyz, lat, packed, SB, TB)
    n_pad, pad, strip = by_hand(ops, n, 64)
    assert saved_rows(sig) == B * n_pad
    d_xyz, d_lat = torch.autograd.grad(sig, (xyz, lat), u)
    xp = pad(xyz0)
    s, masks = ops.density_fwd(xp, lat0, packed, SB, TB, save_masks=True)
    h_lat, h_xyz = ops.density_bwd(xp, lat0, packed, masks, s, pad(u), SB, TB)
    same(n, (sig, d_xyz, d_lat), (strip(s), strip(h_xyz), h_lat))


@pytest.mark.parametrize("n", [63, 64, 65])
def test_ray_surface(amd, dev, decoder, n):  # noqa: F811
    """Rays through the decoder's fog, cut at its median density along them (hits, misses and inside starts all occur)."""
    ops = amd.ops
    _, packed, lat0 = decoder
    g = torch.Generator().manual_seed(300 + n)
    R = B * n
    o0 = ((torch.rand(R, 3, generator=g) - 0.5) * 1.2).to(dev)
    d0 = (torch.randn(R, 3, generator=g) * 0.7).to(dev)
    near, far = (-0.4 * torch.rand(R, generator=g)).to(dev), (0.2 + 0.6 * torch.rand(R, generator=g)).to(dev)
    u = torch.randn(R, generator=g).to(dev)
    level = float(ops.density_fwd(ops.ray_march_points(o0, d0, near, far, 16), lat0, packed, SB, TB)[0].median())
    search = (level, 32, 1, 5, SB, TB)
    o, d, lat = leaf(o0), leaf(d0), leaf(lat0)
    t, state, normal, width = ops.RaySurface.apply(o, d, near, far, lat, packed, *search)
    n_pad, pad, strip = by_hand(ops, n, 64)
    assert saved_rows(t, 5) == B * n_pad                                    # (the hit points x)
    d_o, d_d, d_lat = torch.autograd.grad(t, (o, d, lat), u)
    br = ops.ray_brackets(o0, d0, near, far, lat0, packed, *search)
    h_t, h_width, x = ops.ray_hit_points(o0, d0, *br, level)
    hit = br[4] == 1
    assert 0 < int(hit.sum()) < R
    xp = pad(x)
    s, masks = ops.density_fwd(xp, lat0, packed, SB, TB, save_masks=True)
    grad = strip(ops.density_bwd(xp, lat0, packed, masks, s, torch.ones_like(s), SB, TB, need_latent=False)[1])
    norm = grad.norm(dim=1, keepdim=True)
    good = hit[:, None] & torch.isfinite(norm) & (norm > 0)
    h_normal = torch.where(good, -grad / torch.where(good, norm, torch.ones_like(norm)), torch.zeros_like(grad))
    slope = grad[:, 0] * d0[:, 0] + grad[:, 1] * d0[:, 1] + grad[:, 2] * d0[:, 2]
    c = torch.where(hit, -u / slope, torch.zeros_like(u))
    h_lat, _ = ops.density_bwd(xp, lat0, packed, masks, s, pad(c), SB, TB, need_latent=True, need_xyz=False)
    same(n, (t, state, normal, width, d_o, d_d, d_lat), (h_t, br[4], h_normal, h_width, c[:, None] * grad, (h_t * c)[:, None] * grad, h_lat))
