"""The exact-fp32 fused render forward sums enc_viewdir's direction chunk once per RAY when a workgroup is one ray (csrc/snr_mlp16.hip:
layer_from_acc, the `once` form: S = 64 on the four-wave shape, S = 128 on the eight-wave shape), and once per POINT everywhere else.

Both forms must give every point the same bits: the same MFMAs on the same operands in the same order, only not repeated in every column.
A point's sigma and rgb do not depend on how many samples the launch puts on a ray, so the same rays rendered as S = 32 launches (two or
four rays per workgroup: the per-point form, in the same binary) are the reference, point by point and ReLU bit by ReLU bit.  A wrong tile,
a wrong row of the chunk or a write-back into the wrong slot of the bias row is deterministic and shows on one ray, so the shapes are the
smallest that reach every path: 1 .. 3 rays, two objects, both launch shapes, with and without the tensors the backward needs.  The float64
oracle (tests/oracle_bands.py) then holds the values themselves, and the backward on what the changed forward saved."""
import pytest
import torch

from oracle import supnerf_oracle as O
from oracle_bands import amd, check_all, dev  # noqa: F401  (amd, dev: fixtures)
from relu_bits import decode_relu_bits

pytestmark = pytest.mark.gpu

BLOCKS = [(3, 1), (1, 0), (0, 0)]
# (objects, rays per object)
BATCHES = [(1, 1), (1, 2), (1, 3), (2, 2)]

# neighbouring rays differ; the first is axis-parallel with a -0.0 (and a +0.0) component, the second has one zero component
_DIRS = torch.tensor([[0.0, -0.0, 1.0], [0.3, 0.0, 0.95], [-0.15, 0.25, 0.9], [0.2, -0.3, 1.1]])


def _decoder(amd, dev, sb, tb):
    params = O.init_decoder_params(sb, tb, seed=10 * sb + tb)
    return params, amd.ops.pack_weights({k: v.to(dev) for k, v in params.items()}, sb, tb)


def _latent(params, sb, tb, B, g):
    sc, tc = torch.randn(B, 256, generator=g) * 0.3, torch.randn(B, 256, generator=g) * 0.3
    return O.latent_terms(params, sc, tc) if sb + tb else torch.zeros(B, 1, 256)


def _rays(N, S, g):
    """N rays towards the object from z = -1.2, per-ray depths (N, S) in [0.5, 2)."""
    o = (torch.rand(N, 3, generator=g) - 0.5) * 0.2 - torch.tensor([0.0, 0.0, 1.2])
    d = _DIRS[:N].clone()
    d[1:] = torch.nn.functional.normalize(d[1:], dim=1)          # (row 0 is a unit vector already; normalising it would turn -0.0 into +0.0)
    t = torch.linspace(0.5, 2.0, S + 1)[:-1][None] + torch.rand(N, S, generator=g) * (1.5 / S)
    return o, d, t


def _per_point(ops, dev, o, d, t, lat, packed, S, rays_per_obj, sb, tb):
    """sigma (N, S), rgbs (N, S, 3), ReLU bits per layer (N, S, width) of ONE launch with S samples per ray, and its (rgb, depth, acc)."""
    N = o.shape[0]
    one = torch.ones(lat.shape[0])
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, rays_per_obj, sb, tb, white_bkgd=True, metric_z=True, precision="fp32")
    out = ops.render_fwd(*[x.to(dev) for x in (o, d, t.contiguous(), one, one, lat)], packed, cfg, save_for_bwd=True)
    bits = [b.reshape(N, S, -1) for b in decode_relu_bits(out[5], N * S, sb, tb)]
    return out[3].cpu().reshape(N, S), out[4].cpu().reshape(N, S, 3), bits, [x.cpu() for x in out[:3]]


def _in_pieces(ops, dev, o, d, t, lat, packed, rays_per_obj, sb, tb):
    """The same points from S = 32 launches (the per-point form): slices 0:32, 32:64, .. of the depth table, joined ray by ray."""
    parts = [_per_point(ops, dev, o, d, t[:, k:k + 32], lat, packed, 32, rays_per_obj, sb, tb)[:3] for k in range(0, t.shape[1], 32)]
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), [torch.cat(ls, 1) for ls in zip(*[p[2] for p in parts])]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("S", [64, 128])
def test_once_per_ray_is_once_per_point(amd, dev, blocks, batch, S):
    """Saved per-point sigma, rgbs and ReLU bits of a one-ray-per-workgroup launch against S = 32 launches of the same rays; and the launch
    without the saved tensors (the other instantiation) returns the same rgb, depth, acc."""
    ops = amd.ops
    sb, tb = blocks
    B, n = batch
    N = B * n
    params, packed = _decoder(amd, dev, sb, tb)
    g = torch.Generator().manual_seed(1000 * S + 100 * sb + 10 * tb + N)
    o, d, t = _rays(N, S, g)
    lat = _latent(params, sb, tb, B, g)
    if B > 1 and sb + tb:
        assert not torch.equal(lat[0], lat[1])
    sig, rgbs, bits, comp = _per_point(ops, dev, o, d, t, lat, packed, S, n, sb, tb)
    sig32, rgbs32, bits32 = _in_pieces(ops, dev, o, d, t, lat, packed, n, sb, tb)
    assert bool(torch.isfinite(sig).all()) and bool(torch.isfinite(rgbs).all())
    for r in range(N):
        assert torch.equal(sig[r], sig32[r]), (blocks, batch, S, "sigma of ray", r)
        assert torch.equal(rgbs[r], rgbs32[r]), (blocks, batch, S, "rgbs of ray", r)
        for layer, (a, b) in enumerate(zip(bits, bits32)):
            assert torch.equal(a[r], b[r]), (blocks, batch, S, "ReLU bits of ray", r, "layer", layer)
    one = torch.ones(B)
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, n, sb, tb, white_bkgd=True, metric_z=True, precision="fp32")
    plain = ops.render_fwd(*[x.to(dev) for x in (o, d, t, one, one, lat)], packed, cfg)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(plain[:3], comp)), (blocks, batch, S, "the forward with ReLU bits is not the forward without")


def _against_oracle(ops, dev, params, packed, ins, cfg, z_mode, S, N, wts, want_t, **oracle_kw):
    """render_fwd + render_bwd on (o, d, t, xyz_div, z_scale, latent) against the oracle in fp32 and float64 on the saved ReLU bits."""
    o, d, t, _, zs, lat = ins
    dev_ins = [None if x is None else x.to(dev) for x in ins]
    out = ops.render_fwd(*dev_ins, packed, cfg, save_for_bwd=True)
    plain = ops.render_fwd(*dev_ins, packed, cfg)
    assert all(torch.equal(a, b) for a, b in zip(plain[:3], out[:3]))
    sig, rgbs, masks = out[3:]
    d_o, d_d, d_t, d_lat = ops.render_bwd(*dev_ins, packed, cfg, sig, rgbs, masks, *[w.to(dev) for w in wts], need_t=want_t, need_latent=True)
    bits = decode_relu_bits(masks, N * S, cfg.shape_blocks, cfg.texture_blocks)
    refs = []
    for dt in (torch.float32, torch.float64):
        c = lambda x: x.to(dt)
        leaves = [c(x).clone().requires_grad_() for x in (o, d, lat)]
        tt = c(t).clone().requires_grad_(want_t)
        kw = {k: c(v) for k, v in oracle_kw.items() if torch.is_tensor(v)}
        kw.update({k: v for k, v in oracle_kw.items() if not torch.is_tensor(v)})
        r = O.fused_render({k: c(v) for k, v in params.items()}, leaves[0], leaves[1], tt, z_mode, S, N, c(zs), latent=leaves[2], relu_masks=bits, **kw)
        sum((a * c(w)).sum() for a, w in zip(r, wts)).backward()
        refs.append([x.detach() for x in r] + [leaves[0].grad, leaves[1].grad, tt.grad, leaves[2].grad])
    got = list(out[:3]) + [d_o, d_d, d_t, d_lat]
    names = ["rgb", "depth", "acc", "d_rays_o", "d_rays_d", "d_t", "d_latent"]
    check_all([(nm, a, b, c) for nm, a, b, c in zip(names, got, refs[0], refs[1]) if a is not None], "fp32")
    return out


def test_box_render_against_float64(amd, dev):
    """Family B (box sampling, white background, metric depth) at S = 64, three rays of which the last misses the box; backward on what
    the forward saved."""
    ops = amd.ops
    sb, tb, S, N = 3, 1, 64, 3
    params, packed = _decoder(amd, dev, sb, tb)
    g = torch.Generator().manual_seed(64)
    o = torch.tensor([[0.05, -0.04, -1.5], [-0.06, 0.03, -1.4], [0.02, 0.05, -1.5]])
    d = torch.nn.functional.normalize(torch.tensor([[0.05, 0.08, 1.0], [-0.1, 0.04, 1.0], [1.0, 0.2, 0.3]]), dim=1)
    jit = torch.rand(N, S, generator=g)
    half, zs = torch.tensor([[0.4, 0.5, 0.45]]), torch.tensor([1.3])
    hit = O.slab_intersect(o / zs, d, -half.expand(N, 3), half.expand(N, 3))[2]
    assert hit.tolist() == [True, True, False]
    lat = _latent(params, sb, tb, 1, g)
    wts = [torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)]
    cfg = ops.RenderCfg(S, ops.Z_BOX, N, sb, tb, white_bkgd=True, metric_z=True, precision="fp32", box_half=half.to(dev))
    _against_oracle(ops, dev, params, packed, (o, d, jit, None, zs, lat), cfg, "box", S, N, wts, False, box_half=half, white_bkgd=True, metric_z=True)


def test_shared_depths_against_float64(amd, dev):
    """Family A (one depth table for every ray) at S = 64, three rays; backward on what the forward saved."""
    ops = amd.ops
    sb, tb, S, N = 3, 1, 64, 3
    params, packed = _decoder(amd, dev, sb, tb)
    g = torch.Generator().manual_seed(65)
    o, d, t = _rays(N, S, g)
    lat = _latent(params, sb, tb, 1, g)
    wts = [torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)]
    one = torch.ones(1)
    cfg = ops.RenderCfg(S, ops.Z_SHARED, N, sb, tb, precision="fp32")
    _against_oracle(ops, dev, params, packed, (o, d, t[0].contiguous(), one, one, lat), cfg, "shared", S, N, wts, False)


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_direction_stays_in_its_ray(amd, dev, S, bad):
    """One ray of three has a non-finite direction component: the other rays are bit for bit those of a launch without it, and the poisoned
    ray's per-point outputs are the per-point form's, compared as bit patterns."""
    ops = amd.ops
    sb, tb, N = 3, 1, 3
    params, packed = _decoder(amd, dev, sb, tb)
    g = torch.Generator().manual_seed(S + 7)
    o, d, t = _rays(N, S, g)
    lat = _latent(params, sb, tb, 1, g)
    d_bad = d.clone()
    d_bad[1, 0] = bad
    clean = _per_point(ops, dev, o, d, t, lat, packed, S, N, sb, tb)
    sig, rgbs, bits, comp = _per_point(ops, dev, o, d_bad, t, lat, packed, S, N, sb, tb)
    for r in (0, 2):
        assert torch.equal(sig[r], clean[0][r]) and torch.equal(rgbs[r], clean[1][r]), (S, bad, "per-point outputs of ray", r)
        assert all(torch.equal(a[r], b[r]) for a, b in zip(bits, clean[2])), (S, bad, "ReLU bits of ray", r)
        assert all(torch.equal(a[r], b[r]) for a, b in zip(comp, clean[3])), (S, bad, "rgb, depth, acc of ray", r)
    sig32, rgbs32, bits32 = _in_pieces(ops, dev, o, d_bad, t, lat, packed, N, sb, tb)
    assert _same_bits(sig, sig32) and _same_bits(rgbs, rgbs32), (S, bad, "the poisoned ray's per-point outputs")
    assert all(torch.equal(a, b) for a, b in zip(bits, bits32)), (S, bad, "ReLU bits")
