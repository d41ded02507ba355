"""The density-only backward on the MI355X: the ReLU bits of the density forward against the full forward's, the density backward against the
full fp32 backward at a zero colour gradient (bit for bit), ``geometry.density``'s gradients against float64 autograd of the oracle, normals of
the planted box against their closed form, vertex colours against the decoder forward, and the guard against silently missing weight
gradients."""
import pytest
import torch

from geometry_cases import BOUND_BOX, LEVEL_BOX, box, codes as _codes, model as _model, points as _points
from oracle import supnerf_oracle as O
from oracle_bands import amd, dev, in_band  # noqa: F401  (fixtures)
from planted_decoder import HALF
from relu_bits import decode_relu_bits

pytestmark = pytest.mark.gpu

BLOCKS = [(0, 0), (0, 3), (3, 1), (5, 5), (8, 8)]


@pytest.mark.parametrize("blocks", BLOCKS)
def test_density_masks_and_backward_are_the_full_kernels(amd, dev, blocks):  # noqa: F811
    """snr_density_fwd_masks: sigma of snr_density_fwd and the encoding_xyz / shape-layer bits of snr_decoder_fwd.  snr_density_bwd: d_xyz and
    the shape rows of d_latent of snr_decoder_bwd with d_rgbs = 0, bit for bit (torch.equal: zeros of either sign are equal); texture rows 0."""
    ops = amd.ops
    sb, tb = blocks
    model = _model(amd, dev, sb, tb, seed=sb * 10 + tb + 1)
    packed = model.packed_weights()
    for B in (1, 3):
        sc = _codes(B, 3 + B, dev)
        lat = model.latent_terms(sc, torch.zeros_like(sc)).detach()
        for ppo in (1, 33, 1000, 128):
            P = B * ppo
            xyz, vd, g = _points(P, 1000 * B + ppo, dev)
            tag = (blocks, B, ppo)
            sig0, _ = ops.density_fwd(xyz, lat, packed, sb, tb)
            sig, masks = ops.density_fwd(xyz, lat, packed, sb, tb, save_masks=True)
            assert masks.numel() == amd._lib.lib().snr_mask_bytes(P, sb, tb)
            assert torch.equal(sig, sig0), tag
            sf, _, mf = ops.decoder_fwd(xyz, vd, lat, packed, sb, tb, save_masks=True, precision="fp32")
            assert torch.equal(sig, sf), tag
            bd, bf = decode_relu_bits(masks, P, sb, tb), decode_relu_bits(mf, P, sb, tb)
            for s in range(sb + 1):                                   # encoding_xyz, shape layers 1..sb
                assert torch.equal(bd[s], bf[s]), (tag, s)

            d_sig = torch.randn(P, generator=g).to(dev)
            want_lat = ppo % 64 == 0
            dl, dx = ops.density_bwd(xyz, lat, packed, masks, sig, d_sig, sb, tb, need_latent=want_lat)
            fl, fx, _ = ops.decoder_bwd(xyz, vd, lat, packed, mf, sf, d_sig, torch.zeros(P, 3, device=dev), sb, tb,
                                        need_latent=want_lat, need_dir=False, precision="fp32")
            assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0, tag
            assert torch.equal(dx, fx), (tag, float((dx - fx).abs().max()))
            if want_lat:
                assert dl.shape == lat.shape
                if sb + tb:
                    assert torch.equal(dl[:, :sb], fl[:, :sb]), (tag, float((dl[:, :sb] - fl[:, :sb]).abs().max()))
                    assert sb == 0 or float(dl[:, :sb].abs().max()) > 0, tag
                assert bool((dl[:, sb:] == 0).all()), tag
            else:
                assert dl is None


def test_density_bwd_c_abi_checks(amd, dev):  # noqa: F811
    """The latent gradient needs whole 64-point workgroups per object (SNR_E_UNSUPPORTED), a workspace (SNR_E_WORKSPACE); d_xyz alone takes
    any point count."""
    ops, lib = amd.ops, amd._lib.lib()
    model = _model(amd, dev, 3, 1, seed=4)
    packed = model.packed_weights()
    sc = _codes(2, 9, dev)
    lat = model.latent_terms(sc, torch.zeros_like(sc)).detach().contiguous()
    xyz, _, _ = _points(2 * 96, 5, dev)
    sig, masks = ops.density_fwd(xyz, lat, packed, 3, 1, save_masks=True)
    ones = torch.ones_like(sig)
    d_lat, d_xyz = torch.empty_like(lat), torch.empty_like(xyz)
    ws_bytes = lib.snr_decoder_bwd_ws_bytes(xyz.shape[0], 96, 3, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    p = ops._p
    st = ops._stream(dev)
    args = (p(xyz), p(lat), p(packed), p(masks), p(sig), p(ones), xyz.shape[0], 96, 3, 1)
    assert lib.snr_density_bwd(*args, p(d_lat), p(d_xyz), p(ws), ws_bytes, st) == -5             # 96 % 64
    assert lib.snr_density_bwd(*args[:7], 95, 3, 1, None, p(d_xyz), p(ws), ws_bytes, st) == -2   # 192 % 95
    assert lib.snr_density_bwd(*args[:5], None, *args[6:], None, p(d_xyz), p(ws), ws_bytes, st) == -1
    assert lib.snr_density_bwd(*args, None, p(d_xyz), None, 0, st) == 0
    torch.cuda.synchronize()
    _, ref = ops.density_bwd(xyz, lat, packed, masks, sig, ones, 3, 1, need_latent=False)
    assert torch.equal(d_xyz, ref)
    xyz2, _, _ = _points(2 * 128, 6, dev)
    sig2, masks2 = ops.density_fwd(xyz2, lat, packed, 3, 1, save_masks=True)
    a2 = (p(xyz2), p(lat), p(packed), p(masks2), p(sig2), p(torch.ones_like(sig2)), xyz2.shape[0], 128, 3, 1)
    assert lib.snr_density_bwd(*a2, p(d_lat), None, None, 0, st) == -3
    assert lib.snr_density_fwd_masks(p(xyz2), p(lat), p(packed), xyz2.shape[0], 128, 3, 1, p(sig2), None, st) == -1
    assert lib.snr_density_fwd_masks(p(xyz2), p(lat), p(packed), xyz2.shape[0], 128, 9, 1, p(sig2), p(masks2), st) == -1
    torch.cuda.synchronize()


def _oracle_grads(params64, xyz, sc, w, layers, dtype):
    x = xyz.detach().cpu().to(dtype).view(-1, 1, 3).requires_grad_()
    s = sc.detach().cpu().to(dtype).requires_grad_()
    p = {k: v.to(dtype) for k, v in params64.items()}
    vd = torch.zeros_like(x)
    with O.given_relu_masks(layers):
        sig, _ = O.decoder_forward(p, x, vd, s, torch.zeros_like(s))
    (sig.view(-1) * w.cpu().to(dtype)).sum().backward()
    return sig.detach().view(-1), x.grad.view(-1, 3), s.grad


@pytest.mark.parametrize("blocks", [(3, 1), (5, 5), (1, 0)])
def test_density_gradients_against_float64(amd, dev, blocks):  # noqa: F811
    """geometry.density + backward: d xyz and d shapecode within the fp32 band of float64 autograd of the oracle's sigma, mask-matched on the
    kernel's ReLU bits (the texture-branch slots from a full forward on the same points: sigma does not read them).  Ragged objects (33,
    1000 points) go through the 64-point padding."""
    from supnerf_amd import geometry as G
    ops = amd.ops
    sb, tb = blocks
    model = _model(amd, dev, sb, tb, seed=40 + sb)
    params64 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    packed = model.packed_weights()
    for B, ppo in ((3, 33), (3, 1000), (1, 128), (2, 64)):
        P = B * ppo
        sc = _codes(B, 60 + ppo, dev)
        xyz, vd, g = _points(P, 7 * ppo + B, dev)
        w = torch.randn(P, generator=g).to(dev)
        xk, sk = xyz.clone().requires_grad_(), sc.clone().requires_grad_()
        sig = G.density(model, xk, sk)
        assert torch.equal(sig.detach(), G.query_density(model, xyz, sc))
        (sig * w).sum().backward()
        lat = model.latent_terms(sc, torch.zeros_like(sc)).detach()
        _, masks = ops.density_fwd(xyz, lat, packed, sb, tb, save_masks=True)
        _, _, mf = ops.decoder_fwd(xyz, vd, lat, packed, sb, tb, save_masks=True, precision="fp32")
        bd, bf = decode_relu_bits(masks, P, sb, tb), decode_relu_bits(mf, P, sb, tb)
        layers = [m.double() for m in bd[:sb + 1] + bf[sb + 1:]]
        _, gx64, gs64 = _oracle_grads(params64, xyz, sc, w, layers, torch.float64)
        _, gx32, gs32 = _oracle_grads(params64, xyz, sc, w, [m.float() for m in layers], torch.float32)
        tag = f"{blocks} B={B} ppo={ppo}"
        ok, _, msg = in_band(xk.grad, gx32, gx64, "fp32", "d_xyz " + tag)
        assert ok, msg
        if sb:
            ok, _, msg = in_band(sk.grad, gs32, gs64, "fp32", "d_shapecode " + tag)
            assert ok, msg
        else:
            assert sk.grad is None or float(sk.grad.abs().max()) == 0.0


def _box(amd, dev, sb):  # noqa: F811
    from supnerf_amd import geometry as G
    model = box(amd, dev, sb, 1, seed=sb)
    sc = _codes(2, 20 + sb, dev)
    meshes = G.extract_mesh(model, sc, level=LEVEL_BOX, resolution=96, bound=BOUND_BOX)
    return model, sc, meshes


@pytest.mark.parametrize("sb", [1, 3, 5])
def test_planted_box_normals(amd, dev, sb):  # noqa: F811
    """On the planted box the surface is d1 = H with d1 = sum_a relu(|x_a| - h_a): away from the kinks the outward normal is s / |s|,
    s_a = sign(x_a) [|x_a| > h_a].  Everywhere it agrees with the winding of extract_mesh (positive dot with the area-weighted face normal)."""
    from supnerf_amd import geometry as G
    model, sc, meshes = _box(amd, dev, sb)
    normals = G.vertex_normals(model, meshes, sc)
    assert len(normals) == 2
    half = torch.tensor(HALF, dtype=torch.float64)
    for (v, f), n in zip(meshes, normals):
        assert n.shape == v.shape and n.dtype == torch.float32 and n.is_cuda
        n64, v64 = n.cpu().double(), v.cpu().double()
        assert float((n64.norm(dim=1) - 1).abs().max()) < 1e-6
        gap = v64.abs() - half
        s = torch.sign(v64) * (gap > 0).double()
        want = s / s.norm(dim=1, keepdim=True)
        away = (gap.abs() > 2e-3).all(dim=1)
        assert int(away.sum()) > v.shape[0] // 2
        ang = torch.acos((n64[away] * want[away]).sum(1).clamp(-1, 1))
        assert float(ang.max()) < 1e-3, float(ang.max())
        fn = G.face_normal_sums(v, f).cpu().double()
        dots = (n64 * fn).sum(1)
        assert bool((dots > 0).all()), int((dots <= 0).sum())
        # density_gradient on the same points: sigma is query_density's; the normals are its normalised negative
        sig, grad = G.density_gradient(model, v, sc[:1])
        assert torch.equal(sig, G.query_density(model, v, sc[:1]))
        assert torch.equal(n, -grad / grad.norm(dim=1, keepdim=True))
    # the face-normal fallback: a vertex where the gradient vanishes (the box centre: every one of the planted units is off there)
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], device=dev)
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    n, = G.vertex_normals(model, [(v, f)], sc[:1])
    assert torch.equal(n[0].cpu(), torch.tensor([0.0, 0.0, 1.0]))


def test_vertex_colors_are_the_decoder_forward(amd, dev):  # noqa: F811
    """vertex_colors: the exact fp32 decoder forward at the vertices with view direction -normal, bit for bit, and within the fp32 band of
    the float64 oracle's rgb."""
    from supnerf_amd import geometry as G
    model, sc, meshes = _box(amd, dev, 3)
    tc = _codes(2, 77, dev)
    normals = G.vertex_normals(model, meshes, sc)
    cols = G.vertex_colors(model, meshes, normals, sc, tc)
    with torch.no_grad():
        lat = model.latent_terms(sc, tc)
    params64 = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    for b, ((v, _), n, c) in enumerate(zip(meshes, normals, cols)):
        _, rgb, _ = amd.ops.decoder_fwd(v, -n, lat[b:b + 1], model.packed_weights(), 3, 1, precision="fp32")
        assert c.shape == v.shape and torch.equal(c, rgb)
        x, d = v.cpu().view(-1, 1, 3), (-n).cpu().view(-1, 1, 3)
        o64 = O.decoder_forward(params64, x.double(), d.double(), sc[b:b + 1].cpu().double(), tc[b:b + 1].cpu().double())[1].view(-1, 3)
        o32 = O.decoder_forward({k: t.float() for k, t in params64.items()}, x, d, sc[b:b + 1].cpu(), tc[b:b + 1].cpu())[1].view(-1, 3)
        ok, _, msg = in_band(c, o32, o64, "fp32", f"rgb obj {b}")
        assert ok, msg


def test_density_has_no_silent_weight_gap(amd, dev):  # noqa: F811
    """geometry.density differentiates points and codes only: with train_decoder_weights and grad mode it raises; under no_grad (and with
    constant weights under grad) it returns query_density's values."""
    from supnerf_amd import geometry as G
    model = _model(amd, dev, 3, 1, seed=8)
    sc = _codes(2, 12, dev)
    xyz, _, _ = _points(2 * 40, 13, dev)
    ref = G.query_density(model, xyz, sc)
    assert torch.equal(G.density(model, xyz, sc), ref)
    model.train_decoder_weights = True
    with pytest.raises(amd.SnrError):
        G.density(model, xyz, sc)
    with pytest.raises(amd.SnrError):
        G.density(model, xyz.clone().requires_grad_(), sc)
    with torch.no_grad():
        assert torch.equal(G.density(model, xyz, sc), ref)
