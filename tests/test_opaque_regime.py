"""The kernels on a decoder that renders an opaque object in empty space (tests/planted_decoder.py), against the oracle in float64.

Every other decoder of the suite is a uniform fog; here the softplus threshold branch, subnormal and 1e-10 densities, saturated transmittance
and sharp surfaces are all on the path.  Gradients are mask-matched (tests/relu_bits.py): both oracles differentiate with the ReLU bits the
GPU forward saved.  Each bound is a band: C times the fp32 oracle's own distance from float64 on the same inputs (one sample of the rounding
noise of that quantity on this host), plus a floor, both relative to the tensor's largest float64 entry."""
import numpy as np
import pytest
import torch

import planted_decoder as PD
from oracle import supnerf_oracle as O
from oracle_bands import amd, band_of, check_all, dev, make_model  # noqa: F401  (amd, dev: fixtures)
from relu_bits import relu_bits_of

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ a. points decoder
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_points_decoder_opaque(amd, dev, precision):
    """sigma, rgb and the gradients wrt the points, directions and codes, with upstream d_sig of the composite's scale: 1e10 on the last
    sample of every ray (its interval is 1e10 wide; there sigma ~ 1e-10 on the pinned background)."""
    params = PD.planted_params(far_pre=PD.FAR_PRE, wobble=PD.WOBBLE)
    N, S, B = 64, 64, 2
    o, d, z = PD.box_rays(N, S, seed=5)
    xyz, vd = O.points_on_rays(o, d, z)
    g = torch.Generator().manual_seed(6)
    sc, tc = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    ws = torch.randn(N, S, 1, generator=g)
    ws[:, -1] *= 1e10
    wr = torch.randn(N, S, 3, generator=g)
    m = make_model(amd, dev, params, precision)
    leaves = [t.detach().to(dev).requires_grad_() for t in (xyz, vd, sc, tc)]
    sig, rgb = m(*leaves)
    masks = relu_bits_of(sig, 3, 1)
    ((sig * ws.to(dev)).sum() + (rgb * wr.to(dev)).sum()).backward()
    ref = {}
    for dt in (torch.float32, torch.float64):
        p = {k: v.to(dt) for k, v in params.items()}
        ins = [t.to(dt).clone().requires_grad_() for t in (xyz, vd, sc, tc)]
        s_o, r_o = O.decoder_forward(p, *ins, relu_masks=masks)
        ((s_o * ws.to(dt)).sum() + (r_o * wr.to(dt)).sum()).backward()
        ref[dt] = [s_o.detach(), r_o.detach()] + [t.grad for t in ins]
    got = [sig, rgb] + [t.grad for t in leaves]
    names = ["sigma", "rgb", "d_xyz", "d_viewdir", "d_shapecode", "d_texturecode"]
    assert float((ref[torch.float64][0] > 20).double().mean()) > 0.2 and float((ref[torch.float64][0] < 1e-7).double().mean()) > 0.2
    check_all([(n, a, b, c) for n, a, b, c in zip(names, got, ref[torch.float32], ref[torch.float64])], precision)


# ------------------------------------------------------------------ b. fused render
def oracle_render(params, o, d, t, mode, S, n, white, zs, half, sc, tc, masks, wts, dt):
    """The fused render on the oracle in dtype ``dt``; returns outputs and gradients wrt (rays_o, rays_d, t (per ray only), sc, tc)."""
    c = lambda x: x.to(dt)
    leaves = [c(x).clone().requires_grad_() for x in (o, d, t, sc, tc)]
    if mode != "per_ray":
        leaves[2] = c(t)
    out = O.fused_render({k: c(v) for k, v in params.items()}, *leaves[:3], mode, S, n, c(zs), c(half) if mode == "box" else None,
                         shape_code=leaves[3], texture_code=leaves[4], relu_masks=masks, white_bkgd=white, metric_z=mode in ("per_ray", "box"))
    sum((a * c(w)).sum() for a, w in zip(out, wts)).backward()
    return [x.detach() for x in out], [x.grad if x.requires_grad else None for x in leaves]


RENDER_CASES = [  # (z mode, S, objects, rays per object, white background)
    ("shared", 64, 1, 96, True), ("per_object", 32, 3, 48, False), ("per_ray", 128, 1, 64, True), ("per_ray", 8, 3, 64, False),
    ("box", 64, 1, 96, False), ("box", 32, 3, 40, True)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "auto"])
@pytest.mark.parametrize("case", RENDER_CASES, ids=lambda c: f"{c[0]}-S{c[1]}-B{c[2]}-{'white' if c[4] else 'black'}")
def test_fused_render_opaque(amd, dev, case, precision):
    ops = amd.ops
    mode, S, B, n, white = case
    params = PD.planted_params(far_pre=None)
    N = B * n
    o, d, z = PD.box_rays(N, S, seed=S + 7 * B)
    g = torch.Generator().manual_seed(S * B)
    sc, tc = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    zs = torch.ones(B)
    half = torch.tensor([h + PD.H for h in PD.HALF]).expand(B, 3).contiguous()
    if mode == "shared":
        t = torch.linspace(0.75, 2.25, S + 1)[:-1] + torch.rand(S, generator=g) * (1.5 / S)
    elif mode == "per_object":
        t = torch.linspace(0.75, 2.25, S + 1)[:-1][None] + torch.rand(B, S, generator=g) * (1.5 / S)
    elif mode == "per_ray":
        t = z
    else:
        t = torch.rand(N, S, generator=g)        # the box sampling's jitter table
    wts = [torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)]
    zmode = {"shared": ops.Z_SHARED, "per_object": ops.Z_PER_OBJECT, "per_ray": ops.Z_PER_RAY, "box": ops.Z_BOX}[mode]
    cfg = ops.RenderCfg(S, zmode, n, 3, 1, white_bkgd=white, metric_z=mode in ("per_ray", "box"),
                        box_half=half.to(dev) if mode == "box" else None)
    m = make_model(amd, dev, params, precision)
    leaves = [x.to(dev).requires_grad_() for x in (o, d, t, sc, tc)]
    if mode != "per_ray":
        leaves[2] = t.to(dev)
    out = m.fused_render(leaves[0], leaves[1], leaves[2], torch.ones(B, device=dev), zs.to(dev), leaves[3], leaves[4], cfg)
    if precision == "auto":
        assert m.last_precision["forward"] == "bf16x3", m.last_precision
    masks = relu_bits_of(out[0], 3, 1, n_samples=S)
    sum((a * w.to(dev)).sum() for a, w in zip(out, wts)).backward()
    (r32, g32), (r64, g64) = [oracle_render(params, o, d, t, mode, S, n, white, zs, half, sc, tc, masks, wts, dt)
                              for dt in (torch.float32, torch.float64)]
    assert float((r64[2] < 1e-6).double().mean()) > 0.3                     # opaque rays are there
    pairs = [(nm, a, b, c) for nm, a, b, c in zip(("rgb", "depth", "acc"), out, r32, r64)]
    grads = [leaves[0].grad, leaves[1].grad, leaves[2].grad if mode == "per_ray" else None, leaves[3].grad, leaves[4].grad]
    for nm, a, b, c in zip(("d_rays_o", "d_rays_d", "d_t", "d_shapecode", "d_texturecode"), grads, g32, g64):
        if c is not None:
            pairs.append((nm, a, b, c))
    check_all(pairs, band_of(precision))


@pytest.mark.parametrize("precision", ["fp32", "auto"])
@pytest.mark.parametrize("n,S", [(5, 8), (7, 32)])
def test_fused_render_opaque_forward_ragged_objects(amd, dev, n, S, precision):
    """Three objects whose points per object (40, 224) are no multiple of 64: the forward without code gradients runs unpadded and reads
    the latent terms per lane."""
    ops = amd.ops
    B = 3
    params = PD.planted_params(far_pre=None)
    o, d, z = PD.box_rays(B * n, S, seed=n * S)
    g = torch.Generator().manual_seed(n)
    sc, tc = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, n, 3, 1, white_bkgd=True, metric_z=True)
    m = make_model(amd, dev, params, precision)
    with torch.no_grad():
        out = m.fused_render(o.to(dev), d.to(dev), z.to(dev), torch.ones(B, device=dev), torch.ones(B, device=dev), sc.to(dev), tc.to(dev), cfg)
    refs = []
    for dt in (torch.float32, torch.float64):
        p = {k: v.to(dt) for k, v in params.items()}
        xyz, vd = O.points_on_rays(o.to(dt), d.to(dt), z.to(dt))
        sig, rgb = O.decoder_forward(p, xyz, vd, sc.to(dt), tc.to(dt))
        refs.append(O.composite(sig, rgb, torch.norm(xyz - o.to(dt)[:, None], dim=-1), white_bkgd=True))
    check_all([(nm, a, b, c) for nm, a, b, c in zip(("rgb", "depth", "acc"), out, refs[0], refs[1])], band_of(precision))


# ------------------------------------------------------------------ c. the far field
@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_far_field_gradients_family_a(amd, dev, golden, precision):
    """A family-A optimise iteration (render_rays_v2 + the reference's loss) through a small planted box whose background is pinned at
    pre ~ -23: on the rays that miss it the last, 1e10-wide interval has sigma ~ 1e-10 and an alpha of order 1, so softplus'(pre) ~ sigma
    carries an O(1) share of the code and pose gradients.  Rebuilding it as 1 - exp(-sigma) in fp32 gives 0 there (11 % of the shape code's
    gradient and 33 % of the pose's on these inputs)."""
    g = golden("grads_family_a")
    half, H = (0.1, 0.08, 0.06), 0.1
    params = PD.planted_params(half=half, H=H, far_pre=PD.FAR_PRE, wobble=PD.WOBBLE)
    m = make_model(amd, dev, params, precision)
    amd.utils.JITTER_OVERRIDE = g["jitter"]
    try:
        sc, tc, pose = [g[k].to(dev).requires_grad_() for k in ("shapecode", "texturecode", "cam_pose")]
        out = amd.utils.render_rays_v2(m, dev, g["img"], g["mask_occ"], pose, np.float32(g["obj_diag"]), g["K"], g["roi"], 64, sc, tc, 1, 0, im_sz=8)
    finally:
        amd.utils.JITTER_OVERRIDE = None
    masks = relu_bits_of(out[0], 3, 1, n_samples=64)
    O.optimise_losses(out[0], out[2], out[3], out[4], 0.1)[0].backward()
    ref = {}
    for dt in (torch.float32, torch.float64):
        c = lambda t: t.to(dt)
        p = {k: c(v) for k, v in params.items()}
        sc_o, tc_o, pose_o = [c(g[k]).clone().requires_grad_() for k in ("shapecode", "texturecode", "cam_pose")]
        with O.given_relu_masks(masks):
            r = O.render_rays_v2(p, c(g["img"]), c(g["mask_occ"]), pose_o, float(g["obj_diag"]), c(g["K"]), g["roi"], 64, sc_o, tc_o, True,
                                 im_sz=8, jitter=c(g["jitter"]))
            O.optimise_losses(r[0], r[2], r[3], r[4], 0.1)[0].backward()
        ref[dt] = [x.detach() for x in r[:3]] + [sc_o.grad, tc_o.grad, pose_o.grad]
    acc64 = ref[torch.float64][2]
    assert float((acc64 > 0.99).double().mean()) > 0.5 and float((acc64 < 1e-6).double().mean()) > 0.05     # mostly background
    got = list(out[:3]) + [sc.grad, tc.grad, pose.grad]
    names = ("rgb", "depth", "acc", "d_shapecode", "d_texturecode", "d_cam_pose")
    check_all([(nm, a, b, c) for nm, a, b, c in zip(names, got, ref[torch.float32], ref[torch.float64])], band_of(precision))


# ------------------------------------------------------------------ d. standalone composites with saturating inputs
def saturating_inputs(N, S, seed):
    """sigma * delta up to 1e3, sigma = 0 exactly, equal consecutive depths, and the 1e-10 background."""
    g = torch.Generator().manual_seed(seed)
    sig = torch.exp(torch.rand(N, S, generator=g, dtype=torch.float64) * 36 - 25)         # 1e-11 .. 1e5
    sig[torch.rand(N, S, generator=g) < 0.1] = 0.0
    sig[:, -1] = 1e-10
    z = torch.sort(torch.rand(N, S, generator=g, dtype=torch.float64) * 2 + 1, dim=-1)[0]
    z[:, 1::7] = z[:, 0::7][:, : z[:, 1::7].shape[1]]                                         # delta = 0
    z = torch.sort(z, dim=-1)[0]
    sig = torch.minimum(sig, 1e3 / (torch.cat([z[:, 1:] - z[:, :-1], torch.ones(N, 1, dtype=torch.float64)], -1) + 1e-3))
    rgbs = torch.rand(N, S, 3, generator=g, dtype=torch.float64)
    wts = [torch.randn(N, 3, generator=g, dtype=torch.float64), torch.randn(N, generator=g, dtype=torch.float64),
           torch.randn(N, generator=g, dtype=torch.float64)]
    return sig.float(), rgbs.float(), z.float(), [w.float() for w in wts]


@pytest.mark.parametrize("mode", ["shared", "per_object", "per_ray"])
@pytest.mark.parametrize("S", [2, 64, 65, 130, 256])
def test_composite_saturating(amd, dev, S, mode):
    ops = amd.ops
    N, B = 48, 3
    sig, rgbs, z, wts = saturating_inputs(N, S, S)
    zt = {"shared": z[0], "per_object": z[:: N // B], "per_ray": z}[mode]
    zmode = {"shared": ops.Z_SHARED, "per_object": ops.Z_PER_OBJECT, "per_ray": ops.Z_PER_RAY}[mode]
    for white in (True, False):
        lv = [sig.to(dev).requires_grad_(), rgbs.to(dev).requires_grad_(), zt.to(dev).requires_grad_(mode == "per_ray")]
        out = ops.Composite.apply(lv[0], lv[1], lv[2], zmode, white, N // B if mode == "per_object" else 0)
        sum((a.reshape(w.shape) * w.to(dev)).sum() for a, w in zip(out, wts)).backward()
        refs = []
        for dt in (torch.float32, torch.float64):
            s, r, zz = [x.to(dt).clone().requires_grad_() for x in (sig, rgbs, zt)]
            zb = {"shared": zz, "per_object": zz.repeat_interleave(N // B, 0), "per_ray": zz}[mode]
            o = O.composite(s, r, zb, white_bkgd=white)
            sum((a * w.to(dt)).sum() for a, w in zip(o, wts)).backward()
            refs.append([x.detach() for x in o] + [s.grad, r.grad, zz.grad if mode == "per_ray" else None])
        got = [x.reshape(y.shape) for x, y in zip(out, refs[1][:3])] + [lv[0].grad, lv[1].grad, lv[2].grad if mode == "per_ray" else None]
        names = ("rgb", "depth", "acc", "d_sigma", "d_rgbs", "d_z")
        check_all([(f"{nm} white={white}", a, b, c) for nm, a, b, c in zip(names, got, refs[0], refs[1]) if c is not None], "fp32")


@pytest.mark.parametrize("S", [2, 64, 65, 130, 256])
def test_scene_composite_saturating(amd, dev, S):
    P = 40
    sig, rgbs, z, _ = saturating_inputs(P, S, 100 + S)
    z = z[:, torch.randperm(S, generator=torch.Generator().manual_seed(S))]          # unsorted, with ties: the depth merge
    got = amd.ops.scene_composite(sig.to(dev), rgbs.to(dev), z.to(dev))
    r32 = O.scene_composite(sig, rgbs, z)
    r64 = O.scene_composite(sig.double(), rgbs.double(), z.double())
    check_all([(nm, a, b, c) for nm, a, b, c in zip(("rgb", "depth", "acc"), got, r32, r64)], "fp32")


# ------------------------------------------------------------------ e. loss tail
def test_loss_tail_tiny_transmittance(amd, dev):
    """acc_trans from 1e-30 (an opaque ray) to 1, every occupancy label."""
    ops = amd.ops
    B, n = 3, 64
    g = torch.Generator().manual_seed(9)
    acc = 10.0 ** -(torch.rand(B * n, generator=g) * 30)
    acc[::9] = 1.0
    rgb, tgt = torch.rand(B * n, 3, generator=g), torch.rand(B * n, 3, generator=g)
    occ = (torch.randint(0, 3, (B * n, 1), generator=g) - 1).float()
    a_d, r_d = acc.to(dev).requires_grad_(), rgb.to(dev).requires_grad_()
    loss, _ = ops.LossTail.apply(r_d, a_d, tgt.to(dev), occ.to(dev), 0.1, n)
    wl = torch.randn(B, generator=g)
    (loss * wl.to(dev)).sum().backward()
    refs = []
    for dt in (torch.float32, torch.float64):
        a, r = acc.to(dt).clone().requires_grad_(), rgb.to(dt).clone().requires_grad_()
        ls = torch.stack([O.optimise_losses(r[b * n:(b + 1) * n], a[b * n:(b + 1) * n], tgt.to(dt)[b * n:(b + 1) * n], occ.to(dt)[b * n:(b + 1) * n],
                                            0.1)[0] for b in range(B)])
        (ls * wl.to(dt)).sum().backward()
        refs.append([ls.detach(), r.grad, a.grad])
    check_all([(nm, x, y, z) for nm, x, y, z in zip(("loss", "d_rgb", "d_acc"), [loss, r_d.grad, a_d.grad], refs[0], refs[1])], "fp32")


# ------------------------------------------------------------------ f. training step sigma head
def test_training_sigma_head_gradients(amd, dev):
    """DecoderPointsTrain (fp32) on the planted decoder, composited with the 1e10 last interval: the sigma head's weight and bias
    gradients (ops.sigma_pre_grad) against float64."""
    params = PD.planted_params(far_pre=PD.FAR_PRE, wobble=PD.WOBBLE)
    B, n, S = 2, 32, 64
    o, d, z = PD.box_rays(B * n, S, seed=12)
    xyz, vd = O.points_on_rays(o, d, z)
    g = torch.Generator().manual_seed(13)
    sc, tc = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    wts = [torch.randn(B * n, 3, generator=g), torch.randn(B * n, generator=g), torch.randn(B * n, generator=g)]
    m = make_model(amd, dev, params, "fp32", train=True)
    sig, rgb = m(xyz.to(dev), vd.to(dev), sc.to(dev), tc.to(dev))
    masks = relu_bits_of(sig, 3, 1)
    out = O.composite(sig, rgb, z.to(dev), white_bkgd=False)
    sum((a * w.to(dev)).sum() for a, w in zip(out, wts)).backward()
    got = dict(m.named_parameters())
    refs = []
    for dt in (torch.float32, torch.float64):
        p = {k: v.to(dt).clone().requires_grad_() for k, v in params.items()}
        s, r = O.decoder_forward(p, xyz.to(dt), vd.to(dt), sc.to(dt), tc.to(dt), relu_masks=masks)
        o_ = O.composite(s, r, z.to(dt), white_bkgd=False)
        sum((a * w.to(dt)).sum() for a, w in zip(o_, wts)).backward()
        refs.append(p)
    names = ("sigma.0.weight", "sigma.0.bias", "encoding_shape.weight", "encoding_shape.bias")
    check_all([(k, got[k].grad, refs[0][k].grad, refs[1][k].grad) for k in names], "fp32")


# ------------------------------------------------------------------ g. render at other block counts
@pytest.mark.parametrize("blocks,precision", [((2, 1), "fp32"), ((2, 1), "bf16x3"), ((0, 0), "fp32"), ((0, 0), "bf16x3"),
                                              ((4, 4), "fp32"), ((5, 5), "fp32")])
def test_fused_render_other_block_counts(amd, dev, blocks, precision):
    ops = amd.ops
    sb, tb = blocks
    params = PD.planted_params(sb, tb, far_pre=PD.FAR_PRE if sb else None, wobble=PD.WOBBLE)
    B, n, S = 2, 32, 64
    N = B * n
    o, d, z = PD.box_rays(N, S, seed=sb * 10 + tb)
    g = torch.Generator().manual_seed(sb + 5 * tb)
    sc, tc = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    wts = [torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)]
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, n, sb, tb, white_bkgd=True, metric_z=True)
    m = make_model(amd, dev, params, precision, blocks)
    leaves = [x.to(dev).requires_grad_() for x in (o, d, z, sc, tc)]
    out = m.fused_render(leaves[0], leaves[1], leaves[2], torch.ones(B, device=dev), torch.ones(B, device=dev), leaves[3], leaves[4], cfg)
    masks = relu_bits_of(out[0], sb, tb, n_samples=S)
    sum((a * w.to(dev)).sum() for a, w in zip(out, wts)).backward()
    (r32, g32), (r64, g64) = [oracle_render(params, o, d, z, "per_ray", S, n, True, torch.ones(B), None, sc, tc, masks, wts, dt)
                              for dt in (torch.float32, torch.float64)]
    pairs = [(nm, a, b, c) for nm, a, b, c in zip(("rgb", "depth", "acc"), out, r32, r64)]
    for nm, a, b, c in zip(("d_rays_o", "d_rays_d", "d_t", "d_shapecode", "d_texturecode"), [x.grad for x in leaves], g32, g64):
        if (nm == "d_shapecode" and sb == 0) or (nm == "d_texturecode" and tb == 0):
            continue
        pairs.append((nm, a, b, c))
    check_all(pairs, precision)


# ------------------------------------------------------------------ h. auto on a sharp decoder
@pytest.mark.parametrize("far_pre", [None, pytest.param(PD.FAR_PRE, marks=pytest.mark.xfail(strict=True, reason=(
    "range guard false positive: no weight or activation leaves the fp16 range, but with the background at pre ~ -23 the 1e10-wide last "
    "interval turns an absolute error in pre into alpha at dalpha/dpre ~ 0.37, and pre = K (...) with K = 300 carries K * 2^-22 * |terms| "
    "~ 1e-4 of the split forward's rounding -- above RANGE_TOL = 1e-5 on rgb; the guard measures conditioning here, not range")))])
def test_auto_keeps_the_split_kernels_on_a_sharp_decoder(amd, dev, far_pre):
    """The range guard of 'auto' compares the split forward with the exact one; a sharp but healthy decoder must pass it."""
    ops = amd.ops
    params = PD.planted_params(far_pre=far_pre, wobble=PD.WOBBLE if far_pre else 0.0)
    B, n, S = 1, 256, 64
    o, d, z = PD.box_rays(n, S, seed=21)
    m = make_model(amd, dev, params, "auto")
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, n, 3, 1, white_bkgd=True, metric_z=True)
    sc, tc = torch.zeros(B, 256, device=dev), torch.zeros(B, 256, device=dev)
    with torch.no_grad():
        m.fused_render(o.to(dev), d.to(dev), z.to(dev), torch.ones(B, device=dev), torch.ones(B, device=dev), sc, tc, cfg)
    assert m.last_precision["forward"] == "bf16x3" and m.last_precision["backward"] == "bf16x3", m.last_precision
