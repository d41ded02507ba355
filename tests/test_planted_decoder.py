"""The planted opaque decoder (tests/planted_decoder.py) on the CPU: the float64 oracle shows that it reaches the regime the GPU tests of
tests/test_opaque_regime.py rely on -- asserted here, so that it is never assumed -- and the torch sigma-head derivative of the training step
against autograd."""
import torch
import torch.nn.functional as F

import planted_decoder as PD
from oracle import supnerf_oracle as O

N_RAYS, S = 512, 64


def _render64(far_pre, blocks=(3, 1), n_rays=N_RAYS, wobble=0.0):
    p = {k: v.double() for k, v in PD.planted_params(*blocks, far_pre=far_pre, wobble=wobble).items()}
    o, d, z = PD.box_rays(n_rays, S, seed=1, dtype=torch.float64)
    xyz, vd = O.points_on_rays(o, d, z)
    g = torch.Generator().manual_seed(3)
    sc, tc = [torch.randn(1, 256, generator=g, dtype=torch.float64) * 0.3 for _ in range(2)]
    sig, rgb = O.decoder_forward(p, xyz, vd, sc, tc)
    return o, d, z, xyz, sig[..., 0], O.composite(sig, rgb, z)


def _pre_of(sig):
    """Inverse of softplus in float64 (exact enough wherever sigma is a normal number)."""
    return sig + torch.log(-torch.expm1(-sig))


def test_planted_decoder_computes_the_planted_density():
    """sigma = softplus(K (H - d1)) at every point, for the block counts the GPU tests render (the identity carry through every shape
    layer, none at all for 0 shape blocks)."""
    for blocks in ((3, 1), (0, 0), (2, 1), (5, 5)):
        _, _, _, xyz, sig, _ = _render64(None, blocks, n_rays=64)
        want = F.softplus(PD.analytic_pre(xyz))
        # (the planted constants are fp32: K * rounding of h and H moves pre by ~6e-6)
        assert ((sig - want).abs() <= 1e-4 * want + 1e-300).all(), blocks


def test_planted_decoder_reaches_the_opaque_regime():
    o, d, z, xyz, sig, (rgb, depth, acc) = _render64(None)
    pre = PD.analytic_pre(xyz)
    frac = lambda m: float(m.double().mean())
    assert frac(pre > 20) > 0.3                                  # the softplus threshold branch
    assert frac(sig < 1e-7) > 0.3                                # where 1 - exp(-sigma) is 0 in fp32
    assert frac((sig > 0) & (sig < 1e-30)) > 0.1                 # subnormal in fp32 (and the deep tail underflows to 0)
    assert frac((pre > -30) & (pre < -20)) > 0.01                # the window where sigmoid(pre) ~ sigma carries the last interval
    assert frac((sig > 1e-6) & (sig < 20)) > 0.05                # the surface shell
    assert frac(acc < 1e-6) > 0.6                                # opaque rays (transmittance saturates at products of 1e-10)
    assert frac(acc > 0.99) > 0.15                               # empty rays
    # the rendered depth of an opaque ray lies within one sample spacing of where the continuous density stops it
    op = acc < 1e-6
    dc, Tc = PD.continuous_depth(o, d)
    assert float(Tc[op].max()) < 1e-6
    assert float((depth[op] - dc[op]).abs().max()) < 1.5 / S


def test_planted_far_field_is_pinned():
    """With the clamp the background sits at pre = -23 (sigma ~ 1e-10): every sample outside the clamp distance, i.e. every sample of the
    rays that miss the box, is in the window, and the last, 1e10-wide interval gives those rays an alpha of order 1.  The wobble keeps a
    gradient of pre wrt the points and codes there (tests/test_opaque_regime.py's far-field case) and stays inside +-0.5."""
    far = PD.FAR_PRE
    o, d, z, xyz, sig, (rgb, depth, acc) = _render64(far, wobble=PD.WOBBLE)
    D = PD.H - far / PD.K
    d1 = torch.relu(xyz.abs() - torch.tensor(PD.HALF, dtype=torch.float64)).sum(-1)
    pre = _pre_of(sig)
    bg = d1 > D
    assert float(bg.double().mean()) > 0.3
    assert float((pre[bg] - far).abs().max()) < 0.5
    assert float(((pre > -30) & (pre < -20)).double().mean()) > 0.3
    empty = acc > 0.99
    assert float(empty.double().mean()) > 0.15
    alpha_last = 1 - torch.exp(-sig[empty, -1] * O.LAST_DELTA)
    assert float(alpha_last.min()) > 0.5


def test_sigma_pre_grad_matches_autograd_of_softplus():
    """ops.sigma_pre_grad (the training step's sigma-head derivative, rebuilt from the saved density) against autograd of F.softplus, in
    fp32 over pre in [-40, 40] -- through the threshold at 20 and down where sigma is far below 6e-8 (there 1 - exp(-sigma) is 0)."""
    from supnerf_amd import ops
    pre = torch.linspace(-40, 40, 8001).double()                 # (fp32 values: both sides differentiate at the same points)
    up = torch.rand(pre.shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64) * 2 - 1
    x64 = pre.clone().requires_grad_()
    (F.softplus(x64) * up).sum().backward()
    x32 = pre.float().requires_grad_()
    sig32 = F.softplus(x32)
    (sig32 * up.float()).sum().backward()
    got = ops.sigma_pre_grad(up.float(), sig32.detach())
    assert got.dtype == torch.float32
    # a few fp32 roundings of the true value, like torch's own fp32 derivative
    assert ((got.double() - x64.grad).abs() <= 4e-7 * x64.grad.abs()).all()
    assert ((got.double() - x32.grad.double()).abs() <= 4e-7 * x32.grad.double().abs()).all()
    assert float(got[pre < -20].abs().min()) > 0
