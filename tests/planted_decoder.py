"""Test helper: a decoder with an opaque box planted in it, and rays that look at the box.

Every other decoder of the suite is a fresh ``init_decoder_params`` network with ``sigma_bias=-2``: a uniform fog (sigma 0.12 .. 0.13 at every
point, acc_trans 0.5 .. 0.6 on every ray).  A trained decoder renders opaque objects in empty space, and there the kernels take paths the fog
never reaches: the softplus branch ``pre > 20``, densities so small that ``softplus`` is a subnormal, transmittance products that saturate at
1e-10, and large gradients concentrated on the few samples of a surface.  ``planted_params`` keeps the random init almost everywhere (the MFMA
tiles stay dense and the colour path stays random) and overwrites a handful of units so that the density head computes

    pre = K (H - min(d1, D))          d1 = sum_a relu(|x_a| - h_a)   (L1 distance of the point outside the box +-h)

from the raw-coordinate features 0..2 of the positional encoding:

* ``encoding_xyz.0`` rows 0..5 are relu(+-x_a - h_a); row 6 is a constant 1;
* every shape layer carries rows 0..6 (and the clamp row 7) through an identity block with zero latent rows and zero bias;
* with a far-field clamp, shape layer 1 row 7 is relu(d1 - D): min(d1, D) = d1 - relu(d1 - D) (needs shape_blocks >= 1);
* ``encoding_shape`` row 0 is H u6 - sum u0..5 (+ u7); the sigma head is K on row 0 and zero elsewhere.

Inside the box pre = K H (well past the softplus threshold 20); far from it pre = -K (d1 - H), or K (H - D) with the clamp, which pins the
background at a chosen pre-activation (e.g. -23, where sigma ~ 1e-10 makes the 1e10-wide last interval's alpha of order 1)."""
import torch

from oracle import supnerf_oracle as O

HALF = (0.25, 0.2, 0.15)
H, K = 0.3, 300.0
FAR_PRE, WOBBLE = -23.0, 8.0         # the far-field case: background pinned at pre ~ -23 +- 0.5, with a gradient


def planted_params(shape_blocks=3, texture_blocks=1, seed=0, half=HALF, H=H, K=K, far_pre=None, wobble=0.0):
    """State dict (fp32, reference naming) of the planted decoder.  ``far_pre``: None = no clamp (pre falls without bound outside the box),
    else the background pre-activation K (H - D).  ``wobble``: keep ``encoding_shape`` row 0's random weights on the other units, scaled
    so that they add a smooth term of about this size to pre.  Without it the clamped far field is flat -- pre is the same constant at every
    point and for every code, so nothing upstream of sigma receives a gradient there, whatever the kernels do with softplus' tail."""
    p = O.init_decoder_params(shape_blocks, texture_blocks, seed=seed, sigma_bias=-2.0)
    clamp = far_pre is not None
    if clamp and shape_blocks < 1:
        raise ValueError("the far-field clamp needs a shape layer")
    n_carry = 8 if clamp else 7
    w0, b0 = p["encoding_xyz.0.weight"], p["encoding_xyz.0.bias"]
    w0[:7].zero_()
    for a in range(3):
        w0[2 * a, a], w0[2 * a + 1, a] = 1.0, -1.0
        b0[2 * a] = b0[2 * a + 1] = -half[a]
    b0[6] = 1.0
    for j in range(1, shape_blocks + 1):
        lw, lb = p[f"shape_latent_layer_{j}.0.weight"], p[f"shape_latent_layer_{j}.0.bias"]
        lw[:n_carry].zero_()
        lb[:n_carry].zero_()
        w, b = p[f"shape_layer_{j}.0.weight"], p[f"shape_layer_{j}.0.bias"]
        w[:n_carry].zero_()
        b[:n_carry].zero_()
        for i in range(n_carry):
            w[i, i] = 1.0
        if clamp and j == 1:
            D = H - far_pre / K
            w[7, :6] = 1.0
            w[7, 6] = -D
            w[7, 7] = 0.0
    ws, bs = p["encoding_shape.weight"], p["encoding_shape.bias"]
    ws[0] *= wobble / K
    ws[0, :n_carry] = 0.0
    bs[0] = 0.0
    ws[0, :6] = -1.0
    ws[0, 6] = H
    if clamp:
        ws[0, 7] = 1.0
    p["sigma.0.weight"].zero_()
    p["sigma.0.weight"][0, 0] = K
    p["sigma.0.bias"].zero_()
    return p


def analytic_pre(xyz, half=HALF, H=H, K=K, far_pre=None):
    """The pre-activation the planted decoder computes at object-frame points ``xyz`` (..., 3), in xyz's dtype."""
    d1 = torch.relu(xyz.abs() - torch.tensor(half, dtype=xyz.dtype)).sum(-1)
    if far_pre is not None:
        d1 = torch.clamp(d1, max=H - far_pre / K)
    return K * (H - d1)


def box_rays(n_rays, n_samples, seed=0, miss=0.25, radius=1.5, span=0.75, dtype=torch.float32):
    """Object-frame rays at distance ``radius`` from the box, a fraction ``miss`` of them aimed to pass at least 0.8 from its centre (further
    than the planted surface at L1 distance H), the rest at a point inside the box.  Returns rays_o (N,3), unit viewdir (N,3) and per-ray
    stratified depths z (N,S) over [radius - span, radius + span]."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n_rays, 3, generator=g, dtype=torch.float64)
    o = o / o.norm(dim=-1, keepdim=True) * radius
    aim = (torch.rand(n_rays, 3, generator=g, dtype=torch.float64) * 2 - 1) * torch.tensor(HALF, dtype=torch.float64) * 0.8
    n_miss = int(round(miss * n_rays))
    side = torch.randn(n_miss, 3, generator=g, dtype=torch.float64)
    side = side - (side * o[:n_miss]).sum(-1, keepdim=True) * o[:n_miss] / radius ** 2            # perpendicular to the line of sight
    aim[:n_miss] = side / side.norm(dim=-1, keepdim=True) * (0.8 + 0.2 * torch.rand(n_miss, 1, generator=g, dtype=torch.float64))
    d = aim - o
    d = d / d.norm(dim=-1, keepdim=True)
    step = 2 * span / n_samples
    z = radius - span + (torch.arange(n_samples, dtype=torch.float64) + torch.rand(n_rays, n_samples, generator=g, dtype=torch.float64)) * step
    return o.to(dtype), d.to(dtype), z.to(dtype)


def continuous_depth(o, d, half=HALF, H=H, K=K, far_pre=None, t0=0.75, t1=2.25, steps=30001):
    """Per ray, the expected termination depth of the CONTINUOUS density softplus(analytic_pre) between t0 and t1 (float64 quadrature on
    ``steps`` points) and its transmittance to t1: what the sampled render approximates, independent of the decoder's weights."""
    o, d = o.double(), d.double()
    t = torch.linspace(t0, t1, steps, dtype=torch.float64)
    sig = torch.nn.functional.softplus(analytic_pre(o[:, None, :] + t[None, :, None] * d[:, None, :], half, H, K, far_pre))
    dt = (t1 - t0) / (steps - 1)
    tau = torch.cumsum(sig * dt, -1) - sig * dt                # optical depth in front of each step
    w = torch.exp(-tau) * (1 - torch.exp(-sig * dt))
    return (w * t).sum(-1) / w.sum(-1).clamp_min(1e-300), torch.exp(-(sig * dt).sum(-1))
