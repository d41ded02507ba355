"""Test helper: the scene composite (per-pixel depth merge + composite) restated densely in torch, as the oracle of record for its
GRADIENTS (include/supnerf_hip.h, snr_scene_composite_bwd).

Per pixel, with n samples i = 0..n-1 in memory order:

    lt_i = #{j : z_j < z_i},  eb_i = #{j < i : z_j == z_i},  ea_i = #{j > i : z_j == z_i}
    slot of sample i: pos_i = lt_i + eb_i (a permutation); the sorted depth row is zs[pos_i] = z_i
    slot lt_i receives (sigma_i, rgb_i) from its group's survivor (ea_i == 0, the last member in memory order); the group's other slots
    hold sigma 0 and rgb 0
    the sorted rows are composited by ``oracle.composite`` (relu, LAST_DELTA, TRANS_EPS, white background)

Autograd through these lines IS the backward rule: the survivor receives the d_sigma / d_rgb of slot lt_i, every other member exact zeros,
and every sample the d_z of its own slot.  ``oracle.scene_composite`` (sort, searchsorted, scatter_) has the same forward, and the same
autograd wherever no two real samples of a pixel share a depth; on ties torch's scatter_ / sort backward hands gradients to overwritten
members and splits d_z arbitrarily, which is why the rule is stated here.  Costs P n^2 booleans: evaluated in chunks of pixels."""
import torch

from oracle import supnerf_oracle as O


def ranks(z):
    """lt, eb, ea (P,n) int64 of depths z (P,n)."""
    n = z.shape[1]
    zi, zj = z[:, :, None], z[:, None, :]
    idx = torch.arange(n, device=z.device)
    before = (idx[None, :] < idx[:, None])[None]          # [i, j]: j < i
    eq = zj == zi
    return (zj < zi).sum(-1), (eq & before).sum(-1), (eq & ~before).sum(-1) - 1


def merged_rows(sig, rgb, z):
    """The sorted rows (sigma (P,n), rgb (P,n,3), z (P,n)) the composite runs on."""
    lt, eb, ea = ranks(z)
    pos = lt + eb
    keep = (ea == 0).to(sig.dtype)
    z_sort = torch.zeros_like(z).scatter(1, pos, z)
    s_sort = torch.zeros_like(sig).scatter_add(1, lt, sig * keep)
    c_sort = torch.zeros_like(rgb).scatter_add(1, lt[:, :, None].expand(-1, -1, 3), rgb * keep[:, :, None])
    return s_sort, c_sort, z_sort


def scene_composite(sig, rgb, z, white_bkgd=True, chunk=256):
    """rgb (P,3), depth (P), acc (P); differentiable with respect to all three inputs."""
    outs = []
    for a in range(0, max(z.shape[0], 1), chunk):
        s, c, zz = merged_rows(sig[a:a + chunk], rgb[a:a + chunk], z[a:a + chunk])
        outs.append(O.composite(s, c, zz, white_bkgd))
    return tuple(torch.cat([o[k] for o in outs], 0) for k in range(3))


def grads(sig, rgb, z, w_rgb, w_depth=None, w_acc=None, white_bkgd=True, dtype=torch.float64, chunk=256):
    """(d_sigma, d_rgb, d_z) of sum(w_rgb rgb) + sum(w_depth depth) + sum(w_acc acc) on the CPU in ``dtype``; None weights count as zero."""
    sig, rgb, z = [t.detach().cpu().to(dtype).requires_grad_() for t in (sig, rgb, z)]
    out = scene_composite(sig, rgb, z, white_bkgd, chunk)
    loss = (out[0] * w_rgb.detach().cpu().to(dtype)).sum()
    if w_depth is not None:
        loss = loss + (out[1] * w_depth.detach().cpu().to(dtype)).sum()
    if w_acc is not None:
        loss = loss + (out[2] * w_acc.detach().cpu().to(dtype)).sum()
    return torch.autograd.grad(loss, (sig, rgb, z))


def tie_free(z):
    """(P,) bool: no two REAL samples (depth != -1) of the pixel share a depth."""
    zs = torch.sort(z, 1).values
    same = (zs[:, 1:] == zs[:, :-1]) & (zs[:, 1:] != -1)
    return ~same.any(1)


def shape_case(Nb, S, P, quarters=False):
    """The generator of test_scene_composite_shapes: near + sorted rand * 4, 30 % empty objects at -1, sigma in [-0.3, 1.7]; fp32 CPU tensors
    sig (P,n), rgb (P,n,3), z (P,n).  ``quarters``: depths rounded to quarters, so that every pixel has real ties."""
    gen = torch.Generator().manual_seed(Nb * 1000 + S)
    near = torch.rand(P, Nb, 1, generator=gen) * 20 + 2
    z = near + torch.sort(torch.rand(P, Nb, S, generator=gen), dim=-1)[0] * 4
    sig = torch.rand(P, Nb, S, generator=gen) * 2 - 0.3
    rgb = torch.rand(P, Nb, S, 3, generator=gen)
    empty = torch.rand(P, Nb, generator=gen) < 0.3
    if quarters:
        z = (z * 4).round() / 4
    z[empty] = -1; sig[empty] = 0; rgb[empty] = 1
    return sig.view(P, Nb * S), rgb.view(P, Nb * S, 3), z.view(P, Nb * S)
