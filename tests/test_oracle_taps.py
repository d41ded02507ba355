"""The oracle's training taps (``oracle.decoder_taps``: the X / G slots the training kernels dump) against float64 autograd of
``decoder_forward``, on the CPU.  tests/test_training_dumps.py compares the kernels' dumps with these taps, so they must mean exactly what
the weight gradients are built from: dW_l = G_l^T X_{l-1} and db_l = sum_p G_l for every per-point layer, at every block count."""
import pytest
import torch

from oracle import supnerf_oracle as O

BLOCKS = [(0, 0), (1, 0), (0, 1), (2, 1), (3, 1), (2, 2), (0, 4), (4, 0), (4, 4), (5, 4), (5, 5), (8, 8)]


def inputs(sb, tb, B, n, seed):
    g = torch.Generator().manual_seed(seed)
    P = B * n
    xyz = torch.rand(P, 3, generator=g, dtype=torch.float64) * 2 - 1
    vd = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=torch.float64), dim=-1)
    lat = torch.relu(torch.randn(B, max(sb + tb, 1), 256, generator=g, dtype=torch.float64) * 0.3) * float(sb + tb > 0)
    obj = (torch.arange(P) // n + 1).double()
    d_sig = torch.randn(P, generator=g, dtype=torch.float64) * obj
    d_rgb = torch.randn(P, 3, generator=g, dtype=torch.float64) * obj[:, None]
    return xyz, vd, lat, d_sig, d_rgb


@pytest.mark.parametrize("sb,tb", BLOCKS, ids=lambda v: str(v))
def test_taps_rebuild_every_weight_gradient(sb, tb):
    B, n = 2, 24
    params = {k: v.double() for k, v in O.init_decoder_params(sb, tb, seed=3 + sb + 10 * tb).items()}
    xyz, vd, lat, d_sig, d_rgb = inputs(sb, tb, B, n, seed=sb * 16 + tb)
    X, G, g_sig = O.decoder_taps(params, xyz, vd, lat, d_sig, d_rgb)
    n_slots = sb + tb + 4
    assert len(X) == len(G) == n_slots
    assert [x.shape[1] for x in X] == [256] * (n_slots - 1) + [128] and [g.shape[1] for g in G] == [256] * (n_slots - 1) + [128]

    # float64 autograd of decoder_forward wrt every per-point parameter
    p = {k: v.clone().requires_grad_() for k, v in params.items()}
    sig, rgb = O.decoder_forward(p, xyz.reshape(-1, 1, 3), vd.reshape(-1, 1, 3), None, None, latent=lat)
    ((sig.reshape(-1) * d_sig).sum() + (rgb.reshape(-1, 3) * d_rgb).sum()).backward()

    pe_x, pe_d = O.positional_encoding(xyz, 10), O.positional_encoding(vd, 4)
    names = ["encoding_xyz.0"] + [f"shape_layer_{j}.0" for j in range(1, sb + 1)] + ["encoding_shape", "encoding_viewdir.0"]
    names += [f"texture_layer_{j}.0" for j in range(1, tb + 1)] + ["rgb.0"]
    got = {}
    for l, name in enumerate(names):
        x = pe_x if l == 0 else torch.cat([X[l - 1], pe_d], dim=1) if l == sb + 2 else X[l - 1]
        got[name] = (G[l].T @ x, G[l].sum(0))
    got["sigma.0"] = (g_sig.T @ X[sb + 1], g_sig.sum(0))
    got["rgb.2"] = (d_rgb.T @ X[-1], d_rgb.sum(0))
    assert sorted(got) == sorted(k[:-len(".weight")] for k in p if k.endswith(".weight") and "latent" not in k)
    for name, (dw, db) in got.items():
        for what, a, want in (("weight", dw, p[name + ".weight"].grad), ("bias", db, p[name + ".bias"].grad)):
            assert a.shape == want.shape, (name, what)
            err = float((a - want).abs().max()) / (float(want.abs().max()) + 1e-300)
            assert err < 1e-12, (name, what, err)


def test_taps_follow_the_given_relu_masks():
    """With masks given, the G slots differentiate through those masks (what the GPU kernels saved), the X slots are unchanged."""
    sb, tb, B, n = 2, 1, 1, 16
    params = {k: v.double() for k, v in O.init_decoder_params(sb, tb, seed=8).items()}
    xyz, vd, lat, d_sig, d_rgb = inputs(sb, tb, B, n, seed=9)
    X0, G0, _ = O.decoder_taps(params, xyz, vd, lat, d_sig, d_rgb)
    g = torch.Generator().manual_seed(1)
    masks = [torch.rand(n, 256 if i < sb + tb + 2 else 128, generator=g) < 0.5 for i in range(sb + tb + 3)]
    X1, G1, _ = O.decoder_taps(params, xyz, vd, lat, d_sig, d_rgb, relu_masks=masks)
    assert all(torch.equal(a, b) for a, b in zip(X0, X1))
    assert not torch.equal(G0[0], G1[0])
    # rgb.0 is the last ReLU, encoding_xyz the first: a unit the mask turns off carries no gradient
    assert bool(((G1[-1] != 0) <= masks[-1]).all()) and bool(((G1[0] != 0) <= masks[0]).all())
