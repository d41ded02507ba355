"""Test helper: how the GPU tests judge a kernel against the float64 oracle, and the fixtures and small helpers they share.

A result is compared with the same computation on the oracle in float64 (the true value, up to float64 rounding) and in fp32 (one
sample of the rounding noise of that quantity on this host), mask-matched where a ReLU is on the path (tests/relu_bits.py).  Its band:

    |got - f64| <= C |o32 - f64| + floor,  both relative to the tensor's largest float64 entry,

with C and the floor set by the arithmetic the kernel ran in (``BANDS``).  Gradients per ray are held to the per-ray rule of
``check_per_ray`` instead.  Test modules import the ``amd`` and ``dev`` fixtures by name; each module gets its own instance."""
import pytest
import torch

# fp32 kernels: another sample of the same rounding noise as the fp32 oracle, so a few times its distance
C_FP32, FLOOR_FP32 = 4.0, 2e-5
# split kernels: the backward chain multiplies bf16 pieces, 2^-17 per product where fp32 rounds at 2^-24, i.e. 2^7 times an fp32 rounding;
# the fp32 oracle's distance already sums ~2^4 roundings over a 256-wide layer, leaving 2^3 -- times the fp32 factor 4; floor 2^-14, eight
# 2^-17 roundings
C_BF16X3, FLOOR_BF16X3 = 32.0, 2.0 ** -14
BANDS = {"fp32": (C_FP32, FLOOR_FP32), "bf16x3": (C_BF16X3, FLOOR_BF16X3)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def amd():
    import supnerf_amd
    return supnerf_amd


def make_model(amd, dev, params, precision, blocks=(3, 1), train=False):
    m = amd.CodeNeRF(shape_blocks=blocks[0], texture_blocks=blocks[1])
    m.load_state_dict(params, strict=True)
    m.precision = precision
    m = m.to(dev)
    if train:
        m.train_decoder_weights = True
    return m


def capture_latent(m):
    """Make ``m.latent_terms`` keep its output's gradient: the raw d_latent the backward kernel + reduction returned."""
    orig, got = m.latent_terms, []

    def latent_terms(sc, tc):
        z = orig(sc, tc)
        z.retain_grad()
        got.append(z)
        return z
    m.latent_terms = latent_terms
    return got


def md(a, b):
    return float((a.detach().double().cpu() - torch.as_tensor(b).detach().double().cpu()).abs().max())


def rel(a, b):
    b = torch.as_tensor(b).detach().double().cpu()
    return md(a, b) / (float(b.abs().max()) + 1e-30)


def band_of(precision):
    """The band of the arithmetic the BACKWARD ran in: ``precision`` is a model's precision, or a (forward, backward) pair; "auto"
    counts as split."""
    b = precision[1] if isinstance(precision, tuple) else precision
    return "fp32" if b == "fp32" else "bf16x3"


def in_band(got, o32, o64, band, name=""):
    """(ok, ratio, message): |got - f64| <= C |o32 - f64| + floor relative to max |f64|, ``got`` finite and shaped like the float64 value;
    ratio is the error over the band (inf when not ok); the message names the worst row."""
    c, floor = BANDS[band]
    got, o32, o64 = [torch.as_tensor(t).detach().cpu().double() for t in (got, o32, o64)]
    assert got.shape == o64.shape, (name, tuple(got.shape), tuple(o64.shape))
    top = float(o64.abs().max()) + 1e-30
    err = torch.nan_to_num((got - o64).abs(), nan=float("inf"))
    e_got, e32 = float(err.max()) / top, float((o32 - o64).abs().max()) / top
    lim = c * e32 + floor
    row = int(err.reshape(err.shape[0], -1).amax(1).argmax()) if err.dim() else 0
    ok = bool(torch.isfinite(got).all()) and e_got <= lim
    return ok, (e_got / lim if ok else float("inf")), \
        f"{name} [{band}]: {e_got:.2e} of max {top:.3e} (worst row {row}), fp32 oracle {e32:.2e}, band {lim:.2e}"


def check_all(pairs, band):
    """``pairs``: (name, got, o32, o64); every tensor in its band."""
    res = [in_band(g, a, b, band, n) for n, g, a, b in pairs]
    for _, _, msg in res:
        print(msg)
    print("worst", max(res, key=lambda r: r[1])[2])
    bad = [msg for ok, _, msg in res if not ok]
    assert not bad, bad[:8]


def check_per_object(pairs, band, objects=None):
    """``pairs``: (name, got, o32, o64) with the object as dim 0; every object against its own float64 row."""
    bad, worst = [], {}
    for name, got, o32, o64 in pairs:
        got = torch.as_tensor(got).detach().cpu()
        assert got.shape == o64.shape, (name, tuple(got.shape), tuple(o64.shape))
        for b in range(o64.shape[0]):
            ok, r, msg = in_band(got[b], o32[b], o64[b], band, f"{name}[obj {b if objects is None else objects[b]}]")
            if not ok:
                bad.append(msg)
            if name not in worst or r > worst[name][0]:
                worst[name] = (r, msg)
    for r, msg in worst.values():
        print("worst", msg)
    assert not bad, bad[:8]


def per_ray_errors(got, o32, o64):
    """(error of ``got``, error of the fp32 oracle) per ray (dim 0), each relative to that ray's largest float64 entry."""
    got, o32, o64 = [torch.as_tensor(x).detach().cpu().double() for x in (got, o32, o64)]
    assert got.shape == o64.shape, (tuple(got.shape), tuple(o64.shape))
    got, o32, o64 = [x.reshape(x.shape[0], -1) for x in (got, o32, o64)]
    scale = o64.abs().amax(dim=1).clamp_min(1e-12)
    return (got - o64).abs().amax(dim=1) / scale, (o32 - o64).abs().amax(dim=1) / scale


def check_per_ray(name, got, o32, o64):
    """Every ray within 1e-3 of ITS OWN float64 gradient, or within 8x what the fp32 oracle manages on that ray (grazing rays are
    ill-conditioned in fp32 whoever computes them); a non-finite ray fails.  Returns the rays outside, for the caller's assert."""
    err, floor = per_ray_errors(got, o32, o64)
    bad = ~torch.isfinite(err) | ((err > 1e-3) & (err > 8 * floor))
    print(f"[per-ray {name}] median rel err {float(err.median()):.1e} (fp32 oracle {float(floor.median()):.1e}), 99th pct "
          f"{float(err.quantile(0.99)):.1e} ({float(floor.quantile(0.99)):.1e}), worst {float(err.max()):.1e} (fp32 oracle "
          f"{float(floor.max()):.1e}), rays outside: {int(bad.sum())}")
    return [] if not bool(bad.any()) else [(name, torch.nonzero(bad).flatten()[:10].tolist(), err[bad][:10].tolist(), floor[bad][:10].tolist())]
