"""Ray-cast surfaces on the MI355X: the ``snr_ray_*`` kernels against tests/ray_restatement.py bit for bit when both read the GPU's own
sigma; ``geometry.ray_surface`` against the float64 truth of tests/test_ray_surface_cpu.py (same inputs, same conditions, same derived
bounds); normals against the planted box's closed form and the float64 oracle; the implicit-function gradients against float64 autograd
of the oracle at the same hit points and ReLU bits; and ``surface_depth`` / ``to_decoder_frame`` on a synthetic object."""
import numpy as np
import pytest
import torch

import ray_restatement as RR
from geometry_cases import LEVEL_BOX, box, codes as _codes, model as _model
from oracle_bands import amd, capture_latent, dev, in_band  # noqa: F401  (fixtures)
from planted_decoder import HALF, WOBBLE, box_rays, planted_params
from relu_bits import decode_relu_bits

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.75, 2.25
REFINES = [(0, 2), (8, 3), (4, 5), (2, 17), (1, 257), (3, 17)]


def _np(t):
    return t.detach().cpu().numpy()


def _gpu_sigma(G, model, sc):
    """The GPU's own sigma as a density callable for the restatement."""
    return lambda pts: _np(G.query_density(model, torch.from_numpy(np.ascontiguousarray(pts)).to(sc.device), sc))


def _box_batch(B, N, seed, dev):  # noqa: F811
    """B x N box rays with per-ray bounds around [0.75, 2.25]; ray 5 of every object has near = far."""
    o, d, _ = box_rays(B * N, 64, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    near = NEAR + 0.05 * torch.rand(B * N, generator=g)
    far = FAR - 0.05 * torch.rand(B * N, generator=g)
    far.view(B, N)[:, 5] = near.view(B, N)[:, 5]
    return o.to(dev), d.to(dev), near.to(dev), far.to(dev)


def _fog_batch(B, N, seed, dev):  # noqa: F811
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(B * N, 3, generator=g) - 0.5) * 1.2
    d = torch.randn(B * N, 3, generator=g) * 0.7                                  # not unit: t is in units of |d|
    near = -0.4 * torch.rand(B * N, generator=g)
    far = 0.2 + 0.6 * torch.rand(B * N, generator=g)
    return o.to(dev), d.to(dev), near.to(dev), far.to(dev)


def _march_and_compare(amd, model, sc, o, d, near, far, level, S, refine, tag):  # noqa: F811
    """The search step by step through ``ops``, every intermediate against the restatement fed ``query_density``."""
    from supnerf_amd import geometry as G
    ops = amd.ops
    sb, tb = model.shape_blocks, model.texture_blocks
    lat, packed = model.latent_terms(sc, torch.zeros_like(sc)).detach().contiguous(), model.packed_weights()
    want = RR.ray_surface(_gpu_sigma(G, model, sc), _np(o), _np(d), _np(near), _np(far), level, S, refine)
    ta, tb_ = near.clone(), far.clone()
    va = vb = state = None
    for m, S_m in zip(want["marches"], [S] + [refine[1]] * refine[0]):
        pts = ops.ray_march_points(o, d, ta, tb_, S_m)
        assert np.array_equal(_np(pts), m["points"]), (tag, S_m, "points")
        sig = G.query_density(model, pts, sc)
        assert torch.equal(sig, ops.density_fwd(pts, lat, packed, sb, tb)[0]), (tag, "sigma")
        assert np.array_equal(_np(sig).reshape(-1, S_m), m["sigma"], equal_nan=True), (tag, S_m, "sigma")
        ta, tb_, va, vb, state = ops.ray_first_crossing(sig.view(-1, S_m), ta, tb_, level, va, vb, state)
        for name, got in (("ta", ta), ("tb", tb_), ("va", va), ("vb", vb)):
            assert np.array_equal(_np(got), m[name]), (tag, S_m, name)
    assert np.array_equal(_np(state), want["state"]), (tag, "state")
    t, width, x = ops.ray_hit_points(o, d, ta, tb_, va, vb, state, level)
    for name, got in (("depth", t), ("width", width), ("x", x)):
        assert np.array_equal(_np(got), want[name]), (tag, name)
    assert torch.equal(x, o + t[:, None] * d), (tag, "x = o + t d")
    assert want["lost"] == 0, (tag, "a state-1 ray lost its crossing")
    # the one-call search, twice: the same bits (no atomics)
    for _ in range(2):
        br = ops.ray_brackets(o, d, near, far, lat, packed, level, S, refine[0], refine[1], sb, tb)
        assert all(torch.equal(a, b) for a, b in zip(br, (ta, tb_, va, vb, state))), (tag, "ray_brackets")
    return want, x, va, vb, state


@pytest.mark.parametrize("refine", [(0, 2), (8, 3), (2, 17)])
@pytest.mark.parametrize("S", [2, 37, 64, 200])
def test_kernels_are_the_restatement(amd, dev, S, refine):  # noqa: F811
    from supnerf_amd import geometry as G
    B, N = 3, 1000
    bx = box(amd, dev, 3, 1, seed=1, wobble=WOBBLE)
    sc = _codes(B, 5, dev)
    o, d, near, far = _box_batch(B, N, 3, dev)
    want, x, va, vb, state = _march_and_compare(amd, bx, sc, o, d, near, far, LEVEL_BOX, S, refine, ("box", S, refine))
    hit = state == 1
    assert not bool(hit.view(B, N)[:, 5].any())                                  # near = far: one point marched S times, no crossing
    if S >= 37:
        assert int(hit.sum()) > B * N // 2
        sx = G.query_density(bx, x, sc)
        assert bool(((sx - LEVEL_BOX).abs() <= (vb - va))[hit].all())             # sigma is monotone across the planted surface
    # scalar bounds through the same kernels
    sn, sf = torch.full_like(near, NEAR), torch.full_like(far, FAR)
    _march_and_compare(amd, bx, sc, o, d, sn, sf, LEVEL_BOX, S, refine, ("box scalar", S, refine))
    # the fog cut at its median density: many crossings per ray, pockets thinner than a step; bit equality only
    fog = _model(amd, dev, 3, 1, seed=0)
    o, d, near, far = _fog_batch(B, N, 9, dev)
    level = float(G.query_density(fog, amd.ops.ray_march_points(o, d, near, far, 16), sc).median())
    want, *_ = _march_and_compare(amd, fog, sc, o, d, near, far, level, S, refine, ("fog", S, refine))
    if S >= 37:
        assert {1, 2} <= set(want["state"].tolist())                             # hits and inside starts both occur


@pytest.mark.parametrize("S", [2, 5, 31, 32, 64, 65, 200])
def test_first_crossing_on_planted_sigma(amd, dev, S):  # noqa: F811
    """``ops.ray_first_crossing`` on a sigma array of its own making (both kernels: a thread per ray below 32 samples, a wave per ray from
    32 on): NaN counts as outside, +inf as inside, the first pair wins, a refinement leaves states 0 / 2 alone and a state-1 ray without
    a crossing keeps its bracket."""
    ops = amd.ops
    R = 777
    g = np.random.default_rng(S)
    sig = g.uniform(0, 1, (R, S)).astype(np.float32)
    sig[g.uniform(size=(R, S)) < 0.7] = 0.0                                       # sparse: the first crossing is often late in the row
    sig[g.uniform(size=(R, S)) < 0.03] = np.nan
    sig[g.uniform(size=(R, S)) < 0.03] = np.inf
    sig[::7] = 0.0                                                                # misses
    sig[3::11, 0] = np.inf                                                        # inside starts
    if S > 2:
        sig[5::13] = 0.0
        sig[5::13, S - 1] = 1.0                                                   # the only crossing is the last pair
    level = 0.5
    ta = g.uniform(-1, 1, R).astype(np.float32)
    tb = (ta + g.uniform(0, 2, R).astype(np.float32)).astype(np.float32)
    w = RR.first_crossing(sig, ta, tb, level)
    got = ops.ray_first_crossing(torch.from_numpy(sig).to(dev), torch.from_numpy(ta).to(dev), torch.from_numpy(tb).to(dev), level)
    for name, a, b in zip(("ta", "tb", "va", "vb", "state"), got, w):
        assert np.array_equal(_np(a), b, equal_nan=True), (S, name)
    assert set(w[4].tolist()) == {0, 1, 2}
    sig2 = g.uniform(0, 1, (R, S)).astype(np.float32)
    sig2[g.uniform(size=(R, S)) < 0.05] = np.nan
    sig2[1::5] = 0.0                                                              # no crossing in the refinement
    w2 = RR.first_crossing(sig2, w[0], w[1], level, (w[2], w[3], w[4]))
    got2 = ops.ray_first_crossing(torch.from_numpy(sig2).to(dev), *got[:2], level, *got[2:])
    for name, a, b in zip(("ta", "tb", "va", "vb", "state"), got2, w2):
        assert np.array_equal(_np(a), b, equal_nan=True), (S, "refine", name)
    assert w2[5].any() and np.array_equal(w2[4], w[4])
    t, width, x = ops.ray_hit_points(torch.zeros(R, 3, device=dev), torch.ones(R, 3, device=dev), *got2, level)
    wt, ww, wx = RR.hit_points(np.zeros((R, 3), np.float32), np.ones((R, 3), np.float32), *w2[:5], level)
    assert np.array_equal(_np(t), wt, equal_nan=True) and np.array_equal(_np(width), ww, equal_nan=True)
    assert np.array_equal(_np(x), wx, equal_nan=True)


def test_c_abi_checks(amd, dev):  # noqa: F811
    ops, lib = amd.ops, amd._lib.lib()
    p, st = ops._p, ops._stream(dev)
    o, d = torch.zeros(8, 3, device=dev), torch.ones(8, 3, device=dev)
    ta, tb = torch.zeros(8, device=dev), torch.ones(8, device=dev)
    xyz = torch.empty(8 * 4, 3, device=dev)
    assert lib.snr_ray_march_points(p(o), p(d), p(ta), p(tb), 8, 1, p(xyz), st) == -1
    assert lib.snr_ray_march_points(p(o), p(d), p(ta), None, 8, 4, p(xyz), st) == -1
    assert lib.snr_ray_march_points(p(o), p(d), p(ta), p(tb), 8, 4, p(xyz), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(xyz.view(8, 4, 3)[:, -1], d)                              # the last sample is tb itself
    with pytest.raises(amd.SnrError):
        ops.ray_march_points(o, d[:4], ta, tb, 4)
    with pytest.raises(amd.SnrError):
        ops.ray_march_points(o, d, ta, tb[:4], 4)
    with pytest.raises(amd.SnrError):
        ops.ray_first_crossing(torch.zeros(8, 4, device=dev), ta[:4], tb, 0.5)
    with pytest.raises(amd.SnrError):
        ops.ray_first_crossing(torch.zeros(8, 4, device=dev).t(), ta[:4], tb[:4], 0.5)


@pytest.fixture(scope="module")
def box_truth():
    """The CPU test's case: planted box with wobble, code seed 5, box_rays(512, 64, seed=3), float64 truth."""
    p32 = planted_params(3, 1, seed=1, wobble=WOBBLE)
    p64 = {k: v.double() for k, v in p32.items()}
    code = torch.randn(1, 256, generator=torch.Generator().manual_seed(5)) * 0.5
    o, d, _ = box_rays(512, 64, seed=3)
    state, depth = RR.truth(RR.oracle_sigma_fn(p64, code), o.numpy(), d.numpy(), NEAR, FAR, LEVEL_BOX)
    return dict(p32=p32, code=code, o=o, d=d, state=state, depth=depth)


@pytest.mark.parametrize("refine", REFINES)
def test_ray_surface_against_the_float64_truth(amd, dev, box_truth, refine):  # noqa: F811
    """tests/test_ray_surface_cpu.py's conditions through ``geometry.ray_surface``: all 512 states, |t - truth| <= width, the depth and
    the truth inside the final bracket, width <= 1.01 (far - near) / 63 / (S_r - 1)^levels."""
    from supnerf_amd import geometry as G
    c = box_truth
    model = _model(amd, dev, 3, 1, params=c["p32"])
    sc, o, d = c["code"].to(dev), c["o"].to(dev), c["d"].to(dev)
    r = G.ray_surface(model, o, d, NEAR, FAR, sc, level=LEVEL_BOX, n_samples=64, refine=refine)
    assert r.depth.shape == (512,) and r.state.dtype == torch.uint8 and r.normal.shape == (512, 3) and r.width.shape == (512,)
    state = _np(r.state)
    assert int((c["state"] == 1).sum()) == 384 and int((c["state"] == 0).sum()) == 128
    assert np.array_equal(state, c["state"])
    hit = state == 1
    t, w, truth = _np(r.depth).astype(np.float64), _np(r.width).astype(np.float64), c["depth"]
    err = np.abs(t - truth)[hit]
    bound = 1.01 * (FAR - NEAR) / 63 / (refine[1] - 1) ** refine[0]
    print(f"refine {refine}: max |t - truth| {err.max():.3e}, max width {w[hit].max():.4e} (bound {bound:.4e})")
    assert (err <= w[hit]).all() and w[hit].max() <= bound
    assert (t[~hit] == 0).all() and (w[~hit] == 0).all()
    lat = model.latent_terms(sc, torch.zeros_like(sc)).detach().contiguous()
    ta, tb, va, vb, st = amd.ops.ray_brackets(o, d, torch.full((512,), NEAR, device=dev), torch.full((512,), FAR, device=dev), lat,
                                              model.packed_weights(), LEVEL_BOX, 64, refine[0], refine[1], 3, 1)
    ta, tb = _np(ta).astype(np.float64), _np(tb).astype(np.float64)
    assert np.array_equal(_np(st), state) and np.array_equal((tb - ta)[hit], w[hit])
    assert (t[hit] >= ta[hit]).all() and (t[hit] <= tb[hit]).all() and (truth[hit] >= ta[hit]).all() and (truth[hit] <= tb[hit]).all()
    assert bool((va < LEVEL_BOX)[torch.from_numpy(hit).to(dev)].all()) and bool((vb >= LEVEL_BOX)[torch.from_numpy(hit).to(dev)].all())
    # a (1, N, 3) batch and 0-dim tensor bounds: the same bits
    r3 = G.ray_surface(model, o[None], d[None], torch.tensor(NEAR), torch.tensor(FAR, device=dev), sc, level=LEVEL_BOX, refine=refine)
    assert r3.depth.shape == (1, 512) and r3.normal.shape == (1, 512, 3)
    assert torch.equal(r3.depth[0], r.depth) and torch.equal(r3.state[0], r.state) and torch.equal(r3.normal[0], r.normal)


def test_rays_that_start_inside_and_errors(amd, dev):  # noqa: F811
    from supnerf_amd import geometry as G
    model = box(amd, dev, 3, 1, seed=1, wobble=WOBBLE)
    sc = _codes(1, 5, dev).requires_grad_()
    g = torch.Generator().manual_seed(4)
    o = ((torch.rand(32, 3, generator=g) * 2 - 1) * torch.tensor(HALF) * 0.5).to(dev).requires_grad_()
    d = torch.nn.functional.normalize(torch.randn(32, 3, generator=g), dim=1).to(dev).requires_grad_()
    near = torch.zeros(32, device=dev)
    near[16:] = 0.01
    r = G.ray_surface(model, o, d, near, 2.0, sc, level=LEVEL_BOX, n_samples=16)
    assert bool((r.state == 2).all()) and torch.equal(r.depth.detach(), near) and not bool(r.width.any()) and not bool(r.normal.any())
    r.depth.sum().backward()
    assert not bool(o.grad.any()) and not bool(d.grad.any()) and not bool(sc.grad.any())
    o, d = o.detach(), d.detach()
    for bad in (dict(n_samples=1), dict(refine=(1, 1)), dict(refine=(-1, 3))):
        with pytest.raises(amd.SnrError):
            G.ray_surface(model, o, d, 0.0, 2.0, sc, level=LEVEL_BOX, **bad)
    with pytest.raises(amd.SnrError):
        G.ray_surface(model, o, d, 2.0, 1.0, sc, level=LEVEL_BOX)                # far < near
    with pytest.raises(amd.SnrError):
        G.ray_surface(model, o, d[:8], 0.0, 2.0, sc, level=LEVEL_BOX)
    with pytest.raises(amd.SnrError):
        G.ray_surface(model, o, d, 0.0, 2.0, _codes(2, 1, dev), level=LEVEL_BOX)  # (N, 3) rays take one code
    with pytest.raises(amd.SnrError):
        G.ray_surface(model, o, d, near[:8], 2.0, sc, level=LEVEL_BOX)
    with pytest.raises(amd.SnrError):
        G.ray_surface(model, o.cpu(), d, 0.0, 2.0, sc, level=LEVEL_BOX)
    assert G.ray_surface(model, o, d, 0.0, 2.0, sc, level=LEVEL_BOX, refine=(0, None)).depth.shape == (32,)
    model.train_decoder_weights = True
    with pytest.raises(amd.SnrError):
        G.ray_surface(model, o, d, 0.0, 2.0, sc, level=LEVEL_BOX)
    with torch.no_grad():
        assert bool((G.ray_surface(model, o, d, near, 2.0, sc, level=LEVEL_BOX).state == 2).all())


def test_planted_box_normals(amd, dev, box_truth):  # noqa: F811
    """Without wobble the surface is d1 = H and the outward normal at x is normalise(sign(x_a) [|x_a| > h_a]): piecewise constant.
    Compared on every hit ray whose x keeps | |x_a| - h_a | > 0.005 on all three axes (50 bracket widths: the found point and the true
    one lie in the same piece); at most 10 % of the hit rays are left out and pieces with one, two and three active axes all occur.
    1e-5 per component: through the planted identity rows the components of g are +-K sigmoid(pre) or exactly 0; only the
    normalisation rounds."""
    from supnerf_amd import geometry as G
    c = box_truth
    model = box(amd, dev, 3, 1, seed=1)
    o, d, sc = c["o"].to(dev), c["d"].to(dev), c["code"].to(dev)
    r = G.ray_surface(model, o, d, NEAR, FAR, sc, level=LEVEL_BOX, refine=(2, 17))
    hit = r.state == 1
    assert int(hit.sum()) == 384
    n = r.normal.cpu().double()
    assert float((n[hit.cpu()].norm(dim=1) - 1).abs().max()) < 1e-6 and not bool(r.normal[~hit].any())
    x = (o + r.depth[:, None] * d).cpu().double()
    gap = x.abs() - torch.tensor(HALF, dtype=torch.float64)
    s = torch.sign(x) * (gap > 0).double()
    want = s / s.norm(dim=1, keepdim=True).clamp_min(1e-30)
    keep = hit.cpu() & (gap.abs() > 0.005).all(dim=1)
    kinds = (gap > 0).sum(1)[hit.cpu()]
    print(f"normals: {int(keep.sum())} of 384 compared; active axes 1/2/3: {[int((kinds == k).sum()) for k in (1, 2, 3)]}")
    assert int(keep.sum()) >= 0.9 * 384 and all(int((kinds == k).sum()) > 0 for k in (1, 2, 3))
    assert float((n[keep] - want[keep]).abs().max()) <= 1e-5


def _oracle_rule8(params, x, d, t, state, w, sc, layers, dtype):
    """Rules 7 - 8 on the oracle in ``dtype`` at the hit points x with the kernel's ReLU bits: (g, d rays_o, d rays_d, d shapecode)."""
    p = {k: v.to(dtype) for k, v in params.items()}
    xx = x.detach().cpu().to(dtype).requires_grad_()
    s = sc.detach().cpu().to(dtype).requires_grad_()
    sig = RR.oracle_sigma(p, xx, s, [m.to(dtype) for m in layers])
    g, = torch.autograd.grad(sig.sum(), xx, retain_graph=True)
    d_o, d_d, c = RR.implicit_gradient(g, d.cpu().to(dtype), t.detach().cpu().to(dtype), state, w.cpu().to(dtype))
    d_sc, = torch.autograd.grad((sig * c).sum(), s)
    return g, d_o, d_d, d_sc


@pytest.mark.parametrize("blocks", [(3, 1), (1, 1)])
def test_gradients_against_float64(amd, dev, blocks):  # noqa: F811
    """d rays_o, d rays_d and d shapecode of sum(w depth) against float64 autograd of the oracle evaluating rule 8 at the same x and the
    same ReLU bits, in the fp32 band; normals (with wobble) against the oracle's -grad sigma / |grad sigma| likewise; the latent gradient
    bit for bit ``ops.density_bwd(d_sig = c)`` by hand; misses and inside starts contribute exactly zero; no_grad and inputs without
    requires_grad return the same depth bits."""
    from supnerf_amd import geometry as G
    ops = amd.ops
    sb, tb = blocks
    B, N = 3, 1000
    params = planted_params(sb, tb, seed=10 + sb, wobble=WOBBLE)
    model = _model(amd, dev, sb, tb, params=params)
    sc0 = _codes(B, 21, dev)
    o0, d0, near, far = _box_batch(B, N, 7, dev)
    near.view(B, N)[:, 800:815] = 1.45                                            # aimed rays that start inside the box
    w = torch.randn(B * N, generator=torch.Generator().manual_seed(2)).to(dev)
    got_lat = capture_latent(model)
    o, d, sc = [t.clone().view(s).requires_grad_() for t, s in ((o0, (B, N, 3)), (d0, (B, N, 3)), (sc0, (B, 256)))]
    kw = dict(level=LEVEL_BOX, n_samples=64, refine=(2, 17))
    r = G.ray_surface(model, o, d, near.view(B, N), far.view(B, N), sc, **kw)
    del model.latent_terms                                                        # (capture_latent's wrapper: only this call is watched)
    assert r.depth.requires_grad and not r.normal.requires_grad and not r.width.requires_grad
    (r.depth.view(-1) * w).sum().backward()
    state = r.state.view(-1)
    hit = state == 1
    counts = [int((state == k).sum()) for k in (0, 1, 2)]
    print("states 0/1/2:", counts)
    assert counts[0] > 100 and counts[1] > 1000 and counts[2] >= 30
    assert not bool(o.grad.view(-1, 3)[~hit].any()) and not bool(d.grad.view(-1, 3)[~hit].any())
    assert bool(torch.isfinite(o.grad).all()) and bool(torch.isfinite(d.grad).all()) and bool(torch.isfinite(sc.grad).all())
    # the same depth bits without a graph
    with torch.no_grad():
        assert torch.equal(G.ray_surface(model, o, d, near.view(B, N), far.view(B, N), sc, **kw).depth, r.depth.detach())
    plain = G.ray_surface(model, o0.view(B, N, 3), d0.view(B, N, 3), near.view(B, N), far.view(B, N), sc0, **kw)
    assert plain.depth.grad_fn is None and torch.equal(plain.depth, r.depth.detach()) and torch.equal(plain.normal, r.normal)
    # by hand: the hit points padded to 1024 per object, the density pair, c, the latent gradient
    t = r.depth.detach().view(-1)
    x = o0 + t[:, None] * d0
    lat = model.latent_terms(sc0, torch.zeros_like(sc0)).detach().contiguous()
    packed = model.packed_weights()
    xp = ops._pad_rows(x, B, N, 1024)
    sig, masks = ops.density_fwd(xp, lat, packed, sb, tb, save_masks=True)
    _, gp = ops.density_bwd(xp, lat, packed, masks, sig, torch.ones_like(sig), sb, tb, need_latent=False)
    g = ops._unpad_rows(gp, B, N, 1024)
    slope = g[:, 0] * d0[:, 0] + g[:, 1] * d0[:, 1] + g[:, 2] * d0[:, 2]
    c = torch.where(hit, -w / slope, torch.zeros_like(w))
    d_lat, _ = ops.density_bwd(xp, lat, packed, masks, sig, ops._pad_rows(c, B, N, 1024), sb, tb, need_latent=True, need_xyz=False)
    assert len(got_lat) >= 1 and torch.equal(got_lat[0].grad, d_lat)
    assert torch.equal(o.grad.view(-1, 3), c[:, None] * g) and torch.equal(d.grad.view(-1, 3), (t * c)[:, None] * g)
    # against the oracle at the same x and ReLU bits
    _, m_un = ops.density_fwd(x, lat, packed, sb, tb, save_masks=True)
    layers = decode_relu_bits(m_un, B * N, sb, tb)[:sb + 1]
    assert all(torch.equal(a, b.reshape(B, 1024, -1)[:, :N].reshape(B * N, -1))
               for a, b in zip(layers, decode_relu_bits(masks, B * 1024, sb, tb)[:sb + 1]))
    st = _np(state)
    g64, o64, dd64, s64 = _oracle_rule8(params, x, d0, t, st, w, sc0, layers, torch.float64)
    g32, o32, dd32, s32 = _oracle_rule8(params, x, d0, t, st, w, sc0, layers, torch.float32)
    for name, got, a32, a64 in (("d rays_o", o.grad.view(-1, 3), o32, o64), ("d rays_d", d.grad.view(-1, 3), dd32, dd64),
                                ("d shapecode", sc.grad, s32, s64)):
        ok, _, msg = in_band(got, a32, a64, "fp32", f"{name} {blocks}")
        print(msg)
        assert ok, msg
    ok, _, msg = in_band(r.normal.view(-1, 3), RR.normals(g32, st), RR.normals(g64, st), "fp32", f"normals {blocks}")
    print(msg)
    assert ok, msg
    assert float((r.normal.view(-1, 3)[hit].norm(dim=1) - 1).abs().max()) < 1e-6 and not bool(r.normal.view(-1, 3)[~hit].any())


@pytest.mark.parametrize("family", ["a", "b"])
def test_surface_depth(amd, dev, family):  # noqa: F811
    """A grid call and a ``pixels=`` call on the same pixels agree bit for bit; metric depth x view direction + camera centre, mapped by
    ``to_decoder_frame``, is the decoder-frame hit point to fp32 rounding; the gradient reaches ``cam_pose`` and the shape code."""
    from supnerf_amd import driver, geometry as G, utils as U
    ob = driver.make_objects([11], 16)[0]
    model = box(amd, dev, 3, 1, seed=1, wobble=WOBBLE)
    sc = _codes(1, 5, dev).requires_grad_()
    pose = ob["cam_pose"].float().to(dev).requires_grad_()
    x0, y0, x1, y1 = [int(v) for v in ob["roi"]]
    x0, y0 = (x0 + x1) // 2 - 12, (y0 + y1) // 2 - 10                              # a 24 x 20 window at the centre of the crop
    roi = [x0, y0, x0 + 24, y0 + 20]
    diag = float(ob["obj_diag"])
    # level 60 = softplus(K 0.2): the surface at L1 distance 0.1 from the planted box, at most 0.43 from the centre -- inside family a's
    # bounding sphere of radius 1/2 in decoder units (the surface at LEVEL_BOX reaches 0.55: every central ray would start inside it)
    level = 60.0
    kw = dict(level=level, family=family, shapenet_obj_cood=True)
    grid = G.surface_depth(model, pose, diag, ob["K"], roi, sc, **kw)
    assert grid.depth.shape == (20, 24) and grid.normal.shape == (20, 24, 3) and grid.state.shape == (20, 24)
    ys, xs = np.meshgrid(np.arange(y0, y0 + 20), np.arange(x0, x0 + 24), indexing="ij")
    pix = G.surface_depth(model, pose, diag, ob["K"], roi, sc, pixels=(xs.reshape(-1), ys.reshape(-1)), **kw)
    assert pix.depth.shape == (480,)
    for a, b in zip(grid, pix):
        assert torch.equal(a.reshape(b.shape), b)
    hit = pix.state == 1
    print(f"surface_depth family {family}: states 0/1/2 {[int((pix.state == k).sum()) for k in (0, 1, 2)]} of 480 pixels")
    assert int(hit.sum()) >= 20
    small = G.surface_depth(model, pose, diag, ob["K"], ob["roi"], sc, im_sz=8, **kw)
    assert small.depth.shape == (8, 8)
    # the hit point two ways
    rays_o, viewdir = U.get_rays_specified(ob["K"], pose.detach(), xs.reshape(-1), ys.reshape(-1))
    metric = rays_o + pix.depth.detach()[:, None] * viewdir
    scale = diag if family == "a" else diag / 2
    o = G.to_decoder_frame(rays_o, diag, family, shapenet_obj_cood=True)
    d = G.to_decoder_frame(viewdir, diag, family, shapenet_obj_cood=True, direction=True)
    x = o + (pix.depth.detach() / scale)[:, None] * d
    err = float((G.to_decoder_frame(metric, diag, family, shapenet_obj_cood=True) - x)[hit].abs().max())
    dist = float(rays_o[0].norm()) / scale
    assert err <= 16 * 2.0 ** -24 * dist, (err, dist)                            # a few fp32 roundings at the size of |o|
    sig = G.query_density(model, x[hit], sc.detach())
    assert float((sig - level).abs().max()) < 300.0 * 2 * float(pix.width[hit].max()) / scale + 1e-3       # |grad sigma| <= K sqrt(3)
    back = G.to_decoder_frame(pix.normal, diag, family, shapenet_obj_cood=True, direction=True)
    assert float((back[hit].norm(dim=1) - 1).abs().max()) < 1e-6
    (pix.depth * torch.randn(480, generator=torch.Generator().manual_seed(1)).to(dev)).sum().backward()
    assert pose.grad is not None and bool(torch.isfinite(pose.grad).all()) and float(pose.grad.abs().max()) > 0
    assert sc.grad is not None and float(sc.grad.abs().max()) > 0
